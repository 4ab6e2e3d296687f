"""Shared by test_aromaticity_cpu.py and test_gpu_aromaticity.py: an oracle for csrc/kekule.inc that shares nothing with it -- the
rule of DESIGN.md section 8o restated in plain Python over sets and dicts (recursive enumeration of perfect matchings, hexagons
by brute-force cycle search, the Clar number by its textbook definition: the most pairwise disjoint hexagons whose removal leaves
a perfectly matchable graph) -- the hand-made molecules, and the packed calls of the two entry points."""
import itertools

import networkx as nx
import numpy as np

from gaudi_amd import _lib
from tests.bond_order_helpers import DATASET, C, H, fixture, pack

(OK, NO_KEKULE, NOT_NEUTRAL, NOT_CONNECTED, BAD_VALENCE, BAD_INPUT, OVERFLOW, EMPTY, UNDECIDED) = range(9)
BUDGET, MAX_SEL, MAX_EDGES, MAX_HEX = 1 << 20, 128, 192, 32
_CACHE = {}

SMILES = {
    "benzene": "C1=CC=CC=C1", "naphthalene": "C1=CC=C2C=CC=CC2=C1", "anthracene": "C1=CC=C2C=C3C=CC=CC3=CC2=C1",
    "tetracene": "C1=CC=C2C=C3C=C4C=CC=CC4=CC3=CC2=C1", "phenanthrene": "C1=CC=C2C(=C1)C=CC3=CC=CC=C32",
    "pyrene": "C1=CC2=C3C(=C1)C=CC4=CC=CC(=C43)C=C2", "chrysene": "C1=CC=C2C(=C1)C=CC3=C2C=CC4=CC=CC=C43",
    "triphenylene": "C1=CC=C2C(=C1)C3=CC=CC=C3C4=CC=CC=C24", "perylene": "C1=CC2=C3C(=C1)C4=CC=CC5=C4C(=CC=C5)C3=CC=C2",
    "coronene": "C1=CC2=C3C4=C1C=CC5=C4C6=C(C=C5)C=CC7=C6C3=C(C=C2)C=C7", "pyridine": "C1=CC=NC=C1", "thiophene": "C1=CSC=C1",
    "pyrrole": "C1=CNC=C1", "borole": "C1=CBC=C1", "biphenylene": "C1=CC2=C(C=C1)C3=CC=CC=C23"}
KNOWN = {"benzene": (2, 1), "naphthalene": (3, 1), "anthracene": (4, 1), "tetracene": (5, 1), "phenanthrene": (5, 2), "pyrene": (6, 2),
         "chrysene": (8, 2), "triphenylene": (9, 3), "perylene": (9, 2), "coronene": (20, 3)}  # name -> (K, clar)


def molecule(name):
    """A hand-made molecule -> (atom_types, bonds) with its hydrogens listed (gaudi_amd.gor2goa.read_smiles)."""
    from gaudi_amd.gor2goa import read_smiles
    types, bonds, _, _ = read_smiles(SMILES[name], DATASET)
    return types.astype(np.int32), bonds.astype(np.int32).reshape(-1, 2)


def hand_made():
    return [molecule(k) for k in SMILES]


def ladder(n):
    """2 x n carbons, every one three-coordinate (the four corners carry an implied hydrogen): F(n+1) Kekule structures."""
    bonds = [(2 * k, 2 * k + 1) for k in range(n)]
    for k in range(n - 1):
        bonds += [(2 * k, 2 * k + 2), (2 * k + 1, 2 * k + 3)]
    return np.full(2 * n, C, np.int32), np.array(bonds, np.int32)


def polyene(n):
    """A chain of n carbons, hydrogens implied at the inner atoms and one listed at each end."""
    e = [C] * n + [H, H]
    b = [(k, k + 1) for k in range(n - 1)] + [(0, n), (n - 1, n + 1)]
    return np.array(e, np.int32), np.array(b, np.int32)


def tables():
    from gaudi_amd.gor2goa import c_valence_tables
    return c_valence_tables(DATASET)


def host(mols):
    return _lib.host_kekule(tables(), *pack(mols))


def device(engine, mols):
    return engine.kekule(tables(), *pack(mols))


class HostEngine:
    """What gaudi_amd.aromaticity asks of an engine, on the kernel's host build; counts the calls."""
    calls = 0

    def kekule(self, *args):
        type(self).calls += 1
        return _lib.host_kekule(*args)


def g32_host():
    """The host build's outputs for the whole of g32, computed once, never written to."""
    if "host" not in _CACHE:
        out = host(fixture()[1])
        for a in out.values():
            a.setflags(write=False)
        _CACHE["host"] = out
    return _CACHE["host"]


def g32_oracle():
    if "oracle" not in _CACHE:
        z, mols = fixture()
        _CACHE["oracle"] = [oracle(m["elem"], m["bonds"], z["table_n"], z["table_opt"]) for m in mols]
    return _CACHE["oracle"]


def assert_same_bits(got, want):
    for name in _lib.KEKULE_ARRAYS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert got[name].tobytes() == want[name].tobytes(), (name, np.argwhere(got[name] != want[name])[:5].tolist())


def row(out, i, m):
    """Molecule i of a call as a tuple that does not depend on the batch's padding."""
    r = int(out["n_hex"][i])
    assert not out["double_count"][i, m:].any() and not out["hex_atoms"][i, r:].any() and not out["sextet_count"][i, r:].any()
    return (int(out["status"][i]), int(out["k"][i]), out["double_count"][i, :m].tolist(), r, out["hex_atoms"][i, :r].tolist(),
            out["sextet_count"][i, :r].tolist(), int(out["fries"][i]), int(out["clar"][i]), int(out["n_nodes"][i]))


def _matchings(adj, order):
    """Every perfect matching of the graph as a frozenset of (lo, hi) pairs, and the size of the search tree of the rule: at a
    node the lowest unmatched vertex is matched with each of its unmatched neighbours in ascending order."""
    found, nodes = [], [0]

    def walk(free, edges):
        nodes[0] += 1
        if nodes[0] > BUDGET:
            raise OverflowError
        if not free:
            found.append(frozenset(edges))
            return
        v = min(free)
        for u in sorted(adj[v]):
            if u in free:
                walk(free - {v, u}, edges + [(v, u) if v < u else (u, v)])

    walk(frozenset(order), [])
    return found, nodes[0]


def _hexagons(heavy_adj, sel):
    """The chordless 6-cycles of the heavy-atom graph with all six atoms in sel, by walking every simple path of six atoms."""
    out = {}

    def walk(path):
        if len(path) == 6:
            if path[0] in heavy_adj[path[-1]]:
                inside = sum(1 for a, b in itertools.combinations(path, 2) if b in heavy_adj[a])
                if inside == 6 and all(a in sel for a in path):
                    out[tuple(sorted(path))] = None
            return
        for u in heavy_adj[path[-1]]:
            if u not in path:
                walk(path + [u])

    for a in heavy_adj:
        walk([a])
    rings = []
    for key in sorted(out):
        a = key[0]
        ring_nbrs = sorted(u for u in heavy_adj[a] if u in key)
        cyc, prev = [a, ring_nbrs[0]], a
        while len(cyc) < 6:
            nxt = [u for u in heavy_adj[cyc[-1]] if u in key and u != prev]
            prev = cyc[-1]
            cyc.append(nxt[0])
        rings.append(cyc)
    return rings


def oracle(elem, bonds, table_n, table_opt):
    """-> dict(status, k, double_count [m], hexagons [[6]], sextet_count, fries, clar, n_nodes, n_sel), from the fixture's own
    table.  The order of the statuses is the one DESIGN.md section 8o lists."""
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    n, m = len(elem), len(bonds)
    zero = dict(k=0, double_count=[0] * m, hexagons=[], sextet_count=[], fries=0, clar=0, n_nodes=0, n_sel=-1)
    if n == 0:
        return dict(zero, status=EMPTY)
    if n > 384 or m > 384:
        return dict(zero, status=OVERFLOW)
    if any(e < 0 or e >= table_n.shape[0] for e in elem) or any(i < 0 or i >= n or j < 0 or j >= n or i == j for i, j in bonds):
        return dict(zero, status=BAD_INPUT)
    if (elem != H).sum() > 192:
        return dict(zero, status=OVERFLOW)
    pairs = [(min(i, j), max(i, j)) for i, j in bonds.tolist()]
    if len(set(pairs)) != m:
        return dict(zero, status=BAD_INPUT)
    adj = {a: set() for a in range(n)}
    for i, j in pairs:
        adj[i].add(j)
        adj[j].add(i)
    sigma = [len(adj[a]) + (elem[a] == C and len(adj[a]) == 2) for a in range(n)]
    if any(d > 4 or table_n[e, d] == 0 for e, d in zip(elem, sigma)):
        return dict(zero, status=BAD_VALENCE)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(pairs)
    if not nx.is_connected(g):
        return dict(zero, status=NOT_CONNECTED)
    first = [table_opt[e, d, 0] for e, d in zip(elem, sigma)]
    if any(q != 0 for _, q in first):
        return dict(zero, status=NOT_NEUTRAL)
    sel = {a for a in range(n) if first[a][0] == 1}
    zero["n_sel"] = len(sel)
    sel_adj = {a: {u for u in adj[a] if u in sel} for a in sel}
    n_edges = sum(len(v) for v in sel_adj.values()) // 2
    if len(sel) > MAX_SEL or n_edges > MAX_EDGES or any(len(v) > 3 for v in sel_adj.values()):
        return dict(zero, status=OVERFLOW)
    heavy_adj = {a: {u for u in adj[a] if elem[u] != H} for a in range(n) if elem[a] != H}
    rings = _hexagons(heavy_adj, sel)
    if len(rings) > MAX_HEX:
        return dict(zero, status=OVERFLOW)
    if len(sel) % 2:
        return dict(zero, status=NO_KEKULE)
    try:
        structures, nodes = _matchings(sel_adj, sel)
    except OverflowError:
        return dict(zero, status=UNDECIDED)
    if not structures:
        return dict(zero, status=NO_KEKULE)
    ring_edges = [{(min(c[j], c[(j + 1) % 6]), max(c[j], c[(j + 1) % 6])) for j in range(6)} for c in rings]
    sextets = [[len(s & re) == 3 for re in ring_edges] for s in structures]
    # the Clar number by its definition: disjoint hexagons, most first, whose removal leaves a graph with a perfect matching
    clar = 0
    h = nx.Graph()
    h.add_nodes_from(sel)
    h.add_edges_from((a, u) for a in sel for u in sel_adj[a])
    disjoint = nx.Graph()
    disjoint.add_nodes_from(range(len(rings)))
    disjoint.add_edges_from((r, q) for r, q in itertools.combinations(range(len(rings)), 2) if not set(rings[r]) & set(rings[q]))
    cliques = sorted((c for c in nx.enumerate_all_cliques(disjoint)), key=len, reverse=True) if rings else []
    for chosen in cliques:
        rest = h.subgraph(sel - {a for r in chosen for a in rings[r]})
        if 2 * len(nx.max_weight_matching(rest, maxcardinality=True)) == rest.number_of_nodes():
            clar = len(chosen)
            break
    return dict(status=OK, k=len(structures), double_count=[sum(p in s for s in structures) for p in pairs], hexagons=rings,
                sextet_count=[sum(s[r] for s in sextets) for r in range(len(rings))], fries=max(sum(s) for s in sextets) if rings else 0,
                clar=clar, n_nodes=nodes, n_sel=len(sel))


def assert_equals_oracle(out, i, ref, m):
    """Molecule i of a call against the oracle's dict, every output."""
    got = row(out, i, m)
    want = (ref["status"], ref["k"], ref["double_count"], len(ref["hexagons"]), ref["hexagons"], ref["sextet_count"], ref["fries"],
            ref["clar"], ref["n_nodes"])
    assert got == want, (i, [k for k, (a, b) in enumerate(zip(got, want)) if a != b])
