"""Shared by test_substructure_cpu.py and test_gpu_substructure.py: the named patterns, a plain recursive matcher restated in
Python from the semantics, the networkx oracle, the host build as an engine stand-in, and the fixture's
results computed once."""
import numpy as np

from gaudi_amd import _lib
from tests.bond_order_helpers import C, H, fixture, pack
from tests.canonical_helpers import N_ELEMS

OK, GAVE_UP, BAD_INPUT, OVERFLOW, EMPTY, BAD_PATTERN = range(6)
H_EXACT, CLOSED = 1, 2
FLAG_SETTINGS = (0, H_EXACT, CLOSED, H_EXACT | CLOSED)
B_, N_, S_ = 2, 3, 5  # in ATOMS_LIST["hetro"]: H C B N O S
ARRAYS = ("count", "first", "covered", "steps", "status")
_CACHE = {}


def _ring(elems, extra=()):
    n = len(elems)
    return np.array(elems, np.int32), np.array([(k, (k + 1) % n) for k in range(n)] + list(extra), np.int32).reshape(-1, 2)


def path(n, elem=C):
    return np.full(n, elem, np.int32), np.array([(k, k + 1) for k in range(n - 1)], np.int32).reshape(-1, 2)


def ladder(n, elem=C):
    """n atoms in two rails with a rung between every pair: degree 3 inside."""
    b = [(k, k + 2) for k in range(n - 2)] + [(k, k + 1) for k in range(0, n - 1, 2)]
    return np.full(n, elem, np.int32), np.array(b, np.int32).reshape(-1, 2)


def grid(rows, cols, elem=C):
    """rows x cols atoms on a square grid: degree 4 inside, and far more self-avoiding walks than a ribbon of rings has."""
    b = [(r * cols + c, r * cols + c + 1) for r in range(rows) for c in range(cols - 1)]
    b += [(r * cols + c, (r + 1) * cols + c) for r in range(rows - 1) for c in range(cols)]
    return np.full(rows * cols, elem, np.int32), np.array(b, np.int32).reshape(-1, 2)


def undecided_pattern():
    """A 32-path of 16 carbons, then 16 sulfurs.  Neither element is rarer, so the match order starts at the carbon end; on an
    all-carbon target every root walks its 16-carbon paths and finds no sulfur behind any of them."""
    return np.array([C] * 16 + [S_] * 16, np.int32), path(32)[1]


NAMED = {
    "C": (np.array([C], np.int32), np.zeros((0, 2), np.int32)),
    "CS": (np.array([C, S_], np.int32), np.array([(0, 1)], np.int32)),
    "benzene": _ring([C] * 6),
    "thiophene": _ring([C, C, C, C, S_]),
    "pyridine": _ring([C, C, C, C, C, N_]),
    "naphthalene": _ring([C] * 10, [(0, 5)]),
    "path8": path(8),
    "BN6": _ring([B_, N_, C, C, C, C]),
}
NAMES = tuple(NAMED)


def named_patterns():
    return [NAMED[k] for k in NAMES]


def graph_of(elem, bonds):
    """The graph of the definition -> (heavy atoms ascending, {atom: (element, H count, heavy degree)}, {atom: set of heavy
    neighbours})."""
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    heavy = [a for a in range(len(elem)) if elem[a] != H]
    nbrs = {a: set() for a in heavy}
    n_h = {a: 0 for a in heavy}
    n_b = {a: 0 for a in heavy}
    for i, j in bonds:
        i, j = int(i), int(j)
        for a, o in ((i, j), (j, i)):
            if elem[a] == H:
                continue
            n_b[a] += 1
            if elem[o] == H:
                n_h[a] += 1
            else:
                nbrs[a].add(o)
    attr = {a: (int(elem[a]), n_h[a] + (1 if elem[a] == C and n_b[a] == 2 else 0), len(nbrs[a])) for a in heavy}
    return heavy, attr, nbrs


def _node_ok(pa, ta, flags):
    return pa[0] == ta[0] and (not flags & H_EXACT or pa[1] == ta[1]) and (not flags & CLOSED or pa[2] == ta[2])


def restated(mol, pat, flags=0, limit=None):
    """Every embedding by plain recursion in the pattern's own atom order (no match order, no parents): pattern atom k goes to
    every unused molecule atom that fits and is bonded to the images of k's earlier neighbours.  -> dict(count, first [n_atoms of
    the pattern] or all -1, covered set of atoms, images = the distinct edge-set images).  limit: stop after that many."""
    th, ta, tn = graph_of(*mol)
    ph, pa, pn = graph_of(*pat)
    out = dict(count=0, first=None, covered=set(), images=set())
    pedges = [(a, b) for a in ph for b in pn[a] if a < b]
    m = {}

    def rec(k):
        if limit is not None and out["count"] >= limit:
            return
        if k == len(ph):
            out["count"] += 1
            emb = [m[a] for a in ph]
            if out["first"] is None or emb < out["first"]:
                out["first"] = emb
            out["covered"].update(emb)
            out["images"].add(frozenset(frozenset((m[a], m[b])) for a, b in pedges) if pedges else frozenset(emb))
            return
        a = ph[k]
        earlier = [m[o] for o in pn[a] if o in m]
        cands = sorted(tn[earlier[0]]) if earlier else th
        for t in cands:
            if t in m.values() or not _node_ok(pa[a], ta[t], flags) or any(t not in tn[e] for e in earlier):
                continue
            m[a] = t
            rec(k + 1)
            del m[a]

    rec(0)
    first = np.full(len(pat[0]), -1, np.int64)
    if out["first"] is not None:
        first[ph] = out["first"]
    out["first"] = first
    return out


def networkx_oracle(mol, pat, flags=0):
    """GraphMatcher(target, pattern).subgraph_monomorphisms_iter with element, H count and heavy degree as node attributes ->
    dict(count, first, covered, n_unique = the number of distinct image edge sets)."""
    import networkx as nx
    from networkx.algorithms.isomorphism import GraphMatcher
    graphs = []
    for elem, bonds in (mol, pat):
        heavy, attr, nbrs = graph_of(elem, bonds)
        g = nx.Graph()
        for a in heavy:
            g.add_node(a, attr=attr[a])
        g.add_edges_from((a, b) for a in heavy for b in nbrs[a] if a < b)
        graphs.append(g)
    target, pattern = graphs
    ph = sorted(pattern.nodes())
    gm = GraphMatcher(target, pattern, node_match=lambda t, p: _node_ok(p["attr"], t["attr"], flags))
    count, best, covered, images = 0, None, set(), set()
    for mapping in gm.subgraph_monomorphisms_iter():  # target node -> pattern node
        inv = {p: t for t, p in mapping.items()}
        emb = [inv[a] for a in ph]
        count += 1
        if best is None or emb < best:
            best = emb
        covered.update(emb)
        images.add(frozenset(frozenset((inv[a], inv[b])) for a, b in pattern.edges()) if pattern.number_of_edges() else frozenset(emb))
    first = np.full(len(pat[0]), -1, np.int64)
    if best is not None:
        first[ph] = best
    return dict(count=count, first=first, covered=covered, n_unique=len(images))


def pack_patterns(patterns, flags):
    pe, pna, pb, pnb = pack(patterns)
    fl = np.full(len(patterns), flags, np.int32) if np.isscalar(flags) else np.asarray(flags, np.int32)
    return pe, pna, pb, pnb, np.ascontiguousarray(fl)


def host_search(mols, patterns, flags=0):
    """Fixture molecules or (elem, bonds) pairs against pairs -> the raw outputs of the host build, in the fixture's element list."""
    return _lib.host_substructure_search(N_ELEMS, H, C, *pack(mols), *pack_patterns(patterns, flags))


def device_search(engine, mols, patterns, flags=0):
    return engine.substructure_search(N_ELEMS, H, C, *pack(mols), *pack_patterns(patterns, flags))


class HostEngine:
    """What gaudi_amd.substructure asks of an engine, on the kernel's host build."""

    def substructure_search(self, *args):
        return _lib.host_substructure_search(*args)


def g32_host(flags):
    """The host build's outputs for the whole of g32 against the named patterns, computed once per flag setting, never written to."""
    key = ("g32", flags)
    if key not in _CACHE:
        out = host_search(fixture()[1], named_patterns(), flags)
        for a in out.values():
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def symmetry(patterns, flags=0):
    """count of every pattern against itself -> int64 [P]."""
    return np.diagonal(host_search(patterns, patterns, flags)["count"]).astype(np.int64)


def check_embedding(mol, pat, first, flags=0):
    """first is an embedding: injective, elements (and what the flags ask) equal, every pattern bond on a molecule bond, -1 exactly
    at the pattern's hydrogens and padding."""
    th, ta, tn = graph_of(*mol)
    ph, pa, pn = graph_of(*pat)
    first = np.asarray(first)
    assert (first[[a for a in range(len(first)) if a not in ph]] == -1).all()
    img = {a: int(first[a]) for a in ph}
    assert len(set(img.values())) == len(ph) and all(t in ta for t in img.values())
    for a in ph:
        assert _node_ok(pa[a], ta[img[a]], flags)
        assert all(img[o] in tn[img[a]] for o in pn[a])


def largest_carbon_molecule():
    """The all-carbon (and hydrogen) fixture molecule with the most heavy atoms among those the kernels accept."""
    best, size = None, -1
    for m in fixture()[1]:
        heavy = int((m["elem"] != H).sum())
        if heavy <= 192 and np.isin(m["elem"], (H, C)).all() and heavy > size:
            best, size = m, heavy
    return best
