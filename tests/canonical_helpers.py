"""Shared by test_canonical_cpu.py and test_gpu_canonical.py: the host twin of gaudi_canonical_order as an engine stand-in,
graphs rebuilt from inputs and from codes, the symmetric test graphs, hydrogen stripping, and a parser for exactly the SMILES
grammar gaudi_amd.gor2goa.smiles writes."""
import re

import networkx as nx
import numpy as np

from gaudi_amd import _lib
from tests.bond_order_helpers import DATASET, C, H, pack

OK, GAVE_UP, BAD_INPUT, OVERFLOW, EMPTY = range(5)
ARRAYS = ("status", "nodes", "n_heavy", "n_hbonds", "rank", "label", "cbonds")
N_ELEMS = 6  # len(ATOMS_LIST["hetro"])


def host_canon(mols):
    """Fixture molecules or (elem, bonds) pairs -> the raw outputs of the host twin, in the fixture's element list."""
    return _lib.host_canonical_order(N_ELEMS, H, C, *pack(mols))


class HostEngine:
    """What gaudi_amd.gor2goa asks of an engine for canonical numbering and bond orders, on the kernels' host builds."""

    def canonical_order(self, n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds):
        return _lib.host_canonical_order(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds)

    def bond_orders(self, tables, elem, n_atoms, bonds, n_bonds):
        return _lib.host_bond_orders(tables, elem, n_atoms, bonds, n_bonds)


def input_graph(elem, bonds):
    """The labelled graph of the definition, straight from a molecule's arrays: heavy atoms (by atom index) with
    label = (element, H count), heavy-heavy bonds."""
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    deg = np.bincount(bonds.reshape(-1), minlength=len(elem))
    g = nx.Graph()
    for a, e in enumerate(elem):
        if e != H:
            g.add_node(a, label=(int(e), int(e == C and deg[a] == 2)))
    for i, j in bonds:
        i, j = int(i), int(j)
        if elem[i] != H and elem[j] != H:
            g.add_edge(i, j)
        elif elem[i] != H or elem[j] != H:
            a = i if elem[i] != H else j
            e, n = g.nodes[a]["label"]
            g.nodes[a]["label"] = (e, n + 1)
    return g


def code_graph(raw, i):
    """The graph a molecule's outputs describe: ranks as nodes."""
    nh, ne = int(raw["n_heavy"][i]), int(raw["n_hbonds"][i])
    g = nx.Graph()
    for r in range(nh):
        g.add_node(r, label=(int(raw["label"][i, r]) >> 3, int(raw["label"][i, r]) & 7))
    g.add_edges_from((int(a), int(b)) for a, b in raw["cbonds"][i, :ne])
    return g


def same_labelled_graph(g1, g2):
    return nx.is_isomorphic(g1, g2, node_match=lambda a, b: a["label"] == b["label"])


def carbon_molecule(g):
    """A networkx graph as an all-carbon molecule (no hydrogens listed) -> (elem, bonds)."""
    nodes = sorted(g.nodes())
    at = {v: k for k, v in enumerate(nodes)}
    return np.full(len(nodes), C, np.int32), np.array([(at[a], at[b]) for a, b in g.edges()], np.int32).reshape(-1, 2)


def renumber(elem, bonds, rng):
    """As bond_order_helpers.relabel, for a pair."""
    n = len(elem)
    perm = rng.permutation(n)
    e = np.zeros(n, np.int32)
    e[perm] = elem
    b = perm[np.asarray(bonds).reshape(-1, 2)].astype(np.int32).reshape(-1, 2)
    b = b[rng.permutation(len(b))]
    flip = rng.random(len(b)) < 0.5
    b[flip] = b[flip][:, ::-1]
    return e, b


def symmetric_graphs():
    """[(name, graph)]: the named vertex-transitive graphs and 72 random cubic graphs of 8..30 vertices."""
    out = [("petersen", nx.petersen_graph()), ("heawood", nx.heawood_graph()), ("cube", nx.hypercube_graph(3)),
           ("dodecahedron", nx.dodecahedral_graph()), ("k33", nx.complete_bipartite_graph(3, 3))]
    for n in range(8, 31, 2):
        for seed in range(6):
            out.append((f"cubic{n}_{seed}", nx.random_regular_graph(3, n, seed=1000 * n + seed)))
    return [(name, nx.convert_node_labels_to_integers(g)) for name, g in out]


def benzenes(k):
    """k disjoint six-rings of carbons with two bonds each -> (elem, bonds)."""
    bonds = [(6 * r + a, 6 * r + (a + 1) % 6) for r in range(k) for a in range(6)]
    return np.full(6 * k, C, np.int32), np.array(bonds, np.int32)


def strip_implied_hydrogens(elem, bonds):
    """The molecule without the H of every carbon that has exactly three bonds, one of them to an H: what gor2goa emits with
    place_hydrogens=False for a molecule it emits with the H's when asked to place them.  -> (elem, bonds, removed)."""
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    deg = np.bincount(bonds.reshape(-1), minlength=len(elem))
    nh = np.zeros(len(elem), np.int64)
    for i, j in bonds:
        nh[i] += elem[j] == H
        nh[j] += elem[i] == H
    drop = set()
    for i, j in bonds:
        for a, h in ((i, j), (j, i)):
            if elem[h] == H and elem[a] == C and deg[a] == 3 and nh[a] == 1 and deg[h] == 1:
                drop.add(int(h))
    keep = np.array([a for a in range(len(elem)) if a not in drop], np.int64)
    new = np.full(len(elem), -1, np.int64)
    new[keep] = np.arange(len(keep))
    kb = np.array([(new[i], new[j]) for i, j in bonds if i not in drop and j not in drop], np.int32).reshape(-1, 2)
    return elem[keep].astype(np.int32), kb, len(drop)


VALENCES = {"B": (3,), "C": (4,), "N": (3, 5), "O": (2,), "S": (2, 4, 6)}
_BRACKET = re.compile(r"\[([A-Z][a-z]?)(H\d*)?([+-]\d*)?\]")


def parse_smiles(text):
    """The grammar of gaudi_amd.gor2goa.smiles and nothing else -> a networkx graph: nodes with sym, n_h, charge; edges with
    order.  Anything outside the grammar raises."""
    g = nx.Graph()
    prev, pending, stack, ring, bare = -1, 1, [], {}, []
    i = 0

    def atom(sym, n_h, charge):
        nonlocal prev, pending
        a = g.number_of_nodes()
        g.add_node(a, sym=sym, n_h=n_h, charge=charge)
        if prev >= 0:
            g.add_edge(prev, a, order=pending)
        else:
            assert pending == 1
        prev, pending = a, 1

    def closure(k):
        nonlocal pending
        assert prev >= 0
        if k in ring:
            j = ring.pop(k)
            assert j != prev and not g.has_edge(j, prev)
            g.add_edge(j, prev, order=pending)
        else:
            assert pending == 1, "the '=' of a ring bond stands before the closing digit"
            ring[k] = prev
        pending = 1

    while i < len(text):
        ch = text[i]
        if ch == ".":
            assert not stack and pending == 1
            prev = -1
        elif ch == "(":
            stack.append(prev)
        elif ch == ")":
            prev = stack.pop()
        elif ch == "=":
            assert pending == 1
            pending = 2
        elif ch.isdigit():
            closure(int(ch))
        elif ch == "%":
            assert text[i + 1:i + 3].isdigit() and int(text[i + 1:i + 3]) >= 10
            closure(int(text[i + 1:i + 3]))
            i += 2
        elif ch == "[":
            m = _BRACKET.match(text, i)
            assert m, text[i:i + 8]
            n_h = 0 if not m.group(2) else int(m.group(2)[1:] or 1)
            q = 0 if not m.group(3) else int(m.group(3)[1:] or 1) * (1 if m.group(3)[0] == "+" else -1)
            atom(m.group(1), n_h, q)
            i = m.end() - 1
        else:
            assert ch in VALENCES, ch
            atom(ch, None, 0)
            bare.append(prev)
        i += 1
    assert not ring and not stack and pending == 1
    for a in bare:
        total = sum(d["order"] for _, _, d in g.edges(a, data=True))
        fit = [v for v in VALENCES[g.nodes[a]["sym"]] if v >= total]
        g.nodes[a]["n_h"] = fit[0] - total if fit else 0
    return g


def structure_graph(names, types, bonds, orders, charges):
    """The canonical molecule with its structure as parse_smiles would see it: heavy atoms with sym, n_h, charge; heavy bonds
    with their order."""
    g = nx.Graph()
    heavy = [a for a, t in enumerate(types) if names[int(t)] != "H"]
    for a in heavy:
        g.add_node(a, sym=names[int(types[a])], n_h=0, charge=int(charges[a]))
    for (i, j), o in zip(bonds, orders):
        i, j = int(i), int(j)
        if i in g and j in g:
            g.add_edge(i, j, order=int(o))
        else:
            assert o == 1
            g.nodes[i if i in g else j]["n_h"] += 1
    return g


def same_structure(g1, g2):
    return nx.is_isomorphic(g1, g2, node_match=lambda a, b: (a["sym"], a["n_h"], a["charge"]) == (b["sym"], b["n_h"], b["charge"]),
                            edge_match=lambda a, b: a["order"] == b["order"])
