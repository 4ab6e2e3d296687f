"""Substructure search (csrc/sub.inc) on the kernel's HOST build, no GPU: against a recursive matcher restated
from the semantics and against networkx's subgraph monomorphisms on golden g32, the budget condition, symmetry and n_unique,
renumbering, the edge shapes, every refusal, giving up, read_smiles, and the layers on top.  tests/test_gpu_substructure.py then
asks the device for bit-for-bit equality with this build."""
import os
import re

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import C, DATASET, H, fixture, pack, relabel
from tests.canonical_helpers import N_ELEMS, carbon_molecule, renumber, symmetric_graphs
from tests.similarity_helpers import stars
from tests.substructure_helpers import (B_, BAD_INPUT, BAD_PATTERN, CLOSED, EMPTY, FLAG_SETTINGS, GAVE_UP, H_EXACT, N_, NAMED, NAMES, OK,
                                        OVERFLOW, S_, HostEngine, check_embedding, g32_host, graph_of, host_search, ladder,
                                        largest_carbon_molecule, named_patterns, grid, undecided_pattern, networkx_oracle, pack_patterns, path, restated,
                                        symmetry)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSED = {5: BAD_INPUT, 6: OVERFLOW, 7: EMPTY}  # the fixture's specials


@pytest.fixture(scope="module")
def g32():
    return fixture()


def covered_set(raw, b, p):
    return set(np.nonzero(raw["covered"][b, p])[0].tolist())


@pytest.mark.parametrize("flags", FLAG_SETTINGS)
def test_every_fourth_molecule_against_the_matcher_and_networkx(g32, flags):
    raw, sym = g32_host(flags), symmetry(named_patterns(), flags)
    have_nx = True
    try:
        import networkx  # noqa: F401
    except ImportError:
        have_nx = False
    hits = 0
    for m in g32[1][::4]:
        i = m["index"]
        if m["special"] in REFUSED:
            assert (raw["status"][i] == REFUSED[m["special"]]).all()
            continue
        assert (raw["status"][i] == OK).all(), i
        for p, name in enumerate(NAMES):
            pat = NAMED[name]
            ref = restated((m["elem"], m["bonds"]), pat, flags)
            got = (int(raw["count"][i, p]), raw["first"][i, p, :len(pat[0])].tolist(), covered_set(raw, i, p))
            assert got == (ref["count"], ref["first"].tolist(), ref["covered"]), (i, name)
            assert (raw["first"][i, p, len(pat[0]):] == -1).all()
            assert raw["count"][i, p] // sym[p] == len(ref["images"]), (i, name)
            if have_nx:
                ox = networkx_oracle((m["elem"], m["bonds"]), pat, flags)
                assert got == (ox["count"], ox["first"].tolist(), ox["covered"]), (i, name)
                assert raw["count"][i, p] // sym[p] == ox["n_unique"], (i, name)
            hits += ref["count"] > 0
    assert hits >= (300 if flags == 0 else 5)
    if not have_nx:
        pytest.importorskip("networkx")  # (the restated matcher was compared above; only the second oracle is missing)


def test_the_budget_condition_on_the_whole_fixture(g32):
    """Every (molecule, named pattern, flag setting) ends OK or with the molecule's refusal, and the largest per-root step count is
    at most a sixteenth of the cap: the measurement GAUDI_SUB_MAX_STEPS is sized with."""
    _lib.host_substructure_root_steps(True)
    for flags in FLAG_SETTINGS:
        raw = host_search(g32[1], named_patterns(), flags)
        for m in g32[1]:
            assert (raw["status"][m["index"]] == REFUSED.get(m["special"], OK)).all(), (m["index"], flags)
        assert (raw["count"] % symmetry(named_patterns(), flags)[None, :] == 0).all()
        ok = raw["status"] == OK
        assert not raw["count"][~ok].any() and not raw["covered"][~ok].any() and not raw["steps"][~ok].any() and (raw["first"][~ok] == -1).all()
    worst = _lib.host_substructure_root_steps(True)
    print("largest per-root step count:", worst)
    assert 0 < worst * 16 <= _lib.SUB_MAX_STEPS and _lib.SUB_MAX_STEPS & (_lib.SUB_MAX_STEPS - 1) == 0
    raw = g32_host(0)
    assert (raw["count"] > 0).sum(0).tolist()[2:7] == [372, 92, 135, 169, 366]  # benzene thiophene pyridine naphthalene path8
    assert raw["count"].max(0).tolist()[2:7] == [564, 4, 6, 184, 4512]
    assert sum(m["special"] not in REFUSED for m in g32[1]) == 504


def test_a_molecule_against_itself_and_known_group_orders(g32):
    small = [m for m in g32[1] if m["special"] not in REFUSED and int((m["elem"] != H).sum()) <= 32][:40]
    assert len(small) >= 20
    pairs = [(m["elem"], m["bonds"]) for m in small]
    both = H_EXACT | CLOSED
    raw = host_search(pairs, pairs, both)
    for i, m in enumerate(small):
        if raw["status"][i, i] == BAD_PATTERN:  # (a fixture molecule in several pieces is no pattern)
            continue
        assert raw["status"][i, i] == OK and raw["count"][i, i] >= 1
        heavy = graph_of(*pairs[i])[0]
        assert raw["first"][i, i, heavy].tolist() == heavy  # the identity is the smallest automorphism
        assert covered_set(raw, i, i) == set(heavy)
    assert (np.diagonal(raw["status"]) == OK).sum() >= 20
    import networkx as nx
    known = {"petersen": 120, "heawood": 336, "cube": 48, "dodecahedron": 120, "k33": 72}
    graphs = [(n, g) for n, g in symmetric_graphs() if g.number_of_nodes() <= 32]
    mols = [carbon_molecule(g) for _, g in graphs]
    for flags in (0, both):
        sym = np.concatenate([symmetry(mols[k:k + 64], flags) for k in range(0, len(mols), 64)])
        for (name, g), s in zip(graphs, sym):
            if name in known:
                assert s == known[name], name
            elif g.number_of_nodes() <= 16:
                assert s == sum(1 for _ in nx.algorithms.isomorphism.GraphMatcher(g, g).isomorphisms_iter()), name
    assert set(known) <= {n for n, _ in graphs}


def test_renumbering_changes_nothing_but_first(g32):
    rng = np.random.default_rng(8101)
    mols = [m for m in g32[1] if m["special"] not in REFUSED][5::12]
    twins = [relabel(m, rng) for m in mols]
    pats = named_patterns()
    for flags in (0, H_EXACT | CLOSED):
        a, b = host_search(mols, pats, flags), host_search(twins, pats, flags)
        assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["status"], b["status"]) and (a["status"] == OK).all()
        assert np.array_equal(a["covered"].sum(-1), b["covered"].sum(-1))
        for i in range(0, len(mols), 5):
            for p, name in enumerate(NAMES):
                first = b["first"][i, p, :len(NAMED[name][0])]
                if b["count"][i, p] == 0:
                    assert (first == -1).all()
                    continue
                check_embedding(twins[i], NAMED[name], first, flags)
                assert first.tolist() == restated(twins[i], NAMED[name], flags)["first"].tolist()
    # the pattern renumbered: count and covered stay
    ren = [renumber(e, b, rng) for e, b in pats]
    a, b = host_search(mols, pats, 0), host_search(mols, ren, 0)
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["covered"], b["covered"])


def chain_targets():
    out = [path(n) for n in (1, 63, 64, 65)] + [ladder(n) for n in (128, 129, 192)]
    return out


def test_edge_shapes(g32):
    targets = chain_targets()
    pats = [NAMED["C"], path(2), path(8), ladder(6), path(3, N_)]
    raw = host_search(targets, pats, 0)
    assert (raw["status"] == OK).all()
    sizes = [1, 63, 64, 65, 128, 129, 192]
    assert raw["count"][:, 0].tolist() == sizes  # one vertex: the atoms of that element
    assert raw["count"][:4, 1].tolist() == [0, 124, 126, 128] and raw["count"][:4, 2].tolist() == [0, 112, 114, 116]
    assert not raw["count"][:, 4].any() and (raw["first"][:, 4] == -1).all() and not raw["covered"][:, 4].any()
    for t, tgt in enumerate(targets):
        for p, pat in enumerate(pats):
            ref = restated(tgt, pat, 0)
            assert raw["count"][t, p] == ref["count"] and covered_set(raw, t, p) == ref["covered"], (t, p)
            assert raw["first"][t, p, :len(pat[0])].tolist() == ref["first"].tolist(), (t, p)
    # every root finds its embeddings: a one-vertex pattern covers every atom, whichever lane owns it
    for t, n in enumerate(sizes):
        assert covered_set(raw, t, 0) == set(range(n))
    # a pattern larger than the molecule; a pattern equal to the molecule
    raw = host_search([path(5), ladder(6)], [path(6), ladder(6)], H_EXACT | CLOSED)
    assert raw["count"].tolist() == [[0, 0], [0, 4]] and (raw["status"] == OK).all()
    assert raw["first"][1, 1].tolist() == [0, 1, 2, 3, 4, 5]
    # degree 8: 38 stars of an N with 4 B leaves, and one C with 8 S leaves
    big = (np.array([C] + [S_] * 8, np.int32), np.array([(0, k) for k in range(1, 9)], np.int32))
    star3 = (np.array([N_, B_, B_, B_], np.int32), np.array([(0, 1), (0, 2), (0, 3)], np.int32))
    star8 = (np.array([C] + [S_] * 4, np.int32), np.array([(0, 1), (0, 2), (0, 3), (0, 4)], np.int32))
    raw = host_search([stars(), big], [star3, star8, big], 0)
    assert raw["count"][:, :2].tolist() == [[38 * 24, 0], [0, 8 * 7 * 6 * 5]] and (raw["status"][:, :2] == OK).all()
    assert raw["covered"][0, 0, :190].all() and raw["covered"][1, 1, :9].all() and raw["first"][1, 1, :5].tolist() == [0, 1, 2, 3, 4]
    # all 8! orders of the eight leaves are beyond one root's budget: a lower bound, and the smallest embedding is the first found
    assert raw["status"][:, 2].tolist() == [OK, GAVE_UP] and raw["count"][0, 2] == 0 and 0 < raw["count"][1, 2] < 40320
    assert raw["first"][1, 2].tolist() == list(range(9))
    assert host_search([stars()], [star3], CLOSED)["count"][0, 0] == 0


def test_listed_hydrogens_in_a_pattern():
    # pattern: C(H)(H) bonded to N; the hydrogens count only under H_EXACT, and first has -1 at them
    pat = (np.array([H, C, H, N_], np.int32), np.array([(0, 1), (1, 2), (1, 3)], np.int32))
    mol_a = (np.array([C, N_, H, H], np.int32), np.array([(0, 1), (0, 2), (0, 3)], np.int32))  # CH2-N
    mol_b = (np.array([C, N_, H], np.int32), np.array([(0, 1), (0, 2)], np.int32))  # a carbon with two bonds: 1 listed + 1 implied
    mol_c = (np.array([C, N_, C, C, H], np.int32), np.array([(0, 1), (0, 2), (0, 3), (1, 4)], np.int32))  # C without H, N with one
    for flags, want in ((0, [1, 1, 1]), (H_EXACT, [1, 1, 0])):
        raw = host_search([mol_a, mol_b, mol_c], [pat], flags)
        assert raw["count"][:, 0].tolist() == want and (raw["status"] == OK).all()
        assert raw["first"][0, 0].tolist() == [-1, 0, -1, 1]


def test_pattern_counts_and_the_python_chunking(g32):
    from gaudi_amd.substructure import search
    mols = [m for m in g32[1] if m["special"] not in REFUSED][::50]
    pairs = [(m["elem"], m["bonds"]) for m in mols]
    base = named_patterns()
    many = [base[k % len(base)] for k in range(65)]
    one = host_search(mols, many[:1], 0)
    full = host_search(mols, many[:64], 0)
    assert one["count"].shape == (len(mols), 1) and np.array_equal(one["count"][:, 0], full["count"][:, 0])
    with pytest.raises(_lib.GaudiError):
        host_search(mols, many, 0)  # 65 patterns in one call: GAUDI_E_CAPACITY
    out = search(pairs, many, DATASET, engine=HostEngine())
    assert out["count"].shape == (len(mols), 65) and out["covered"].shape[:2] == (len(mols), 65)
    assert np.array_equal(out["count"][:, :64], full["count"]) and np.array_equal(out["count"][:, 64], full["count"][:, 0])
    assert np.array_equal(out["covered"][:, :64], full["covered"]) and np.array_equal(out["covered"][:, 64], full["covered"][:, 0])
    assert np.array_equal(out["symmetry"], symmetry(many[:8], 0)[np.arange(65) % 8])
    assert np.array_equal(out["n_unique"], out["count"] // out["symmetry"][None, :]) and np.array_equal(out["hit"], out["count"] > 0)
    assert not out["undecided"].any() and len(out["first"]) == len(mols) and len(out["first"][0]) == 65
    assert out["first"][0][64].tolist() == full["first"][0, 0, :1].tolist()


def bad_patterns():
    return {
        "empty": (np.zeros(0, np.int32), np.zeros((0, 2), np.int32)),
        "only hydrogens": (np.array([H, H], np.int32), np.array([(0, 1)], np.int32)),
        "disconnected": (np.array([C, C, C], np.int32), np.array([(0, 1)], np.int32)),
        "33 vertices": path(33),
        "bad index": (np.array([C, C], np.int32), np.array([(0, 2)], np.int32)),
        "negative index": (np.array([C, C], np.int32), np.array([(0, -1)], np.int32)),
        "self bond": (np.array([C, C], np.int32), np.array([(0, 1), (1, 1)], np.int32)),
        "duplicate bond": (np.array([C, C], np.int32), np.array([(0, 1), (1, 0)], np.int32)),
        "bad element": (np.array([C, N_ELEMS], np.int32), np.array([(0, 1)], np.int32)),
    }


def test_every_refusal_leaves_the_other_cells_alone(g32):
    normal = [m for m in g32[1] if m["special"] not in REFUSED][:6]
    special = [next(m for m in g32[1] if m["special"] == k) for k in (5, 6, 7)]
    assert int((special[1]["elem"] != H).sum()) == 194
    good = named_patterns()
    ref = host_search(normal, good, 0)
    bad = bad_patterns()
    mols = normal[:2] + [special[0]] + normal[2:4] + [special[1], special[2]] + normal[4:]
    keep_m = [0, 1, 3, 4, 7, 8]
    pats = good[:3] + list(bad.values())[:5] + good[3:] + list(bad.values())[5:]
    keep_p = [0, 1, 2] + list(range(8, 13))
    bad_p = [3, 4, 5, 6, 7] + list(range(13, 17))
    raw = host_search(mols, pats, 0)
    for k in ("count", "first", "steps", "status"):
        got = raw[k][np.ix_(keep_m, keep_p)]
        assert np.array_equal(got if k != "first" else got[..., :ref["first"].shape[2]], ref[k]), k
    width = ref["covered"].shape[2]
    assert np.array_equal(raw["covered"][np.ix_(keep_m, keep_p)][..., :width], ref["covered"])
    assert (raw["status"][:, bad_p] == BAD_PATTERN).all()  # the whole column, refused molecules included
    for row, code in ((2, BAD_INPUT), (5, OVERFLOW), (6, EMPTY)):
        assert (raw["status"][row, keep_p] == code).all()
    refused = raw["status"] > GAVE_UP
    assert refused.sum() == len(mols) * len(bad_p) + 3 * len(keep_p)
    assert not raw["count"][refused].any() and not raw["steps"][refused].any() and not raw["covered"][refused].any()
    assert (raw["first"][refused] == -1).all()
    # an unknown flag refuses its pattern only; n_atoms beyond the arrays' width is the pattern's fault, not the call's
    pe, pna, pb, pnb, fl = pack_patterns(good[:3], np.array([0, 4, 3], np.int32))
    pna = pna.copy()
    pna[0] = pe.shape[1] + 1
    out = _lib.host_substructure_search(N_ELEMS, H, C, *pack(normal), pe, pna, pb, pnb, fl)
    assert (out["status"][:, :2] == BAD_PATTERN).all() and (out["status"][:, 2] == OK).all()


def test_giving_up(g32):
    from gaudi_amd.substructure import search
    big = largest_carbon_molecule()
    assert int((big["elem"] != H).sum()) >= 100
    mol, pat = (big["elem"], big["bonds"]), path(32)
    raw = host_search([mol], [pat, NAMED["benzene"]], 0)
    assert raw["status"][0].tolist() == [GAVE_UP, OK]
    assert raw["count"][0, 0] > 0 and raw["steps"][0, 0] > _lib.SUB_MAX_STEPS
    check_embedding(mol, pat, raw["first"][0, 0, :32], 0)  # (the restated matcher cannot finish a 32-path in test time)
    cov = covered_set(raw, 0, 0)
    assert set(raw["first"][0, 0, :32].tolist()) <= cov <= set(graph_of(*mol)[0])
    again = host_search([mol, mol], [pat], 0)
    assert all(np.array_equal(again[k][0], again[k][1]) and np.array_equal(again[k][0], raw[k][0, :1]) for k in raw)
    out = search([mol], [pat], DATASET, engine=HostEngine())
    assert out["hit"][0, 0] and not out["undecided"][0, 0] and out["status"][0, 0] == GAVE_UP and out["symmetry"][0] == 2
    # undecided: a search cut before its first embedding.  16 carbons, then 16 sulfurs: neither element is rarer, so the match
    # order starts at the carbon end, and every root walks the 16-carbon paths of a 3 x 64 grid to find no sulfur behind any
    out = search([grid(3, 64)], [undecided_pattern()], DATASET, engine=HostEngine())
    assert out["status"][0, 0] == GAVE_UP and out["count"][0, 0] == 0 and out["undecided"][0, 0] and not out["hit"][0, 0]
    assert not out["covered"][0, 0].any() and (out["first"][0][0] == -1).all()


@pytest.fixture(scope="module")
def records(g32):
    """As tests/test_canonical_cpu.py forms them: every fixture molecule with a numbering as rings_to_atoms(canonical=True,
    bond_orders=True) would hand it on, through the canonical and the bond-order kernels' host builds."""
    from gaudi_amd.gor2goa import _bond_orders, _canonical_raw, _molecule_from_code
    from tests.canonical_helpers import HostEngine as CanonHost
    from tests.canonical_helpers import host_canon
    host = host_canon(g32[1])
    mols = [m for m in g32[1] if host["status"][m["index"]] == 0]
    batch = [(m["elem"], m["bonds"]) for m in mols]
    extras, codes = _canonical_raw(batch, DATASET, CanonHost())
    structs = _bond_orders([_molecule_from_code(c, DATASET) for c in codes], DATASET, engine=CanonHost())
    return [dict(status=0, atom_types=e, bonds=b, **x, **{"canon_" + k: v for k, v in s.items()}) for (e, b), x, s in zip(batch, extras, structs)]


def test_read_smiles_inverts_smiles(records):
    from gaudi_amd.gor2goa import _canonical_raw, atoms_list, read_smiles, smiles
    from tests.canonical_helpers import HostEngine as CanonHost
    from tests.canonical_helpers import parse_smiles, same_structure, structure_graph
    names = atoms_list(DATASET)
    texts = [(r, smiles(r, DATASET)) for r in records]
    texts = [(r, t) for r, t in texts if t is not None]
    assert len(texts) >= 300
    parsed = [read_smiles(t, DATASET) for _, t in texts]
    _, codes = _canonical_raw([(p[0], p[1]) for p in parsed], DATASET, CanonHost())
    for (r, t), p, code in zip(texts, parsed, codes):
        assert code == r["canon_key"], t
    for (r, t), p in zip(texts, parsed):
        assert same_structure(parse_smiles(t), structure_graph(names, *p)), t


@pytest.mark.parametrize("text,what", [("c1ccccc1", "lower-case"), ("C[C@H](N)C", "bracket"), ("C/C=C/C", "stereo"), ("C#N", "unsupported"),
                                       ("C1CC", "never closed"), ("CC(", "open branch"), ("C=", "trailing"), ("[13C]", "bracket"),
                                       ("C%1C", "two digits"), ("CCl", "lower-case"), ("[Si]", "outside"), ("C==C", "misplaced"),
                                       ("C11", "repeats"), ("=C", "misplaced"), ("C-C", "unsupported"), ("C:C", "unsupported")])
def test_read_smiles_refuses(text, what):
    from gaudi_amd.gor2goa import read_smiles
    with pytest.raises(_lib.GaudiError, match="position"):
        read_smiles(text, DATASET)


def test_read_smiles_by_hand():
    from gaudi_amd.gor2goa import atoms_list, read_smiles
    from gaudi_amd.substructure import pattern, ring_pattern
    from gaudi_amd.substructure import read_smiles as as_pattern
    names = atoms_list(DATASET)
    t, b, o, q = read_smiles("C1=CC=CS1.[NH4+]", DATASET)
    assert [names[k] for k in t] == list("CCCCSN") + ["H"] * 8 and q.tolist() == [0] * 5 + [1] + [0] * 8
    assert sorted(o[:5].tolist()) == [1, 1, 1, 2, 2] and (o[5:] == 1).all() and len(b) == 13
    thio = as_pattern("C1=CC=CS1", DATASET)
    ring = ring_pattern("CCCCS", DATASET)
    assert ring[0].tolist() == [C, C, C, C, S_] and ring[1].tolist() == [[0, 1], [1, 2], [2, 3], [3, 4], [4, 0]]
    assert pattern(["C", S_], [(0, 1)], DATASET)[0].tolist() == [C, S_]
    with pytest.raises(_lib.GaudiError):
        pattern(["Xx"], [], DATASET)
    raw = host_search([thio], [ring, thio], H_EXACT)
    assert raw["count"].tolist() == [[2, 2]]


def test_search_and_the_layers_on_top(g32, monkeypatch):
    import torch
    import gaudi_amd.gor2goa as G
    from gaudi_amd import analyze, generation_guidance
    from gaudi_amd.substructure import contains, search
    mols = [m for m in g32[1] if m["special"] not in REFUSED][3::40]
    recs = [dict(status=0, atom_types=m["elem"], bonds=m["bonds"], fingerprint=1000 + k) for k, m in enumerate(mols)]
    recs.insert(2, dict(status=2, fingerprint=0))
    pats = [NAMED["benzene"], NAMED["thiophene"], recs[0]]  # a record is accepted as a pattern as it is, if it is small enough
    out = search(recs, pats, DATASET, engine=HostEngine())
    raw = host_search(mols, pats[:2], 0)
    keep = [k for k in range(len(recs)) if k != 2]
    assert np.array_equal(out["count"][keep][:, :2], raw["count"]) and (out["status"][2, :2] == EMPTY).all() and not out["hit"][2].any()
    assert out["status"][0, 2] in (OK, BAD_PATTERN) and (out["status"][0, 2] == BAD_PATTERN or out["hit"][0, 2])
    assert np.array_equal(contains(recs, pats[1], DATASET, engine=HostEngine()), out["hit"][:, 1])
    tight = search(recs, pats[:2], DATASET, hydrogens="exact", closed=True, engine=HostEngine())
    assert np.array_equal(tight["count"][keep], host_search(mols, pats[:2], H_EXACT | CLOSED)["count"])
    with pytest.raises(_lib.GaudiError):
        search(recs, pats, DATASET, hydrogens="some", engine=HostEngine())
    empty = search([], pats[:2], DATASET, engine=HostEngine())
    assert empty["count"].shape == (0, 2) and empty["symmetry"].tolist() == [12, 2]
    assert search(recs, [], DATASET, engine=HostEngine())["count"].shape == (len(recs), 0)

    calls = []

    def fake(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None, **kw):
        calls.append(kw)
        return recs

    class Engine(HostEngine):
        searches = 0

        def substructure_search(self, *a):
            Engine.searches += 1
            return HostEngine.substructure_search(self, *a)

    monkeypatch.setattr(G, "rings_to_atoms", fake)
    given = [(np.zeros((1, 3), np.float32), np.zeros(1, np.int64)) for _ in recs]
    plain, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Engine())
    assert Engine.searches == 0 and "pattern_hits" not in plain and "pattern_fraction" not in plain
    d, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Engine(), patterns=pats[:2])
    assert Engine.searches == 2 and set(d) == set(plain) | {"pattern_hits", "pattern_fraction"}
    assert d["pattern_hits"].dtype == bool and np.array_equal(d["pattern_hits"], out["hit"][:, :2]) and not d["pattern_hits"][2].any()
    assert np.allclose(d["pattern_fraction"], out["hit"][:, :2].sum(0) / len(mols))
    t, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Engine(), patterns=pats[:2],
                                               pattern_options=dict(hydrogens="exact", closed=True))
    assert np.array_equal(t["pattern_hits"], tight["hit"])
    # what design / design_sweep / refine add after sampling (the sampling itself needs a device: tests/test_gpu_substructure.py)
    n = len(recs)
    x, one_hot, mask = torch.zeros(n, 2, 3), torch.zeros(n, 2, 4), torch.ones(n, 2, 1)
    Engine.searches = 0
    plain = generation_guidance._atoms(x, one_hot, mask, DATASET, Engine())
    assert Engine.searches == 0 and "contains" not in plain
    got = generation_guidance._atoms(x, one_hot, mask, DATASET, Engine(), patterns=pats[:2])
    assert set(got) == set(plain) | {"contains"} and np.array_equal(got["contains"], out["hit"][:, :2])
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance._evaluate(None, None, None, None, None, 1.0, x, one_hot, mask, None, 1.0, patterns=pats[:2])


def test_declarations_and_argument_checks(g32):
    import ctypes as Ct
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    assert "#define GAUDI_ABI_VERSION 7" in header and lib.gaudi_abi_version() == 7
    ctype = {"int": Ct.c_int, "gaudi_handle*": Ct.c_void_p, "const int32_t*": _lib.IP, "int32_t*": _lib.IP,
             "uint8_t*": Ct.POINTER(Ct.c_uint8), "double*": Ct.POINTER(Ct.c_double)}
    for name in ("gaudi_substructure_search", "gaudi_host_substructure_search", "gaudi_substructure_profile_get",
                 "gaudi_host_substructure_root_steps"):
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, name
        args = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).replace("\n", " ").split(",")]
        assert _lib.EXPORTS[name] == (Ct.c_int, args), name
        assert hasattr(lib, name)
    for k, v in (("MAX_QUERY", 32), ("MAX_PATTERNS", 64), ("MAX_STEPS", _lib.SUB_MAX_STEPS), ("H_EXACT", 1), ("CLOSED", 2), ("OK", 0),
                 ("GAVE_UP", 1), ("BAD_INPUT", 2), ("OVERFLOW", 3), ("EMPTY", 4), ("BAD_PATTERN", 5)):
        assert re.search(rf"#define GAUDI_SUB_{k} +{v}\b", header) and getattr(_lib, "SUB_" + k) == v, k
    mols, pats = pack(g32[1][:2]), pack_patterns(named_patterns()[:2], 0)
    out = _lib.sub_outputs(2, 2, mols[0].shape[1], pats[0].shape[1])
    args = list(_lib.sub_args(N_ELEMS, H, C, *mols, *pats, out))
    assert lib.gaudi_host_substructure_search(*args) == 0
    for at, value in ((0, 9), (1, 7), (3, -1), (10, -1), (11, 0), (12, 0), (13, None), (17, None), (18, None), (21, None), (22, None)):
        broken = list(args)
        broken[at] = value
        assert lib.gaudi_host_substructure_search(*broken) == -1, at
    # first and covered may be left out
    lean = list(args)
    lean[19], lean[20] = None, None
    again = _lib.sub_outputs(2, 2, mols[0].shape[1], pats[0].shape[1])
    lean[18], lean[21], lean[22] = (again[k].ctypes.data_as(_lib.IP) for k in ("count", "steps", "status"))
    assert lib.gaudi_host_substructure_search(*lean) == 0
    assert all(np.array_equal(again[k], out[k]) for k in ("count", "steps", "status"))
    assert lib.gaudi_host_substructure_search(*(args[:3] + [0] + args[4:])) == 0  # B = 0
