"""Canonical numbering, exact identity keys and SMILES (csrc/canon.inc, gaudi_amd.gor2goa) through the kernel's HOST build,
gaudi_host_canonical_order: the outputs describe the input graph, do not depend on the numbering, separate exactly the
isomorphism classes (g30's iso_class; symmetric and random cubic graphs against networkx), ignore whether hydrogens were placed,
and carry the statuses; on top, canonical_molecule, the SMILES writer against a parser of its grammar, the exact counting of
analyze_atoms_for_molecules and the three declarations."""
import io
import os
import re

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import C, DATASET, H, fixture, pack, relabel, verify
from tests.canonical_helpers import (BAD_INPUT, EMPTY, GAVE_UP, OK, OVERFLOW, HostEngine, benzenes, carbon_molecule, code_graph,
                                     host_canon, input_graph, parse_smiles, renumber, same_labelled_graph, same_structure,
                                     strip_implied_hydrogens, structure_graph, symmetric_graphs)
from tests.gor2goa_helpers import unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = ("n_heavy", "n_hbonds", "label", "cbonds")


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def host(g32):
    """The whole fixture in one call of the host twin."""
    return host_canon(g32[1])


@pytest.fixture(scope="module")
def records(g32, host):
    """Every fixture molecule with a numbering as rings_to_atoms(canonical=True, bond_orders=True) would hand it on, and the
    same for a renumbered twin -- the canonical and the bond-order kernels both in their host builds."""
    from gaudi_amd.gor2goa import _bond_orders, _canonical_raw, _molecule_from_code
    rng = np.random.default_rng(3301)
    mols = [m for m in g32[1] if host["status"][m["index"]] == OK]
    out = []
    for batch in ([(m["elem"], m["bonds"]) for m in mols], [relabel(m, rng) for m in mols]):
        extras, codes = _canonical_raw(batch, DATASET, HostEngine())
        structs = _bond_orders([_molecule_from_code(c, DATASET) for c in codes], DATASET, engine=HostEngine())
        out.append([dict(status=0, atom_types=e, bonds=b, **x, **{"canon_" + k: v for k, v in s.items()})
                    for (e, b), x, s in zip(batch, extras, structs)])
    return mols, out[0], out[1]


def test_outputs_describe_the_input_graph(g32, host):
    n = 0
    for m in g32[1]:
        i, na = m["index"], len(m["elem"])
        if host["status"][i] != OK:
            continue
        heavy = m["elem"] != H
        rank = host["rank"][i]
        assert sorted(rank[:na][heavy].tolist()) == list(range(host["n_heavy"][i])) == list(range(int(heavy.sum())))
        assert (rank[:na][~heavy] == -1).all() and (rank[na:] == -1).all()
        g, cg = input_graph(m["elem"], m["bonds"]), code_graph(host, i)
        assert same_labelled_graph(g, cg), i
        # ... and rank_out is such an isomorphism
        assert g.number_of_edges() == cg.number_of_edges() and all(cg.has_edge(int(rank[a]), int(rank[b])) for a, b in g.edges())
        assert all(g.nodes[a]["label"] == cg.nodes[int(rank[a])]["label"] for a in g.nodes())
        pairs = host["cbonds"][i, :host["n_hbonds"][i]].tolist()
        assert pairs == sorted(pairs) and all(lo < hi for lo, hi in pairs)
        assert not host["label"][i, host["n_heavy"][i]:].any() and not host["cbonds"][i, host["n_hbonds"][i]:].any()
        n += 1
    assert n >= 500


def test_renumbering_changes_nothing(g32, host):
    assert GAVE_UP not in host["status"] and host["nodes"].max() <= 4096
    for seed in (1, 2, 3):
        rng = np.random.default_rng(3310 + seed)
        twins = [relabel(m, rng) if host["status"][m["index"]] == OK else (m["elem"], m["bonds"]) for m in g32[1]]
        out = host_canon(twins)
        assert np.array_equal(out["status"], host["status"]) and out["nodes"].max() <= 4096
        for k in CODE:
            assert out[k].tobytes() == host[k].tobytes(), (seed, k)


def _key(raw, i):
    from gaudi_amd.gor2goa import canon_code
    return canon_code(raw, i)


def test_keys_equal_the_isomorphism_classes_of_g30(golden):
    """On the atoms and bonds the reference built: equal keys <=> equal iso_class."""
    mols = [m for m in unpack(golden("g30_gor2goa")) if not m["threw"]]
    raw = host_canon([(m["ref_types"].astype(np.int32), m["ref_bonds"].astype(np.int32)) for m in mols])
    assert (raw["status"] == OK).all() and len(mols) == 160
    keys = [_key(raw, i) for i in range(len(mols))]
    by_key, by_class = {}, {}
    for k, m in zip(keys, mols):
        by_key.setdefault(k, set()).add(m["iso_class"])
        by_class.setdefault(m["iso_class"], set()).add(k)
    assert all(len(v) == 1 for v in by_key.values()) and all(len(v) == 1 for v in by_class.values())
    assert len(by_key) == len(by_class) == 128


def test_keys_equal_isomorphism_on_symmetric_and_cubic_graphs():
    import networkx as nx
    graphs = symmetric_graphs()
    assert len(graphs) == 77
    mols = [carbon_molecule(g) for _, g in graphs]
    raw = host_canon(mols)
    assert (raw["status"] == OK).all() and raw["nodes"].max() <= 4096
    keys = [_key(raw, i) for i in range(len(mols))]
    pairs = 0
    for i in range(len(graphs)):
        for j in range(i):
            if graphs[i][1].number_of_nodes() != graphs[j][1].number_of_nodes():
                continue
            assert (keys[i] == keys[j]) == nx.is_isomorphic(graphs[i][1], graphs[j][1]), (graphs[i][0], graphs[j][0])
            pairs += 1
    assert pairs >= 150
    rng = np.random.default_rng(3320)
    again = host_canon([renumber(e, b, rng) for e, b in mols])
    assert [_key(again, i) for i in range(len(mols))] == keys and np.array_equal(again["nodes"], raw["nodes"])


def test_placed_hydrogens_do_not_change_the_key(g32, host):
    """place_hydrogens true and false, at the array level: the H of every carbon with two heavy neighbours taken away."""
    mols, bare, n = [], [], 0
    for m in g32[1]:
        if host["status"][m["index"]] != OK:
            continue
        e, b, removed = strip_implied_hydrogens(m["elem"], m["bonds"])
        if removed:
            mols.append(m)
            bare.append((e, b))
            n += removed
    assert len(mols) >= 200 and n >= 1000
    out = host_canon(bare)
    for j, m in enumerate(mols):
        assert _key(out, j) == _key(host, m["index"]), m["index"]


def test_statuses(g32, host):
    e5 = next(m for m in g32[1] if m["special"] == 4)  # BAD_VALENCE of the bond orders: a carbon with five bonds
    assert max(np.bincount(e5["bonds"].reshape(-1))) == 5
    out = host_canon([benzenes(3), benzenes(2), benzenes(1), e5])
    assert out["status"].tolist() == [GAVE_UP, OK, OK, OK] and out["nodes"].tolist()[:3] == [4096, 469, 19]
    # GAVE_UP still hands back a numbering
    assert sorted(out["rank"][0, :18].tolist()) == list(range(18)) and out["n_heavy"][0] == 18 and out["n_hbonds"][0] == 18
    assert same_labelled_graph(input_graph(*benzenes(3)), code_graph(out, 0))
    want = {5: BAD_INPUT, 6: OVERFLOW, 7: EMPTY}  # the fixture's specials by their bond-order status
    seen = set()
    for m in g32[1]:
        if m["special"] in want:
            i = m["index"]
            assert host["status"][i] == want[m["special"]], (i, m["special"])
            assert not any(host[k][i].any() for k in ("rank", "n_heavy", "label", "n_hbonds", "cbonds", "nodes"))
            seen.add(m["special"])
    assert seen == set(want)
    # a vertex of degree 9, eight hydrogens on one atom, an element outside the list, a repeated bond; degree 8 is taken (the
    # arms have different lengths: eight equal ones would be a tree of 8! leaves)
    arms, ab = [C], []
    for k in range(8):
        prev = 0
        for _ in range(k + 1):
            arms.append(C)
            ab.append((prev, len(arms) - 1))
            prev = len(arms) - 1
    star = (np.full(10, C, np.int32), np.array([(0, k) for k in range(1, 10)], np.int32))
    hs = (np.array([3] + [H] * 8, np.int32), np.array([(0, k) for k in range(1, 9)], np.int32))
    out = host_canon([star, hs, (np.array([C, 6], np.int32), np.array([(0, 1)], np.int32)),
                      (np.array([C, C], np.int32), np.array([(0, 1), (1, 0)], np.int32)),
                      (np.array(arms, np.int32), np.array(ab, np.int32)),
                      (np.full(9, C, np.int32), np.array([(0, k) for k in range(1, 9)], np.int32))])
    assert out["status"].tolist() == [OVERFLOW, OVERFLOW, BAD_INPUT, BAD_INPUT, OK, GAVE_UP] and out["nodes"][4] == 1
    assert same_labelled_graph(input_graph(np.array(arms), np.array(ab)), code_graph(out, 4))
    with pytest.raises(_lib.GaudiError):
        _lib.host_canonical_order(9, H, C, *pack([benzenes(1)]))


def test_canonical_molecule_and_its_structure(g32, records):
    from gaudi_amd.gor2goa import canonical_molecule
    z = g32[0]
    mols, recs, twins = records
    n = 0
    for m, r, t in zip(mols, recs, twins):
        types, bonds = canonical_molecule(r, DATASET)
        t2, b2 = canonical_molecule(t, DATASET)
        assert np.array_equal(types, t2) and np.array_equal(bonds, b2)
        heavy = int((m["elem"] != H).sum())
        assert (types[:heavy] != H).all() and (types[heavy:] == H).all() and (bonds[:, 0] <= bonds[:, 1]).all()
        assert bonds.tolist() == sorted(bonds.tolist()) and np.all(np.diff(bonds[bonds[:, 1] >= heavy][:, 0]) >= 0)
        for k in ("canon_kekule_status", "canon_n_charged"):
            assert r[k] == t[k]
        assert np.array_equal(r["canon_orders"], t["canon_orders"]) and np.array_equal(r["canon_charges"], t["canon_charges"])
        if r["canon_kekule_status"] == 0:
            verify(z["table_n"], z["table_opt"], types, bonds, r["canon_orders"], r["canon_charges"], r["canon_n_charged"])
            n += 1
    assert n >= 250
    # without a key on the record the numbering is computed (here on the host build), hydrogens implied or listed
    e, b = benzenes(1)
    types, bonds = canonical_molecule((e, b), DATASET, engine=HostEngine())
    assert types.tolist() == [C] * 6 + [H] * 6 and len(bonds) == 12
    with pytest.raises(_lib.GaudiError):
        canonical_molecule((np.array([C, C], np.int32), np.array([(0, 5)], np.int32)), DATASET, engine=HostEngine())


def test_smiles(g32, records):
    from gaudi_amd.gor2goa import atoms_list, canonical_molecule, smiles, write_smiles
    names = atoms_list(DATASET)
    mols, recs, twins = records
    n, charged = 0, 0
    for m, r, t in zip(mols, recs, twins):
        text = smiles(r, DATASET)
        if r["canon_kekule_status"] != 0:
            assert text is None
            continue
        assert text == smiles(t, DATASET) and re.fullmatch(r"[BCNOSH\[\]()=%.+\-0-9]+", text)
        types, bonds = canonical_molecule(r, DATASET)
        assert same_structure(parse_smiles(text), structure_graph(names, types, bonds, r["canon_orders"], r["canon_charges"])), text
        if m["min_charged"] == 2:
            assert re.search(r"\[[A-Z]H?\d?\+\]", text) and re.search(r"\[[A-Z]H?\d?-\]", text), text
            charged += 1
        n += 1
    assert n >= 250 and charged >= 10
    benzene = next(r for m, r in zip(mols, recs) if len(m["elem"]) == 12 and (m["elem"] == C).sum() == 6 and len(m["bonds"]) == 12)
    assert smiles(benzene, DATASET) in ("C1=CC=CC=C1", "C1C=CC=CC=1")
    assert smiles(dict(benzene, canon_status=GAVE_UP), DATASET) is None and smiles(dict(status=2), DATASET) is None
    f = io.StringIO()
    assert write_smiles(f, [benzene, dict(status=2), benzene], DATASET) == 2
    assert f.getvalue().splitlines() == [smiles(benzene, DATASET), "", smiles(benzene, DATASET)]


def test_smiles_of_hand_made_structures():
    """Branches, two components, a ring number above 9 and bracket atoms, from records written by hand."""
    from gaudi_amd.gor2goa import canon_code, smiles
    N, O = 3, 4

    def record(elem, bonds, orders, charges):
        raw = host_canon([(np.array(elem, np.int32), np.array(bonds, np.int32).reshape(-1, 2))])
        assert raw["status"][0] == OK
        from gaudi_amd.gor2goa import _molecule_from_code
        key = canon_code(raw, 0)
        types, cb = _molecule_from_code(key, DATASET)
        rank = raw["rank"][0]
        # carry the hand-made orders and charges over to the canonical arrays (heavy-heavy bonds only; the rest are single)
        by_pair = {tuple(sorted((int(rank[i]), int(rank[j])))): o for (i, j), o in zip(bonds, orders) if rank[i] >= 0 and rank[j] >= 0}
        co = np.array([by_pair.get((int(i), int(j)), 1) for i, j in cb])
        cq = np.zeros(len(types), np.int64)
        for a, q in enumerate(charges):
            if rank[a] >= 0:
                cq[rank[a]] = q
        return dict(status=0, canon_status=0, canon_key=key, canon_kekule_status=0, canon_orders=co, canon_charges=cq)

    # formaldehyde next to ammonium: two components, "=" before a child, a bracket atom with four hydrogens
    text = smiles(record([C, O, H, H, N, H, H, H, H], [(0, 1), (0, 2), (0, 3), (4, 5), (4, 6), (4, 7), (4, 8)],
                         [2, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 1, 0, 0, 0, 0]), DATASET)
    assert sorted(text.split(".")) == ["C=O", "[NH4+]"]
    # isobutene: three children, all but the last in parentheses
    text = smiles(record([C, C, C, C] + [H] * 8, [(0, 1), (0, 2), (0, 3), (1, 4), (1, 5), (2, 6), (2, 7), (2, 8), (3, 9), (3, 10), (3, 11)],
                         [2] + [1] * 10, [0] * 12), DATASET)
    g = parse_smiles(text)
    assert text.count("(") == 2 and text.count("=") == 1 and sorted(d for _, d in g.degree()) == [1, 1, 1, 3]
    # eight atoms, all bonded to each other and told apart by element and H count (a graph, not chemistry): a depth-first walk
    # is a path, and past its fourth atom 15 ring closures are open at once
    elem = [2, C, N, O, 5, 2, C, N] + [H] * 3
    bonds = [(i, j) for i in range(8) for j in range(i)]
    hb = [(5, 8), (6, 9), (7, 10)]
    text = smiles(record(elem, bonds + hb, [1] * (len(bonds) + 3), [0] * len(elem)), DATASET)
    g = parse_smiles(text)
    assert "%10" in text and "%15" in text and g.number_of_edges() == 28
    assert sorted((d["sym"], d["n_h"]) for _, d in g.nodes(data=True)) == sorted(
        [("B", 0), ("C", 0), ("N", 0), ("O", 0), ("S", 0), ("B", 1), ("C", 1), ("N", 1)])


def test_analyze_atoms_exact(monkeypatch):
    """The counting alone, from a stand-in for the batched call: the defaults return the earlier dict key for key; exact=True
    counts classes by key, with ("fp", fingerprint) for a molecule whose search gave up."""
    import gaudi_amd.gor2goa as G
    from gaudi_amd import analyze
    fps = [11, 22, 11, 0, 33, 22, 44]
    status = [0, 0, 0, 2, 0, 0, 0]
    keys = [b"a", b"b", b"c", None, None, b"b", None]  # 11 splits into a / c (a fingerprint collision); 33 and 44 gave up
    calls = []

    def fake(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None, **kw):
        calls.append(kw)
        recs = [dict(status=s, fingerprint=k) for s, k in zip(status, fps)]
        if kw.get("canonical"):
            for r, k in zip(recs, keys):
                r.update(canon_key=k, canon_status=(OK if k is not None else GAVE_UP) if r["status"] == 0 else EMPTY)
        return recs

    monkeypatch.setattr(G, "rings_to_atoms", fake)
    mols = [(np.zeros((1, 3), np.float32), np.zeros(1, np.int64)) for _ in fps]
    plain, _ = analyze.analyze_atoms_for_molecules(mols, dataset="cata", train_fingerprints=[22, 99])
    assert calls == [{}] and set(plain) == {"mol_built", "mol_unique", "molecule_built_bool", "fingerprints", "mol_novel"}
    assert plain["mol_unique"] == 4 / 6 and plain["mol_novel"] == 4 / 6 and plain["fingerprints"] == fps
    same, _ = analyze.analyze_atoms_for_molecules(mols, dataset="cata", train_fingerprints=[22, 99], exact=False, train_keys=[b"a"])
    assert same == plain
    d, built = analyze.analyze_atoms_for_molecules(mols, dataset="cata", exact=True, train_keys=[b"b", b"zz"])
    assert calls[-1] == {"canonical": True} and len(built) == 6
    assert set(d) == set(plain) | {"canon_keys", "mol_undecided"}
    assert d["canon_keys"] == [b"a", b"b", b"c", None, ("fp", 33), b"b", ("fp", 44)]
    assert d["mol_unique"] == 5 / 6 and d["mol_undecided"] == 2 / 6 and d["mol_novel"] == 4 / 6 and d["fingerprints"] == fps
    d, _ = analyze.analyze_atoms_for_molecules(mols, dataset="cata", exact=True)
    assert "mol_novel" not in d


def test_the_three_declarations_are_exported_and_bound():
    import ctypes as Ct
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    assert "#define GAUDI_ABI_VERSION 7" in header and lib.gaudi_abi_version() == 7
    ctype = {"int": Ct.c_int, "gaudi_handle*": Ct.c_void_p, "const int32_t*": _lib.IP, "int32_t*": _lib.IP,
             "uint8_t*": Ct.POINTER(Ct.c_uint8), "uint16_t*": Ct.POINTER(Ct.c_uint16), "double*": Ct.POINTER(Ct.c_double)}
    for name in ("gaudi_canonical_order", "gaudi_host_canonical_order", "gaudi_canon_profile_get"):
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, name
        args = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).replace("\n", " ").split(",")]
        assert _lib.EXPORTS[name] == (Ct.c_int, args), name
        assert hasattr(lib, name)
    for k, v in (("OK", 0), ("GAVE_UP", 1), ("BAD_INPUT", 2), ("OVERFLOW", 3), ("EMPTY", 4)):
        assert re.search(rf"#define GAUDI_CANON_{k} {v}\b", header) and getattr(_lib, "CANON_" + k) == v
    for k in ("MAX_ATOMS", "MAX_HEAVY", "MAX_BONDS", "MAX_DEGREE", "MAX_NODES", "MAX_DEPTH"):
        assert re.search(rf"#define GAUDI_CANON_{k} {getattr(_lib, 'CANON_' + k)}\b", header), k
