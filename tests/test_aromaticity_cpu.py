"""Kekule counts, Pauling bond orders, sextets, Fries and Clar numbers (csrc/kekule.inc) through the kernel's HOST build,
gaudi_host_kekule: textbook values, every molecule of golden g32 against an oracle that shares nothing with the kernel
(tests/aromaticity_helpers.py), invariants, agreement with gaudi_host_bond_orders, relabelling, the budget, the other statuses and
the Python layers on top."""
import os

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.aromaticity_helpers import (BAD_INPUT, BAD_VALENCE, BUDGET, DATASET, EMPTY, KNOWN, MAX_SEL, NO_KEKULE, NOT_CONNECTED,
                                       NOT_NEUTRAL, OK, OVERFLOW, SMILES, UNDECIDED, HostEngine, assert_equals_oracle, g32_host,
                                       g32_oracle, host, ladder, molecule, oracle, polyene, row, tables)
from tests.bond_order_helpers import C, H, fixture, pack, relabel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g32():
    return fixture()


def _heavy_bonds(elem, bonds):
    return [k for k, (i, j) in enumerate(bonds) if elem[i] != H and elem[j] != H]


def test_known_values_pin_the_oracle_and_the_kernel(g32):
    z = g32[0]
    names = list(SMILES)
    mols = [molecule(k) for k in names]
    out = host(mols)
    for i, (name, (e, b)) in enumerate(zip(names, mols)):
        ref = oracle(e, b, z["table_n"], z["table_opt"])
        assert_equals_oracle(out, i, ref, len(b))
        if name in KNOWN:
            assert (ref["k"], ref["clar"]) == KNOWN[name] == (out["k"][i], out["clar"][i]), name
    k = dict(zip(names, out["k"].tolist()))
    assert k["pyridine"] == 2 and k["thiophene"] == k["pyrrole"] == k["borole"] == 1 and k["biphenylene"] == 5
    assert [out["n_hex"][names.index(n)] for n in ("pyridine", "thiophene", "pyrrole", "borole", "biphenylene")] == [1, 0, 0, 0, 2]
    # naphthalene: 2/3 on the four bonds between an alpha and a beta carbon (the 1,2-type bonds), 1/3 elsewhere
    e, b = mols[names.index("naphthalene")]
    dc = out["double_count"][names.index("naphthalene")]
    heavy_deg = np.bincount(np.array([b[k] for k in _heavy_bonds(e, b)]).reshape(-1), minlength=len(e))
    fused = {a for a in range(len(e)) if heavy_deg[a] == 3}
    alpha = {a for a in range(len(e)) if e[a] == C and a not in fused and any(a in b[k] and set(b[k]) & fused for k in _heavy_bonds(e, b))}
    for kk in _heavy_bonds(e, b):
        i, j = b[kk]
        one_two = not {i, j} & fused and len({i, j} & alpha) == 1
        assert dc[kk] == (2 if one_two else 1), (kk, i, j)
    assert sum(dc[kk] == 2 for kk in _heavy_bonds(e, b)) == 4 and len(_heavy_bonds(e, b)) == 11
    # phenanthrene: the 9,10 bond (atoms 6 and 7 of the SMILES) is double in four of five structures
    e, b = mols[names.index("phenanthrene")]
    dc = out["double_count"][names.index("phenanthrene")]
    k910 = [kk for kk, (i, j) in enumerate(b) if {int(i), int(j)} == {6, 7}]
    assert len(k910) == 1 and dc[k910[0]] == 4 == dc[:len(b)].max() and (dc[:len(b)] == 4).sum() == 1
    for kk, (i, j) in enumerate(b):  # bonds to hydrogen are outside G[sel]
        assert (e[i] == H or e[j] == H) == (kk not in _heavy_bonds(e, b)) and (dc[kk] == 0 or kk in _heavy_bonds(e, b))


def test_every_g32_molecule_equals_the_oracle(g32):
    out, refs = g32_host(), g32_oracle()
    assert UNDECIDED not in out["status"]
    for m, ref in zip(g32[1], refs):
        assert_equals_oracle(out, m["index"], ref, len(m["bonds"]))
    st = np.bincount(out["status"], minlength=9)
    assert st[OK] >= 250 and st[NO_KEKULE] >= 100 and st[NOT_NEUTRAL] >= 50 and out["k"].max() == 256
    assert max(r["n_nodes"] for r in refs) * 40 < BUDGET  # the budget is far from every molecule of the fixture


def test_invariants_on_every_counted_molecule(g32):
    out, refs = g32_host(), g32_oracle()
    n = quinoid = 0
    for m, ref in zip(g32[1], refs):
        i, nb = m["index"], len(m["bonds"])
        if out["status"][i] != OK:
            assert row(out, i, nb)[1:] == (0, [0] * nb, 0, [], [], 0, 0, 0)
            continue
        n += 1
        K, r = int(out["k"][i]), int(out["n_hex"][i])
        around = np.zeros(len(m["elem"]), np.int64)
        np.add.at(around, m["bonds"][:, 0], out["double_count"][i, :nb])
        np.add.at(around, m["bonds"][:, 1], out["double_count"][i, :nb])
        assert set(around.tolist()) <= {0, K} and (around == K).sum() == ref["n_sel"]  # every sel atom has one double bond per structure
        assert (out["sextet_count"][i, :r] <= K).all()
        # 1 <= clar <= fries <= n_hex wherever a hexagon is a sextet of some structure.  A hexagon alone does not make one: twelve
        # molecules of the fixture (2H-isoindole-like: the five-ring's lone-pair heteroatom fixes two exocyclic double bonds on
        # the six-ring) have hexagons, K >= 1 and no sextet in any structure; there clar = fries = 0, as the oracle's textbook
        # Clar number (test_every_g32_molecule_equals_the_oracle) says too
        assert out["clar"][i] <= out["fries"][i] <= r
        assert (out["clar"][i] >= 1) == (out["fries"][i] >= 1) == bool(out["sextet_count"][i, :r].any())
        quinoid += r > 0 and out["clar"][i] == 0
    assert n >= 250 and quinoid == 12


def test_agreement_with_bond_orders(g32):
    """Where gaudi_host_bond_orders decides (OK, NO_STRUCTURE, CAPPED): Kekule structures are counted exactly where it returns a
    structure without a charged atom.  The one thing that can stand between the two is this kernel's smaller capacity (128 sel
    atoms against 192 heavy atoms): those molecules are OVERFLOW, and the oracle's own sel count says they are beyond it."""
    out, refs = g32_host(), g32_oracle()
    bo = _lib.host_bond_orders(tables(), *pack(g32[1]))
    n = beyond = 0
    for m, ref in zip(g32[1], refs):
        i = m["index"]
        if bo["status"][i] not in (0, 1, 2):
            continue
        if out["status"][i] == OVERFLOW:
            assert ref["n_sel"] > MAX_SEL
            beyond += 1
            continue
        n += 1
        assert (out["status"][i] == OK) == (bo["status"][i] == 0 and bo["n_charged"][i] == 0), i
    assert n >= 480 and beyond <= 4


def test_relabelling(g32):
    out = g32_host()
    pick = [m for m in g32[1] if out["status"][m["index"]] == OK and out["n_hex"][m["index"]] >= 2][::7][:32]
    assert len(pick) == 32
    for seed in (1, 2, 3):
        rng = np.random.default_rng(8700 + seed)
        twins = []
        for m in pick:
            n = len(m["elem"])
            perm, order = rng.permutation(n), rng.permutation(len(m["bonds"]))
            elem = np.zeros(n, np.int32)
            elem[perm] = m["elem"]
            twins.append((elem, perm[m["bonds"]].astype(np.int32).reshape(-1, 2)[order], order))
        got = host([(e, b) for e, b, _ in twins])
        for j, (m, (_, b, order)) in enumerate(zip(pick, twins)):
            i, nb, r = m["index"], len(b), int(out["n_hex"][m["index"]])
            assert (got["status"][j], got["k"][j], got["fries"][j], got["clar"][j], got["n_hex"][j]) == \
                (OK, out["k"][i], out["fries"][i], out["clar"][i], r)
            assert np.array_equal(got["double_count"][j, :nb], out["double_count"][i, :nb][order])  # follows the bond permutation
            assert sorted(got["sextet_count"][j, :r].tolist()) == sorted(out["sextet_count"][i, :r].tolist())
    e, b = relabel(pick[0], np.random.default_rng(8704))  # (the helper the other suites use: shuffled and flipped bonds)
    one = host([(e, b)])
    assert one["k"][0] == out["k"][pick[0]["index"]] and sorted(one["double_count"][0, :len(b)].tolist()) == \
        sorted(out["double_count"][pick[0]["index"], :len(b)].tolist())


def test_the_budget(g32):
    """F(n + 1) structures on the 2 x n ladder: 233 at n = 12; at n = 30 the 1 346 269 structures alone are more nodes than the
    budget, whatever the numbering: UNDECIDED, everything zero, the neighbours untouched."""
    benz = molecule("benzene")
    out = host([benz, ladder(12), ladder(30), benz])
    assert out["status"].tolist() == [OK, OK, UNDECIDED, OK] and out["k"].tolist() == [2, 233, 0, 2]
    ref = oracle(*ladder(12), g32[0]["table_n"], g32[0]["table_opt"])
    assert ref["k"] == 233 and ref["hexagons"] == []
    assert_equals_oracle(out, 1, ref, len(ladder(12)[1]))
    assert row(out, 2, len(ladder(30)[1]))[1:] == (0, [0] * len(ladder(30)[1]), 0, [], [], 0, 0, 0)
    assert row(out, 0, len(benz[1])) == row(out, 3, len(benz[1])) == row(host([benz]), 0, len(benz[1]))
    fib = [1, 1]
    while len(fib) < 12:
        fib.append(fib[-1] + fib[-2])
    small = host([ladder(n) for n in range(2, 11)])
    assert small["k"].tolist() == fib[2:11] and (small["status"] == OK).all()


def test_other_statuses(g32):
    z, mols = g32
    out = g32_host()
    assert out["status"][501] == OVERFLOW and (mols[501]["elem"] != H).sum() == 194
    seen = {}
    for m in mols:
        if m["special"] >= 0:
            seen.setdefault(m["special"], []).append(int(out["status"][m["index"]]))
    # the specials of the bond-order fixture: OK, NO_STRUCTURE, NOT_CONNECTED, BAD_VALENCE, BAD_INPUT, OVERFLOW, EMPTY
    assert seen[3] == [NOT_CONNECTED] and seen[4] == [BAD_VALENCE] and seen[5] == [BAD_INPUT] and seen[6] == [OVERFLOW] and seen[7] == [EMPTY]
    benz = molecule("benzene")
    two = (np.concatenate([benz[0], benz[0]]), np.concatenate([benz[1], benz[1] + len(benz[0])]))  # two benzenes in one record
    odd = polyene(3)                                                                               # three sel atoms
    from gaudi_amd.gor2goa import atoms_list
    N = atoms_list(DATASET).index("N")
    t = tables()
    assert t.n_options[N][4] == 1 and t.option[N][4][0][1] == 1  # an ammonium nitrogen has only a charged option
    ammonium = (np.array([N, H, H, H, H], np.int32), np.array([(0, 1), (0, 2), (0, 3), (0, 4)], np.int32))
    methane = (np.array([C, H, H, H, H], np.int32), np.array([(0, 1), (0, 2), (0, 3), (0, 4)], np.int32))  # sel empty: K = 1
    twice = (benz[0], np.concatenate([benz[1], benz[1][:1, ::-1]]))                                         # a bond listed twice
    outside = (benz[0], np.concatenate([benz[1], [[0, len(benz[0])]]]).astype(np.int32))
    got = host([two, odd, ammonium, methane, twice, outside, (np.zeros(0, np.int32), np.zeros((0, 2), np.int32)), benz])
    assert got["status"].tolist() == [NOT_CONNECTED, NO_KEKULE, NOT_NEUTRAL, OK, BAD_INPUT, BAD_INPUT, EMPTY, OK]
    assert got["k"].tolist() == [0, 0, 0, 1, 0, 0, 0, 2] and got["n_nodes"].tolist() == [0, 0, 0, 1, 0, 0, 0, 7]
    for i in (0, 1, 2, 4, 5, 6):
        assert not got["double_count"][i].any() and not got["hex_atoms"][i].any() and got["n_hex"][i] == 0
    for e, b in (two, odd, ammonium, methane, twice):
        ref = oracle(e, b, z["table_n"], z["table_opt"])
        assert_equals_oracle(host([(e, b)]), 0, ref, len(b))
    # capacity edges: 128 sel atoms are taken, 130 are not; a polyene's one structure leaves every second bond localized
    edge = host([polyene(128), polyene(130)])
    assert edge["status"].tolist() == [OK, OVERFLOW] and edge["k"].tolist() == [1, 0] and edge["n_nodes"][0] == 65
    assert edge["double_count"][0, :127].tolist() == [1, 0] * 63 + [1]


def test_bad_tables_are_refused(g32):
    t = tables()
    t.option[2][3][0][1] = -1  # of two options the first must be neutral
    with pytest.raises(_lib.GaudiError):
        _lib.host_kekule(t, *pack(g32[1][:1]))
    elem, na, bonds, nb = pack(g32[1][:1])
    nb[0] = bonds.shape[1] + 1
    with pytest.raises(_lib.GaudiError):
        _lib.host_kekule(tables(), elem, na, bonds, nb)
    lib = _lib.load_library()
    out = _lib.kekule_outputs(1, bonds.shape[1])
    args = list(_lib.kekule_args(*pack(g32[1][:1]), out))
    args[7] = None  # k_out
    assert lib.gaudi_host_kekule(tables(), *args) != 0


def test_declarations():
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    for name in ("gaudi_kekule(", "gaudi_host_kekule(", "gaudi_kekule_profile_get(", "GAUDI_KEKULE_BUDGET (1 << 20)",
                 "GAUDI_KEKULE_MAX_SEL 128", "GAUDI_KEKULE_MAX_EDGES 192", "GAUDI_KEKULE_UNDECIDED 8", "GAUDI_KEKULE_EMPTY 7"):
        assert name in header, name
    assert "#define GAUDI_ABI_VERSION 7" in header
    assert (_lib.KEKULE_BUDGET, _lib.KEKULE_MAX_SEL, _lib.KEKULE_MAX_EDGES) == (BUDGET, 128, 192)
    assert (_lib.KEKULE_OK, _lib.KEKULE_NO_KEKULE, _lib.KEKULE_NOT_NEUTRAL, _lib.KEKULE_NOT_CONNECTED, _lib.KEKULE_BAD_VALENCE,
            _lib.KEKULE_BAD_INPUT, _lib.KEKULE_OVERFLOW, _lib.KEKULE_EMPTY, _lib.KEKULE_UNDECIDED) == tuple(range(9))
    lib = _lib.load_library()
    assert all(hasattr(lib, n) for n in ("gaudi_kekule", "gaudi_host_kekule", "gaudi_kekule_profile_get"))


def test_resonance_and_the_layers_on_top(g32, monkeypatch):
    import torch
    import gaudi_amd.gor2goa as G
    from gaudi_amd import analyze, aromaticity, generation_guidance
    out = g32_host()
    mols = [m for m in g32[1] if m["g30"] >= 0][5::6][:24]  # built g30 molecules, as the fixture keeps them
    assert len(mols) == 24 and sum(out["status"][m["index"]] == OK for m in mols) >= 8
    recs = [dict(status=0, atom_types=m["elem"].astype(np.int64), bonds=m["bonds"].astype(np.int64), fingerprint=2000 + k) for k, m in enumerate(mols)]
    recs.insert(3, dict(status=2, fingerprint=0))
    keep = [k for k in range(len(recs)) if k != 3]
    res = aromaticity.resonance(recs, DATASET, engine=HostEngine())
    assert len(res) == len(recs) and res[3]["status"] == EMPTY and res[3]["kekule_count"] == 0 and len(res[3]["double_count"]) == 0
    assert set(aromaticity.STATUS_NAMES) == set(range(9))
    for k, m in zip(keep, mols):
        i, nb, r = m["index"], len(m["bonds"]), res[k]
        want = row(out, i, nb)
        assert (r["status"], r["kekule_count"], r["double_count"].tolist(), len(r["hexagons"]), r["hexagons"].tolist(),
                r["sextet_count"].tolist(), r["fries"], r["clar"], r["n_nodes"]) == want
        assert isinstance(r["kekule_count"], int) and r["pauling_bond_order"].dtype == np.float64 and r["hexagons"].shape == (want[3], 6)
        if r["status"] == OK:
            K = r["kekule_count"]
            assert np.array_equal(r["pauling_bond_order"], r["double_count"] / K) and np.array_equal(r["sextet_fraction"], r["sextet_count"] / K)
            heavy = np.array([m["elem"][i_] != H and m["elem"][j_] != H for i_, j_ in m["bonds"]])
            assert set(r["localized_double"].tolist()) == set(np.flatnonzero(r["double_count"] == K).tolist())
            assert set(r["localized_single"].tolist()) <= set(np.flatnonzero(heavy & (r["double_count"] == 0)).tolist())
            assert all(r["pauling_bond_order"][b_] == 0.0 for b_ in r["localized_single"])
        else:
            assert np.isnan(r["pauling_bond_order"]).all() and len(r["pauling_bond_order"]) == nb and len(r["localized_double"]) == 0
    pairs = [(m["elem"], m["bonds"]) for m in mols]
    kc, cl = aromaticity.kekule_count(recs, DATASET, engine=HostEngine()), aromaticity.clar_number(pairs, DATASET, engine=HostEngine())
    assert kc.dtype == np.int64 and kc[3] == 0 and kc[keep].tolist() == [int(out["k"][m["index"]]) for m in mols]
    assert cl.tolist() == [int(out["clar"][m["index"]]) for m in mols]
    assert aromaticity.resonance([], DATASET, engine=HostEngine()) == [] and aromaticity.kekule_count([], DATASET, engine=HostEngine()).shape == (0,)
    # a polyene: every second bond is a localized double bond, the others localized single bonds
    p = aromaticity.resonance([polyene(6)], DATASET, engine=HostEngine())[0]
    assert p["localized_double"].tolist() == [0, 2, 4] and p["localized_single"].tolist() == [1, 3] and p["pauling_bond_order"][:5].tolist() == [1, 0, 1, 0, 1]
    # rings_to_atoms / analyze_atoms_for_molecules on these records (the conversion itself needs a device: tests/test_gpu_aromaticity.py)
    fields = aromaticity.record_fields(recs, DATASET, engine=HostEngine())
    assert set(fields[0]) == {"kekule_count", "clar", "fries", "max_pauling_order", "resonance_status"} and fields[3]["resonance_status"] == EMPTY
    for k, m in zip(keep, mols):
        f, r = fields[k], res[k]
        assert (f["kekule_count"], f["clar"], f["fries"], f["resonance_status"]) == (r["kekule_count"], r["clar"], r["fries"], r["status"])
        assert f["max_pauling_order"] == r["pauling_bond_order"].max() if r["status"] == OK else np.isnan(f["max_pauling_order"])

    def fake(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None, **kw):
        got = [dict(r) for r in recs]
        if kw.get("aromaticity"):
            for r, extra in zip(got, aromaticity.record_fields(got, dataset, engine=engine)):
                r.update(extra)
        return got

    monkeypatch.setattr(G, "rings_to_atoms", fake)
    given = [(np.zeros((1, 3), np.float32), np.zeros(1, np.int64)) for _ in recs]
    HostEngine.calls = 0
    plain, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=HostEngine())
    assert HostEngine.calls == 0 and not any("kekule" in k or "clar" in k for k in plain)
    d, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=HostEngine(), aromaticity=True)
    assert HostEngine.calls == 1 and set(d) == set(plain) | {"mol_kekule_count", "mol_clar", "mean_log_kekule_per_center"}
    assert all(np.array_equal(d[k], plain[k]) for k in plain)
    assert d["mol_kekule_count"].tolist() == kc[keep].tolist() and d["mol_clar"].tolist() == cl.tolist()
    logs = [np.log(float(out["k"][m["index"]])) / float((m["elem"] != H).sum()) for m in mols if out["status"][m["index"]] == OK]
    assert d["mean_log_kekule_per_center"] == float(np.mean(logs)) > 0.0
    unbuilt = dict(kekule_count=0, clar=0, fries=0, max_pauling_order=float("nan"), resonance_status=EMPTY)
    monkeypatch.setattr(G, "rings_to_atoms", lambda *a, **kw: [dict(status=2, fingerprint=0, **(unbuilt if kw.get("aromaticity") else {}))])
    none, _ = analyze.analyze_atoms_for_molecules(given[:1], dataset=DATASET, engine=HostEngine(), aromaticity=True)
    assert none["mean_log_kekule_per_center"] == 0.0 and len(none["mol_kekule_count"]) == 0 and len(none["mol_clar"]) == 0
    monkeypatch.setattr(G, "rings_to_atoms", fake)
    # what design / design_sweep / refine add after sampling (the sampling itself needs a device)
    n = len(recs)
    x, one_hot, mask = torch.zeros(n, 2, 3), torch.zeros(n, 2, 4), torch.ones(n, 2, 1)
    HostEngine.calls = 0
    plain = generation_guidance._atoms(x, one_hot, mask, DATASET, HostEngine())
    assert HostEngine.calls == 0 and "kekule_count" not in plain
    got = generation_guidance._atoms(x, one_hot, mask, DATASET, HostEngine(), aromaticity=True)
    assert set(got) == set(plain) | {"kekule_count", "clar"} and np.array_equal(got["kekule_count"], kc)
    assert got["clar"][keep].tolist() == cl.tolist() and got["clar"][3] == 0
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance._evaluate(None, None, None, None, None, 1.0, x, one_hot, mask, None, 1.0, aromaticity=True)
