"""Hueckel levels, gaps, charges and bond orders (csrc/huckel.inc) on the kernel's HOST build: against an oracle restated in
Python with float64 numpy.linalg.eigh (tests/huckel_helpers.py) on golden g32, the closed forms, the sizes at which the rotation
schedule and the capacity tiers change, every refusal, renumbering, the parameter table, the declarations and the layers on top.
tests/test_gpu_huckel.py holds the device to this build bit for bit.

Tolerances: float64 eigvalsh is the yardstick; levels, homo, lumo, gap, charges and bond orders agree within
2e-5 |beta| absolute and e_pi within 2e-5 * n_pi.  Measured on this build: levels 9.0e-7, frontier 2.6e-7, e_pi / n_pi 3.4e-7,
charges 2.0e-6, bond orders 1.4e-6 over g32; 1.2e-6 on the 128-centre path."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import C, H, fixture, pack, relabel
from tests.huckel_helpers import (ATOMS, B_, BAD_INPUT, BAD_TABLE, DATASET, DEGENERATE, EMPTY, N_, NO_PI, O_, OK, OPEN_SHELL,
                                  OVERFLOW, S_, SIZES, TOL, HostEngine, benzene, c_tables, g32_host, g32_oracle, host, ladder,
                                  naphthalene, oracle, path, polyene, ring, row, assert_rows_equal, size_molecules, table, with_h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g32():
    return fixture()


def compare(out, i, ref, n_atoms, n_bonds, vectors):
    """Row i of the host build's outputs against one oracle result."""
    assert out["status"][i] == ref["status"], i
    n = ref["n_pi"]
    assert (out["n_pi"][i], out["n_electrons"][i], out["n_excluded"][i]) == (n, ref["n_electrons"], ref["n_excluded"]), i
    assert bool(out["flags"][i] & OPEN_SHELL) == ref["open_shell"], i
    if ref["status"] != OK:
        for k in _lib.HUCKEL_ARRAYS:
            assert k == "status" or not out[k][i].any(), (i, k)  # a refused molecule's rows are zero
        return np.zeros(5)
    assert np.array_equal(out["site_class"][i, :n_atoms], ref["site_class"]), i
    assert np.array_equal(out["occupation"][i, :n], ref["occupation"]) and not out["occupation"][i, n:].any(), i
    assert not out["levels"][i, n:].any(), i
    if not 5e-4 <= ref["spacing"] <= 2e-3:
        assert bool(out["flags"][i] & DEGENERATE) == (ref["spacing"] < 1e-3), i
    err = np.zeros(5)
    err[0] = np.abs(out["levels"][i, :n] - ref["levels"]).max()
    err[1] = max(abs(out[k][i] - ref[k]) for k in ("homo", "lumo", "gap"))
    err[2] = abs(out["e_pi"][i] - ref["e_pi"]) / n
    assert err[:3].max() <= TOL, (i, err)
    assert abs(np.float32(out["homo"][i] - out["lumo"][i]) - out["gap"][i]) == 0.0
    if vectors:
        err[3] = np.abs(out["pi_charge"][i, :n_atoms] - ref["pi_charge"]).max()
        err[4] = np.abs(out["pi_bond_order"][i, :n_bonds] - ref["pi_bond_order"]).max()
        assert err[3:].max() <= TOL, (i, err)
        assert not out["pi_charge"][i, n_atoms:].any() and not out["pi_bond_order"][i, n_bonds:].any()
    return err


def test_g32_levels(g32):
    out, refs = g32_host(), g32_oracle()
    worst = np.zeros(5)
    for m, ref in zip(g32[1], refs):
        worst = np.maximum(worst, compare(out, m["index"], ref, len(m["elem"]), len(m["bonds"]), False))
    print("g32 max |error|: levels %.3g  homo/lumo/gap %.3g  e_pi / n_pi %.3g" % tuple(worst[:3]))
    st = np.bincount(out["status"], minlength=7)
    assert st[OK] >= 490 and st[BAD_INPUT] >= 1 and st[OVERFLOW] >= 1 and st[EMPTY] >= 1 and st[NO_PI] >= 1
    assert 1 <= out["sweeps"][out["status"] == OK].max() <= _lib.HUCKEL_MAX_SWEEPS // 2


def test_g32_charges_and_bond_orders(g32):
    out, refs = g32_host(), g32_oracle()
    even = [m for m, r in zip(g32[1], refs) if r["status"] == OK and not r["open_shell"]]
    kept = [m for m in even if refs[m["index"]]["gap"] >= 0.02 and out["flags"][m["index"]] == 0]
    assert len(even) >= 300 and len(even) - len(kept) <= 0.05 * len(even), (len(even), len(kept))
    worst = np.zeros(5)
    for m in kept:
        worst = np.maximum(worst, compare(out, m["index"], refs[m["index"]], len(m["elem"]), len(m["bonds"]), True))
    print("g32 max |error|: pi charge %.3g  pi bond order %.3g  (%d of %d even-electron molecules)" % (worst[3], worst[4], len(kept), len(even)))
    for m in kept[::7]:  # what a neutral closed shell conserves: the charges sum to zero, hydrogens carry none
        i, n = m["index"], len(m["elem"])
        assert abs(out["pi_charge"][i, :n].sum()) <= TOL * out["n_pi"][i] and not out["pi_charge"][i, :n][m["elem"] == H].any()


def test_benzene_and_naphthalene():
    out = host([benzene(), naphthalene()])
    assert out["status"].tolist() == [OK, OK] and out["n_pi"].tolist() == [6, 10] and out["flags"].tolist() == [0, 0]
    assert np.abs(out["levels"][0, :6] - [2, 1, 1, -1, -1, -2]).max() <= TOL and abs(out["gap"][0] - 2.0) <= TOL
    assert np.abs(out["pi_bond_order"][0, :6] - 2.0 / 3.0).max() <= TOL and np.abs(out["pi_charge"][0, :6]).max() <= TOL
    assert abs(out["e_pi"][0] - 8.0) <= 6 * TOL and out["occupation"][0, :6].tolist() == [2, 2, 2, 0, 0, 0]
    assert abs(out["gap"][1] - 1.236068) <= TOL and abs(out["homo"][1] - 0.618034) <= TOL and abs(out["lumo"][1] + 0.618034) <= TOL


@pytest.mark.parametrize("n", [2, 3, 7, 32])
def test_a_carbon_path(n):
    out = host([polyene(n)])
    want = 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))
    assert out["status"][0] == OK and out["n_pi"][0] == n and out["n_electrons"][0] == n and out["n_excluded"][0] == 0
    assert np.abs(out["levels"][0, :n] - want).max() <= TOL
    assert bool(out["flags"][0] & OPEN_SHELL) == bool(n % 2)
    if n % 2:
        assert out["homo"][0] == out["lumo"][0] and out["gap"][0] == 0.0 and abs(out["homo"][0]) <= TOL
        assert out["occupation"][0, :n].tolist() == [2] * (n // 2) + [1] + [0] * (n // 2)
    else:
        assert abs(out["gap"][0] - 4.0 * np.cos(n / 2 * np.pi / (n + 1))) <= TOL


def test_electron_counts_by_site():
    cyclobutadiene = ring([C] * 4)
    pyridine, pyrrole = ring([C] * 5 + [N_]), with_h(*ring([C] * 4 + [N_]), [0, 0, 0, 0, 1])
    borabenzene, borane = ring([C] * 5 + [B_]), with_h(*ring([C] * 5 + [B_]), [0, 0, 0, 0, 0, 1])
    furan, thiophene = ring([C] * 4 + [O_]), ring([C] * 4 + [S_])
    carbonyl = with_h(np.array([C, O_], np.int32), np.array([(0, 1)], np.int32), [2, 0])
    oxonium = with_h(*ring([C] * 4 + [O_]), [0, 0, 0, 0, 1])  # a three-coordinate O is no pi centre
    mols = [cyclobutadiene, pyridine, pyrrole, borabenzene, borane, furan, thiophene, carbonyl, oxonium]
    out = host(mols)
    names = list(table()["classes"])
    assert out["status"].tolist() == [OK] * 9
    assert out["n_pi"].tolist() == [4, 6, 5, 6, 6, 5, 5, 2, 4] and out["n_excluded"].tolist() == [0] * 8 + [1]
    assert out["n_electrons"].tolist() == [4, 6, 6, 6, 5, 6, 6, 2, 4]
    assert out["flags"].tolist() == [DEGENERATE, 0, 0, 0, OPEN_SHELL, 0, 0, 0, 0]
    hetero = [names[out["site_class"][i, len(m[0][m[0] != H]) - 1]] for i, m in enumerate(mols[1:8], 1)]
    assert hetero == ["N.", "N:", "B.", "B", "O:", "S:", "O."]
    assert out["site_class"][8, 4] == -1 and out["site_class"][2, 5] == -1 and out["pi_charge"][8, 4] == 0.0
    for i, m in enumerate(mols):
        compare(out, i, oracle(m), len(m[0]), len(m[1]), i not in (0, 4))
    assert out["pi_charge"][1, 5] < -0.05 < 0.05 < out["pi_charge"][2, 4]  # pyridine's N pulls density in, pyrrole's N gives it


def test_hydrogens_listed_or_implied_give_the_same_bits():
    e, b = naphthalene()
    counts = [0 if a in (0, 5) else 1 for a in range(10)]
    placed = with_h(e, b, counts)  # appended after the other atoms
    k = sum(counts)  # template-like: the hydrogens first, their bonds first
    front = (np.concatenate([np.full(k, H, np.int32), e]),
             np.concatenate([np.array([(j, k + a) for j, a in enumerate(a for a in range(10) if counts[a])], np.int32), b + k]))
    out = host([(e, b), placed, front])
    assert out["status"].tolist() == [OK] * 3
    for name in ("levels", "occupation", "n_pi", "n_electrons", "n_excluded", "sweeps", "flags", "homo", "lumo", "gap", "e_pi"):
        assert out[name][0].tobytes() == out[name][1].tobytes() == out[name][2].tobytes(), name
    assert out["pi_charge"][0, :10].tobytes() == out["pi_charge"][1, :10].tobytes() == out["pi_charge"][2, k:k + 10].tobytes()
    assert out["pi_bond_order"][0, :11].tobytes() == out["pi_bond_order"][1, :11].tobytes() == out["pi_bond_order"][2, k:k + 11].tobytes()
    assert not out["pi_bond_order"][1, 11:].any() and not out["pi_bond_order"][2, :k].any() and (out["site_class"][2, :k] == -1).all()


def test_a_charge_moves_the_electron_count():
    out = host([benzene()] * 5, charge=[0, 1, -1, 13, -7])
    assert out["status"].tolist() == [OK, OK, OK, BAD_INPUT, BAD_INPUT]
    assert out["n_electrons"].tolist() == [6, 5, 7, 0, 0] and out["flags"].tolist() == [0, OPEN_SHELL, OPEN_SHELL | DEGENERATE, 0, 0]
    assert out["occupation"][1, :6].tolist() == [2, 2, 1, 0, 0, 0] and out["occupation"][2, :6].tolist() == [2, 2, 2, 1, 0, 0]
    assert abs(out["homo"][1] - 1.0) <= TOL and out["homo"][1] == out["lumo"][1] and abs(out["homo"][2] + 1.0) <= TOL and out["gap"][2] == 0.0
    assert abs(out["pi_charge"][1, :6].sum() - 1.0) <= 6 * TOL and abs(out["pi_charge"][2, :6].sum() + 1.0) <= 6 * TOL
    for i, ch in enumerate((0, 1, -1, 13, -7)):
        compare(out, i, oracle(benzene(), charge=ch), 6, 6, False)
    full = host([benzene()] * 2, charge=[6, -6])  # no electron, no empty level: both names on one level, gap zero
    assert full["status"].tolist() == [OK, OK] and full["n_electrons"].tolist() == [0, 12] and full["gap"].tolist() == [0.0, 0.0]
    assert abs(full["homo"][0] - 2.0) <= TOL and abs(full["lumo"][1] + 2.0) <= TOL and abs(full["e_pi"][0]) == 0.0


def test_sizes_where_the_schedule_and_the_tiers_change():
    mols = size_molecules()
    out = host(mols)
    assert out["status"].tolist() == [OK] * len(SIZES) and out["n_pi"].tolist() == list(SIZES)
    for i, n in enumerate(SIZES):
        want = 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))
        assert np.abs(out["levels"][i, :n] - want).max() <= TOL, n
        assert bool(out["flags"][i] & OPEN_SHELL) == bool(n % 2), n
        compare(out, i, oracle(mols[i]), len(mols[i][0]), len(mols[i][1]), n % 2 == 0 and n <= 64)
        alone = host([mols[i]])  # the tier and the batch leave no trace
        assert_rows_equal(row(alone, 0, len(mols[i][0]), len(mols[i][1])), row(out, i, len(mols[i][0]), len(mols[i][1])))
    assert out["sweeps"].max() <= 12 and out["sweeps"][0] == 0


def test_refusals_leave_zero_rows():
    methane = with_h(np.array([C], np.int32), np.zeros((0, 2), np.int32), [4])
    lone_h = (np.array([H], np.int32), np.zeros((0, 2), np.int32))
    star = (np.array([C] * 10, np.int32), np.array([(0, k) for k in range(1, 10)], np.int32))
    cases = [(polyene(129), OVERFLOW), (ladder(192), OVERFLOW), (methane, NO_PI), (path(2), NO_PI), (lone_h, NO_PI),
             ((np.zeros(0, np.int32), np.zeros((0, 2), np.int32)), EMPTY),
             ((np.array([C, C], np.int32), np.array([(0, 2)], np.int32)), BAD_INPUT),
             ((np.array([C, C], np.int32), np.array([(0, -1)], np.int32)), BAD_INPUT),
             ((np.array([C, C], np.int32), np.array([(1, 1)], np.int32)), BAD_INPUT),
             ((np.array([C, C], np.int32), np.array([(0, 1), (1, 0)], np.int32)), BAD_INPUT),
             ((np.array([C, 6], np.int32), np.array([(0, 1)], np.int32)), BAD_INPUT),
             ((np.array([C, -1], np.int32), np.array([(0, 1)], np.int32)), BAD_INPUT),
             (star, OVERFLOW), (ladder(193), OVERFLOW), (with_h(*path(2), [8, 0]), OVERFLOW),
             ((np.full(385, H, np.int32), np.zeros((0, 2), np.int32)), OVERFLOW),
             ((np.array([C] * 2 + [H] * 4, np.int32), np.array([(k % 2, 2 + k % 4) for k in range(385)], np.int32)), OVERFLOW)]
    mols = [benzene()] + [m for m, _ in cases] + [naphthalene()]
    out = host(mols)
    assert out["status"].tolist() == [OK] + [s for _, s in cases] + [OK]
    for k in _lib.HUCKEL_ARRAYS:
        if k != "status":
            assert not out[k][1:-1].any(), k
    alone = host([benzene(), naphthalene()])  # ... and never disturb their neighbours
    assert_rows_equal(row(out, 0, 6, 6), row(alone, 0, 6, 6))
    assert_rows_equal(row(out, len(mols) - 1, 10, 11), row(alone, 1, 10, 11))
    for (m, status) in cases[:6]:
        assert oracle(m)["status"] == status


def test_renumbering(g32):
    out, refs = g32_host(), g32_oracle()
    picked = [m for m in g32[1] if refs[m["index"]]["status"] == OK][5::37]
    assert len(picked) >= 10
    perms = [np.random.default_rng(8300 + k).permutation(len(m["elem"])) for k, m in enumerate(picked)]
    moved = [relabel(m, np.random.default_rng(8300 + k)) for k, m in enumerate(picked)]
    again = host(moved)
    for k, (m, perm) in enumerate(zip(picked, perms)):
        i, n, na = m["index"], out["n_pi"][m["index"]], len(m["elem"])
        assert again["status"][k] == OK
        for name in ("n_pi", "n_electrons", "n_excluded"):
            assert again[name][k] == out[name][i]
        assert np.array_equal(again["occupation"][k], out["occupation"][i])
        assert np.array_equal(again["site_class"][k, :na][perm], out["site_class"][i, :na])
        # both are within TOL of the same exact values: twice that apart at most
        assert np.abs(again["levels"][k, :n] - out["levels"][i, :n]).max() <= 2 * TOL and abs(again["gap"][k] - out["gap"][i]) <= 2 * TOL
        ref = refs[i]
        if not ref["open_shell"] and ref["gap"] >= 0.02:
            assert np.abs(again["pi_charge"][k, :na][perm] - out["pi_charge"][i, :na]).max() <= 2 * TOL
            compare(again, k, oracle(moved[k]), na, len(m["bonds"]), True)


def test_the_table_and_parameters():
    from gaudi_amd import huckel
    T = table()
    assert "Streitwieser" in T["source"] and "No source can be consulted" in T["source"]
    want = {("C", 3): ("C", 0, 1, 1), ("B", 2): ("B.", -1.0, 1, 0.7), ("B", 3): ("B", -1.0, 0, 0.7), ("N", 2): ("N.", 0.5, 1, 1.0),
            ("N", 3): ("N:", 1.5, 2, 0.8), ("O", 1): ("O.", 1.0, 1, 1.0), ("O", 2): ("O:", 2.0, 2, 0.8), ("S", 2): ("S:", 1.11, 2, 0.69)}
    got = {(sym, int(c)): (name, T["classes"][name]["h"], T["classes"][name]["n_e"], T["classes"][name]["k"])
           for sym, by in T["sites"].items() for c, name in by.items()}
    assert got == want
    t = c_tables()
    assert (t.n_elems, t.h_elem, t.c_elem, t.n_classes) == (6, 0, 1, 8)
    names = list(T["classes"])
    for e, sym in enumerate(ATOMS):
        for c in range(5):
            assert t.site_class[e][c] == (names.index(want[(sym, c)][0]) if (sym, c) in want else -1)
    assert all(np.isnan(t.k_pair[i][j]) for i in range(16) for j in range(16))
    assert huckel.c_huckel_tables("cata").n_elems == 2 and set(huckel.tables("cata")["sites"]) == {"C"}
    # overrides reach the result: every k doubled doubles a hydrocarbon's levels
    base = host([naphthalene()])
    double = host([naphthalene()], parameters={"classes": {n: {"k": 2.0 * T["classes"][n]["k"]} for n in names}})
    # (M_rs = k_r k_s, so doubling EVERY k multiplies a hydrocarbon's matrix, and its levels, by 2 * 2; doubling the bond element
    # itself, through k_pair, multiplies them by 2)
    assert np.abs(double["levels"][0, :10] - 4.0 * base["levels"][0, :10]).max() <= 4 * TOL
    assert np.abs(double["levels"][0, :10] - oracle(naphthalene(), scale_k=2.0)["levels"]).max() <= TOL
    pair = host([naphthalene()], parameters={"k_pair": {"C|C": 2.0}})
    assert np.abs(pair["levels"][0, :10] - 2.0 * base["levels"][0, :10]).max() <= 2 * TOL
    shifted = host([naphthalene()], parameters={"classes": {"C": {"h": 0.25}}})
    assert np.abs(shifted["levels"][0, :10] - (base["levels"][0, :10] + 0.25)).max() <= TOL
    gone = host([naphthalene()], parameters={"sites": {"C": {3: None}}})
    assert gone["status"][0] == NO_PI
    new = host([ring([C] * 5 + [N_])], parameters={"classes": {"N+": {"h": 2.0, "n_e": 1, "k": 1.0}}, "sites": {"N": {2: "N+"}}})
    assert new["status"][0] == OK and new["site_class"][0, 5] == 8 and new["n_electrons"][0] == 6
    with pytest.raises(_lib.GaudiError):
        huckel.c_huckel_tables(DATASET, {"sites": {"N": {2: "nothing"}}})
    with pytest.raises(_lib.GaudiError):
        huckel.c_huckel_tables(DATASET, {"levels": {}})


def test_a_table_that_cannot_be_read():
    mols = pack([benzene(), naphthalene()])
    for change in ("class", "negative", "count", "electrons", "pair", "nan"):
        t = c_tables()
        if change == "class":
            t.site_class[C][3] = t.n_classes
        elif change == "negative":
            t.site_class[S_][2] = -2
        elif change == "count":
            t.n_classes = 17
        elif change == "electrons":
            t.n_e[0] = 3
        elif change == "pair":
            t.k_pair[0][1], t.k_pair[1][0] = 1.0, 2.0
        else:
            t.h[0] = float("nan")
        out = _lib.host_huckel(t, *mols)
        assert out["status"].tolist() == [BAD_TABLE, BAD_TABLE], change
        assert not any(out[k].any() for k in _lib.HUCKEL_ARRAYS if k != "status"), change


def test_declarations_and_argument_checks():
    import ctypes as Ct
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    assert "#define GAUDI_ABI_VERSION 7" in header and lib.gaudi_abi_version() == 7
    added = re.search(r"\(Entry points ADDED since(.*?)\*/", header, re.S).group(1)
    ctype = {"int": Ct.c_int, "gaudi_handle*": Ct.c_void_p, "const int32_t*": _lib.IP, "int32_t*": _lib.IP, "float*": _lib.FP,
             "uint8_t*": Ct.POINTER(Ct.c_uint8), "int8_t*": Ct.POINTER(Ct.c_int8), "double*": Ct.POINTER(Ct.c_double),
             "const gaudi_huckel_tables*": Ct.POINTER(_lib.HuckelTables)}
    for name in ("gaudi_huckel", "gaudi_host_huckel", "gaudi_huckel_profile_get"):
        assert re.search(r"\b" + name + r"\b", added), name
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, name
        args = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).replace("\n", " ").split(",")]
        assert _lib.EXPORTS[name] == (Ct.c_int, args), name
        assert hasattr(lib, name)
    for k, v in (("MAX_PI", 128), ("MAX_CLASSES", 16), ("MAX_SWEEPS", _lib.HUCKEL_MAX_SWEEPS), ("OK", 0), ("NOT_CONVERGED", 1),
                 ("BAD_INPUT", 2), ("OVERFLOW", 3), ("EMPTY", 4), ("NO_PI", 5), ("BAD_TABLE", 6), ("OPEN_SHELL", 1), ("DEGENERATE", 2)):
        assert re.search(rf"#define GAUDI_HUCKEL_{k} +{v}\b", header) and getattr(_lib, "HUCKEL_" + k) == v, k
    assert Ct.sizeof(_lib.HuckelTables) == 4 * (4 + 40 + 16 * 3 + 256)
    mols = pack([benzene(), naphthalene()])
    out = _lib.huckel_outputs(2, mols[0].shape[1], mols[2].shape[1])
    args = list(_lib.huckel_args(c_tables(), *mols, None, out))
    assert lib.gaudi_host_huckel(*args) == 0 and out["status"].tolist() == [OK, OK]
    for at, value in [(0, None), (1, -1), (2, 0), (3, 0), (4, None), (5, None), (6, None), (7, None)] + [(k, None) for k in range(9, 24)]:
        broken = list(args)
        broken[at] = value
        assert lib.gaudi_host_huckel(*broken) == -1, at
    for field, value in (("n_elems", 9), ("n_elems", 0), ("h_elem", 6), ("c_elem", -1)):
        t = c_tables()
        setattr(t, field, value)
        assert lib.gaudi_host_huckel(Ct.byref(t), *args[1:]) == -1, field
    assert lib.gaudi_host_huckel(*(args[:1] + [0] + args[2:])) == 0  # B = 0


def test_orbitals_gap_and_the_layers_on_top(g32, monkeypatch):
    import torch
    import gaudi_amd.gor2goa as G
    from gaudi_amd import analyze, generation_guidance, huckel
    refs = g32_oracle()
    mols = [m for m in g32[1] if refs[m["index"]]["status"] == OK][3::40]
    recs = [dict(status=0, atom_types=m["elem"], bonds=m["bonds"], fingerprint=1000 + k) for k, m in enumerate(mols)]
    recs.insert(2, dict(status=2, fingerprint=0))
    keep = [k for k in range(len(recs)) if k != 2]
    raw = host(mols)
    orbs = huckel.orbitals(recs, DATASET, engine=HostEngine())
    assert len(orbs) == len(recs) and orbs[2]["status"] == EMPTY and len(orbs[2]["levels"]) == 0 and len(orbs[2]["pi_charge"]) == 0
    for j, k in enumerate(keep):
        o, m = orbs[k], mols[j]
        n = raw["n_pi"][j]
        assert o["status"] == OK and o["n_pi"] == n and o["levels"].tobytes() == raw["levels"][j, :n].tobytes()
        assert o["gap"] == float(raw["gap"][j]) and o["homo"] == float(raw["homo"][j]) and o["e_pi"] == float(raw["e_pi"][j])
        assert o["pi_charge"].tobytes() == raw["pi_charge"][j, :len(m["elem"])].tobytes() and len(o["pi_bond_order"]) == len(m["bonds"])
        assert o["open_shell"] == bool(raw["flags"][j] & OPEN_SHELL) and o["degenerate"] == bool(raw["flags"][j] & DEGENERATE)
        assert len(o["site_class"]) == len(m["elem"]) and len(o["occupation"]) == n
    gaps = huckel.gap(recs, DATASET, engine=HostEngine())
    assert gaps.dtype == np.float64 and np.isnan(gaps[2]) and np.array_equal(gaps[keep], raw["gap"].astype(np.float64))
    pairs = [(m["elem"], m["bonds"]) for m in mols]
    assert np.array_equal(huckel.gap(pairs, DATASET, engine=HostEngine()), gaps[keep])
    plus = huckel.orbitals(pairs[:3], DATASET, charge=[0, 1, -1], engine=HostEngine())
    assert [p["n_electrons"] - o["n_electrons"] for p, o in zip(plus, [orbs[k] for k in keep[:3]])] == [0, -1, 1]
    assert huckel.orbitals(pairs[:2], DATASET, charge=1, engine=HostEngine())[1]["n_electrons"] == plus[1]["n_electrons"]
    wide = huckel.gap(pairs[:2], DATASET, parameters={"classes": {"C": {"k": 2.0}}}, engine=HostEngine())
    assert not np.array_equal(wide, gaps[keep][:2])
    assert huckel.orbitals([], DATASET, engine=HostEngine()) == [] and huckel.gap([], DATASET, engine=HostEngine()).shape == (0,)
    with pytest.raises(_lib.GaudiError):
        huckel.gap(pairs[:2], DATASET, charge=[0, 0, 0], engine=HostEngine())
    assert set(huckel.STATUS_NAMES) == set(range(7))
    a, b = huckel.calibrate([1.0, 2.0, 3.0, 4.0], [3.5, 5.5, 7.5, 9.5])
    assert abs(a - 1.5) < 1e-9 and abs(b - 2.0) < 1e-9
    with pytest.raises(_lib.GaudiError):
        huckel.calibrate([1.0, 1.0], [2.0, 3.0])

    class Engine(HostEngine):
        calls = 0

        def huckel(self, *a):
            Engine.calls += 1
            return HostEngine.huckel(self, *a)

    def fake(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None, **kw):
        out = [dict(r) for r in recs]
        if kw.get("huckel"):
            for r, extra in zip(out, huckel.record_fields(out, dataset, engine=engine)):
                r.update(extra)
        return out

    monkeypatch.setattr(G, "rings_to_atoms", fake)
    given = [(np.zeros((1, 3), np.float32), np.zeros(1, np.int64)) for _ in recs]
    plain, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Engine())
    assert Engine.calls == 0 and not any(k.startswith("huckel") for k in plain)
    d, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Engine(), huckel=True)
    assert Engine.calls == 1 and set(d) == set(plain) | {"huckel_gap", "huckel_open_shell_fraction"}
    assert all(np.array_equal(d[k], plain[k]) for k in plain)
    assert np.array_equal(d["huckel_gap"], gaps[keep])  # over the built molecules
    assert d["huckel_open_shell_fraction"] == sum(bool(f & OPEN_SHELL) for f in raw["flags"]) / len(mols)
    fields = huckel.record_fields(recs, DATASET, engine=HostEngine())
    assert fields[2]["huckel_status"] == EMPTY and set(fields[0]) == {"huckel_gap", "huckel_homo", "huckel_lumo", "huckel_flags", "huckel_status"}
    assert [f["huckel_gap"] for f in fields if f["huckel_status"] == OK] == raw["gap"].astype(np.float64).tolist()
    # what design / design_sweep / refine add after sampling (the sampling itself needs a device: tests/test_gpu_huckel.py)
    n = len(recs)
    x, one_hot, mask = torch.zeros(n, 2, 3), torch.zeros(n, 2, 4), torch.ones(n, 2, 1)
    Engine.calls = 0
    plain = generation_guidance._atoms(x, one_hot, mask, DATASET, Engine())
    assert Engine.calls == 0 and "huckel_gap" not in plain
    got = generation_guidance._atoms(x, one_hot, mask, DATASET, Engine(), huckel=True)
    assert set(got) == set(plain) | {"huckel_gap"} and np.array_equal(got["huckel_gap"], gaps, equal_nan=True)
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance._evaluate(None, None, None, None, None, 1.0, x, one_hot, mask, None, 1.0, huckel=True)


def test_the_host_build_under_the_sanitizers():
    """tools/huckel_host_check.py: the stand-alone program only (never code loaded into python)."""
    import glob
    if not glob.glob(os.path.join(ROOT, "gaudi_amd", "csrc", "build", "kern*.o")):  # the program links the ordinary build's kernel objects
        from gaudi_amd.build import build
        build(force=True)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "huckel_host_check.py")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "exit status 0 (clean)" in run.stdout and "own inputs: status counts" in run.stdout
