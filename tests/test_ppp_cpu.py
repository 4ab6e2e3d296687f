"""PPP self-consistent pi levels, gaps, charges and bond orders (csrc/ppp.inc) on the kernel's HOST build: against a float64
oracle restated in numpy (tests/ppp_helpers.py) on golden g30, the hand-made molecules and the tier-edge set; physics that needs
no oracle; invariance; every refusal; the declarations and the layers on top.  tests/test_gpu_ppp.py holds the device to this build
bit for bit.

Tolerances (tests/ppp_helpers.py): measured on this build against the fixed point, levels / homo / lumo /
gap / e_electronic per centre 7.25e-5 eV and charges / bond orders 2.88e-5 over g30 and the tier-edge set; the tests hold four
times that, TOL_EV = 2.9e-4 eV and TOL_P = 1.152e-4."""
import os
import re

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import H
from tests.ppp_helpers import (BAD_GEOMETRY, BAD_INPUT, BAD_TABLE, CAP, DATASET, DEGENERATE, EDGE_SIZES, EMPTY, JACOBI_CAP,
                               NOT_CONVERGED, OK, OPEN_SHELL, OVERFLOW, SCF_CAP, TOL_EV, TOL_P, HostEngine, assert_rows_equal,
                               benzene, c_tables, chain_molecule, edge_host_one, edge_oracle_one, edge_set, errors, g30_host,
                               g30_molecules, g30_oracle, hand_made, host, naphthalene, oracle, pack, phenacene, pyridine, row)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_values(out, refs, mols):
    """Every converged molecule against the fixed point -> the number compared."""
    seen = 0
    for i, (ref, mol) in enumerate(zip(refs, mols)):
        if ref["status"] != OK or out["status"][i] != OK or not ref["fixed"]:
            continue
        n, na, nb = ref["n_pi"], len(mol[0]), len(mol[1])
        assert (out["n_pi"][i], out["n_electrons"][i], out["n_excluded"][i]) == (n, ref["n_electrons"], ref["n_excluded"]), i
        assert np.array_equal(out["site_class"][i, :na], ref["site_class"]), i
        assert np.array_equal(out["occupation"][i, :n], ref["occupation"]) and not out["occupation"][i, n:].any(), i
        assert not out["levels"][i, n:].any() and (np.diff(out["levels"][i, :n]) >= 0).all(), i
        ev, p = errors(out, i, ref, mol)
        print(f"molecule {i}: n_pi {n}, iterations {out['iterations'][i]}, error {ev:.3g} eV, {p:.3g} in P, gap {ref['gap']:.3f}")
        assert ev <= TOL_EV, (i, ev)
        if ref["gap"] >= 0.1:
            assert p <= TOL_P, (i, p)
        assert abs(out["e_core"][i] - ref["e_core"]) <= TOL_EV * max(1.0, abs(ref["e_core"]) * 1e-3), i  # (a sum of n^2 / 2 terms of order 5 eV)
        assert out["gap"][i] == np.float32(out["lumo"][i] - out["homo"][i]) and out["gap"][i] >= 0
        assert not out["pi_charge"][i, na:].any() and not out["pi_bond_order"][i, nb:].any()
        assert 0 < out["delta_p"][i] <= 2.0 ** -16 and out["sweeps"][i] >= out["iterations"][i]
        seen += 1
    return seen


def test_g30_statuses_and_iterations():
    out, refs = g30_host(), g30_oracle()
    closed = [i for i, r in enumerate(refs) if r["status"] in (OK, NOT_CONVERGED)]
    decisive = [i for i in closed if refs[i]["decisive"]]
    assert len(closed) >= 150 and len(closed) - len(decisive) <= 0.02 * len(closed)
    for i, r in enumerate(refs):
        if r["status"] in (OK, NOT_CONVERGED) and not r["decisive"]:
            continue
        assert out["status"][i] == r["status"], i
        if r["status"] == OK:
            assert abs(int(out["iterations"][i]) - r["iterations"]) <= 2, i
            assert not out["flags"][i] & (SCF_CAP | JACOBI_CAP)
        elif r["status"] == NOT_CONVERGED:
            assert out["iterations"][i] == CAP and out["flags"][i] & SCF_CAP and out["delta_p"][i] > 2.0 ** -16
            assert np.isfinite(out["levels"][i]).all() and out["n_pi"][i] == r["n_pi"]
        else:
            for k in _lib.PPP_ARRAYS:
                assert k == "status" or not out[k][i].any(), (i, k)  # a refused molecule's rows are zero
    st = np.bincount(out["status"], minlength=9)
    assert st[OK] >= 150 and st[NOT_CONVERGED] >= 1 and st[OPEN_SHELL] >= 1


def test_g30_values():
    assert check_values(g30_host(), g30_oracle(), g30_molecules()) >= 150


@pytest.mark.parametrize("k", range(len(EDGE_SIZES)), ids=[str(n) for n in EDGE_SIZES])
def test_a_tier_edge_molecule(k):
    mols, charge = edge_set()
    out, ref = edge_host_one(k), edge_oracle_one(k)
    assert out["n_pi"][0] == EDGE_SIZES[k] and out["status"][0] == OK and out["n_electrons"][0] == EDGE_SIZES[k] - charge[k]
    assert abs(int(out["iterations"][0]) - ref["iterations"]) <= 2 and ref["decisive"]
    assert check_values(out, [ref], [mols[k]]) == 1


@pytest.mark.parametrize("repulsion", ["mataga-nishimoto", "ohno"])
def test_the_hand_made_molecules(repulsion):
    made = hand_made()
    mols, charge = [m for m, _ in made.values()], np.array([c for _, c in made.values()], np.int32)
    out = host(mols, charge, repulsion=["mataga-nishimoto", "ohno"].index(repulsion))
    refs = [oracle(m, int(c), repulsion) for m, c in zip(mols, charge)]
    assert out["status"].tolist() == [OK] * len(mols) == [r["status"] for r in refs]
    assert out["n_pi"].tolist() == [2, 3, 6, 10, 6, 5, 5, 5, 6] and out["n_electrons"].tolist() == [2, 2, 6, 10, 6, 6, 6, 6, 6]
    assert check_values(out, refs, mols) == len(mols)


def test_physics_that_needs_no_oracle():
    mols = [benzene(), naphthalene(), phenacene(3), phenacene(7), phenacene(15)]
    out = host(mols)
    assert (out["status"] == OK).all()
    for i, m in enumerate(mols):  # neutral alternant hydrocarbons: no charge anywhere, levels paired about one centre
        n = out["n_pi"][i]
        lev = out["levels"][i, :n].astype(np.float64)
        assert np.abs(out["pi_charge"][i]).max() <= TOL_P, i
        sums = lev + lev[::-1]
        assert np.ptp(sums) <= 2 * TOL_EV, (i, np.ptp(sums))
    lev = out["levels"][0, :6]
    assert abs(lev[1] - lev[2]) <= TOL_EV and abs(lev[3] - lev[4]) <= TOL_EV and lev[2] - lev[0] > 1.0 and lev[3] - lev[2] > 5.0
    assert not out["flags"][0] & DEGENERATE  # (the frontier PAIRS are degenerate, homo and lumo are not)
    py = host([pyridine()])
    assert py["pi_charge"][0, 0] < -0.05 and abs(py["pi_charge"][0, :6].sum()) <= 6 * TOL_P
    ohno = host(mols[:2], repulsion=1)
    assert (ohno["status"] == OK).all() and (np.abs(ohno["gap"] - out["gap"][:2]) > 0.5).all()
    assert np.allclose(out["e_core"][0], ohno["e_core"][0], atol=30) and out["e_core"][0] != ohno["e_core"][0]


def test_the_batch_the_place_and_the_padding_leave_no_trace():
    mols, charge = edge_set()
    pick = np.random.default_rng(5).permutation([0, 1, 2, 3, 4, 5, 6, 7, 8, 11])  # every tier; one of the 128-centre molecules
    moved = host([mols[k] for k in pick], charge[pick], A=400, M=390)
    for j, k in enumerate(pick):
        na, nb = len(mols[k][0]), len(mols[k][1])
        assert_rows_equal(row(moved, j, na, nb), row(edge_host_one(k), 0, na, nb))


def test_rigid_motion_and_renumbering():
    rng = np.random.default_rng(11)
    mols = [g30_molecules()[k] for k in (3, 40, 90, 150)] + [pyridine(), phenacene(7, 2)]
    base = host(mols)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    turned = host([(e, b, np.asarray(x) @ q.T + np.array([3.0, -7.0, 11.0])) for e, b, x in mols])
    shuffled = []
    for e, b, x in mols:
        perm = rng.permutation(len(e))  # new index of old atom a: perm[a]
        inv = np.argsort(perm)
        shuffled.append((e[inv], perm[np.asarray(b)], np.asarray(x)[inv]))
    renum = host(shuffled)
    for other in (turned, renum):
        assert other["status"].tolist() == base["status"].tolist() and other["n_pi"].tolist() == base["n_pi"].tolist()
        ok = base["status"] == OK
        assert ok.sum() >= 5 and np.abs(other["levels"][ok] - base["levels"][ok]).max() <= TOL_EV
        assert np.abs(other["gap"][ok] - base["gap"][ok]).max() <= TOL_EV


def test_refusals_leave_zero_rows():
    ethylene, allyl = chain_molecule(2), chain_molecule(3)
    e, b, x = benzene()
    coincident = (e, b, np.where(np.arange(6)[:, None] == 1, x[0] + [0.3, 0.0, 0.0], x))
    nan_at = (e, b, np.where(np.arange(6)[:, None] == 4, np.nan, x))
    he, hb, hx = ethylene
    h_at_origin = (he, hb, np.where((he == H)[:, None], 0.0, hx))  # template hydrogens parked at the origin are not pi centres
    h_nan = (he, hb, np.where((he == H)[:, None], np.nan, hx))
    big = phenacene(32)  # 130 centres
    empty = (np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 3)))
    mols = [allyl, coincident, nan_at, big, empty, ethylene, h_at_origin, h_nan, allyl]
    out = host(mols, charge=[0, 0, 0, 0, 0, 0, 0, 0, 5])
    assert out["status"].tolist() == [OPEN_SHELL, BAD_GEOMETRY, BAD_GEOMETRY, OVERFLOW, EMPTY, OK, OK, OK, BAD_INPUT]
    for i, st in enumerate(out["status"]):
        if st != OK:
            for k in _lib.PPP_ARRAYS:
                assert k == "status" or not out[k][i].any(), (i, k)
    assert out["levels"][5].tobytes() == out["levels"][6].tobytes() == out["levels"][7].tobytes()
    assert host([allyl], charge=[1])["status"][0] == OK and host([allyl], charge=[-1])["status"][0] == OK
    assert host([ethylene], damping=0.0)["status"][0] == OK  # damping 0 is accepted


def test_a_table_or_a_setting_that_cannot_be_used():
    mols = [benzene(), naphthalene()]
    good = host(mols)
    assert good["status"].tolist() == [OK, OK]
    bad = [{"classes": {"C": {"gamma": 0.0}}}, {"classes": {"C": {"gamma": -1.0}}}, {"classes": {"C": {"gamma": float("nan")}}},
           {"classes": {"C": {"gamma": float("inf")}}}, {"classes": {"C": {"I": float("inf")}}}, {"classes": {"C": {"z": 3}}},
           {"classes": {"C": {"z": -1}}}, {"classes": {"C": {"k": float("nan")}}}, {"beta0": float("nan")},
           {"beta_pair": {"C|C": float("inf")}}]
    for parameters in bad:
        out = host(mols, parameters=parameters)
        assert out["status"].tolist() == [BAD_TABLE, BAD_TABLE], parameters
        assert all(k == "status" or not out[k].any() for k in _lib.PPP_ARRAYS), parameters
    for kw in ({"damping": 1.0}, {"damping": -0.1}, {"damping": float("nan")}, {"repulsion": 2}, {"repulsion": -1}):
        assert host(mols, **kw)["status"].tolist() == [BAD_TABLE, BAD_TABLE], kw
    t = c_tables()
    t.site_class[1][3] = t.n_classes
    assert _lib.host_ppp(t, *pack(mols))["status"].tolist() == [BAD_TABLE, BAD_TABLE]
    t = c_tables()
    t.beta_pair[0][1], t.beta_pair[1][0] = -1.0, -2.0
    assert _lib.host_ppp(t, *pack(mols))["status"].tolist() == [BAD_TABLE, BAD_TABLE]
    t = c_tables()
    t.n_elems = 9
    with pytest.raises(_lib.GaudiError):
        _lib.host_ppp(t, *pack(mols))
    pair = host(mols, parameters={"beta_pair": {"C|C": -2.0}})  # a listed pair replaces the product; a parameter changes the result
    assert pair["status"].tolist() == [OK, OK] and (pair["gap"] < good["gap"] - 0.3).all()
    assert (host(mols, parameters={"beta0": -2.0})["gap"] == pair["gap"]).all()


def test_declarations():
    import ctypes as Ct
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    assert "#define GAUDI_ABI_VERSION 7" in header and lib.gaudi_abi_version() == 7
    added = re.search(r"\(Entry points ADDED since(.*?)\*/", header, re.S).group(1)
    ctype = {"int": Ct.c_int, "float": Ct.c_float, "gaudi_handle*": Ct.c_void_p, "const int32_t*": _lib.IP, "int32_t*": _lib.IP,
             "float*": _lib.FP, "const float*": _lib.FP, "uint8_t*": Ct.POINTER(Ct.c_uint8), "int8_t*": Ct.POINTER(Ct.c_int8),
             "double*": Ct.POINTER(Ct.c_double), "const gaudi_ppp_tables*": Ct.POINTER(_lib.PPPTables)}
    for name in ("gaudi_ppp", "gaudi_host_ppp", "gaudi_ppp_profile_get"):
        assert re.search(r"\b" + name + r"\b", added), name
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, name
        args = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).replace("\n", " ").split(",")]
        assert _lib.EXPORTS[name] == (Ct.c_int, args), name
        assert hasattr(lib, name)
    for k, v in (("MAX_ITERATIONS", 64), ("OPEN_SHELL", 7), ("BAD_GEOMETRY", 8), ("DEGENERATE", 2), ("SCF_CAP", 4), ("JACOBI_CAP", 8),
                 ("MATAGA_NISHIMOTO", 0), ("OHNO", 1)):
        assert re.search(rf"#define GAUDI_PPP_{k} +{v}\b", header) and getattr(_lib, "PPP_" + k) == v, k
    assert Ct.sizeof(_lib.PPPTables) == 4 * (4 + 40 + 16 * 4 + 1 + 256)
    mols = pack([benzene(), naphthalene()])
    out = _lib.ppp_outputs(2, mols[0].shape[1], mols[2].shape[1])
    args = list(_lib.ppp_args(c_tables(), *mols, None, 0, 0.25, out))
    assert lib.gaudi_host_ppp(*args) == 0 and out["status"].tolist() == [OK, OK]
    for at, value in [(0, None), (1, -1), (2, 0), (3, 0), (4, None), (5, None), (6, None), (7, None), (8, None)] + \
                     [(k, None) for k in range(12, 30)]:
        broken = list(args)
        broken[at] = value
        assert lib.gaudi_host_ppp(*broken) == -1, at


def test_orbitals_gap_and_the_layers_on_top(monkeypatch):
    import torch
    import gaudi_amd.gor2goa as G
    from gaudi_amd import analyze, generation_guidance, ppp
    mols = [g30_molecules()[k] for k in (4, 30, 77, 120)] + [chain_molecule(3)]
    raw = host(mols)
    assert raw["status"].tolist() == [OK] * 4 + [OPEN_SHELL]
    recs = [dict(status=0, atom_types=e, bonds=b, atoms3d=np.asarray(x, np.float64), fingerprint=1000 + k) for k, (e, b, x) in enumerate(mols)]
    recs.insert(2, dict(status=2, fingerprint=0))
    keep = [k for k in range(len(recs)) if k != 2]
    orbs = ppp.orbitals(recs, DATASET, engine=HostEngine())
    assert len(orbs) == len(recs) and orbs[2]["status"] == EMPTY and len(orbs[2]["levels"]) == 0
    for j, k in enumerate(keep):
        o, n = orbs[k], raw["n_pi"][j]
        assert o["status"] == raw["status"][j] and o["levels"].tobytes() == raw["levels"][j, :n].tobytes()
        assert (o["gap"], o["homo"], o["lumo"]) == (float(raw["gap"][j]), float(raw["homo"][j]), float(raw["lumo"][j]))
        assert o["ip"] == -o["homo"] and o["ea"] == -o["lumo"] and o["e_total"] == o["e_electronic"] + o["e_core"]
        assert o["pi_charge"].tobytes() == raw["pi_charge"][j, :len(mols[j][0])].tobytes() and len(o["pi_bond_order"]) == len(mols[j][1])
        assert o["open_shell"] == (raw["status"][j] == OPEN_SHELL) and o["degenerate"] == bool(raw["flags"][j] & DEGENERATE)
        assert o["iterations"] == raw["iterations"][j] and o["sweeps"] == raw["sweeps"][j]
    gaps = ppp.gap(recs, DATASET, engine=HostEngine())
    assert gaps.dtype == np.float64 and np.isnan(gaps[[2, 5]]).all() and np.array_equal(gaps[keep[:4]], raw["gap"][:4].astype(np.float64))
    assert np.array_equal(ppp.gap(mols, DATASET, engine=HostEngine()), gaps[keep], equal_nan=True)
    assert ppp.orbitals(mols[4:], DATASET, charge=1, engine=HostEngine())[0]["status"] == OK
    ohno = ppp.gap(mols[:2], DATASET, repulsion="ohno", engine=HostEngine())
    assert np.array_equal(ohno, host(mols[:2], repulsion=1)["gap"].astype(np.float64)) and not np.array_equal(ohno, gaps[:2])
    undamped = ppp.orbitals(mols[:1], DATASET, damping=0.0, engine=HostEngine())[0]
    assert undamped["status"] == OK and undamped["iterations"] == host(mols[:1], damping=0.0)["iterations"][0]
    wide = ppp.gap(mols[:2], DATASET, parameters={"beta0": -3.0}, engine=HostEngine())
    assert (wide > gaps[:2]).all()
    assert ppp.orbitals([], DATASET, engine=HostEngine()) == [] and ppp.gap([], DATASET, engine=HostEngine()).shape == (0,)
    with pytest.raises(_lib.GaudiError, match="coordinates"):
        ppp.gap([dict(status=0, atom_types=mols[0][0], bonds=mols[0][1])], DATASET, engine=HostEngine())
    with pytest.raises(_lib.GaudiError, match="coordinates"):
        ppp.gap([(mols[0][0], mols[0][1])], DATASET, engine=HostEngine())
    with pytest.raises(_lib.GaudiError):
        ppp.gap(mols[:1], DATASET, repulsion="coulomb", engine=HostEngine())
    with pytest.raises(_lib.GaudiError):
        ppp.gap(mols[:1], DATASET, parameters={"gamma": {}}, engine=HostEngine())
    assert set(ppp.STATUS_NAMES) == set(range(9))
    T = ppp.default_parameters()
    assert "recalled" in T["source"] and "unverified" in T["source"] and T["beta0"] == -2.40 and T["classes"]["C"]["gamma"] == 11.13

    class Engine(HostEngine):
        calls = 0

        def ppp(self, *a):
            Engine.calls += 1
            return HostEngine.ppp(self, *a)

    def fake(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None, **kw):
        out = [dict(r) for r in recs]
        if kw.get("ppp"):
            for r, extra in zip(out, ppp.record_fields(out, dataset, engine=engine)):
                r.update(extra)
        return out

    fields = ppp.record_fields(recs, DATASET, engine=HostEngine())
    assert fields[2]["ppp_status"] == EMPTY and set(fields[0]) == {"ppp_gap", "ppp_homo", "ppp_lumo", "ppp_flags", "ppp_status"}
    assert [f["ppp_gap"] for f in fields if f["ppp_status"] == OK] == raw["gap"][:4].astype(np.float64).tolist()
    monkeypatch.setattr(G, "rings_to_atoms", fake)
    given = [(np.zeros((1, 3), np.float32), np.zeros(1, np.int64)) for _ in recs]
    plain, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Engine())
    assert Engine.calls == 0 and not any(k.startswith("ppp") for k in plain)
    d, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Engine(), ppp=True)
    assert Engine.calls == 1 and set(d) == set(plain) | {"ppp_gap", "ppp_not_converged_fraction"}
    assert all(np.array_equal(d[k], plain[k]) for k in plain)
    assert np.array_equal(d["ppp_gap"], gaps[keep], equal_nan=True) and d["ppp_not_converged_fraction"] == 0.0
    n = len(recs)
    x, one_hot, mask = torch.zeros(n, 2, 3), torch.zeros(n, 2, 4), torch.ones(n, 2, 1)
    Engine.calls = 0
    plain = generation_guidance._atoms(x, one_hot, mask, DATASET, Engine())
    assert Engine.calls == 0 and not any(k.startswith("ppp") for k in plain)
    got = generation_guidance._atoms(x, one_hot, mask, DATASET, Engine(), ppp=True)
    assert Engine.calls == 1 and set(got) == set(plain) | {"ppp_gap", "ppp_ip", "ppp_ea"}
    assert np.array_equal(got["ppp_gap"], gaps, equal_nan=True)
    assert np.array_equal(got["ppp_ip"][keep[:4]], -raw["homo"][:4].astype(np.float64)) and np.isnan(got["ppp_ea"][2])
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance._evaluate(None, None, None, None, None, 1.0, x, one_hot, mask, None, 1.0, ppp=True)
