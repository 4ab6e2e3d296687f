"""PPP for open shells by the half-electron method (csrc/ppp_open.inc, ppp_molecule<P, true> of csrc/ppp.inc) on the kernel's HOST
build: against a float64 oracle restated in numpy (tests/ppp_open_helpers.py) on golden g30 under the four state kinds, the
hand-made molecules as ions and triplets, the tier-edge molecules with one electron removed and odd neutral radicals; the analytic
fixed points; bit identity with gaudi_host_ppp, across batches and across the two ways to name a multiplicity; every refusal; the
digests of gaudi_host_ppp and gaudi_host_ppp_cis; the declarations and the layers on top.  tests/test_gpu_ppp_open.py holds the
device to this build bit for bit.

Tolerances (tests/ppp_open_helpers.py): measured on this build against the fixed point over the compared rows,
levels / homo / lumo / gap / e_state per centre 3.32e-4 eV, he_correction 2.42e-4 eV, charges / bond orders / spin densities 1.68e-4,
the differences ip / ea / t1 2.34e-4 eV.  The tests hold the energies to four times that; the densities to 2e-4, section 8m's hard
condition, which is tighter than four times the measured figure.

Statuses.  They are asserted on every decisive row that is also settled (tests/ppp_open_helpers.py: oracle).  The decisive rows
that are not: g30's exact-symmetry ties (the oracle's solver and the kernel's choose differently within the degenerate pair in every
iteration, and 35 of the 36 rows still agree -- the one that does not is a cation whose oracle converges at iteration 53 where the
host build oscillates), the benzene cation, anion and triplet (the same: the oracle converges, the host build oscillates, the flag
is set), and the 126-centre phenacene with one electron removed, where delta_p dips to 3.4e-6 at iteration 25 in float64 and grows
again by 1.235 per iteration towards a symmetry-broken state: in fp32 the seed is larger and the dip stays above 2^-16.  Only such a
graze is excused (delta_p above 2^-16 again within 64 iterations and never below 2^-16 / 8); a deeper dip stays asserted.  This is
narrower than "every decisive row"; the floors of agreeing decisive rows (150 / 150 / 145) count all decisive rows, ties included."""
import hashlib
import os
import re

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.ppp_helpers import (BAD_GEOMETRY, BAD_INPUT, BAD_TABLE, CAP, DATASET, EDGE_SIZES, EMPTY, NOT_CONVERGED, OK, OVERFLOW, SCF_CAP,
                               benzene, c_tables, chain_molecule, edge_set, g30_molecules, naphthalene, pack, phenacene, table)
from tests.ppp_helpers import host as host_closed
from tests.ppp_open_helpers import (KINDS, OPEN_TIE, TOL_DIFF, TOL_EV, TOL_HE, TOL_P, HostEngine, assert_same_bits, comparable, errors,
                                    g30_closed, g30_rows, host, hosts, long_host, long_rows, one_centre, oracles, radicals, row,
                                    small_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what the float64 prototype counted on g30's 157 closed-shell molecules (converged within 64, decisive, exact ties, comparable)
PROTOTYPE = {"cation": (143, 155, 12, 142), "anion": (144, 154, 12, 142), "triplet": (130, 149, 12, 127)}
COMPARED_FLOOR = {"cation": 140, "anion": 140, "triplet": 125, "singlet": 150}
AGREE_FLOOR = {"cation": 150, "anion": 150, "triplet": 145, "singlet": 150}
# sha256 over the output arrays of gaudi_host_ppp / gaudi_host_ppp_cis (in argument order) on g30 and on the tier-edge set: the
# same before and after ppp_molecule gained its open-shell flag
DIGESTS = {("g30", "ppp"): "ba31c9eb551097f4a00d2854ba11eff6be1e3615ac623f7be5e1b11d77fa0868",
           ("g30", "ppp_cis"): "978a56a150aff31101b4d12a836ba87728de18ff0f8d26aa8d37979ac7aa4d7e",
           ("edge", "ppp"): "192c05c2eab28321d80884e10d3e6300f841307243adb4d4b382b5bdd3ed58f6",
           ("edge", "ppp_cis"): "cc3a1dd4bceffa6724207d293baf6e9bff4d1ae902903453281d1f2986ee07c3"}


def check_rows(out, refs, rows):
    """Statuses, flags and values of a row set against the oracle -> (compared, agreeing decisive rows), per label."""
    mols, charge, mult, label = rows
    compared, agree = {}, {}
    for i, (ref, mol) in enumerate(zip(refs, mols)):
        assert ref["status"] in (OK, NOT_CONVERGED), (i, label[i])
        n, na, nb = ref["n_pi"], len(mol[0]), len(mol[1])
        assert (out["n_pi"][i], out["n_electrons"][i], out["n_excluded"][i], out["n_open"][i]) == \
               (n, ref["n_electrons"], ref["n_excluded"], ref["n_open"]), i
        assert out["somo"][i].tolist() == ref["somo"] and np.array_equal(out["occupation"][i, :n], ref["occupation"]), i
        assert not out["occupation"][i, n:].any() and not out["levels"][i, n:].any() and (np.diff(out["levels"][i, :n]) >= 0).all(), i
        assert np.array_equal(out["site_class"][i, :na], ref["site_class"]), i
        flagged = bool(out["flags"][i] & OPEN_TIE)
        print(f"row {i} ({label[i]}): n_pi {n}, oracle status {ref['status']} in {ref['iterations']}, host {out['status'][i]} in "
              f"{out['iterations'][i]}, tie {ref['tie']:.3g}, flag {flagged}")
        if ref["tie"] < 1e-4:
            assert flagged, (i, label[i])
        if ref["tie"] >= 1e-2:
            assert not flagged, (i, label[i])
        if ref["n_open"] == 0:
            assert not flagged and out["he_correction"][i] == 0.0 and not out["spin_density"][i].any(), i
        if ref["decisive"]:
            agree[label[i]] = agree.get(label[i], 0) + int(out["status"][i] == ref["status"])
            if ref["settled"]:
                assert out["status"][i] == ref["status"], (i, label[i])
        if out["status"][i] == NOT_CONVERGED and ref["decisive"] and ref["settled"]:
            assert out["iterations"][i] == CAP and out["flags"][i] & SCF_CAP and np.isfinite(out["e_state"][i])
        if not comparable(ref):
            continue
        assert out["status"][i] == OK and abs(int(out["iterations"][i]) - ref["iterations"]) <= 2, (i, label[i])
        ev, he, p = errors(out, i, ref, mol)
        print(f"    errors {ev:.3g} eV, {he:.3g} eV in the correction, {p:.3g} in P and the spin density")
        assert ev <= TOL_EV and he <= TOL_HE and p <= TOL_P, (i, label[i], ev, he, p)
        assert abs(float(out["spin_density"][i, :na].sum()) - ref["n_open"]) <= 1e-5 and (out["spin_density"][i] >= 0).all(), i
        assert not out["pi_charge"][i, na:].any() and not out["pi_bond_order"][i, nb:].any() and not out["spin_density"][i, na:].any()
        assert 0 < out["delta_p"][i] <= 2.0 ** -16 and out["gap"][i] == np.float32(out["lumo"][i] - out["homo"][i])
        compared[label[i]] = compared.get(label[i], 0) + 1
    return compared, agree


def test_g30_under_the_four_state_kinds():
    rows = g30_rows()
    refs, out = oracles("g30", rows), hosts("g30", rows)
    assert len(g30_closed()) == 157
    kind = rows[3]
    for name, want in PROTOTYPE.items():  # the oracle against the prototype's counts: more than two apart is a misread contract
        mine = [r for r, k in zip(refs, kind) if k == name]
        got = (sum(r["status"] == OK for r in mine), sum(r["decisive"] for r in mine), sum(r["tie"] < 1e-4 for r in mine),
               sum(comparable(r) for r in mine))
        print(name, got, want)
        assert all(abs(g - w) <= 2 for g, w in zip(got, want)), (name, got, want)
    assert not any(1e-4 <= r["tie"] < 1e-2 for r in refs)  # the flag conditions are sharp on g30
    compared, agree = check_rows(out, refs, rows)
    print(compared, agree)
    for name in KINDS:
        assert compared[name] >= COMPARED_FLOOR[name] and agree[name] >= AGREE_FLOOR[name], (name, compared, agree)


def test_g30_ip_ea_and_t1():
    """The differences the feature is for, and that relaxation lowers the ionisation potential below Koopmans'."""
    rows = g30_rows()
    refs, out = oracles("g30", rows), hosts("g30", rows)
    n = len(rows[0]) // 4
    got = out["e_state"].reshape(n, 4)
    want = np.array([r["e_state"] for r in refs]).reshape(n, 4)
    ok = np.array([comparable(r) for r in refs]).reshape(n, 4)
    koopmans = -out["homo"].astype(np.float64).reshape(n, 4)[:, 3]
    for j, (name, floor) in enumerate((("ip", 140), ("ea", 140), ("t1", 125))):
        sel = ok[:, j] & ok[:, 3]
        sign = -1.0 if name == "ea" else 1.0
        err = np.abs(sign * (got[:, j] - got[:, 3]) - sign * (want[:, j] - want[:, 3]))[sel]
        print(f"{name}: {sel.sum()} molecules, largest error {err.max():.3g} eV")
        assert sel.sum() >= floor and err.max() <= TOL_DIFF, (name, sel.sum(), err.max())
    sel = ok[:, 0] & ok[:, 3]
    relaxation = (koopmans - (got[:, 0] - got[:, 3]))[sel]
    print(f"Koopmans - delta-SCF ip: mean {relaxation.mean():.3f}, {relaxation.min():.3f} .. {relaxation.max():.3f} eV")
    assert (relaxation > 0).all() and 0.05 <= relaxation.mean() <= 0.15


def test_hand_made_ions_triplets_tier_edges_and_radicals():
    rows = small_rows()
    compared, _ = check_rows(hosts("small", rows), oracles("small", rows), rows)
    assert sum(compared.values()) >= 36, compared
    for name in radicals():
        assert compared.get(name) == 1, name
    for n in EDGE_SIZES:
        if n < 126:
            assert compared.get(f"edge {n} minus one electron") == 1, n
    out, label = hosts("small", rows), rows[3]
    for i in (label.index("benzene cation"), label.index("benzene anion"), label.index("benzene triplet")):
        assert out["flags"][i] & OPEN_TIE and np.isfinite(out["e_state"][i]) and out["levels"][i, :6].any()  # flagged, still returned
    i = label.index("allyl")  # the allyl radical: the unpaired electron on the two ends, none on the middle carbon
    assert np.allclose(out["spin_density"][i, :3], [0.5, 0.0, 0.5], atol=1e-5) and abs(out["pi_charge"][i, :3]).max() <= 1e-5


def test_the_long_rows_and_their_record():
    """The 126-, 127- and 128-centre rows: tests/golden/ppp_open_long_jobs.npz is what the live host build gives, and the oracle."""
    rows = long_rows()
    out = hosts("long", rows)
    assert_same_bits(out, long_host())
    assert out["n_pi"].tolist() == [126, 127, 128] and out["n_open"].tolist() == [1, 1, 1]
    compared, _ = check_rows(out, oracles("long", rows), rows)
    assert compared == {"edge 127": 1}


def test_the_analytic_fixed_points():
    """A single centre with one electron has e_state = -I; triplet ethylene has e_state = -2 I_C: whatever the table holds.  (The
    fp64 sums run over fp32 elements F_rr and H_rr, a handful of fp32 roundings at 11 .. 17 eV: 1e-5 eV.)"""
    ion = table()["classes"]["C"]["I"]
    out = host([one_centre(), chain_molecule(2), one_centre()], charge=[0, 0, 0], multiplicity=[0, 3, 2],
               parameters={"classes": {"C": {"I": 9.5, "gamma": 10.25}}})
    assert out["status"].tolist() == [OK] * 3 and out["n_pi"].tolist() == [1, 2, 1] and out["n_open"].tolist() == [1, 2, 1]
    assert np.abs(out["e_state"] - [-9.5, -19.0, -9.5]).max() <= 1e-5
    out = host([one_centre(), chain_molecule(2)], multiplicity=[0, 3])
    assert np.abs(out["e_state"] - [-ion, -2 * ion]).max() <= 1e-5 and abs(out["e_state"][1] + 22.32) <= 1e-5
    assert out["he_correction"][0] == -0.25 * np.float64(np.float32(table()["classes"]["C"]["gamma"]))
    assert out["spin_density"][0, 0] == 1.0 and np.allclose(out["spin_density"][1, :2], 1.0, atol=1e-6)
    assert out["occupation"][0, 0] == 1 and out["occupation"][1, :2].tolist() == [1, 1] and out["somo"].tolist() == [[0, -1], [0, 1]]
    assert out["homo"][0] == out["lumo"][0] == out["levels"][0, 0] and out["iterations"][1] == 1 and not (out["flags"] & OPEN_TIE).any()


def test_multiplicity_one_is_gaudi_ppp_bit_for_bit():
    rows = g30_rows()
    out = hosts("g30", rows)
    closed = host_closed(g30_closed())
    pick = np.arange(3, len(rows[0]), 4)
    assert_same_bits({k: out[k][pick] for k in _lib.PPP_ARRAYS}, closed, names=_lib.PPP_ARRAYS)
    assert not (out["flags"][pick] & OPEN_TIE).any() and not out["n_open"][pick].any() and (out["somo"][pick] == -1).all()
    assert not out["he_correction"][pick].any() and not out["spin_density"][pick].any()
    st = out["status"][pick]
    e_total = out["e_electronic"][pick].astype(np.float64) + out["e_core"][pick]
    scale = np.abs(out["e_electronic"][pick].astype(np.float64))
    assert (np.abs(out["e_state"][pick] - e_total) <= 1e-5 * scale)[st == OK].all()  # (fp32 sums of n^2 terms against fp64 ones)
    mols, charge = edge_set()
    for k in (0, 1, 4, 7):  # 2, 3, 33 and 64 centres, with the charge that closes the shell, both ways to ask
        want = host_closed([mols[k]], charge[k:k + 1])
        for mult in (1, 0, None):
            assert_same_bits(host([mols[k]], charge[k:k + 1], mult), want, names=_lib.PPP_ARRAYS)
    # ... and where gaudi_ppp refuses for the parity alone, the new entry solves
    assert host_closed([chain_molecule(3)])["status"][0] == 7 and host([chain_molecule(3)])["status"][0] == OK


def test_a_row_alone_and_in_a_mixed_batch_and_multiplicity_zero():
    rows = g30_rows()
    mols, charge, mult, kind = rows
    out = hosts("g30", rows)
    for i in (0, 1, 2, 3, 201, 402, 483, 624, 625, 626):
        alone = host([mols[i]], charge[i:i + 1], mult[i:i + 1])
        na, nb = len(mols[i][0]), len(mols[i][1])
        a, b = row(alone, 0, na, nb), row(out, i, na, nb)
        for k in _lib.PPP_OPEN_ARRAYS:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (i, kind[i], k)
    sub = slice(0, 160)  # forty molecules under the four kinds: 0 names the lowest multiplicity, which the triplet is not
    lowest = np.where(mult[sub] == 3, 3, 0).astype(np.int32)
    A, M = out["pi_charge"].shape[1], out["pi_bond_order"].shape[1]
    again = host(mols[sub], charge[sub], lowest, A=A, M=M)
    assert_same_bits(again, {k: out[k][sub] for k in _lib.PPP_OPEN_ARRAYS})
    padded = host(mols[:8], charge[:8], mult[:8], A=A + 5, M=M + 3)
    for i in range(8):
        a, b = row(padded, i, len(mols[i][0]), len(mols[i][1])), row(out, i, len(mols[i][0]), len(mols[i][1]))
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in _lib.PPP_OPEN_ARRAYS), i


def test_refusals_leave_zero_rows():
    ethylene, allyl = chain_molecule(2), chain_molecule(3)
    e, b, x = benzene()
    coincident = (e, b, np.where(np.arange(6)[:, None] == 1, x[0] + [0.3, 0.0, 0.0], x))
    nan_at = (e, b, np.where(np.arange(6)[:, None] == 4, np.nan, x))
    empty = (np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 3)))
    cases = [(ethylene, 0, 2, BAD_INPUT),        # wrong parity: two electrons cannot be a doublet
             (ethylene, 1, 1, BAD_INPUT),        # ... nor one electron a singlet
             (ethylene, 1, 3, BAD_INPUT),        # ... or a triplet
             (allyl, 0, 1, BAD_INPUT), (allyl, 0, 3, BAD_INPUT),
             (ethylene, -2, 3, BAD_INPUT),       # four electrons as a triplet: n_c + n_open = 3 levels of 2
             (ethylene, 2, 3, BAD_INPUT),        # no electron as a triplet: n_el - n_open < 0
             (ethylene, 0, 4, BAD_INPUT), (ethylene, 0, -1, BAD_INPUT), (allyl, 0, 4, BAD_INPUT),
             ((e, b, x), -7, 0, BAD_INPUT),      # benzene with 13 electrons
             ((e, b, x), 7, 0, BAD_INPUT),
             (coincident, 1, 0, BAD_GEOMETRY), (nan_at, 0, 3, BAD_GEOMETRY), (phenacene(32), 1, 0, OVERFLOW), (empty, 0, 0, EMPTY),
             (empty, 0, 7, EMPTY), (phenacene(32), 0, 9, OVERFLOW),  # (the graph's refusals come before the multiplicity's)
             (ethylene, 0, 3, OK), (ethylene, -1, 2, OK), (ethylene, 1, 0, OK), (allyl, 0, 0, OK), ((e, b, x), -6, 0, OK),
             ((e, b, x), 6, 1, OK), (ethylene, -2, 1, OK)]
    out = host([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert out["status"].tolist() == [c[3] for c in cases]
    for i, st in enumerate(out["status"]):
        if st != OK:
            for k in _lib.PPP_OPEN_ARRAYS:
                assert k == "status" or not out[k][i].any(), (i, k)  # a refused row is zero, somo included
    assert out["n_electrons"][-3:].tolist() == [12, 0, 4] and out["n_open"][-3:].tolist() == [0, 0, 0]
    bad_bond = (np.array(ethylene[0]), np.array([[0, 9]] + ethylene[1][1:].tolist(), np.int32), ethylene[2])
    assert host([bad_bond], [1], [2])["status"][0] == BAD_INPUT


def test_a_table_or_a_setting_that_cannot_be_used():
    mols, charge, mult = [benzene(), naphthalene()], [1, 0], [2, 3]
    assert host(mols, charge, mult)["status"].tolist() == [NOT_CONVERGED, OK]  # (the benzene cation: an exact tie that oscillates)
    bad = [{"classes": {"C": {"gamma": 0.0}}}, {"classes": {"C": {"gamma": -1.0}}}, {"classes": {"C": {"gamma": float("nan")}}},
           {"classes": {"C": {"gamma": float("inf")}}}, {"classes": {"C": {"I": float("inf")}}}, {"classes": {"C": {"z": 3}}},
           {"classes": {"C": {"z": -1}}}, {"classes": {"C": {"k": float("nan")}}}, {"beta0": float("nan")},
           {"beta_pair": {"C|C": float("inf")}}]
    for parameters in bad:
        out = host(mols, charge, mult, parameters=parameters)
        assert out["status"].tolist() == [BAD_TABLE, BAD_TABLE], parameters
        assert all(k == "status" or not out[k].any() for k in _lib.PPP_OPEN_ARRAYS), parameters
    for kw in ({"damping": 1.0}, {"damping": -0.1}, {"damping": float("nan")}, {"repulsion": 2}, {"repulsion": -1}):
        assert host(mols, charge, mult, **kw)["status"].tolist() == [BAD_TABLE, BAD_TABLE], kw
    t = c_tables()
    t.site_class[1][3] = t.n_classes
    assert _lib.host_ppp_open(t, *pack(mols))["status"].tolist() == [BAD_TABLE, BAD_TABLE]
    t = c_tables()
    t.n_elems = 9
    with pytest.raises(_lib.GaudiError):
        _lib.host_ppp_open(t, *pack(mols))
    ohno = host(mols[1:], [1], [2], repulsion=1)
    assert ohno["status"][0] == OK and ohno["e_state"][0] != host(mols[1:], [1], [2])["e_state"][0]


def test_the_digests_of_the_closed_shell_entries():
    """ppp_molecule<P, false> is operation for operation what it was: gaudi_host_ppp and gaudi_host_ppp_cis give the bytes they gave
    before the flag existed."""
    mols, charge = edge_set()
    for name, ms, ch in (("g30", g30_molecules(), None), ("edge", mols, charge)):
        for entry, fn, arrays in (("ppp", _lib.host_ppp, _lib.PPP_ARRAYS),
                                  ("ppp_cis", _lib.host_ppp_cis, _lib.PPP_ARRAYS + _lib.PPP_CIS_ARRAYS)):
            out = fn(c_tables(), *pack(ms), ch)
            h = hashlib.sha256()
            for k in arrays:
                h.update(np.ascontiguousarray(out[k]).tobytes())
            assert h.hexdigest() == DIGESTS[name, entry], (name, entry)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert all(d in design for d in DIGESTS.values())


def test_declarations():
    import ctypes as Ct
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    assert "#define GAUDI_ABI_VERSION 7" in header and lib.gaudi_abi_version() == 7
    added = re.search(r"\(Entry points ADDED since(.*?)\*/", header, re.S).group(1)
    ctype = {"int": Ct.c_int, "float": Ct.c_float, "gaudi_handle*": Ct.c_void_p, "const int32_t*": _lib.IP, "int32_t*": _lib.IP,
             "float*": _lib.FP, "const float*": _lib.FP, "uint8_t*": Ct.POINTER(Ct.c_uint8), "int8_t*": Ct.POINTER(Ct.c_int8),
             "double*": Ct.POINTER(Ct.c_double), "const gaudi_ppp_tables*": Ct.POINTER(_lib.PPPTables)}
    for name in ("gaudi_ppp_open", "gaudi_host_ppp_open", "gaudi_ppp_open_profile_get"):
        assert re.search(r"\b" + name + r"\b", added), name
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, name
        args = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).replace("\n", " ").split(",")]
        assert _lib.EXPORTS[name] == (Ct.c_int, args), name
        assert hasattr(lib, name)
    assert re.search(r"#define GAUDI_PPP_OPEN_TIE +256\b", header) and _lib.PPP_OPEN_TIE == 256 == OPEN_TIE
    assert _lib.PPP_OPEN_ARRAYS == _lib.PPP_ARRAYS + ("spin_density", "e_state", "he_correction", "n_open", "somo")
    mols = pack([benzene(), naphthalene()])
    out = _lib.ppp_open_outputs(2, mols[0].shape[1], mols[2].shape[1])
    assert out["e_state"].dtype == out["he_correction"].dtype == np.float64 and out["somo"].shape == (2, 2)
    args = list(_lib.ppp_open_args(c_tables(), *mols, None, None, 0, 0.25, out))
    assert len(args) == 13 + 23 and lib.gaudi_host_ppp_open(*args) == 0 and out["status"].tolist() == [OK, OK]
    for at, value in [(0, None), (1, -1), (2, 0), (3, 0), (4, None), (5, None), (6, None), (7, None), (8, None)] + \
                     [(k, None) for k in range(13, 36)]:
        broken = list(args)
        broken[at] = value
        assert lib.gaudi_host_ppp_open(*broken) == -1, at
    source = open(os.path.join(ROOT, "gaudi_amd", "csrc", "ppp.inc")).read()
    assert "static_assert(sizeof(PppSmem<128>) <= 160 * 1024" in source


def test_states_ionization_triplet_and_the_layers_on_top():
    from gaudi_amd import ppp
    g, ref = g30_closed(), hosts("g30", g30_rows())
    fine = ((ref["status"] == OK) & ((ref["flags"] & OPEN_TIE) == 0)).reshape(-1, 4).all(1)  # solved in all four state kinds
    mols = [g[k] for k in np.flatnonzero(fine)[[4, 30, 77]]] + [chain_molecule(3), benzene()]
    recs = [dict(status=0, atom_types=e, bonds=b, atoms3d=np.asarray(x, np.float64), fingerprint=1000 + k) for k, (e, b, x) in enumerate(mols)]
    recs.insert(2, dict(status=2, fingerprint=0))
    keep = [0, 1, 3, 4, 5]
    eng = HostEngine()
    raw = host(mols, [1, 1, 1, 0, 1], 0)
    st = ppp.states(recs, DATASET, charge=[1, 1, 0, 1, 0, 1], engine=eng)
    assert len(st) == 6 and st[2]["status"] == EMPTY and len(st[2]["levels"]) == 0 and st[2]["multiplicity"] == 0
    for j, k in enumerate(keep):
        s, n = st[k], raw["n_pi"][j]
        assert s["status"] == raw["status"][j] and s["levels"].tobytes() == raw["levels"][j, :n].tobytes()
        assert s["e_state"] == raw["e_state"][j] and s["he_correction"] == raw["he_correction"][j] and isinstance(s["e_state"], float)
        assert s["spin_density"].tobytes() == raw["spin_density"][j, :len(mols[j][0])].tobytes()
        assert s["n_open"] == 1 and s["multiplicity"] == 2 and s["somo"] == [int(raw["somo"][j, 0])] and not s["open_shell"]
        assert s["open_tie"] == bool(raw["flags"][j] & OPEN_TIE) and s["occupation"].max() == 2 and (s["occupation"] == 1).sum() == 1
    assert st[5]["open_tie"] and not st[0]["open_tie"]
    assert ppp.states(mols[:1], DATASET, multiplicity=3, engine=eng)[0]["somo"] == [raw["somo"][0, 0], raw["somo"][0, 0] + 1]
    assert ppp.states(mols[:1], DATASET, multiplicity=2, engine=eng)[0]["status"] == BAD_INPUT
    assert ppp.states([], DATASET, engine=eng) == []
    ion = ppp.ionization(recs, DATASET, engine=eng)
    three = host(mols * 3, [0, 0, 0, 0, 0] + [1] * 5 + [-1] * 5, 0)
    e = three["e_state"].reshape(3, 5)
    assert all(ion[k].dtype == np.float64 and ion[k].shape == (6,) for k in ("ip", "ea", "fundamental_gap", "ip_koopmans", "ea_koopmans"))
    assert np.isnan([ion[k][2] for k in ("ip", "ea", "fundamental_gap", "ip_koopmans", "ea_koopmans")]).all()
    assert three["status"].reshape(3, 5)[:, :4].tolist() == [[OK] * 4] * 3  # the allyl radical among them: a neutral radical works
    assert np.array_equal(ion["ip"][keep[:4]], (e[1] - e[0])[:4]) and np.array_equal(ion["ea"][keep[:4]], (e[0] - e[2])[:4])
    assert np.array_equal(ion["fundamental_gap"][keep[:4]], ion["ip"][keep[:4]] - ion["ea"][keep[:4]])
    assert np.array_equal(ion["ip_koopmans"][keep[:4]], -three["homo"][:4].astype(np.float64))
    assert np.isnan(ion["ip"][5]) and ion["open_tie"][5] and not ion["open_tie"][:2].any()  # the benzene cation does not converge
    assert (ion["ip"][keep[:3]] < ion["ip_koopmans"][keep[:3]]).all() and (ion["ea"][keep[:3]] > ion["ea_koopmans"][keep[:3]]).all()
    assert ion["status"].shape == (3, 6) and ion["status"][:, 2].tolist() == [EMPTY] * 3
    t = ppp.triplet(mols, DATASET, engine=eng)
    both = host(mols[:3] * 2, 0, [1] * 3 + [3] * 3)["e_state"].reshape(2, 3)
    assert np.array_equal(t["t1"][:3], both[1] - both[0]) and np.isnan(t["t1"][3]) and t["status"][:, 3].tolist() == [BAD_INPUT] * 2
    assert (t["t1"][:3] > 0).all()
    extra = ppp.dscf_fields(recs, DATASET, engine=eng)
    assert np.array_equal(extra["ppp_ip_dscf"], ion["ip"], equal_nan=True) and extra["ppp_dscf_status"].tolist() == [0, 0, EMPTY, 0, 0, 1]
    assert ppp.ionization([], DATASET, engine=eng)["ip"].shape == (0,) and ppp.triplet([], DATASET, engine=eng)["t1"].shape == (0,)
    assert "states" in ppp.orbitals.__doc__
