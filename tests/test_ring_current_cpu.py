"""Hueckel-London ring currents (csrc/ring_current.inc) on the kernel's HOST build: the textbook values, every
g30 molecule and the tier-edge set against the finite-field float64 oracle of tests/ring_current_helpers.py (which shares nothing
with the kernel), the laws the currents obey (Kirchhoff, scaling, rigid motions, relabelling), every status and flag, the Python
layers and the header.  The device is held to this build bit for bit by tests/test_gpu_ring_current.py.

MEASURED on the host build: the largest |value - oracle| / max(1, |oracle|) over every float output is 2.0e-5 on g30 (the residual
of a molecule with ring currents down to -19.7; 3.1e-6 over bond currents, 1.6e-6 over ring currents) and 4.2e-5 on the tier-edge
set; the issue's bound is TOL = 1e-4."""
import os

import numpy as np
import pytest

from gaudi_amd import _lib
from tests import ppp_helpers as pp
from tests.huckel_helpers import polyene, with_h
from tests.ring_current_helpers import (BAD_GEOMETRY, BAD_INPUT, BAD_TABLE, C, DATASET, EMPTY, KNOWN, NO_PI, OK, OPEN_SHELL, OVERFLOW,
                                        RINGS_UNDEFINED, SMALL_GAP, TOL, HostEngine, acene, bent, biphenyl, by_cell, c_tables,
                                        cyclobutadiene, g30_host, g30_molecules, g30_oracle, host, known, oracle, record, relabelled,
                                        rotated, worst)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
H = pp.H


def flat(mol):
    """A polyene of huckel_helpers with coordinates nobody looks at."""
    e, b = mol
    return e, b, np.zeros((len(e), 3))


def test_textbook_ring_currents():
    for name, (_, want) in KNOWN.items():
        mol = known(name)
        rec = record(host([mol]), 0, mol)
        assert rec["status"] == OK and rec["flags"] == 0 and rec["n_rings"] == len(want), name
        got = by_cell(name, rec, mol)
        print(name, np.round(got, 5), "largest error", np.abs(np.array(got) - want).max())
        assert np.abs(np.array(got) - want).max() <= 5e-4, name
        assert np.abs(np.array(by_cell(name, oracle(mol), mol)) - want).max() <= 5e-4, name  # ... and they pin the oracle
        assert np.allclose(rec["ring_area"], 1.5 * np.sqrt(3.0) * 1.40 ** 2, atol=1e-5) and rec["normal"].tolist() == [0.0, 0.0, 1.0]
    mol = known("benzene")
    rec = record(host([mol]), 0, mol)
    xyz, (ring,) = mol[2], rec["rings"]
    assert ring[0] == min(ring) and np.cross(xyz[ring[1]] - xyz[ring[0]], xyz[ring[2]] - xyz[ring[1]])[2] > 0  # counter-clockwise
    for k, (i, j) in enumerate(mol[1]):  # +1 along the ring's direction on every bond
        along = (ring.index(j) - ring.index(i)) % 6 == 1
        assert abs(rec["bond_current"][k] - (1.0 if along else -1.0)) <= 5e-4


def test_every_g30_molecule_equals_the_oracle():
    mols, out, want = g30_molecules(), g30_host(), g30_oracle()
    assert len(mols) == 160
    errs = np.array([worst(record(out, i, m), want[i]) for i, m in enumerate(mols)])
    print("largest error", errs.max(), "molecule", int(errs.argmax()))
    assert errs.max() <= TOL
    st = np.bincount(out["status"], minlength=10)
    assert (st[OK], st[OPEN_SHELL], st[SMALL_GAP], st[OVERFLOW]) == (155, 1, 3, 1) and st.sum() == 160 and not out["flags"].any()
    for k in _lib.RING_CURRENT_ARRAYS:  # any status other than OK writes zero rows
        if k != "status":
            assert not out[k][out["status"] != OK].any(), k
    ok = out["status"] == OK
    assert out["n_rings"][ok].max() >= 10 and out["ring_current"].min() < -19.0 and out["ring_current"].max() > 1.8
    sizes = out["ring_size"][ok][np.arange(32)[None, :] < out["n_rings"][ok][:, None]]
    assert set(sizes.tolist()) <= {4, 5, 6} and len(set(sizes.tolist())) >= 2
    pad = np.arange(6)[None, None, :] >= out["ring_size"][ok][:, :, None]
    assert (out["ring_atoms"][ok][pad] == -1).all() and (out["ring_atoms"][ok][~pad] >= 0).all()


def test_the_tier_edge_set_equals_the_oracle():
    mols, charge = pp.edge_set()
    out = host(mols, charge)
    errs = [worst(record(out, i, m), oracle(m, int(charge[i]))) for i, m in enumerate(mols)]
    print("largest error", max(errs))
    assert max(errs) <= TOL and out["status"].tolist() == [OK] * len(mols) and out["n_pi"].tolist() == list(pp.EDGE_SIZES)
    assert out["n_rings"].tolist() == [0 if n < 6 else (n - 2) // 4 for n in pp.EDGE_SIZES]
    for i, m in enumerate(mols):  # a molecule's bits do not depend on the batch, its place in it or the padding
        alone = host([m], charge[i:i + 1], A=len(m[0]) + 3, M=len(m[1]) + 5)
        for k in _lib.RING_CURRENT_ARRAYS:
            a, b = alone[k][0], out[k][i]
            if k == "bond_current":
                a, b = a[:len(m[1])], b[:len(m[1])]
            assert a.tobytes() == b.tobytes(), (k, i)


def test_kirchhoff():
    mols, out = g30_molecules(), g30_host()
    worst_sum = 0.0
    for i, (e, b, _) in enumerate(mols):
        if out["status"][i] != OK:
            continue
        net = np.zeros(len(e))
        np.add.at(net, b[:, 0], -out["bond_current"][i, :len(b)].astype(np.float64))
        np.add.at(net, b[:, 1], out["bond_current"][i, :len(b)].astype(np.float64))
        worst_sum = max(worst_sum, float(np.abs(net).max()))
    print("largest net current at a centre", worst_sum)
    assert worst_sum <= 1e-4


@pytest.mark.parametrize("scale", [2.0, 0.5])
def test_scaled_coordinates_scale_every_current(scale):
    # a power of two scales every fp32 operand exactly, so the currents are 4 (or 1/4) times the same bits
    mols = [known("coronene"), known("phenanthrene"), pp.hand_made()["pyrrole"][0], g30_molecules()[119]]
    out = host(mols)
    big = host([(e, b, np.asarray(x) * scale) for e, b, x in mols])
    assert out["status"].tolist() == [OK] * 4 and big["status"].tolist() == [OK] * 4
    for k in ("bond_current", "ring_current", "ring_area", "residual"):
        assert np.array_equal(big[k], out[k] * np.float32(scale * scale)), k
    assert np.array_equal(big["rms_out_of_plane"], out["rms_out_of_plane"] * np.float32(scale))
    for k in ("normal", "gap", "ring_atoms", "ring_size", "n_rings", "flags"):
        assert np.array_equal(big[k], out[k]), k


def test_rigid_motions():
    want, mols = g30_oracle(), g30_molecules()
    picked = [i for i in range(len(mols)) if want[i]["status"] == OK and want[i]["n_rings"] >= 2][::5][:24]
    moved = [rotated(mols[i], 4100 + i) for i in picked]
    out = host([m[:3] for m in moved])
    for k, i in enumerate(picked):
        got, w = record(out, k, mols[i]), want[i]
        assert worst(got, oracle(moved[k][:3])) <= TOL
        sign = float(np.sign(got["normal"] @ (moved[k][3] @ w["normal"])))
        assert abs(sign) == 1.0 and np.abs(got["normal"] - sign * (moved[k][3] @ w["normal"])).max() <= TOL
        assert np.abs(got["bond_current"] - sign * w["bond_current"]).max() <= TOL * max(1.0, np.abs(w["bond_current"]).max())
        assert np.abs(got["ring_current"] - w["ring_current"]).max() <= TOL * max(1.0, np.abs(w["ring_current"]).max())
        assert np.abs(got["ring_area"] - w["ring_area"]).max() <= TOL * max(1.0, w["ring_area"].max())
        for r_got, r_want in zip(got["rings"], w["rings"]):  # the same rings, turned round where the normal points the other way
            assert r_got == (r_want if sign > 0 else (r_want[0],) + tuple(reversed(r_want[1:])))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_relabelling(seed):
    want, mols = g30_oracle(), g30_molecules()
    picked = [i for i in range(len(mols)) if want[i]["status"] == OK and want[i]["n_rings"] >= 1][seed::3][:32]
    assert len(picked) == 32
    moved = [relabelled(mols[i], 7700 + 100 * seed + i) for i in picked]
    out = host([m[0] for m in moved])
    for k, i in enumerate(picked):
        (mol, perm, order, swapped), w = moved[k], want[i]
        got = record(out, k, mol)
        assert got["status"] == OK and got["flags"] == 0 and got["n_rings"] == w["n_rings"]
        back = np.where(swapped, -1.0, 1.0) * got["bond_current"]
        assert np.abs(back - w["bond_current"][order]).max() <= TOL * max(1.0, np.abs(w["bond_current"]).max())
        mine = {frozenset(int(a) for a in r): c for r, c in zip(got["rings"], got["ring_current"])}
        theirs = {frozenset(int(perm[a]) for a in r): c for r, c in zip(w["rings"], w["ring_current"])}
        assert set(mine) == set(theirs)
        assert max(abs(mine[r] - theirs[r]) / max(1.0, abs(theirs[r])) for r in mine) <= TOL
        assert [tuple(sorted(r)) for r in got["rings"]] == sorted(tuple(sorted(r)) for r in got["rings"])
        assert all(r[0] == min(r) for r in got["rings"]) and (got["ring_area"] > 0).all()


def test_bonds_on_no_cycle_carry_exactly_nothing():
    (mol, link), chain = biphenyl(), flat(polyene(8))
    tail, _ = pp.edge_molecule(33)  # seven fused hexagons and a chain of three carbons
    out = host([mol, chain, tail], np.array([0, 0, 1], np.int32))
    assert out["status"].tolist() == [OK, OK, OK] and out["flags"].tolist() == [0, 0, 0] and out["n_rings"].tolist() == [2, 0, 7]
    assert out["bond_current"][0, link] == 0.0 and (np.abs(out["bond_current"][0, :link]) > 0.9).all()
    assert worst(record(out, 0, mol), oracle(mol)) <= TOL and out["ring_current"][0, 0] == out["ring_current"][0, 1]
    assert 0.9 < out["ring_current"][0, 0] < 1.0  # two benzene rings, each a little weaker for the conjugation through the link
    assert not out["bond_current"][1].any() and not out["normal"][1].any() and out["rms_out_of_plane"][1] == 0.0
    assert out["n_pi"][1] == 8 and out["gap"][1] > 0.5 and (out["ring_atoms"][1] == -1).all()
    e, b, _ = tail
    in_chain = [k for k, (i, j) in enumerate(b) if e[i] == C and e[j] == C and max(i, j) >= 30]
    assert len(in_chain) == 3 and not out["bond_current"][2, in_chain].any() and np.count_nonzero(out["bond_current"][2]) == 36


def test_hand_made_heterocycles():
    made = pp.hand_made()
    mols, charge = [m for m, _ in made.values()], np.array([c for _, c in made.values()], np.int32)
    out = host(mols, charge)
    for i, (name, (m, c)) in enumerate(made.items()):
        got, w = record(out, i, m), oracle(m, c)
        assert worst(got, w) <= TOL and got["status"] == OK, name
        print(name, got["ring_current"])
    cur = {name: out["ring_current"][i, 0] for i, name in enumerate(made)}
    assert out["ring_size"][:, 0].tolist() == [0, 0, 6, 6, 6, 5, 5, 5, 6]
    assert abs(cur["benzene"] - 1.0) < 1e-5 and 0.8 < cur["pyridine"] < 1.0  # all diatropic; the five-rings that section 8o cannot see
    assert all(0.3 < cur[name] < 1.0 for name in ("pyrrole", "furan", "thiophene"))


def test_cyclobutadiene_and_other_small_gaps():
    lone = (np.array([pp.N_, H, H, H], np.int32), np.array([(0, 1), (0, 2), (0, 3)], np.int32), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]]))
    mols = [cyclobutadiene(), known("benzene"), pp.cycle([C] * 8), lone]  # lone: one centre, two electrons, no empty level
    out = host(mols)
    assert out["status"].tolist() == [SMALL_GAP, OK, SMALL_GAP, SMALL_GAP]
    assert [oracle(m)["status"] for m in mols] == out["status"].tolist()
    for k in _lib.RING_CURRENT_ARRAYS:
        if k != "status":
            assert not out[k][[0, 2, 3]].any(), k
    # the dication of cyclobutadiene has a gap, and a two-electron four-ring is diatropic
    ion = host([cyclobutadiene()], np.array([2], np.int32))
    assert ion["status"][0] == OK and ion["ring_size"][0, 0] == 4 and ion["ring_current"][0, 0] > 0.0
    assert worst(record(ion, 0, mols[0]), oracle(mols[0], 2)) <= TOL


def test_a_bent_molecule_reports_its_distance_from_the_plane():
    mol = bent(known("anthracene"), 20.0)
    got, w = record(host([mol]), 0, mol), oracle(mol)
    assert worst(got, w) <= TOL and got["status"] == OK
    assert 0.2 < got["rms_out_of_plane"] < 1.0 and abs(got["rms_out_of_plane"] - w["rms_out_of_plane"]) <= TOL
    flat_rec = record(host([known("anthracene")]), 0, mol)
    assert flat_rec["rms_out_of_plane"] == 0.0 and got["ring_area"].max() < flat_rec["ring_area"].max()


def test_every_status_and_flag():
    benz = known("benzene")
    methane = with_h(np.array([C], np.int32), np.zeros((0, 2), np.int32), [4])
    nan = (benz[0], benz[1], benz[2].copy())
    nan[2][3, 1] = np.nan
    close = (benz[0], benz[1], benz[2].copy())
    close[2][1] = close[2][0] + [0.3, 0.0, 0.0]
    annulene = pp.cycle([C] * 10)  # one cycle, and no ring of 4 to 6 centres to carry it
    azulene = (np.array([C] * 10, np.int32), np.array([(k, (k + 1) % 10) for k in range(10)] + [(0, 4)], np.int32),
               np.array(pp.cycle([C] * 10)[2]))
    cases = [(acene(33), 0, OVERFLOW), (flat(methane), 0, NO_PI), ((np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 3))), 0, EMPTY),
             ((benz[0], np.array([(0, 9)], np.int32), benz[2]), 0, BAD_INPUT), (benz, 9, BAD_INPUT), (benz, 1, OPEN_SHELL),
             (cyclobutadiene(), 0, SMALL_GAP), (nan, 0, BAD_GEOMETRY), (close, 0, BAD_GEOMETRY)]
    mols = [benz] + [m for m, _, _ in cases] + [annulene, azulene, known("naphthalene")]
    charge = np.array([0] + [c for _, c, _ in cases] + [0, 0, 0], np.int32)
    out = host(mols, charge)
    assert out["status"].tolist() == [OK] + [s for _, _, s in cases] + [OK, OK, OK]
    assert out["flags"].tolist() == [0] * (1 + len(cases)) + [RINGS_UNDEFINED, RINGS_UNDEFINED, 0]
    for k in _lib.RING_CURRENT_ARRAYS:
        if k != "status":
            assert not out[k][1:1 + len(cases)].any(), k
    for m, c, s in cases:
        assert oracle(m, c)["status"] == s
    # rings undefined: the ring rows are zero, the bond currents stay valid
    for i, m in ((len(mols) - 3, annulene), (len(mols) - 2, azulene)):
        got, w = record(out, i, m), oracle(m)
        assert w["flags"] == RINGS_UNDEFINED and worst(got, w) <= TOL
        assert got["n_rings"] == 0 and not out["ring_atoms"][i].any() and not out["ring_size"][i].any() and not out["ring_current"][i].any()
        assert np.abs(got["bond_current"][:10]).min() > 0.1 and got["residual"] == 0.0
    print("[10]annulene", out["bond_current"][len(mols) - 3, :10])
    assert np.ptp(out["bond_current"][len(mols) - 3, :10]) < 1e-4 and out["bond_current"][len(mols) - 3, 0] > 1.0  # one current, diatropic
    # ... and a refused molecule leaves its neighbours' bits alone
    alone = host([benz, known("naphthalene")])
    for k in _lib.RING_CURRENT_ARRAYS:
        cut = (slice(None), slice(0, alone[k].shape[1])) if k == "bond_current" else (slice(None),)
        assert out[k][[0, -1]][cut].tobytes() == alone[k].tobytes(), k
    t = c_tables()
    t.n_classes = 17
    bad = _lib.host_ring_currents(t, *pp.pack([benz]), None)
    assert bad["status"].tolist() == [BAD_TABLE] and not bad["bond_current"].any()


def test_declarations_and_argument_checks():
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    for name in ("gaudi_ring_currents(", "gaudi_host_ring_currents(", "gaudi_ring_currents_profile_get(", "GAUDI_RING_CURRENT_MAX_RINGS 32",
                 "GAUDI_RING_CURRENT_MAX_SIZE 6", "GAUDI_RING_CURRENT_SMALL_GAP 9", "GAUDI_RING_CURRENT_RINGS_UNDEFINED 1"):
        assert name in header, name
    assert "#define GAUDI_ABI_VERSION 7" in header
    assert (_lib.RING_CURRENT_MAX_RINGS, _lib.RING_CURRENT_MAX_SIZE, _lib.RING_CURRENT_SMALL_GAP, _lib.RING_CURRENT_RINGS_UNDEFINED) == (32, 6, SMALL_GAP, 1)
    assert len(_lib.RING_CURRENT_ARRAYS) == 15
    lib = _lib.load_library()
    assert all(hasattr(lib, n) for n in ("gaudi_ring_currents", "gaudi_host_ring_currents", "gaudi_ring_currents_profile_get"))
    packed = pp.pack([known("benzene")])
    out = _lib.ring_current_outputs(1, packed[2].shape[1])
    args = list(_lib.ring_current_args(c_tables(), *packed, None, out))
    assert lib.gaudi_host_ring_currents(*args) == 0 and out["status"][0] == OK
    for missing in (0, 8, 10, 24):  # the table, xyz, an output
        broken = list(args)
        broken[missing] = None
        assert lib.gaudi_host_ring_currents(*broken) != 0, missing


def test_the_python_layers(monkeypatch):
    import gaudi_amd.gor2goa as G
    from gaudi_amd import analyze, aromaticity, generation_guidance
    mols, raw = g30_molecules(), g30_host()
    idx = [2, 14, 119, 156, 159] + list(range(20, 32))
    recs = [dict(status=0, atom_types=mols[i][0].astype(np.int64), bonds=mols[i][1].astype(np.int64), atoms3d=mols[i][2], fingerprint=3000 + i)
            for i in idx]
    recs.insert(2, dict(status=2, fingerprint=0))
    keep = [k for k in range(len(recs)) if k != 2]
    res = aromaticity.ring_currents(recs, DATASET, engine=HostEngine())
    assert len(res) == len(recs) and res[2]["status"] == EMPTY and len(res[2]["bond_current"]) == 0 and res[2]["rings"] == []
    assert set(aromaticity.RING_CURRENT_STATUS_NAMES) == set(range(10)) and res[2]["status_name"] == "no atoms (not built)"
    for k, i in zip(keep, idx):
        r, m = res[k], len(mols[i][1])
        assert (r["status"], r["n_pi"], r["flags"], r["sweeps"]) == (raw["status"][i], raw["n_pi"][i], raw["flags"][i], raw["sweeps"][i])
        assert r["bond_current"].tobytes() == raw["bond_current"][i, :m].tobytes() and len(r["rings"]) == raw["n_rings"][i]
        assert r["ring_current"].tobytes() == raw["ring_current"][i, :len(r["rings"])].tobytes() and r["normal"].tobytes() == raw["normal"][i].tobytes()
        assert [a.tolist() for a in r["rings"]] == [raw["ring_atoms"][i, q, :raw["ring_size"][i, q]].tolist() for q in range(len(r["rings"]))]
        if r["status"] == OK and r["rings"]:
            assert (r["ring_current_max"], r["ring_current_min"]) == (r["ring_current"].max(), r["ring_current"].min()) and not r["rings_undefined"]
        else:
            assert r["status"] != OK and np.isnan(r["ring_current_max"]) and np.isnan(r["ring_current_min"])
    triples = [mols[i] for i in idx]
    ext = aromaticity.ring_current_extremes(triples, DATASET, engine=HostEngine())
    assert set(ext) == {"ring_current_max", "ring_current_min", "status"} and ext["status"].tolist() == raw["status"][idx].tolist()
    assert np.array_equal(ext["ring_current_max"], [res[k]["ring_current_max"] for k in keep], equal_nan=True)
    assert np.array_equal(ext["ring_current_min"], [res[k]["ring_current_min"] for k in keep], equal_nan=True)
    assert ext["ring_current_min"][2] < -19.0 and np.isnan(ext["ring_current_max"][[0, 1, 3, 4]]).all()
    assert aromaticity.ring_currents([], DATASET, engine=HostEngine()) == []
    assert aromaticity.ring_current_extremes([], DATASET, engine=HostEngine())["status"].shape == (0,)
    # a chain has no ring: zero, not NaN; an annulene's rings are undefined: NaN; a charge and a parameter reach the kernel
    odd = aromaticity.ring_currents([flat(polyene(4)), pp.cycle([C] * 10), known("benzene")], DATASET, engine=HostEngine())
    assert (odd[0]["status"], odd[0]["ring_current_max"], odd[0]["ring_current_min"]) == (OK, 0.0, 0.0)
    assert odd[1]["status"] == OK and odd[1]["rings_undefined"] and np.isnan(odd[1]["ring_current_max"])
    assert aromaticity.ring_currents([known("benzene")], DATASET, charge=1, engine=HostEngine())[0]["status"] == OPEN_SHELL
    weak = aromaticity.ring_currents([known("benzene")], DATASET, parameters={"classes": {"C": {"k": 0.5}}}, engine=HostEngine())[0]
    assert abs(weak["ring_current"][0] - 0.25 * odd[2]["ring_current"][0]) < 1e-5  # J is linear in beta: k_rs = 0.25
    with pytest.raises(_lib.GaudiError):
        aromaticity.ring_currents([(mols[20][0], mols[20][1])], DATASET, engine=HostEngine())  # no coordinates
    # rings_to_atoms / analyze_atoms_for_molecules on these records (the conversion itself needs a device: tests/test_gpu_ring_current.py)
    fields = aromaticity.ring_current_fields(recs, DATASET, engine=HostEngine())
    assert set(fields[0]) == {"ring_current_max", "ring_current_min", "ring_current_status"} and fields[2]["ring_current_status"] == EMPTY

    class Counting(HostEngine):
        calls = 0

        def ring_currents(self, *args):
            Counting.calls += 1
            return HostEngine.ring_currents(self, *args)

    def fake(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None, **kw):
        got = [dict(r) for r in recs]
        if kw.get("ring_currents"):
            for r, extra in zip(got, aromaticity.ring_current_fields(got, dataset, engine=engine)):
                r.update(extra)
        return got

    monkeypatch.setattr(G, "rings_to_atoms", fake)
    given = [(np.zeros((1, 3), np.float32), np.zeros(1, np.int64)) for _ in recs]
    plain, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Counting())
    assert Counting.calls == 0 and not any("ring_current" in k or "paratropic" in k for k in plain)
    off, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Counting(), ring_currents=False)
    assert Counting.calls == 0 and set(off) == set(plain)
    d, _ = analyze.analyze_atoms_for_molecules(given, dataset=DATASET, engine=Counting(), ring_currents=True)
    assert Counting.calls == 1 and set(d) == set(plain) | {"mol_ring_current_max", "paratropic_fraction"}
    assert all(np.array_equal(d[k], plain[k]) for k in plain)
    assert np.array_equal(d["mol_ring_current_max"], ext["ring_current_max"], equal_nan=True)
    solved = ext["ring_current_min"][~np.isnan(ext["ring_current_min"])]
    assert d["paratropic_fraction"] == (solved < 0).sum() / float(len(solved)) and 0.0 < d["paratropic_fraction"] < 1.0
    import torch
    x, one_hot, mask = torch.zeros(1, 2, 3), torch.zeros(1, 2, 4), torch.ones(1, 2, 1)
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance._evaluate(None, None, None, None, None, 1.0, x, one_hot, mask, None, 1.0, ring_currents=True)
