"""Hueckel localization energies (csrc/reactivity.inc) on the kernel's HOST build (gaudi_host_reactivity: the
same source text run serially) against the float64 oracle of tests/reactivity_helpers.py, the textbook values, and its own bits
under every way of cutting the work.  No device."""
import hashlib
import os

import numpy as np
import pytest

from gaudi_amd import _lib
from tests import huckel_helpers as hh
from tests import reactivity_helpers as rx
from tests import ring_current_helpers as rc
from tests.bond_order_helpers import C, fixture, pack
from tests.reactivity_helpers import (BAD_INPUT, BAD_TABLE, EMPTY, NO_PI, OK, OVERFLOW, RINGS_TRUNCATED, TEXTBOOK, TEXTBOOK_TOL, TOL,
                                      HostEngine, acene, assert_rows_equal, assert_same_bits, c_tables, flake, hetero_rings, host,
                                      known, minima, oracle, record, row, worst)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = np.uint32(rx.NAN_BITS)
# sha256 over the output arrays of gaudi_host_huckel on g32 and of gaudi_host_ring_currents on g30 (in _lib.HUCKEL_ARRAYS /
# _lib.RING_CURRENT_ARRAYS order), recorded on the commit before reactivity.inc was included: their bits must not move
HUCKEL_G32_SHA256 = "ca24678175a21202b346c4b5fb44b5e612856495700eb81106f964f2fd7ac51d"
RING_CURRENT_G30_SHA256 = "a34e4bf3ca26da6594bed77a8bf72ab2adfdd614cf147b6ceb509364b093697a"


def check_against_oracle(mols, charge=0, with_bonds=True):
    """Every molecule's host result against the oracle: the same entries defined, the worst error returned."""
    out = host(mols, charge, with_bonds=with_bonds)
    err = 0.0
    for i, m in enumerate(mols):
        want = oracle(m, charge, with_bonds)
        got = record(out, i, m)
        err = max(err, worst(got, want, free_valence=want["unique_orders"]))
        assert abs(want["e_pi"] - hh.oracle(m, charge)["e_pi"]) < 1e-9  # this file's matrix is huckel_helpers.oracle's
    return out, err


def test_textbook_values():
    for name, (make, e_pi, atom, para, ortho) in TEXTBOOK.items():
        mol = make()
        out = host([mol])
        got, want = record(out, 0, mol), oracle(mol)
        a, p, o = minima(got, want["with_h"])
        print(name, got["n_jobs"], got["e_pi"], a, p, o)
        assert got["status"] == OK and got["flags"] == 0
        for value, listed in ((got["e_pi"], e_pi), (a, atom), (p, para), (o, ortho)):
            assert listed is None or abs(value - listed) <= TEXTBOOK_TOL, (name, value, listed)
        # an alternant hydrocarbon: the three kinds agree
        L = got["atom_localization"]
        assert np.nanmax(np.abs(L - L[1])) <= TOL, name
        assert worst(got, want) <= TOL
    mol = TEXTBOOK["acene11"][0]()
    assert int(host([mol])["n_jobs"][0]) == 135
    # where they occur: anthracene's position 9 and its 9,10 pair; naphthalene's alpha and beta positions; phenanthrene's 9,10 bond
    mol = known("anthracene")
    got = record(host([mol]), 0, mol)
    deg = np.bincount(mol[1].reshape(-1), minlength=len(mol[0]))
    nbr = {a: set(mol[1][(mol[1] == a).any(1)].reshape(-1)) - {a} for a in range(len(mol[0]))}
    meso = [a for a in range(len(mol[0])) if deg[a] == 2 and all(deg[b] == 3 for b in nbr[a])]
    assert len(meso) == 2 and int(np.nanargmin(np.where(deg == 2, got["atom_localization"][1], np.nan))) in meso
    k, p = divmod(int(np.nanargmin(got["para_localization"])), 3)
    assert {got["rings"][k][p], got["rings"][k][p + 3]} == set(meso)
    mol = known("naphthalene")
    got = record(host([mol]), 0, mol)
    deg = np.bincount(mol[1].reshape(-1), minlength=10)
    nbr = {a: set(mol[1][(mol[1] == a).any(1)].reshape(-1)) - {a} for a in range(10)}
    alpha = [a for a in range(10) if deg[a] == 2 and any(deg[b] == 3 for b in nbr[a])]
    beta = [a for a in range(10) if deg[a] == 2 and a not in alpha]
    assert np.abs(got["atom_localization"][1][alpha] - 2.2986).max() <= TEXTBOOK_TOL
    assert np.abs(got["atom_localization"][1][beta] - 2.4797).max() <= TEXTBOOK_TOL
    mol = known("phenanthrene")
    got = record(host([mol]), 0, mol)
    deg = np.bincount(mol[1].reshape(-1), minlength=14)
    i, j = mol[1][int(np.nanargmin(got["ortho_localization"]))]
    assert deg[i] == 2 and deg[j] == 2  # the 9,10 bond joins two CH centres ...
    assert all(deg[b] == 3 for b in set(mol[1][(mol[1] == i).any(1)].reshape(-1)) - {i, j})  # ... each next to a ring fusion


@pytest.mark.parametrize("charge", [-1, 0, 1])
def test_every_g32_molecule_equals_the_oracle(charge):
    mols = fixture()[1]
    out, err = check_against_oracle(mols, charge)
    print(f"g32 charge {charge}: worst error {err:.3e}, statuses {np.bincount(out['status']).tolist()}")
    assert err <= TOL
    assert (out["status"] == OK).sum() >= 490


def test_the_tier_edges_equal_the_oracle():
    mols = hh.size_molecules()
    out, err = check_against_oracle(mols)
    print(f"sizes {hh.SIZES}: worst error {err:.3e}, jobs {out['n_jobs'].tolist()}")
    assert err <= TOL and out["status"].tolist() == [OK] * len(mols)
    assert out["n_pi"].tolist() == list(hh.SIZES)
    assert out["n_jobs"].tolist() == [n + (n - 1) for n in hh.SIZES]  # a chain: its centres and its bonds, no ring
    assert (out["sweeps"][3:] > out["n_jobs"][3:]).all()  # (a single centre needs no sweep at all)
    # the recorded results the device tests compare the two longest chains with are the host build's
    packed = pack(mols)
    for k in (-2, -1):
        assert_rows_equal(row(rx.long_host()[0], k, packed[1][k], packed[3][k]), row(out, k, packed[1][k], packed[3][k]))
    # a single centre: only the radical kind is defined, and it costs nothing; the two-centre chain's bond leaves an empty system
    one = record(out, 0, mols[0])
    assert np.isnan(one["atom_localization"][[0, 2], 0]).all() and one["atom_localization"][1, 0] == 0.0
    two = record(out, 1, mols[1])
    assert two["ortho_localization"][0] == 2.0 and two["e_pi"] == 2.0


def test_five_rings_with_a_heteroatom():
    mols = hetero_rings()
    out, err = check_against_oracle(mols)
    print(f"pyrrole, furan, thiophene, borole: worst error {err:.3e}")
    assert err <= TOL and out["status"].tolist() == [OK] * 4 and out["n_rings"].tolist() == [1] * 4
    assert out["n_electrons"].tolist() == [6, 6, 6, 4]
    for i, m in enumerate(mols):
        got = record(out, i, m)
        assert len(got["rings"][0]) == 5 and np.isnan(got["para_localization"]).all()  # a five-ring has no opposite positions
        L = got["atom_localization"][:, :5]
        assert not np.isnan(L).any() and np.abs(L[2] - L[0]).max() > 0.1  # not alternant: the kinds differ, and h_r entered
    # pyrrole reacts with electrophiles at the carbons next to the nitrogen
    L = record(out, 0, mols[0])["atom_localization"][2]
    assert int(np.nanargmin(L[:4])) in (0, 3)


def test_more_than_32_rings_are_truncated_by_smallest_centre():
    mols = rx.long_molecules()[1]
    out, err = check_against_oracle(mols, with_bonds=False)
    assert_same_bits(out, rx.long_host()[1])  # the recorded results the device tests use are the host build's
    print(f"36 hexagons, 63 four-rings: worst error {err:.3e}, kept {out['n_rings'].tolist()}")
    assert err <= TOL and out["flags"].tolist() == [RINGS_TRUNCATED] * 2
    assert 28 <= out["n_rings"][0] <= 32 and 28 <= out["n_rings"][1] <= 32
    assert np.isnan(out["para_localization"][1]).all() and out["n_jobs"][1] == 128
    assert out["n_jobs"][0] == 96 + 3 * out["n_rings"][0]


def test_slices_batches_and_bonds_do_not_move_a_bit():
    mols = [known("pyrene"), hh.polyene(33), hetero_rings()[0], acene(5), hh.polyene(65), known("benzene")]
    one = host(mols, slices=1)
    for slices in (0, 5, 16):
        assert_same_bits(host(mols, slices=slices), one)
    # a molecule alone gives the bytes of its row in the mixed batch
    packed = pack(mols)
    for i, m in enumerate(mols):
        alone = host([m], slices=3)
        assert_rows_equal(row(alone, 0, packed[1][i], packed[3][i]), row(one, i, packed[1][i], packed[3][i]))
    # ... and so does every molecule of g32 that the fixture's batch solved
    g32 = rx.g32_host()
    picks = [i for i in range(0, len(fixture()[1]), 37)]
    sub = host([fixture()[1][i] for i in picks], slices=4)
    full = pack(fixture()[1])
    for k, i in enumerate(picks):
        assert_rows_equal(row(sub, k, full[1][i], full[3][i]), row(g32, i, full[1][i], full[3][i]))
    # with_bonds = 0: only the ortho values and the job count differ
    without = host(mols, with_bonds=False, slices=2)
    assert_same_bits(without, one, skip=("ortho_localization", "n_jobs", "sweeps"))
    for i in range(len(mols)):
        assert (without["ortho_localization"][i].view(np.uint32) == NAN_BITS).all()
        n_pib = int((~np.isnan(one["ortho_localization"][i])).sum())
        assert without["n_jobs"][i] == one["n_jobs"][i] - n_pib and without["sweeps"][i] < one["sweeps"][i]
    # every NaN is THE quiet NaN
    for k in ("atom_localization", "free_valence", "para_localization", "ortho_localization"):
        bits = one[k].view(np.uint32)
        assert (bits[np.isnan(one[k])] == NAN_BITS).all(), k


def test_huckel_and_ring_current_bits_did_not_move():
    def digest(out, names):
        h = hashlib.sha256()
        for k in names:
            h.update(out[k].tobytes())
        return h.hexdigest()
    assert digest(hh.g32_host(), _lib.HUCKEL_ARRAYS) == HUCKEL_G32_SHA256
    assert digest(rc.g30_host(), _lib.RING_CURRENT_ARRAYS) == RING_CURRENT_G30_SHA256
    # ... and the parent energy this kernel reports is gaudi_huckel's, bit for bit
    assert rx.g32_host()["e_pi"].tobytes() == np.where(hh.g32_host()["status"] == OK, hh.g32_host()["e_pi"], 0).astype(np.float32).tobytes()
    assert rx.g32_host()["status"].tolist() == hh.g32_host()["status"].tolist()


def test_refusals_and_undefined_kinds():
    benz = known("benzene")
    methane = hh.with_h(np.array([C], np.int32), np.zeros((0, 2), np.int32), [4])
    empty = (np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    cases = [(benz, 9, BAD_INPUT), (benz, -9, BAD_INPUT), (methane, 0, NO_PI), (empty, 0, EMPTY), (acene(33), 0, OVERFLOW),
             ((benz[0], np.array([(0, 9)], np.int32)), 0, BAD_INPUT)]
    mols = [benz] + [m for m, _, _ in cases] + [known("naphthalene")]
    charge = np.array([0] + [c for _, c, _ in cases] + [0], np.int32)
    out = host(mols, charge)
    assert out["status"].tolist() == [OK] + [s for _, _, s in cases] + [OK]
    for k in _lib.REACTIVITY_ARRAYS:
        if k != "status":
            assert not out[k][1:1 + len(cases)].view(np.uint32 if out[k].dtype == np.float32 else out[k].dtype).any(), k  # zero rows, not NaN
    for m, c, s in cases:
        assert oracle(m, c)["status"] == s
    alone = host([benz, known("naphthalene")])
    packed = pack(mols)
    for k, i in ((0, 0), (1, len(mols) - 1)):
        assert_rows_equal(row(alone, k, packed[1][i], packed[3][i]), row(out, i, packed[1][i], packed[3][i]))
    t = c_tables()
    t.n_classes = 17
    bad = _lib.host_reactivity(t, *pack([benz]), None)
    assert bad["status"].tolist() == [BAD_TABLE] and not bad["atom_localization"].view(np.uint32).any()
    # a charge the parent carries and a residual system does not: benzene with 12 electrons has only its electrophilic kind, with
    # none only its nucleophilic kind; one electron in, two kinds are defined; none of the four has a pair value (a pair keeps two
    # electrons and leaves four centres: 0 <= n_el - 2 <= 8 fails for 12, 11, 1 and 0 electrons)
    for c, kinds in ((-6, [2]), (6, [0]), (-5, [1, 2]), (5, [0, 1])):
        got, want = record(host([benz], c), 0, benz), oracle(benz, c)
        assert got["status"] == OK and worst(got, want, free_valence=want["unique_orders"]) <= TOL
        defined = ~np.isnan(got["atom_localization"][:, :6])
        assert [q for q in range(3) if defined[q].all()] == kinds and all(defined[q].all() or not defined[q].any() for q in range(3))
        assert np.isnan(got["para_localization"]).all() and np.isnan(got["ortho_localization"]).all()
    got = record(host([benz], 4), 0, benz)  # two electrons: the pair values are back
    assert not np.isnan(got["para_localization"]).any() and not np.isnan(got["ortho_localization"]).any()


def test_declarations_and_argument_checks():
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    for name in ("gaudi_reactivity(", "gaudi_host_reactivity(", "gaudi_reactivity_profile_get(", "GAUDI_REACTIVITY_KINDS 3",
                 "GAUDI_REACTIVITY_MAX_SLICES 16", "GAUDI_REACTIVITY_SWEEP_CAP 1", "GAUDI_REACTIVITY_RINGS_TRUNCATED 2"):
        assert name in header, name
    assert "#define GAUDI_ABI_VERSION 7" in header
    assert (_lib.REACTIVITY_KINDS, _lib.REACTIVITY_MAX_SLICES, _lib.REACTIVITY_SWEEP_CAP, _lib.REACTIVITY_RINGS_TRUNCATED) == (3, 16, 1, 2)
    assert len(_lib.REACTIVITY_ARRAYS) == 13
    lib = _lib.load_library()
    assert all(hasattr(lib, n) for n in ("gaudi_reactivity", "gaudi_host_reactivity", "gaudi_reactivity_profile_get"))
    packed = pack([known("benzene")])
    out = _lib.reactivity_outputs(1, packed[0].shape[1], packed[2].shape[1])
    args = list(_lib.reactivity_args(c_tables(), *packed, None, True, 0, out))
    assert lib.gaudi_host_reactivity(*args) == 0 and out["status"][0] == OK
    for missing in (0, 4, 11, 16, 23):  # the table, elem, an output
        broken = list(args)
        broken[missing] = None
        assert lib.gaudi_host_reactivity(*broken) != 0, missing
    for slices in (-1, 17):
        broken = list(args)
        broken[10] = slices
        assert lib.gaudi_host_reactivity(*broken) != 0, slices


def test_the_python_layers(monkeypatch):
    import gaudi_amd.gor2goa as G
    from gaudi_amd import analyze, generation_guidance, reactivity
    named = [known("anthracene"), known("phenanthrene"), hetero_rings()[0], hh.polyene(4), known("benzene")]
    recs = [dict(status=0, atom_types=e.astype(np.int64), bonds=b.astype(np.int64), fingerprint=4000 + i) for i, (e, b) in enumerate(named)]
    recs.insert(2, dict(status=2, fingerprint=0))
    keep = [k for k in range(len(recs)) if k != 2]
    raw = host(named)
    res = reactivity.localization(recs, rx.DATASET, engine=HostEngine())
    assert len(res) == len(recs) and res[2]["status"] == EMPTY and res[2]["status_name"] == "no atoms (not built)"
    assert np.isnan(res[2]["min_para_localization"]) and res[2]["rings"] == [] and len(res[2]["free_valence"]) == 0
    assert set(reactivity.STATUS_NAMES) == set(range(7)) and reactivity.KINDS == ("nucleophilic", "radical", "electrophilic")
    for k, i in zip(keep, range(len(named))):
        r, (e, b) = res[k], named[i]
        want = oracle(named[i])
        assert (r["status"], r["n_pi"], r["n_jobs"], r["sweeps"], r["flags"]) == tuple(int(raw[x][i]) for x in ("status", "n_pi", "n_jobs", "sweeps", "flags"))
        for q, name in enumerate(reactivity.KINDS):
            assert r["atom_localization"][name].tobytes() == raw["atom_localization"][i, q, :len(e)].tobytes()
        assert r["free_valence"].tobytes() == raw["free_valence"][i, :len(e)].tobytes() and r["e_pi"] == raw["e_pi"][i]
        assert r["ortho_localization"].tobytes() == raw["ortho_localization"][i, :len(b)].tobytes()
        assert [a.tolist() for a in r["rings"]] == [list(t) for t in want["rings"]] and r["para_localization"].shape == (len(want["rings"]), 3)
        a, p, o = minima(record(raw, i, named[i]), want["with_h"])
        assert np.array_equal([r["min_atom_localization"], r["min_para_localization"], r["min_ortho_localization"]], [a, p, o], equal_nan=True)
        if not np.isnan(p):
            ring, pair = r["min_para_localization_ring"], r["min_para_localization_pair"]
            assert r["para_localization"][ring, pair] == np.float32(p)
        assert r["atom_localization"]["radical"][r["min_atom_localization_atom"]] == np.float32(a) and want["with_h"][r["min_atom_localization_atom"]]
        assert r["ortho_localization"][r["min_ortho_localization_bond"]] == np.float32(o)
    assert abs(res[0]["min_para_localization"] - 3.3137) < TEXTBOOK_TOL and abs(res[1]["min_ortho_localization"] - 3.0649) < TEXTBOOK_TOL
    assert np.isnan(res[3]["min_para_localization"]) and res[3]["min_para_localization_ring"] == -1  # pyrrole: no six-ring
    assert np.isnan(res[4]["min_para_localization"]) and not np.isnan(res[4]["min_atom_localization"])  # a chain
    ext = reactivity.most_reactive(named, rx.DATASET, engine=HostEngine())
    assert set(ext) == {"min_atom_localization", "min_para_localization", "min_ortho_localization", "status"}
    for key in ("min_atom_localization", "min_para_localization", "min_ortho_localization"):
        assert ext[key].dtype == np.float64 and np.array_equal(ext[key], [res[k][key] for k in keep], equal_nan=True)
    assert reactivity.localization([], rx.DATASET, engine=HostEngine()) == []
    assert reactivity.most_reactive([], rx.DATASET, engine=HostEngine())["status"].shape == (0,)
    refused = reactivity.most_reactive([known("benzene")], rx.DATASET, charge=9, engine=HostEngine())
    assert refused["status"].tolist() == [BAD_INPUT] and np.isnan(refused["min_atom_localization"]).all()
    no_bonds = reactivity.localization([known("benzene")], rx.DATASET, bonds=False, engine=HostEngine())[0]
    assert np.isnan(no_bonds["ortho_localization"]).all() and np.isnan(no_bonds["min_ortho_localization"]) and no_bonds["n_jobs"] == 9
    weak = reactivity.localization([known("benzene")], rx.DATASET, parameters={"classes": {"C": {"k": 0.5}}}, engine=HostEngine())[0]
    assert abs(weak["min_para_localization"] - 0.25 * 4.0) < TOL  # every energy is linear in beta: k_rs = 0.25
    cation = reactivity.localization([known("benzene")], rx.DATASET, charge=1, engine=HostEngine())[0]
    assert cation["n_electrons"] == 5 and cation["status"] == OK
    # rings_to_atoms / analyze_atoms_for_molecules / design on these records (the conversion itself needs a device)
    fields = reactivity.record_fields(recs, rx.DATASET, engine=HostEngine())
    assert set(fields[0]) == {"min_atom_localization", "min_para_localization", "reactivity_status"} and fields[2]["reactivity_status"] == EMPTY
    assert fields[0]["min_para_localization"] == res[0]["min_para_localization"]

    class Counting(HostEngine):
        calls = 0

        def reactivity(self, *args, **kw):
            Counting.calls += 1
            return HostEngine.reactivity(self, *args, **kw)

    def fake(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None, **kw):
        got = [dict(r) for r in recs]
        if kw.get("reactivity"):
            for r, extra in zip(got, reactivity.record_fields(got, dataset, engine=engine)):
                r.update(extra)
        return got

    monkeypatch.setattr(G, "rings_to_atoms", fake)
    given = [(np.zeros((1, 3), np.float32), np.zeros(1, np.int64)) for _ in recs]
    plain, _ = analyze.analyze_atoms_for_molecules(given, dataset=rx.DATASET, engine=Counting())
    assert Counting.calls == 0 and not any("localization" in k for k in plain)
    off, _ = analyze.analyze_atoms_for_molecules(given, dataset=rx.DATASET, engine=Counting(), reactivity=False)
    assert Counting.calls == 0 and set(off) == set(plain)
    d, _ = analyze.analyze_atoms_for_molecules(given, dataset=rx.DATASET, engine=Counting(), reactivity=True)
    assert Counting.calls == 1 and set(d) == set(plain) | {"mol_min_para_localization", "mol_min_atom_localization"}
    assert all(np.array_equal(d[k], plain[k]) for k in plain)
    assert np.array_equal(d["mol_min_para_localization"], ext["min_para_localization"], equal_nan=True)
    assert np.array_equal(d["mol_min_atom_localization"], ext["min_atom_localization"], equal_nan=True)
    import torch
    x, one_hot, mask = torch.zeros(len(recs), 2, 3), torch.zeros(len(recs), 2, 4), torch.ones(len(recs), 2, 1)
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance._evaluate(None, None, None, None, None, 1.0, x, one_hot, mask, None, 1.0, reactivity=True)
    base = generation_guidance._atoms(x, one_hot, mask, rx.DATASET, Counting())
    assert Counting.calls == 1 and not any("localization" in k for k in base)
    more = generation_guidance._atoms(x, one_hot, mask, rx.DATASET, Counting(), reactivity=True)
    assert Counting.calls == 2 and set(more) == set(base) | {"min_para_localization", "min_atom_localization"}
    assert np.isnan(more["min_para_localization"][2]) and np.array_equal(more["min_para_localization"][keep], ext["min_para_localization"], equal_nan=True)


def test_the_host_build_under_the_sanitizers():
    """tools/reactivity_host_check.py: the stand-alone program only (never code loaded into python)."""
    import glob
    import subprocess
    import sys
    if not glob.glob(os.path.join(ROOT, "gaudi_amd", "csrc", "build", "kern*.o")):  # the program links the ordinary build's kernel objects
        from gaudi_amd.build import build
        build(force=True)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "reactivity_host_check.py")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "exit status 0 (clean)" in run.stdout and "own inputs: status counts" in run.stdout
