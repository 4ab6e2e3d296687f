"""Hueckel localization energies on the device (csrc/reactivity.inc): gaudi_reactivity against the kernel's host build, bit for bit
in all thirteen outputs -- the whole of g32, the tier-edge sizes in one mixed call and alone, batches of 1, 2, 3 and 129, every
way of slicing a molecule's jobs over waves, the 128-centre chain (255 solves in one molecule) and the 11-ring acene -- and the
layers on top through a real Engine.  Only here do the 64 lanes, the (molecule, slice) grid, the three tiers' launches and the
fences run; what the outputs must satisfy is checked on the host build by tests/test_reactivity_cpu.py, and equality with it
carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests import huckel_helpers as hh
from tests import reactivity_helpers as rx
from tests.bond_order_helpers import fixture, pack
from tests.reactivity_helpers import (BAD_INPUT, EMPTY, OK, OVERFLOW, acene, assert_rows_equal, assert_same_bits, device, hetero_rings,
                                      host, known, row)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def test_g32_equals_the_host_build(engine):
    dev = device(engine, fixture()[1])
    assert_same_bits(dev, rx.g32_host())
    assert (dev["status"] == OK).sum() >= 490 and dev["n_jobs"].max() > 60


def test_the_tier_edges_in_one_mixed_call_and_alone(engine):
    mols = hh.size_molecules()[:-2] + [known("pyrene"), hetero_rings()[0]]  # (127 and 128 centres: the test of the long jobs below)
    ref = host(mols)
    dev = device(engine, mols)
    assert_same_bits(dev, ref)
    assert dev["n_pi"].tolist() == list(hh.SIZES[:-2]) + [16, 5]
    packed = pack(mols)
    for i in (0, 1, 2, 4, 5, 7, 8):  # 1, 2, 3, 32, 33, 64, 65 centres alone
        alone = device(engine, [mols[i]])
        assert_rows_equal(row(alone, 0, packed[1][i], packed[3][i]), row(ref, i, packed[1][i], packed[3][i]))


@pytest.mark.parametrize("B", [1, 2, 3, 129])
def test_batch_sizes(engine, B):
    pool = [known("naphthalene"), hetero_rings()[2], hh.polyene(5), known("benzene"), acene(3)]
    mols = [pool[k % len(pool)] for k in range(B)]
    charge = np.array([(0, 1, -1)[k % 3] for k in range(B)], np.int32)
    assert_same_bits(device(engine, mols, charge), host(mols, charge))


def test_slices_and_the_profile(engine):
    mols = [known("pyrene"), hh.polyene(33), hetero_rings()[0], acene(11), known("benzene"), hh.polyene(65)]
    ref = host(mols)
    engine.profile_reset(True)
    assert engine.reactivity_profile_get() == (0, 0.0)
    for k, slices in enumerate((0, 1, 7)):
        assert_same_bits(device(engine, mols, slices=slices), ref)
        n, ms = engine.reactivity_profile_get()
        assert n == 3 * (k + 1) and ms > 0.0  # 16, 5 and 6 centres; 33 and 46; 65: one launch per tier present
    engine.profile_reset(False)
    device(engine, [known("benzene")])
    assert engine.reactivity_profile_get()[0] == 0
    assert ref["n_jobs"].tolist()[3:] == [135, 15, 129]
    without = device(engine, mols, with_bonds=False, slices=5)
    assert_same_bits(without, host(mols, with_bonds=False))
    assert_same_bits(without, ref, skip=("ortho_localization", "n_jobs", "sweeps"))


def test_the_long_jobs(engine):
    """255 solves in one molecule (the 128-centre chain, the largest tier), 253 in the 127-centre one, 135 in the 11-ring acene; 36
    hexagons and 63 squares, of which the rings of the lowest centres are kept: against the host build's recorded results
    (tests/golden/reactivity_long_jobs.npz, which tests/test_reactivity_cpu.py holds to the live host build)."""
    chains, rings = rx.long_molecules()
    want_chains, want_rings = rx.long_host()
    dev = device(engine, chains)
    assert_same_bits(dev, want_chains)
    assert dev["n_jobs"].tolist() == [253, 255] and dev["status"].tolist() == [OK] * 2
    dev = device(engine, rings, with_bonds=False)
    assert_same_bits(dev, want_rings)
    assert dev["flags"].tolist() == [rx.RINGS_TRUNCATED] * 2 and dev["n_pi"].tolist() == [96, 128]
    mol = acene(11)
    dev, ref = device(engine, [mol]), host([mol])
    assert_same_bits(dev, ref)
    assert dev["n_jobs"].tolist() == [135] and abs(np.nanmin(dev["para_localization"][0]) - 3.1250) < rx.TEXTBOOK_TOL


def test_refused_molecules_leave_their_neighbours_untouched(engine):
    benz, naph = known("benzene"), known("naphthalene")
    empty = (np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    mols = [benz, acene(33), naph, empty, benz, naph]
    charge = np.array([0, 0, 0, 0, 9, 0], np.int32)
    dev, ref = device(engine, mols, charge), host(mols, charge)
    assert_same_bits(dev, ref)
    assert dev["status"].tolist() == [OK, OVERFLOW, OK, EMPTY, BAD_INPUT, OK]
    for k in _lib.REACTIVITY_ARRAYS:
        if k != "status":
            assert not dev[k][[1, 3, 4]].view(np.uint32 if dev[k].dtype == np.float32 else dev[k].dtype).any(), k
    t = rx.c_tables()
    t.n_classes = 17
    bad = engine.reactivity(t, *pack([benz]), None)
    assert bad["status"].tolist() == [rx.BAD_TABLE] and not bad["atom_localization"].view(np.uint32).any()


def test_rings_to_atoms_with_reactivity(golden, engine):
    from gaudi_amd import reactivity
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    from tests.gor2goa_helpers import unpack
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "hetro"][:12]
    mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    plain_recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine)
    engine.profile_reset(True)
    off = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine, reactivity=False)
    assert engine.reactivity_profile_get()[0] == 0 and all(set(r) == set(p) for r, p in zip(off, plain_recs))
    recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine, reactivity=True)
    assert 1 <= engine.reactivity_profile_get()[0] <= 3
    engine.profile_reset(False)
    added = {"min_atom_localization", "min_para_localization", "reactivity_status"}
    ext = reactivity.most_reactive(plain_recs, "hetro", bonds=False, engine=engine)
    assert sum(r["reactivity_status"] == OK for r in recs) >= 6
    for k, (r, p) in enumerate(zip(recs, plain_recs)):
        assert set(r) == set(p) | added and all(np.array_equal(r[key], p[key]) for key in p)
        assert r["reactivity_status"] == ext["status"][k] and (r["reactivity_status"] != EMPTY or r["status"] != 0)
        assert np.array_equal([r["min_atom_localization"], r["min_para_localization"]],
                              [ext["min_atom_localization"][k], ext["min_para_localization"][k]], equal_nan=True)
    plain, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine)
    d, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine, reactivity=True)
    assert set(d) == set(plain) | {"mol_min_para_localization", "mol_min_atom_localization"} and all(np.array_equal(d[k], plain[k]) for k in plain)
    assert len(d["mol_min_para_localization"]) == sum(r["status"] == 0 for r in recs)


def test_design_with_reactivity():
    import types

    import torch  # noqa: F401
    from gaudi_amd import generation_guidance, reactivity, synth
    from gaudi_amd.models_edm import get_cond_predictor_model, get_model
    from tests.helpers import TINY, TINY_P
    eargs = synth.edm_args(dataset="cata", diffusion_steps=40, **TINY)
    pargs = synth.pred_args(dataset="cata", **TINY_P)
    model, _, _ = get_model(eargs, state_dict=synth.synth_edm_state_dict(eargs, 1, seed=3))
    cp = get_cond_predictor_model(pargs, model=model, state_dict=synth.synth_predictor_state_dict(pargs, 1, 5, seed=4))
    model.seed = 5
    args = types.SimpleNamespace(device="cuda", dataset="cata", max_nodes=9, batch_size=6)

    def tf_gap(z, nm, em, t):
        return -cp(z, nm, em, t)[:, 1]

    plain = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True)
    model.sample_offset = 0
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, reactivity=True)
    assert set(out) == set(plain) | {"min_para_localization", "min_atom_localization"}
    for k in ("fingerprints", "mol_unique", "best"):
        assert np.array_equal(out[k], plain[k]), k
    ext = reactivity.most_reactive(out["atoms"], "cata", bonds=False, engine=model.engine)
    assert out["min_para_localization"].shape == (6,) and out["min_para_localization"].dtype == np.float64
    assert np.array_equal(out["min_para_localization"], ext["min_para_localization"], equal_nan=True)
    assert np.array_equal(out["min_atom_localization"], ext["min_atom_localization"], equal_nan=True)
    for rec, st in zip(out["atoms"], ext["status"]):
        assert (st == EMPTY) == (rec["status"] != 0)
    model.engine.close()
