"""Hueckel-London ring currents on the device (csrc/ring_current.inc): gaudi_ring_currents against the kernel's host build, bit for bit
in all fifteen outputs -- the whole of g30, the tier-edge set (31 / 32 / 33, 63 / 64 / 65, 127 / 128 centres) and the textbook
molecules in one batch and again in shuffled order, refused molecules among solved ones -- and the layers on top through a real
Engine.  Only here do the 64 lanes, the three tiers' launches and the fences run; what the outputs must satisfy is checked on the
host build by tests/test_ring_current_cpu.py, and equality with it carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests import ppp_helpers as pp
from tests.gor2goa_helpers import unpack
from tests.ring_current_helpers import (BAD_GEOMETRY, EMPTY, OK, OPEN_SHELL, OVERFLOW, SMALL_GAP, acene, assert_same_bits, cyclobutadiene,
                                        device, g30_host, g30_molecules, host, known)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


@pytest.fixture(scope="module")
def batch():
    """g30, the tier-edge set, benzene and naphthalene with the charges that close their shells, and the host build's outputs."""
    edge, edge_charge = pp.edge_set()
    mols = list(g30_molecules()) + list(edge) + [known("benzene"), known("naphthalene")]
    charge = np.concatenate([np.zeros(160, np.int32), edge_charge, np.zeros(2, np.int32)])
    ref = host(mols, charge)
    for a in ref.values():
        a.setflags(write=False)
    return mols, charge, ref


def test_one_batch_equals_the_host_build(engine, batch):
    mols, charge, ref = batch
    dev = device(engine, mols, charge)
    assert_same_bits(dev, ref)
    st = np.bincount(dev["status"], minlength=10)
    assert (st[OK], st[OPEN_SHELL], st[SMALL_GAP], st[OVERFLOW]) == (155 + 14, 1, 3, 1) and st.sum() == len(mols)
    assert dev["n_pi"][160:172].tolist() == list(pp.EDGE_SIZES) and dev["n_rings"][-2:].tolist() == [1, 2]
    for k in ("status", "n_rings", "ring_atoms", "ring_current", "ring_area", "gap", "residual"):  # g30 alone gave the host the same bits
        assert dev[k][:160].tobytes() == g30_host()[k].tobytes(), k


def test_the_shuffled_batch_equals_it_too(engine, batch):
    mols, charge, ref = batch
    order = np.random.default_rng(71).permutation(len(mols))
    dev = device(engine, [mols[i] for i in order], charge[order])
    assert_same_bits(dev, ref, rows=order)


def test_refused_molecules_leave_their_neighbours_untouched(engine):
    benz, naph = known("benzene"), known("naphthalene")
    nan = (benz[0], benz[1], benz[2].copy())
    nan[2][2, 0] = np.inf
    empty = (np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 3)))
    mols = [benz, cyclobutadiene(), naph, acene(33), benz, nan, empty, naph, benz]
    charge = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0], np.int32)
    dev, ref = device(engine, mols, charge), host(mols, charge)
    assert_same_bits(dev, ref)
    assert dev["status"].tolist() == [OK, SMALL_GAP, OK, OVERFLOW, OPEN_SHELL, BAD_GEOMETRY, EMPTY, OK, OK]
    for k in _lib.RING_CURRENT_ARRAYS:
        if k != "status":
            assert not dev[k][[1, 3, 4, 5, 6]].any(), k
    alone = device(engine, [benz, naph])
    for i, j in ((0, 0), (2, 1), (7, 1), (8, 0)):
        for k in _lib.RING_CURRENT_ARRAYS:
            a = alone[k][j]
            assert dev[k][i][..., :a.shape[-1]].tobytes() == a.tobytes() if k == "bond_current" else dev[k][i].tobytes() == a.tobytes(), (k, i)
    assert abs(dev["ring_current"][0, 0] - 1.0) < 1e-5


def test_the_profile_counts_one_launch_per_tier(engine):
    engine.profile_reset(True)
    assert engine.ring_currents_profile_get() == (0, 0.0)
    device(engine, [known("benzene"), acene(10), known("naphthalene")])  # 6 and 10 centres: one tier; 42: the next
    n, ms = engine.ring_currents_profile_get()
    assert n == 2 and ms > 0.0
    engine.profile_reset(False)
    device(engine, [known("benzene")])
    assert engine.ring_currents_profile_get()[0] == 0


def test_rings_to_atoms_with_ring_currents(golden, engine):
    from gaudi_amd import aromaticity
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "hetro"][:24]
    mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    plain_recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine)
    engine.profile_reset(True)
    off = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine, ring_currents=False)
    assert engine.ring_currents_profile_get()[0] == 0 and all(set(r) == set(p) for r, p in zip(off, plain_recs))
    recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine, ring_currents=True)
    assert 1 <= engine.ring_currents_profile_get()[0] <= 3
    engine.profile_reset(False)
    added = {"ring_current_max", "ring_current_min", "ring_current_status"}
    res = aromaticity.ring_currents(plain_recs, "hetro", engine=engine)
    assert sum(r["status"] == 0 for r in recs) >= 16 and sum(r["ring_current_status"] == OK for r in recs) >= 12
    for r, p, o in zip(recs, plain_recs, res):
        assert set(r) == set(p) | added and all(np.array_equal(r[k], p[k]) for k in p)
        assert r["ring_current_status"] == o["status"] and (r["ring_current_status"] != EMPTY or r["status"] != 0)
        assert np.array_equal([r["ring_current_max"], r["ring_current_min"]], [o["ring_current_max"], o["ring_current_min"]], equal_nan=True)
        if o["status"] == OK and o["rings"]:
            assert r["ring_current_max"] == o["ring_current"].max() and r["ring_current_min"] == o["ring_current"].min()
    plain, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine)
    d, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine, ring_currents=True)
    assert set(d) == set(plain) | {"mol_ring_current_max", "paratropic_fraction"} and all(np.array_equal(d[k], plain[k]) for k in plain)
    assert len(d["mol_ring_current_max"]) == sum(r["status"] == 0 for r in recs) and 0.0 <= d["paratropic_fraction"] <= 1.0
    ext = aromaticity.ring_current_extremes(plain_recs, "hetro", engine=engine)
    assert np.array_equal(ext["ring_current_max"], [r["ring_current_max"] for r in recs], equal_nan=True)


def test_design_with_ring_currents():
    import types

    import torch  # noqa: F401
    from gaudi_amd import aromaticity, generation_guidance, synth
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
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, ring_currents=True)
    assert set(out) == set(plain) | {"ring_current_max", "ring_current_min"}
    for k in ("fingerprints", "mol_unique", "best"):
        assert np.array_equal(out[k], plain[k]), k
    ext = aromaticity.ring_current_extremes(out["atoms"], "cata", engine=model.engine)
    assert out["ring_current_max"].shape == (6,) and out["ring_current_max"].dtype == np.float64
    assert np.array_equal(out["ring_current_max"], ext["ring_current_max"], equal_nan=True)
    assert np.array_equal(out["ring_current_min"], ext["ring_current_min"], equal_nan=True)
    for rec, st in zip(out["atoms"], ext["status"]):
        assert (st == EMPTY) == (rec["status"] != 0)
    model.engine.close()
