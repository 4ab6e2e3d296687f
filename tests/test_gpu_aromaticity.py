"""Kekule counts on the device (csrc/kekule.inc): gaudi_kekule against the kernel's host build, bit for bit in all nine outputs --
golden g32 plus the hand-made molecules, the batch sizes around a workgroup, the small shapes of the search (one edge; a queue
that never fills; more open nodes than lanes), a molecule's place in the batch, the budget -- and the layers on top through a
real Engine.  Only here do the 64-lane queue and the LDS counters run; what the outputs must satisfy is checked on the host build
by tests/test_aromaticity_cpu.py, and equality with it carries that over."""
import numpy as np
import pytest

from tests.aromaticity_helpers import (EMPTY, OK, UNDECIDED, assert_same_bits, device, g32_host, hand_made, host, ladder, molecule,
                                       polyene, row)
from tests.bond_order_helpers import fixture
from tests.gor2goa_helpers import unpack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def test_the_fixture_and_the_hand_made_molecules_equal_the_host_build(g32, engine):
    mols = [(m["elem"], m["bonds"]) for m in g32[1]] + hand_made()
    dev, ref = device(engine, mols), host(mols)
    assert_same_bits(dev, ref)
    n = len(g32[1])
    assert all(dev[k][:n, ...].tobytes() == np.ascontiguousarray(g32_host()[k][:n, ...]).tobytes() for k in ("k", "status", "n_nodes", "clar"))
    st = np.bincount(dev["status"], minlength=9)
    assert st[OK] >= 265 and (st[1:8] >= 1).all() and st[UNDECIDED] == 0 and dev["k"].max() == 256


@pytest.mark.parametrize("B", [1, 3])
def test_batches_whose_last_workgroup_has_an_idle_wave(g32, engine, B):
    ref = g32_host()
    mols = sorted((m for m in g32[1] if ref["status"][m["index"]] == OK), key=lambda m: -int(ref["n_nodes"][m["index"]]))[:B]
    dev = device(engine, mols)
    assert_same_bits(dev, host(mols))
    assert (dev["status"] == OK).all() and dev["n_nodes"].min() > 1000


def test_small_search_shapes(engine):
    ethylene = polyene(2)
    mols = [ethylene, polyene(10), molecule("benzene"), ladder(12)]
    dev = device(engine, mols)
    assert_same_bits(dev, host(mols))
    assert dev["status"].tolist() == [OK] * 4 and dev["k"].tolist() == [1, 1, 2, 233] and dev["n_nodes"].tolist()[:3] == [2, 6, 7]
    for i, m in enumerate(mols):  # and alone
        assert row(device(engine, [m]), 0, len(m[1])) == row(dev, i, len(m[1]))


def test_the_place_in_the_batch_leaves_no_trace(g32, engine):
    ref = g32_host()
    m = max((m for m in g32[1] if ref["status"][m["index"]] == OK), key=lambda m: int(ref["n_hex"][m["index"]]))
    others = [(o["elem"], o["bonds"]) for o in g32[1][40:47]] + [ladder(12), molecule("coronene")]
    me = (m["elem"], m["bonds"])
    want = row(ref, m["index"], len(m["bonds"]))
    assert want[0] == OK and want[3] >= 10
    for place, batch in ((0, [me] + others), (1, others[:1] + [me] + others[1:]), (len(others), others[::-1] + [me])):
        assert row(device(engine, batch), place, len(m["bonds"])) == want


def test_the_budget_bounds_the_work(engine):
    benz = molecule("benzene")
    mols = [benz, ladder(30), benz]
    dev = device(engine, mols)
    assert_same_bits(dev, host(mols))
    assert dev["status"].tolist() == [OK, UNDECIDED, OK] and dev["k"].tolist() == [2, 0, 2] and dev["n_nodes"].tolist() == [7, 0, 7]
    assert not dev["double_count"][1].any() and not dev["sextet_count"][1].any()


def test_bad_tables_and_the_profile(engine):
    from gaudi_amd import _lib
    from tests.aromaticity_helpers import tables
    from tests.bond_order_helpers import pack
    t = tables()
    t.n_elems = 9
    with pytest.raises(_lib.GaudiError):
        engine.kekule(t, *pack([molecule("benzene")]))
    engine.profile_reset(True)
    assert engine.kekule_profile_get() == (0, 0.0)
    device(engine, [molecule("benzene"), molecule("naphthalene"), ladder(12)])
    n, ms = engine.kekule_profile_get()
    assert n == 1 and ms > 0.0  # one launch per call
    engine.profile_reset(False)
    device(engine, [molecule("benzene")])
    assert engine.kekule_profile_get()[0] == 0


def test_the_layers_on_top_through_an_engine(golden, engine):
    from gaudi_amd import aromaticity
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "hetro"][:40]
    mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    plain_recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine)
    recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine, aromaticity=True)
    added = {"kekule_count", "clar", "fries", "max_pauling_order", "resonance_status"}
    res = aromaticity.resonance(plain_recs, "hetro", engine=engine)
    raw = host([(r["atom_types"].astype(np.int32), r["bonds"].astype(np.int32)) if r["status"] == 0 else (np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
                for r in plain_recs])
    assert sum(r["status"] == 0 for r in recs) >= 30
    for j, (r, p, o) in enumerate(zip(recs, plain_recs, res)):
        assert set(r) == set(p) | added and all(np.array_equal(r[k], p[k]) for k in p)
        assert (r["resonance_status"], r["kekule_count"], r["clar"], r["fries"]) == (o["status"], o["kekule_count"], o["clar"], o["fries"])
        assert (o["status"], o["kekule_count"], o["clar"], o["n_nodes"]) == (raw["status"][j], raw["k"][j], raw["clar"][j], raw["n_nodes"][j])
        assert r["resonance_status"] != EMPTY or r["status"] != 0
        if o["status"] == OK:
            assert r["max_pauling_order"] == o["pauling_bond_order"].max() and 0.0 < r["max_pauling_order"] <= 1.0
        else:
            assert np.isnan(r["max_pauling_order"]) and r["kekule_count"] == 0
    assert sum(r["kekule_count"] >= 2 for r in recs) >= 10
    plain, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine)
    engine.profile_reset(True)
    d, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine, aromaticity=True)
    assert engine.kekule_profile_get()[0] == 1
    engine.profile_reset(False)
    assert set(d) == set(plain) | {"mol_kekule_count", "mol_clar", "mean_log_kekule_per_center"} and all(np.array_equal(d[k], plain[k]) for k in plain)
    # hydrogens implied (as analyze builds them) or placed: the same counts
    assert d["mol_kekule_count"].tolist() == [r["kekule_count"] for r in recs if r["status"] == 0]
    assert d["mol_clar"].tolist() == [r["clar"] for r in recs if r["status"] == 0] and d["mean_log_kekule_per_center"] > 0.0
    assert np.array_equal(aromaticity.kekule_count(plain_recs, "hetro", engine=engine), [r["kekule_count"] for r in recs])
    assert np.array_equal(aromaticity.clar_number(plain_recs, "hetro", engine=engine), [r["clar"] for r in recs])


def test_design_with_aromaticity():
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
    off = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, aromaticity=False)
    model.sample_offset = 0
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, aromaticity=True)
    assert set(off) == set(plain) and set(out) == set(plain) | {"kekule_count", "clar"}
    for k in ("fingerprints", "mol_unique", "best"):
        assert np.array_equal(off[k], plain[k]) and np.array_equal(out[k], plain[k]), k
    assert np.array_equal(off["target_function_values"], plain["target_function_values"])
    assert out["kekule_count"].shape == (6,) and out["kekule_count"].dtype == np.int64 and out["clar"].shape == (6,)
    assert np.array_equal(out["kekule_count"], aromaticity.kekule_count(out["atoms"], "cata", engine=model.engine))
    assert np.array_equal(out["clar"], aromaticity.clar_number(out["atoms"], "cata", engine=model.engine))
    for rec, k in zip(out["atoms"], out["kekule_count"]):
        assert (k > 0) == (rec["status"] == 0 and aromaticity.resonance([rec], "cata", engine=model.engine)[0]["status"] == OK)
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, aromaticity=True)
    ref = generation_guidance.refine(args, model, cp, tf_gap, out["x"], out["one_hot"], out["node_mask"], out["edge_mask"],
                                     t_start=10, scale=0.6, n_steps=5, with_atoms=True, aromaticity=True)
    assert ref["kekule_count"].shape == (6,) and ref["clar"].shape == (6,)
    model.engine.close()
