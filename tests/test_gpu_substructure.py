"""Substructure search on the device (csrc/sub.inc): gaudi_substructure_search against the kernel's host build, bit for bit in
all five outputs -- golden g32 against the named patterns under the four flag settings, the searches that give up, the batch
sizes around a workgroup, one and 64 patterns, a shuffled batch, the root-to-lane boundaries, degree 8, every refusal -- and the
layers on top through a real Engine.  What the outputs must satisfy is checked on the host build by
tests/test_substructure_cpu.py; equality with it carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import C, DATASET, H, fixture
from tests.gor2goa_helpers import unpack
from tests.similarity_helpers import stars
from tests.substructure_helpers import (ARRAYS, BAD_INPUT, BAD_PATTERN, CLOSED, EMPTY, FLAG_SETTINGS, GAVE_UP, H_EXACT, N_, NAMED, OK,
                                        OVERFLOW, S_, device_search, g32_host, grid, host_search, ladder, largest_carbon_molecule,
                                        named_patterns, path, restated, undecided_pattern)

pytestmark = pytest.mark.gpu
REFUSED = {5: BAD_INPUT, 6: OVERFLOW, 7: EMPTY}


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def same(dev, ref):
    for k in ARRAYS:
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape and np.array_equal(dev[k], ref[k]), k


@pytest.mark.parametrize("flags", FLAG_SETTINGS)
def test_the_fixture_equals_the_host_build(g32, engine, flags):
    mols = g32[1]
    assert len(mols) % 2 == 1  # an odd count: the last workgroup has one wave idle
    dev, ref = device_search(engine, mols, named_patterns(), flags), g32_host(flags)
    same(dev, ref)
    for m in mols:
        assert (dev["status"][m["index"]] == REFUSED.get(m["special"], OK)).all()
    if flags == 0:
        assert (dev["count"] > 0).sum(0).tolist()[2:7] == [372, 92, 135, 169, 366] and dev["count"].max() == 4512


def test_giving_up_equals_the_host_build(engine):
    big = largest_carbon_molecule()
    star = (np.array([C] + [S_] * 8, np.int32), np.array([(0, k) for k in range(1, 9)], np.int32))
    mols = [(big["elem"], big["bonds"]), grid(3, 64), star, ladder(192)]
    pats = [path(32), undecided_pattern(), star, NAMED["benzene"]]
    dev, ref = device_search(engine, mols, pats, 0), host_search(mols, pats, 0)
    same(dev, ref)
    assert dev["status"][0, 0] == GAVE_UP and dev["count"][0, 0] > 0 and dev["steps"][0, 0] > _lib.SUB_MAX_STEPS
    assert dev["status"][1, 1] == GAVE_UP and dev["count"][1, 1] == 0  # undecided
    assert dev["status"][2, 2] == GAVE_UP and 0 < dev["count"][2, 2] < 40320
    assert (dev["status"][:, 3] == OK).all()


@pytest.mark.parametrize("B", [1, 2, 3, 129])
def test_batch_sizes(g32, engine, B):
    mols = sorted((m for m in g32[1] if m["special"] not in REFUSED), key=lambda m: -len(m["elem"]))[:B]
    flags = H_EXACT if B == 2 else 0
    dev, ref = device_search(engine, mols, named_patterns(), flags), host_search(mols, named_patterns(), flags)
    same(dev, ref)
    assert (dev["status"] == OK).all() and dev["count"][:, 0].min() > 0


@pytest.mark.parametrize("P", [1, 64])
def test_pattern_counts(g32, engine, P):
    mols = g32[1][100:133]
    base = named_patterns()
    pats = [base[(k + 6) % len(base)] for k in range(P)]
    fl = np.arange(P, dtype=np.int32) % 4
    dev, ref = device_search(engine, mols, pats, fl), host_search(mols, pats, fl)
    same(dev, ref)
    assert dev["count"].shape == (33, P) and dev["count"].any()


def test_a_result_does_not_depend_on_the_place_in_the_batch(g32, engine):
    mols = g32[1][:97]
    perm = np.random.default_rng(8201).permutation(len(mols))
    a = device_search(engine, mols, named_patterns(), CLOSED)
    b = device_search(engine, [mols[k] for k in perm], named_patterns(), CLOSED)
    for k in ARRAYS:
        assert np.array_equal(a[k][perm], b[k]), k


def test_edge_shapes_and_refusals(g32, engine):
    targets = [path(n) for n in (1, 63, 64, 65)] + [ladder(n) for n in (128, 129, 192)] + [stars()]
    pats = [NAMED["C"], path(2), path(8), ladder(6), path(3, N_),
            (np.array([N_, 2, 2, 2], np.int32), np.array([(0, 1), (0, 2), (0, 3)], np.int32))]
    for flags in (0, H_EXACT | CLOSED):
        dev, ref = device_search(engine, targets, pats, flags), host_search(targets, pats, flags)
        same(dev, ref)
    dev = device_search(engine, targets, pats, 0)
    assert dev["count"][:7, 0].tolist() == [1, 63, 64, 65, 128, 129, 192] and dev["count"][7, 5] == 38 * 24
    for t, n in enumerate((1, 63, 64, 65, 128, 129, 192)):
        assert dev["covered"][t, 0, :n].all()  # every root's embedding arrives, whichever lane owns the root
    special = [next(m for m in g32[1] if m["special"] == k) for k in (5, 6, 7)]
    normal = [m for m in g32[1] if m["special"] not in REFUSED][:4]
    mols = normal[:2] + special[:1] + normal[2:3] + special[1:] + normal[3:]
    bad = [(np.zeros(0, np.int32), np.zeros((0, 2), np.int32)), (np.array([C, C, C], np.int32), np.array([(0, 1)], np.int32)), path(33),
           (np.array([C, C], np.int32), np.array([(0, 2)], np.int32)), (np.array([C, C], np.int32), np.array([(0, 1), (1, 1)], np.int32)),
           (np.array([C, C], np.int32), np.array([(0, 1), (1, 0)], np.int32)), (np.array([H], np.int32), np.zeros((0, 2), np.int32))]
    good = named_patterns()
    pats = good[:2] + bad[:4] + good[2:] + bad[4:]
    dev, ref = device_search(engine, mols, pats, 0), host_search(mols, pats, 0)
    same(dev, ref)
    bad_p = [2, 3, 4, 5, 12, 13, 14]
    assert (dev["status"][:, bad_p] == BAD_PATTERN).all()
    keep_p = [p for p in range(len(pats)) if p not in bad_p]
    assert dev["status"][np.ix_([2, 4, 5], keep_p)].tolist() == [[BAD_INPUT] * 8, [OVERFLOW] * 8, [EMPTY] * 8]
    assert (dev["status"][np.ix_([0, 1, 3, 6], keep_p)] == OK).all()
    with pytest.raises(_lib.GaudiError):
        device_search(engine, normal, [good[0]] * 65, 0)
    device_search(engine, normal, good, 0)  # (the engine goes on working)


def test_search_contains_and_analyze_through_an_engine(golden, engine):
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import atoms_list, rings_to_atoms
    from gaudi_amd.substructure import contains, pattern, ring_pattern, search
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "hetro"][:40]
    mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine)
    assert atoms_list("hetro").index("S") == S_
    pats = [ring_pattern("CCCCCC", "hetro"), ring_pattern("CCCCS", "hetro"), pattern("CCCCCCCC", [(k, k + 1) for k in range(7)], "hetro")]
    engine.profile_reset(True)
    out = search(recs, pats, "hetro", engine=engine)
    assert engine.substructure_profile_get()[0] == 2  # the patterns against themselves, the molecules against the patterns
    built = np.array([r["status"] == 0 for r in recs])
    assert built.sum() >= 30 and out["symmetry"].tolist() == [12, 2, 2] and not out["hit"][~built].any()
    seen = 0
    for b, r in enumerate(recs):
        if not built[b]:
            assert (out["status"][b] == EMPTY).all()
            continue
        for p, pat in enumerate(pats):
            ref = restated((r["atom_types"], r["bonds"]), pat, 0)
            assert out["count"][b, p] == ref["count"] and out["first"][b][p].tolist() == ref["first"].tolist()
            assert set(np.nonzero(out["covered"][b, p])[0].tolist()) == ref["covered"] and out["n_unique"][b, p] == len(ref["images"])
            seen += ref["count"] > 0
    assert seen >= 30 and out["hit"][:, 1].any() and not out["hit"][:, 1].all()
    assert np.array_equal(contains(recs, pats[1], "hetro", engine=engine), out["hit"][:, 1])
    plain, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine)
    d, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine, patterns=pats)
    assert set(d) == set(plain) | {"pattern_hits", "pattern_fraction"} and all(np.array_equal(d[k], plain[k]) for k in plain)
    assert np.array_equal(d["pattern_hits"], out["hit"]) and np.allclose(d["pattern_fraction"], out["hit"].sum(0) / built.sum())
    engine.profile_reset(False)


def test_the_profile_counts_one_launch_per_call(g32, engine):
    engine.profile_reset(True)
    assert engine.substructure_profile_get() == (0, 0.0)
    for calls in (1, 2, 3):
        device_search(engine, g32[1][:5 * calls], named_patterns()[:calls], 0)
        n, ms = engine.substructure_profile_get()
        assert n == calls and ms > 0.0
    engine.profile_reset(False)
    device_search(engine, g32[1][:5], named_patterns(), 0)
    assert engine.substructure_profile_get()[0] == 0


def test_design_with_patterns():
    import types

    import torch  # noqa: F401
    from gaudi_amd import generation_guidance, synth
    from gaudi_amd.models_edm import get_cond_predictor_model, get_model
    from gaudi_amd.substructure import ring_pattern
    from tests.helpers import TINY, TINY_P
    eargs = synth.edm_args(dataset="cata", diffusion_steps=40, **TINY)
    pargs = synth.pred_args(dataset="cata", **TINY_P)
    model, _, _ = get_model(eargs, state_dict=synth.synth_edm_state_dict(eargs, 1, seed=3))
    cp = get_cond_predictor_model(pargs, model=model, state_dict=synth.synth_predictor_state_dict(pargs, 1, 5, seed=4))
    model.seed = 5
    args = types.SimpleNamespace(device="cuda", dataset="cata", max_nodes=9, batch_size=6)

    def tf_gap(z, nm, em, t):
        return -cp(z, nm, em, t)[:, 1]

    pats = [ring_pattern("CCCCCC"), ring_pattern("CCCCC")]
    plain = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True)
    model.sample_offset = 0
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, patterns=pats)
    assert set(out) == set(plain) | {"contains"} and out["contains"].shape == (6, 2) and out["contains"].dtype == bool
    for rec, row in zip(out["atoms"], out["contains"]):
        want = [restated((rec["atom_types"], rec["bonds"]), p)["count"] > 0 for p in pats] if rec["status"] == 0 else [False, False]
        assert row.tolist() == want
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, patterns=pats)
    ref = generation_guidance.refine(args, model, cp, tf_gap, out["x"], out["one_hot"], out["node_mask"], out["edge_mask"],
                                     t_start=10, scale=0.6, n_steps=5, with_atoms=True, patterns=pats)
    assert ref["contains"].shape == (6, 2)
    model.engine.close()
