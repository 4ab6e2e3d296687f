"""Hueckel levels on the device (csrc/huckel.inc): gaudi_huckel against the kernel's host build, bit for bit in all fifteen outputs
-- golden g32, the sizes at which the rotation schedule and the capacity tiers change in one mixed call and alone, the batch sizes
around a workgroup, a shuffled batch, the largest molecules (the 132 KB tier), every refusal -- and the layers on top through a
real Engine.  What the outputs must satisfy is checked on the host build by tests/test_huckel_cpu.py; equality with it carries
that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import fixture
from tests.gor2goa_helpers import unpack
from tests.huckel_helpers import (BAD_INPUT, EMPTY, NO_PI, OK, OVERFLOW, SIZES, assert_rows_equal, assert_same_bits, benzene, device,
                                  g32_host, host, ladder, naphthalene, path, polyene, row, size_molecules)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def test_the_fixture_equals_the_host_build(g32, engine):
    mols = g32[1]
    assert len(mols) % 2 == 1
    dev, ref = device(engine, mols), g32_host()
    assert_same_bits(dev, ref)
    st = np.bincount(dev["status"], minlength=7)
    assert st[OK] >= 490 and st[BAD_INPUT] >= 1 and st[OVERFLOW] >= 1 and st[EMPTY] >= 1 and st[NO_PI] >= 1
    charged = np.arange(len(mols), dtype=np.int32) % 3 - 1
    assert_same_bits(device(engine, mols, charged), host(mols, charged))


def test_the_sizes_in_one_mixed_call_and_alone(engine):
    extra = [polyene(129), ladder(192), path(2), (np.zeros(0, np.int32), np.zeros((0, 2), np.int32)), benzene(), naphthalene()]
    mols = size_molecules() + extra
    dev, ref = device(engine, mols), host(mols)
    assert_same_bits(dev, ref)
    assert dev["status"].tolist() == [OK] * len(SIZES) + [OVERFLOW, OVERFLOW, NO_PI, EMPTY, OK, OK]
    assert dev["n_pi"][:len(SIZES)].tolist() == list(SIZES)
    for i, m in enumerate(mols[:len(SIZES)] + mols[-2:]):  # the tier and the batch leave no trace
        j = i if i < len(SIZES) else len(mols) - 2 + (i - len(SIZES))
        alone = device(engine, [m])
        assert_rows_equal(row(alone, 0, len(m[0]), len(m[1])), row(dev, j, len(m[0]), len(m[1])))
    perm = np.random.default_rng(8401).permutation(len(mols))
    moved = device(engine, [mols[k] for k in perm])
    for k in _lib.HUCKEL_ARRAYS:
        assert moved[k].tobytes() == np.ascontiguousarray(dev[k][perm]).tobytes(), k


@pytest.mark.parametrize("B", [1, 2, 3, 129])
def test_batch_sizes(g32, engine, B):
    ref = g32_host()
    mols = sorted((m for m in g32[1] if ref["status"][m["index"]] == OK), key=lambda m: -len(m["elem"]))[:B]
    dev = device(engine, mols)
    assert_same_bits(dev, host(mols))
    assert (dev["status"] == OK).all() and dev["n_pi"].min() > 0


def test_the_largest_molecules(g32, engine):
    ref = g32_host()
    big = max((m for m in g32[1] if ref["status"][m["index"]] == OK), key=lambda m: ref["n_pi"][m["index"]])
    mols = [(big["elem"], big["bonds"]), polyene(128), ladder(128)]
    dev = device(engine, mols)
    assert_same_bits(dev, host(mols))
    assert dev["status"].tolist() == [OK, OK, OK] and dev["n_pi"].tolist() == [ref["n_pi"][big["index"]], 128, 128]
    assert_rows_equal(row(dev, 0, len(big["elem"]), len(big["bonds"])), row(ref, big["index"], len(big["elem"]), len(big["bonds"])))


def test_a_table_that_cannot_be_read_and_bad_arguments(engine):
    from tests.bond_order_helpers import pack
    from tests.huckel_helpers import BAD_TABLE, c_tables
    t = c_tables()
    t.site_class[1][3] = t.n_classes
    out = engine.huckel(t, *pack([benzene(), naphthalene()]))
    assert out["status"].tolist() == [BAD_TABLE, BAD_TABLE] and not out["levels"].any()
    t = c_tables()
    t.n_elems = 9
    with pytest.raises(_lib.GaudiError):
        engine.huckel(t, *pack([benzene()]))
    assert_same_bits(device(engine, [benzene()]), host([benzene()]))  # (the engine goes on working)


def test_the_profile_counts_one_launch_per_tier(engine):
    engine.profile_reset(True)
    assert engine.huckel_profile_get() == (0, 0.0)
    device(engine, [benzene(), naphthalene()])
    assert engine.huckel_profile_get()[0] == 1
    device(engine, [benzene(), polyene(40), polyene(100), polyene(33)])
    n, ms = engine.huckel_profile_get()
    assert n == 4 and ms > 0.0
    engine.profile_reset(False)
    device(engine, [benzene()])
    assert engine.huckel_profile_get()[0] == 0


def test_orbitals_gap_and_analyze_through_an_engine(golden, g32, engine):
    from gaudi_amd import huckel
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    ref = g32_host()
    pick = [m for m in g32[1] if ref["status"][m["index"]] == OK][::25]
    pairs = [(m["elem"], m["bonds"]) for m in pick]
    orbs, gaps = huckel.orbitals(pairs, "hetro", engine=engine), huckel.gap(pairs, "hetro", engine=engine)
    for o, g, m in zip(orbs, gaps, pick):
        i, n = m["index"], ref["n_pi"][m["index"]]
        assert o["status"] == OK and o["levels"].tobytes() == ref["levels"][i, :n].tobytes() and g == float(ref["gap"][i]) == o["gap"]
        assert o["pi_charge"].tobytes() == ref["pi_charge"][i, :len(m["elem"])].tobytes()
        assert o["pi_bond_order"].tobytes() == ref["pi_bond_order"][i, :len(m["bonds"])].tobytes()
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "hetro"][:40]
    mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    plain_recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine)
    recs = rings_to_atoms(mols, "hetro", 0.1, place_hydrogens=True, engine=engine, huckel=True)
    added = {"huckel_gap", "huckel_homo", "huckel_lumo", "huckel_flags", "huckel_status"}
    raw = huckel.orbitals(plain_recs, "hetro", engine=engine)
    built = np.array([r["status"] == 0 for r in recs])
    assert built.sum() >= 30
    for r, p, o in zip(recs, plain_recs, raw):
        assert set(r) == set(p) | added and all(np.array_equal(r[k], p[k]) for k in p)
        assert (r["huckel_status"], r["huckel_gap"], r["huckel_homo"], r["huckel_lumo"], r["huckel_flags"]) == \
            (o["status"], o["gap"], o["homo"], o["lumo"], o["flags"])
        assert r["huckel_status"] == (OK if r["status"] == 0 else EMPTY)
    assert sum(r["huckel_gap"] > 0.1 for r in recs) >= 20
    plain, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine)
    engine.profile_reset(True)
    d, _ = analyze_atoms_for_molecules(mols, 0.1, "hetro", engine=engine, huckel=True)
    assert 1 <= engine.huckel_profile_get()[0] <= 3
    engine.profile_reset(False)
    assert set(d) == set(plain) | {"huckel_gap", "huckel_open_shell_fraction"} and all(np.array_equal(d[k], plain[k]) for k in plain)
    bare = rings_to_atoms(mols, "hetro", 0.1, engine=engine, huckel=True)  # as analyze builds them: no hydrogens placed
    assert np.array_equal(d["huckel_gap"], np.array([r["huckel_gap"] for r in bare if r["status"] == 0]))
    assert d["huckel_open_shell_fraction"] == sum(bool(r["huckel_flags"] & 1) for r in bare if r["status"] == 0) / built.sum()
    # hydrogens implied or placed: the same pi system
    assert np.allclose(d["huckel_gap"], [r["huckel_gap"] for r in recs if r["status"] == 0], atol=4e-5)


def test_design_with_huckel():
    import types

    import torch  # noqa: F401
    from gaudi_amd import generation_guidance, huckel, synth
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
    off = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, huckel=False)
    model.sample_offset = 0
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, huckel=True)
    assert set(off) == set(plain) and set(out) == set(plain) | {"huckel_gap"}
    for k in ("fingerprints", "mol_unique", "best"):
        assert np.array_equal(off[k], plain[k]) and np.array_equal(out[k], plain[k]), k
    assert np.array_equal(off["target_function_values"], plain["target_function_values"])
    assert out["huckel_gap"].shape == (6,) and out["huckel_gap"].dtype == np.float64
    want = huckel.gap(out["atoms"], "cata", engine=model.engine)
    assert np.array_equal(out["huckel_gap"], want, equal_nan=True)
    for rec, g in zip(out["atoms"], out["huckel_gap"]):
        assert np.isnan(g) == (rec["status"] != 0 or huckel.orbitals([rec], "cata", engine=model.engine)[0]["status"] != OK)
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, huckel=True)
    ref = generation_guidance.refine(args, model, cp, tf_gap, out["x"], out["one_hot"], out["node_mask"], out["edge_mask"],
                                     t_start=10, scale=0.6, n_steps=5, with_atoms=True, huckel=True)
    assert ref["huckel_gap"].shape == (6,)
    model.engine.close()
