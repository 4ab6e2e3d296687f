"""Circular count fingerprints and nearest-neighbour similarity on the device (csrc/fp.inc): gaudi_circular_fingerprint against the
kernel's host build bit for bit on golden g32; gaudi_fp_nearest against gaudi_host_fp_nearest, exact, at the smallest shapes that
take every path (one and two queries per lane, a partial tile, several splits, a partial last query block, k beyond M, zero
rows); the splits knob and the resident library; gaudi_fp_common against numpy; and the layers on top.  What the outputs must
satisfy is checked on the host builds by tests/test_similarity_cpu.py; equality with them carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import fixture
from tests.gor2goa_helpers import unpack
from tests.similarity_helpers import (BAD_INPUT, EMPTY, OK, OVERFLOW, device_fp, g32_fingerprints, host_fp, numpy_common,
                                      numpy_diversity)

pytestmark = pytest.mark.gpu
NAMES = ("idx", "common", "union")


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def rows_of(n_bins, count, seed, perturb=True):
    """`count` rows from g32's real fingerprints, tiled (so rows repeat) and, where asked, every third row perturbed in a few
    bins (so near-duplicates sit next to exact ones)."""
    base = g32_fingerprints(2, n_bins)["fp"]
    rng = np.random.default_rng(seed)
    rows = np.array(base[(np.arange(count) * 5 + seed) % len(base)])
    if perturb:
        for r in range(0, count, 3):
            at = rng.integers(0, n_bins, 4)
            rows[r, at] = (rows[r, at].astype(np.int64) + rng.integers(0, 3, 4)).clip(0, 255)
    return rows


def quot(common, union):
    """common / union in float64, 0.0 where union = 0."""
    common, union = np.asarray(common, np.float64), np.asarray(union, np.float64)
    return np.divide(common, union, out=np.zeros_like(common), where=union > 0)


def same(dev, ref):
    for n in NAMES:
        assert dev[n].dtype == ref[n].dtype == np.int32 and np.array_equal(dev[n], ref[n]), n


def test_fingerprint_equals_the_host_build(g32, engine):
    mols = g32[1]
    assert len(mols) % 2 == 1  # an odd count: the last workgroup has one wave idle
    assert max(len(m["elem"]) for m in mols) >= 190
    for radius, n_bins in ((2, 1024), (3, 256)):
        dev, ref = device_fp(engine, mols, radius, n_bins), g32_fingerprints(radius, n_bins)
        for k in ("fp", "total", "status"):
            assert dev[k].dtype == ref[k].dtype and np.array_equal(dev[k], ref[k]), (k, radius, n_bins)
    assert (dev["status"] == OK).sum() == 504
    for code, special in ((BAD_INPUT, 5), (OVERFLOW, 6), (EMPTY, 7)):
        i = next(m["index"] for m in mols if m["special"] == special)
        assert dev["status"][i] == code and not dev["fp"][i].any() and dev["total"][i] == 0


@pytest.mark.parametrize("B", [1, 3])
def test_fingerprint_small_batches(g32, engine, B):
    mols = sorted((m for m in g32[1] if m["special"] < 0), key=lambda m: -len(m["elem"]))[:B]
    dev, ref = device_fp(engine, mols), host_fp(mols)
    for k in ("fp", "total", "status"):
        assert np.array_equal(dev[k], ref[k]), k
    assert (dev["status"] == OK).all() and dev["total"].min() > 0


def test_fingerprint_does_not_depend_on_the_place_in_the_batch(g32, engine):
    mols = g32[1]
    probe = next(m for m in mols if m["min_charged"] == 4)
    da, db = device_fp(engine, [probe] + mols[10:41]), device_fp(engine, mols[200:233] + [probe])
    assert da["status"][0] == db["status"][-1] == OK and da["total"][0] == db["total"][-1] > 0
    assert da["fp"][0].tobytes() == db["fp"][-1].tobytes()


@pytest.mark.parametrize("B,M,k,n_bins", [(1, 1, 1, 256), (3, 65, 4, 1024), (65, 33, 16, 512), (64, 2049, 1, 1024), (5, 4, 16, 256)])
def test_nearest_equals_the_host_loops(engine, B, M, k, n_bins):
    q, lib = rows_of(n_bins, B, 1), rows_of(n_bins, M, 2, perturb=M != 2049)  # (2049 rows of 504: exact duplicates)
    dev, ref = engine.fp_nearest(q, lib, k), _lib.host_fp_nearest(q, lib, k)
    same(dev, ref)
    if k > M:
        assert (dev["idx"][:, M:] == -1).all() and not dev["common"][:, M:].any() and not dev["union"][:, M:].any()
        assert (np.sort(dev["idx"][:, :M], axis=1) == np.arange(M)).all()
    if M == 2049:
        first = {}
        for i, row in enumerate(lib):
            first.setdefault(row.tobytes(), i)
        assert all(first[lib[i].tobytes()] == i for i in dev["idx"][:, 0])  # of equal rows the lowest index


def test_nearest_with_zero_rows_on_both_sides(engine):
    q, lib = rows_of(256, 6, 3), rows_of(256, 70, 4)
    q[[0, 4]] = 0
    lib[[0, 33, 69]] = 0
    dev = engine.fp_nearest(q, lib, 16)
    same(dev, _lib.host_fp_nearest(q, lib, 16))
    assert dev["idx"][0].tolist() == list(range(16)) and not dev["common"][0].any() and dev["union"][0, 0] == 0


def test_splits_and_the_resident_library(engine, monkeypatch):
    from gaudi_amd.engine import Engine
    from gaudi_amd.similarity import Library, nearest
    q, lib = rows_of(1024, 70, 5), rows_of(1024, 999, 6)
    ref = _lib.host_fp_nearest(q, lib, 5)
    for splits in ("1", "7"):
        monkeypatch.setenv("GAUDI_FP_SPLITS", splits)
        same(engine.fp_nearest(q, lib, 5), ref)
    monkeypatch.delenv("GAUDI_FP_SPLITS")
    eng = Engine(0)  # (an engine of its own: the resident library is the engine's)
    res = Library(lib, engine=eng)
    same(eng.fp_nearest(q, None, 5, M=res.M), ref)
    idx, sim = res.nearest(q, 5)
    one = nearest(q, lib, 5, engine=eng)
    assert idx.dtype == np.int64 and sim.dtype == np.float64 and np.array_equal(idx, ref["idx"])
    assert np.array_equal(sim, quot(ref["common"], ref["union"])) and np.array_equal(one[0], idx) and np.array_equal(one[1], sim)
    # replaced: the new rows answer
    lib2 = rows_of(1024, 40, 7)
    res2 = Library(lib2, engine=eng)
    same(eng.fp_nearest(q, None, 5, M=res2.M), _lib.host_fp_nearest(q, lib2, 5))
    with pytest.raises(_lib.GaudiError, match="no longer resident"):
        res.nearest(q)
    # closed: a query of the resident library is an error, and the engine goes on working
    res2.close()
    with pytest.raises(_lib.GaudiError, match="no resident fingerprint library"):
        eng.fp_nearest(q, None, 5, M=40)
    with pytest.raises(_lib.GaudiError, match="no resident fingerprint library"):
        eng.fp_common(q, None, M=40)
    same(eng.fp_nearest(q, lib, 5), ref)
    eng.close()


@pytest.mark.parametrize("B,M", [(3, 65), (65, 3)])
def test_common_equals_numpy(engine, B, M):
    from gaudi_amd.similarity import similarity_matrix
    q, lib = rows_of(512, B, 8), rows_of(512, M, 9)
    dev = engine.fp_common(q, lib)
    assert dev.dtype == np.int32 and dev.shape == (B, M) and np.array_equal(dev, numpy_common(q, lib))
    t = q.sum(-1, dtype=np.int64)[:, None] + lib.sum(-1, dtype=np.int64)[None, :]
    assert np.array_equal(similarity_matrix(q, lib, engine=engine), quot(dev, t - dev))


def test_analyze_with_a_training_library(golden, engine):
    """g30: a library from half of the molecules.  A built molecule whose exact key is in that half has a nearest training
    molecule at similarity exactly 1.0, every other one below; a molecule and its twin (other ring positions, another atom
    numbering) get the same row."""
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    from gaudi_amd.similarity import Library, fingerprints
    g30 = unpack(golden("g30_gor2goa"))
    n_one = n_below = 0
    for ds in ("cata", "hetro"):
        idx = [i for i, m in enumerate(g30) if m["dataset"] == ds]
        mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
        recs = rings_to_atoms(mols, ds, 0.1, canonical=True, engine=engine)
        twins = rings_to_atoms([(g30[i]["twin_x"], g30[i]["twin_types"]) for i in idx], ds, 0.1, place_hydrogens=True, engine=engine)
        fp = fingerprints(recs, ds, engine=engine)
        built = np.array([r["status"] == 0 for r in recs])
        assert np.array_equal(fp["status"] == OK, built) and (fp["status"][~built] == EMPTY).all()
        assert all(t["status"] == 0 for t, ok in zip(twins, built) if ok)
        assert np.array_equal(fingerprints(twins, ds, engine=engine)["fp"][built], fp["fp"][built])
        half = [j for j in range(0, len(recs), 2) if built[j]]
        train_keys = {recs[j]["canon_key"] for j in half}
        plain, _ = analyze_atoms_for_molecules(mols, 0.1, ds, engine=engine)
        lib = Library(fp["fp"][half], engine=engine)
        d, _ = analyze_atoms_for_molecules(mols, 0.1, ds, engine=engine, similarity=True, train_library=lib)
        lib.close()
        assert set(d) == set(plain) | {"diversity", "nearest_train_similarity", "nearest_train_index"}
        assert all(np.array_equal(d[k], plain[k]) for k in plain)
        only, _ = analyze_atoms_for_molecules(mols, 0.1, ds, engine=engine, similarity=True)
        assert set(only) == set(plain) | {"diversity"}
        assert d["diversity"] == only["diversity"] == numpy_diversity(fp["fp"], fp["total"]) and 0.0 < d["diversity"] < 1.0
        sim, near = d["nearest_train_similarity"], d["nearest_train_index"]
        assert sim.shape == near.shape == (len(recs),) and sim.dtype == np.float64
        for j, r in enumerate(recs):
            if not built[j]:
                assert sim[j] == 0.0 and near[j] == -1
            elif r["canon_key"] in train_keys:
                assert sim[j] == 1.0 and recs[half[near[j]]]["canon_key"] == r["canon_key"]
                n_one += 1
            else:
                assert 0.0 < sim[j] < 1.0 and 0 <= near[j] < len(half)
                n_below += 1
    assert n_one >= 70 and n_below >= 20


def test_design_and_refine_with_similarity():
    import types

    import torch  # noqa: F401
    from gaudi_amd import generation_guidance, synth
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
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, similarity=True)
    assert set(out) == set(plain) | {"diversity"} and 0.0 <= out["diversity"] <= 1.0
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, similarity=True)
    ref = generation_guidance.refine(args, model, cp, tf_gap, out["x"], out["one_hot"], out["node_mask"], out["edge_mask"],
                                     t_start=10, scale=0.6, n_steps=5, with_atoms=True, similarity=True)
    assert set(ref) == set(out) | {"seed_target_function_values", "similarity_to_seed"}
    s = ref["similarity_to_seed"]
    assert s.shape == (6,) and s.dtype == np.float64 and ((0.0 <= s) & (s <= 1.0)).all()
    for rec, seed, v in zip(ref["atoms"], out["atoms"], s):
        assert (v > 0.0) == (rec["status"] == 0 and seed["status"] == 0)
    model.engine.close()
