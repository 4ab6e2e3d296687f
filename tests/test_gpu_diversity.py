"""Neighbour lists, Butina clusters and MaxMin picks on the device (csrc/fp_select.inc) against their host twins, every output
exactly equal, at the smallest shapes that take every path: one and two queries per lane, a partial tile, a partial last query
block, 2049 rows tiled from 507 (duplicates and ties), several splits and slices, the capacity protocol, seeds passed in and
resident, threshold stops inside a chunk of rounds and behind one, zero rows on both sides; independence of the grid; launch
counts; and the layers on top.  What the outputs must satisfy is checked on the host twins by tests/test_diversity_cpu.py;
equality with them carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests.diversity_helpers import CL_KEYS, MID, NB_KEYS, PK_KEYS, distinct_rows, rows_of, same
from tests.gor2goa_helpers import unpack

pytestmark = pytest.mark.gpu
_REF = {}


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def batch(N, n_bins):
    """The rows of a shape, and the host twins' answers at MID, computed once."""
    key = (N, n_bins)
    if key not in _REF:
        rows = rows_of(n_bins, N, N % 7, perturb=N != 2049)  # (2049 rows of 507: exact duplicates, zero rows among them)
        if N == 130:
            rows[[0, 77, 129]] = 0
        rows.setflags(write=False)
        _REF[key] = (rows, _lib.host_fp_neighbours(rows, *MID), _lib.host_fp_cluster(rows, *MID))
    return _REF[key]


@pytest.mark.parametrize("N,n_bins", [(1, 256), (3, 1024), (65, 512), (65, 256), (130, 1024), (130, 512), (2049, 1024), (2049, 256)])
def test_neighbours_and_clusters_equal_the_host_twins(engine, N, n_bins):
    rows, nb, cl = batch(N, n_bins)
    same(engine.fp_neighbours(rows, *MID), nb, NB_KEYS)
    same(engine.fp_cluster(rows, *MID), cl, CL_KEYS)
    if N == 2049:
        assert cl["n_clusters"] > 1 and cl["size"].max() >= 12 and (cl["cluster"] == -1).sum() == (~rows.any(-1)).sum() > 0


@pytest.mark.parametrize("thr", [(0, 1), (1, 1)])
def test_the_end_thresholds(engine, thr):
    rows = batch(130, 1024)[0]
    same(engine.fp_neighbours(rows, *thr), _lib.host_fp_neighbours(rows, *thr), NB_KEYS)
    same(engine.fp_cluster(rows, *thr), _lib.host_fp_cluster(rows, *thr), CL_KEYS)


def test_splits_give_the_same_bits(engine, monkeypatch):
    for N, n_bins in ((130, 1024), (2049, 256)):
        rows, nb, cl = batch(N, n_bins)
        for splits in ("1", "7"):
            monkeypatch.setenv("GAUDI_FP_SPLITS", splits)
            same(engine.fp_neighbours(rows, *MID), nb, NB_KEYS)
            same(engine.fp_cluster(rows, *MID), cl, CL_KEYS)


def test_capacity_protocol(engine):
    rows, ref, _ = batch(130, 512)
    total = int(ref["offsets"][-1])
    u8, ip = rows.ctypes.data_as(_lib.U8P), (lambda a: a.ctypes.data_as(_lib.IP))
    count, offsets = np.zeros(130, np.int32), np.zeros(131, np.int64)
    call = lambda cap, lst: engine.lib.gaudi_fp_neighbours(engine.h, 512, 130, u8, MID[0], MID[1], ip(count), cap,  # noqa: E731
                                                           offsets.ctypes.data_as(_lib.I64P), lst)
    assert call(0, None) == 0 and np.array_equal(count, ref["count"]) and np.array_equal(offsets, ref["offsets"])
    count[:], offsets[:] = 0, 0
    small = np.full(total, -7, np.int32)
    assert call(total - 1, ip(small)) == _lib.E_CAPACITY  # refused AFTER the counts and offsets are written
    assert np.array_equal(count, ref["count"]) and np.array_equal(offsets, ref["offsets"]) and (small == -7).all()
    exact = np.full(total + 1, -7, np.int32)
    assert call(total, ip(exact)) == 0 and np.array_equal(exact[:total], ref["list"]) and exact[total] == -7
    with pytest.raises(_lib.GaudiError, match="threshold"):
        engine.fp_cluster(rows, 3, 2)
    with pytest.raises(_lib.GaudiError, match="2\\^20 rows"):
        engine._check(engine.lib.gaudi_fp_cluster(engine.h, 512, (1 << 20) + 1, u8, 1, 2, *[ip(count)] * 5), "gaudi_fp_cluster")
    zero = np.zeros((70, 256), np.uint8)  # every row zero: no entry, no cluster
    same(engine.fp_neighbours(zero, 0, 1), _lib.host_fp_neighbours(zero, 0, 1), NB_KEYS)
    same(engine.fp_cluster(zero, 0, 1), _lib.host_fp_cluster(zero, 0, 1), CL_KEYS)
    none = np.zeros((0, 256), np.uint8)
    assert engine.fp_cluster(none, 1, 2)["n_clusters"] == 0 and engine.fp_pick_diverse(none, 3)["n_picked"] == 0


@pytest.mark.parametrize("N,n_bins,k", [(1, 256, 1), (1, 512, 5), (3, 1024, 1), (3, 256, 5), (65, 512, 5), (65, 1024, 40), (65, 256, 80),
                                        (999, 1024, 40), (999, 256, 5), (999, 512, 1)])
def test_picks_equal_the_host_twin(engine, monkeypatch, N, n_bins, k):
    rows = rows_of(n_bins, N, 3)
    ref = _lib.host_fp_pick_diverse(rows, k)
    for slices in ("1", "7"):
        monkeypatch.setenv("GAUDI_FP_SPLITS", slices)
        same(engine.fp_pick_diverse(rows, k), ref, PK_KEYS)
    monkeypatch.delenv("GAUDI_FP_SPLITS")
    same(engine.fp_pick_diverse(rows, k), ref, PK_KEYS)
    assert ref["n_picked"] == min(k, N)
    if N >= 65:
        first = N // 2
        same(engine.fp_pick_diverse(rows, k, first=first), _lib.host_fp_pick_diverse(rows, k, first=first), PK_KEYS)


def test_picks_with_seeds_passed_in_and_resident(monkeypatch):
    from gaudi_amd.engine import Engine
    from gaudi_amd.similarity import Library, pick_diverse
    rows, seeds = rows_of(1024, 999, 4), rows_of(1024, 70, 9)
    seeds[30] = rows[12]
    for S, k, thr in ((1, 9, (0, 0)), (70, 9, (0, 0)), (70, 40, MID)):
        ref = _lib.host_fp_pick_diverse(rows, k, *thr, seeds=seeds[:S])
        eng = Engine.default()
        for slices in ("1", "7"):
            monkeypatch.setenv("GAUDI_FP_SPLITS", slices)
            same(eng.fp_pick_diverse(rows, k, *thr, seeds=seeds[:S]), ref, PK_KEYS)
        monkeypatch.delenv("GAUDI_FP_SPLITS")
    assert ref["owner"][12] == -2 - 30
    eng = Engine(0)  # (an engine of its own: the resident library is the engine's)
    lib = Library(seeds, engine=eng)
    same(eng.fp_pick_diverse(rows, 40, *MID, seeds=None, S=70), ref, PK_KEYS)
    out = pick_diverse(rows, 40, threshold=0.7, seeds=lib, engine=eng)
    assert np.array_equal(out["picked"], ref["picked"][:ref["n_picked"]]) and np.array_equal(out["owner"], ref["owner"])
    with pytest.raises(_lib.GaudiError, match="resident fingerprint library"):
        eng.fp_pick_diverse(rows, 5, seeds=None, S=69)
    lib.close()
    with pytest.raises(_lib.GaudiError, match="no longer resident"):
        pick_diverse(rows, 5, seeds=lib, engine=eng)
    with pytest.raises(_lib.GaudiError, match="no resident fingerprint library"):
        eng.fp_pick_diverse(rows, 5, seeds=None, S=70)
    eng.close()


def test_threshold_stops_inside_a_chunk_and_behind_one(engine):
    # inside the first chunk of 256 rounds
    rows = batch(130, 1024)[0]
    ref = _lib.host_fp_pick_diverse(rows, 200, *MID)
    same(engine.fp_pick_diverse(rows, 200, *MID), ref, PK_KEYS)
    assert 1 < ref["n_picked"] < 127
    # k = 300 at thr 1/1 on 999 rows tiled from 280 different ones: every different row is picked once, the stop comes in the
    # second chunk
    rows = np.array(distinct_rows()[np.arange(999) % 280])
    ref = _lib.host_fp_pick_diverse(rows, 300, 1, 1)
    same(engine.fp_pick_diverse(rows, 300, 1, 1), ref, PK_KEYS)
    assert ref["n_picked"] == 280 and sorted(ref["picked"][:280].tolist()) == list(range(280))
    # ... and without a stop both chunks run to the end
    same(engine.fp_pick_diverse(rows, 300), _lib.host_fp_pick_diverse(rows, 300), PK_KEYS)
    with pytest.raises(_lib.GaudiError, match="not a live row"):
        engine.fp_pick_diverse(batch(130, 1024)[0], 5, first=77)
    with pytest.raises(_lib.GaudiError, match="out of range"):
        engine.fp_pick_diverse(rows, 5, first=999)


def test_zero_rows_on_both_sides(engine, monkeypatch):
    rows, seeds = rows_of(256, 70, 3), rows_of(256, 6, 4)
    rows[[0, 33, 69]] = 0
    seeds[[0, 4]] = 0
    for kw in (dict(), dict(seeds=seeds), dict(seeds=seeds[:1]), dict(seeds=np.zeros((3, 256), np.uint8))):
        ref = _lib.host_fp_pick_diverse(rows, 80, **kw)
        for slices in ("1", "7"):
            monkeypatch.setenv("GAUDI_FP_SPLITS", slices)
            same(engine.fp_pick_diverse(rows, 80, **kw), ref, PK_KEYS)
        assert ref["n_picked"] <= 67 and (ref["owner"][[0, 33, 69]] == -1).all()


def test_results_do_not_depend_on_the_grid(engine):
    """The same rows inside a larger batch -- zero rows strewn in between, so other tiles, splits, slices and lane groups -- give
    the same clusters and the same picks after mapping the indices back.  Ties go to the smaller index, so the rows keep their
    relative order (under a permutation equal neighbour counts or equal similarities of different pairs may resolve otherwise),
    and the rows are pairwise different."""
    sub = np.array(distinct_rows()[::3][:130])
    rng = np.random.default_rng(8)
    pos = np.sort(rng.permutation(700)[:130])
    big = np.zeros((700, 1024), np.uint8)
    big[pos] = sub
    a, b = engine.fp_cluster(sub, *MID), engine.fp_cluster(big, *MID)
    assert a["n_clusters"] == b["n_clusters"] and np.array_equal(b["cluster"][pos], a["cluster"]) and (np.delete(b["cluster"], pos) == -1).all()
    assert np.array_equal(pos[a["centroid"][:a["n_clusters"]]], b["centroid"][:b["n_clusters"]])
    assert np.array_equal(a["size"], b["size"][:130]) and np.array_equal(a["count"], b["count"][pos])
    pa, pb = engine.fp_pick_diverse(sub, 40), engine.fp_pick_diverse(big, 40)
    assert np.array_equal(pos[pa["picked"]], pb["picked"]) and np.array_equal(pos[pa["owner"]], pb["owner"][pos])
    for k in ("pick_common", "pick_union"):
        assert np.array_equal(pa[k], pb[k])
    for k in ("owner_common", "owner_union"):
        assert np.array_equal(pa[k], pb[k][pos])


def test_launch_counts(engine):
    """gaudi_fp_profile_get counts every launch: a cluster call makes a constant number, a pick call of n rounds n plus a constant."""
    rows = batch(130, 1024)[0]
    engine.profile_reset(True)
    try:
        counts = []
        for N in (65, 130):
            before = engine.fp_profile_get()[0]
            engine.fp_cluster(rows[:N], *MID)
            counts.append(engine.fp_profile_get()[0] - before)
        assert counts[0] == counts[1] == 5  # COUNT, offsets, FILL, the sort, the walk
        picks = []
        for k in (3, 20, 120):
            before = engine.fp_profile_get()[0]
            assert engine.fp_pick_diverse(rows, k)["n_picked"] == k
            picks.append(engine.fp_profile_get()[0] - before - k)
        assert picks[0] == picks[1] == picks[2] == 3  # the cleared state, the round that makes no pick, the totals as yardstick
        st = engine.fp_select_stages_get()
        assert st["pick_rounds"] > 0.0 and st["pick_setup"] > 0.0 and st["totals"] > 0.0 and st["count"] == st["walk"] == 0.0
        engine.fp_cluster(rows, *MID)
        st = engine.fp_select_stages_get()
        assert min(st[k] for k in ("count", "offsets", "fill", "sort", "walk")) > 0.0 and st["pick_rounds"] == st["totals"] == 0.0
        assert engine.fp_profile_get()[1] > 0.0
    finally:
        engine.profile_reset(False)


def test_analyze_with_clusters(golden, engine):
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    from gaudi_amd.similarity import cluster, fingerprints
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "cata"]
    mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    plain, _ = analyze_atoms_for_molecules(mols, 0.1, "cata", engine=engine, similarity=True)
    d, _ = analyze_atoms_for_molecules(mols, 0.1, "cata", engine=engine, similarity=True, cluster_threshold=0.7)
    assert set(d) == set(plain) | {"n_clusters", "largest_cluster_fraction"} and d["diversity"] == plain["diversity"]
    recs = rings_to_atoms(mols, "cata", 0.1, engine=engine)
    fp = fingerprints(recs, "cata", engine=engine)
    ref = _lib.host_fp_cluster(fp["fp"], *MID)
    n_built = sum(r["status"] == 0 for r in recs)
    assert d["n_clusters"] == ref["n_clusters"] > 1 and d["largest_cluster_fraction"] == ref["size"].max() / n_built
    assert cluster(fp["fp"], 0.7, engine=engine)["n_clusters"] == ref["n_clusters"]
    with pytest.raises(ValueError, match="similarity=True"):
        analyze_atoms_for_molecules(mols, 0.1, "cata", engine=engine, cluster_threshold=0.7)


def test_design_and_refine_with_clusters_and_picks():
    import types

    import torch  # noqa: F401
    from gaudi_amd import generation_guidance, synth
    from gaudi_amd.models_edm import get_cond_predictor_model, get_model
    from gaudi_amd.similarity import fingerprints
    from tests.helpers import TINY, TINY_P
    eargs = synth.edm_args(dataset="cata", diffusion_steps=40, **TINY)
    pargs = synth.pred_args(dataset="cata", **TINY_P)
    model, _, _ = get_model(eargs, state_dict=synth.synth_edm_state_dict(eargs, 1, seed=3))
    cp = get_cond_predictor_model(pargs, model=model, state_dict=synth.synth_predictor_state_dict(pargs, 1, 5, seed=4))
    model.seed = 5
    args = types.SimpleNamespace(device="cuda", dataset="cata", max_nodes=9, batch_size=6)

    def tf_gap(z, nm, em, t):
        return -cp(z, nm, em, t)[:, 1]

    plain = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, similarity=True)
    model.sample_offset = 0
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, similarity=True,
                                     cluster_threshold=0.7, diverse=4)
    assert set(out) == set(plain) | {"n_clusters", "largest_cluster_fraction", "diverse_indices"}
    built = np.array([r["status"] == 0 for r in out["atoms"]])
    fp = fingerprints(out["atoms"], "cata", engine=model.engine)["fp"]
    fp[~built] = 0
    cl, pk = _lib.host_fp_cluster(fp, *MID), _lib.host_fp_pick_diverse(fp, 4)
    assert out["n_clusters"] == cl["n_clusters"] and np.array_equal(out["diverse_indices"], pk["picked"][:pk["n_picked"]])
    assert out["largest_cluster_fraction"] == (cl["size"].max() / built.sum() if built.any() else 0.0)
    assert built[out["diverse_indices"]].all() and len(out["diverse_indices"]) == min(4, built.sum())
    for kw in (dict(cluster_threshold=0.7), dict(diverse=4)):
        with pytest.raises(ValueError, match="with_atoms"):
            generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, similarity=True, **kw)
    base = generation_guidance.refine(args, model, cp, tf_gap, out["x"], out["one_hot"], out["node_mask"], out["edge_mask"],
                                      t_start=10, scale=0.6, n_steps=5, with_atoms=True, similarity=True)
    ref = generation_guidance.refine(args, model, cp, tf_gap, out["x"], out["one_hot"], out["node_mask"], out["edge_mask"],
                                     t_start=10, scale=0.6, n_steps=5, with_atoms=True, similarity=True, diverse=3)
    assert set(ref) == set(base) | {"diverse_indices"}
    ok = np.array([r["status"] == 0 for r in ref["atoms"]])
    assert ok[ref["diverse_indices"]].all() and len(ref["diverse_indices"]) == min(3, ok.sum())
    model.engine.close()
