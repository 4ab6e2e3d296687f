"""Neighbour lists, Butina clusters and MaxMin picks of fingerprint batches (csrc/fp_select.inc) through the HOST twins,
gaudi_host_fp_neighbours, gaudi_host_fp_cluster and gaudi_host_fp_pick_diverse: every output equals an oracle in Python integers
and Fractions (tests/diversity_helpers.py), the results satisfy what defines them, the refusals, and the Python layer on a host
engine.  tests/test_gpu_diversity.py compares the device with these twins."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.diversity_helpers import (CL_KEYS, MID, NB_KEYS, PK_KEYS, HostEngine, distinct_rows, oracle_cluster, oracle_neighbours,
                                     oracle_pick, rows_of, same, sims)
from tests.similarity_helpers import g32_fingerprints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gaudi_fp_neighbours", "gaudi_fp_cluster", "gaudi_fp_pick_diverse", "gaudi_host_fp_neighbours", "gaudi_host_fp_cluster",
       "gaudi_host_fp_pick_diverse")
THRESHOLDS = [(0, 1), (1, 1), MID]


@pytest.fixture(scope="module")
def g32_rows():
    return g32_fingerprints()["fp"]  # 507 rows, the three zero rows of the refused specials inside


@pytest.fixture(scope="module")
def g32_table(g32_rows):
    return sims(g32_rows)


def sim(rows, i, j):
    a, b = rows[i].astype(np.int64), rows[j].astype(np.int64)
    c = int(np.minimum(a, b).sum())
    u = int(a.sum() + b.sum()) - c
    return Fraction(c, u) if u else Fraction(0)


def check_neighbours(rows, nb, thr):
    N = len(rows)
    live = rows.astype(np.int64).sum(-1) > 0
    lists = [nb["list"][nb["offsets"][i]:nb["offsets"][i + 1]].tolist() for i in range(N)]
    assert nb["offsets"][0] == 0 and np.array_equal(np.diff(nb["offsets"]), nb["count"])
    for i, x in enumerate(lists):
        assert x == sorted(set(x))  # ascending, no repeats
        assert (i in x) == bool(live[i])
        assert live[i] or not x
        for j in x:
            assert live[j] and i in lists[j]  # symmetric
    return lists


def check_clusters(rows, cl, thr):
    N = len(rows)
    thr = Fraction(*thr)
    live = rows.astype(np.int64).sum(-1) > 0
    n = cl["n_clusters"]
    assert np.array_equal(cl["cluster"] >= 0, live) and (cl["cluster"] < n).all()  # every live row in exactly one cluster
    assert np.array_equal(np.bincount(cl["cluster"][live], minlength=N)[:n], cl["size"][:n]) and (cl["size"][:n] >= 1).all()
    assert (cl["centroid"][n:] == -1).all() and not cl["size"][n:].any()
    cents = cl["centroid"][:n].tolist()
    assert len(set(cents)) == n and all(cl["cluster"][c] == k for k, c in enumerate(cents))
    for i in np.nonzero(live)[0]:
        assert sim(rows, i, cents[cl["cluster"][i]]) >= thr  # every member is at least thr to its centroid
    for a in range(n):
        for b in range(a):
            assert sim(rows, cents[a], cents[b]) < thr  # a centroid within thr of an earlier one would have been claimed
    assert all(cl["count"][cents[k]] >= cl["count"][cents[k + 1]] for k in range(n - 1))


def check_picks(rows, pk, thr=None, seeds=None):
    live = rows.astype(np.int64).sum(-1) > 0
    n = pk["n_picked"]
    picked = pk["picked"][:n].tolist()
    assert len(set(picked)) == n and all(live[p] for p in picked)
    assert (pk["picked"][n:] == -1).all() and not pk["pick_common"][n:].any() and not pk["pick_union"][n:].any()
    ps = [Fraction(int(c), int(u)) if u else Fraction(0) for c, u in zip(pk["pick_common"][:n], pk["pick_union"][:n])]
    start = 0 if seeds is not None and len(seeds) else 1
    assert all(ps[t] <= ps[t + 1] for t in range(start, n - 1))  # never decreases from the second pick on
    t = rows.astype(np.int64).sum(-1)
    for p in picked:  # a picked row owns itself
        assert pk["owner"][p] == p and pk["owner_common"][p] == pk["owner_union"][p] == t[p]
    assert (pk["owner"][~live] == -1).all()
    chosen = n > 0 or (seeds is not None and len(seeds) > 0)
    for i in np.nonzero(live)[0]:
        o = pk["owner"][i]
        if not chosen:
            assert o == -1
            continue
        other = rows[o] if o >= 0 else seeds[-2 - o]
        assert o in picked or -len(seeds) - 1 <= o <= -2
        c = int(np.minimum(rows[i].astype(np.int64), other.astype(np.int64)).sum())
        assert (pk["owner_common"][i], pk["owner_union"][i]) == (c, int(t[i] + other.astype(np.int64).sum()) - c)


def test_the_in_between_threshold_means_something(g32_rows, g32_table):
    """On the oracle alone: at MID the g32 rows fall into more than one cluster and fewer than there are live rows, with a cluster
    of three or more and a singleton."""
    assert MID in [(n, 10) for n in range(5, 10)]
    cl = oracle_cluster(g32_rows, MID, g32_table)
    n_live = int((g32_rows.astype(np.int64).sum(-1) > 0).sum())
    sizes = cl["size"][:cl["n_clusters"]]
    assert n_live == 504 and 1 < cl["n_clusters"] < n_live
    assert (sizes >= 3).any() and (sizes == 1).any()


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_g32_against_the_oracle(g32_rows, g32_table, thr):
    nb = _lib.host_fp_neighbours(g32_rows, *thr)
    same(nb, oracle_neighbours(g32_rows, thr, g32_table), NB_KEYS)
    check_neighbours(g32_rows, nb, thr)
    cl = _lib.host_fp_cluster(g32_rows, *thr)
    same(cl, oracle_cluster(g32_rows, thr, g32_table), CL_KEYS)
    check_clusters(g32_rows, cl, thr)
    if thr == (0, 1):
        assert cl["n_clusters"] == 1 and cl["size"][0] == 504 and (nb["count"][g32_rows.any(-1)] == 504).all()
    if thr == (1, 1):
        assert cl["n_clusters"] == 432  # the isomorphism classes: only equal rows have similarity 1


def test_g32_picks_against_the_oracle(g32_rows, g32_table):
    for k, thr in ((40, None), (600, MID), (600, (1, 1))):
        pk = _lib.host_fp_pick_diverse(g32_rows, k, *(thr or (0, 0)))
        same(pk, oracle_pick(g32_rows, k, thr, table=g32_table), PK_KEYS)
        check_picks(g32_rows, pk, thr)
        if thr is None:
            assert pk["n_picked"] == k
        else:  # a threshold stop: every live row is at least thr to its owner
            live = g32_rows.any(-1)
            assert 0 < pk["n_picked"] < 504
            assert all(Fraction(int(c), int(u)) >= Fraction(*thr) for c, u in zip(pk["owner_common"][live], pk["owner_union"][live]))
        if thr == (1, 1):
            assert pk["n_picked"] == 432  # one pick per distinct row, and of equal rows the smallest index
            first = {}
            for i, row in enumerate(g32_rows):
                first.setdefault(row.tobytes(), i)
            assert all(first[g32_rows[p].tobytes()] == p for p in pk["picked"][:432])


@pytest.mark.parametrize("n_bins", [256, 512, 1024])
def test_tiled_and_perturbed_rows_with_zero_rows(n_bins):
    """Exact duplicates and near-duplicates side by side, zero rows at the front, in the middle and at the end."""
    rows = rows_of(n_bins, 130, 11)
    rows[[0, 1, 64, 129]] = 0
    rows[100:110] = rows[20:30]  # (exact duplicates whatever the tiling gives)
    table = sims(rows)
    for thr in THRESHOLDS:
        nb = _lib.host_fp_neighbours(rows, *thr)
        same(nb, oracle_neighbours(rows, thr, table), NB_KEYS)
        lists = check_neighbours(rows, nb, thr)
        cl = _lib.host_fp_cluster(rows, *thr)
        same(cl, oracle_cluster(rows, thr, table), CL_KEYS)
        check_clusters(rows, cl, thr)
        assert lists[0] == lists[64] == lists[129] == [] and cl["cluster"][[0, 1, 64, 129]].tolist() == [-1] * 4
        if thr == (1, 1):  # of duplicate rows the smaller index is the centroid
            assert all(cl["centroid"][cl["cluster"][100 + d]] <= 20 + d for d in range(10))
            assert all(cl["cluster"][100 + d] == cl["cluster"][20 + d] for d in range(10))
    for k, thr, first in ((20, None, -1), (200, MID, -1), (7, None, 105), (200, (1, 1), -1)):
        pk = _lib.host_fp_pick_diverse(rows, k, *(thr or (0, 0)), first=first)
        same(pk, oracle_pick(rows, k, thr, first=first, table=table), PK_KEYS)
        check_picks(rows, pk, thr)
    assert _lib.host_fp_pick_diverse(rows, 20)["picked"][0] == 2  # the first live row
    assert _lib.host_fp_pick_diverse(rows, 7, first=105)["picked"][0] == 105
    pk = _lib.host_fp_pick_diverse(rows, 200, 1, 1)
    assert not set(range(100, 110)) & set(pk["picked"].tolist())  # ties go to the smaller index: 20..29, never their copies
    assert all(pk["owner"][100 + d] == pk["owner"][20 + d] <= 20 + d for d in range(10))


def test_one_row_no_live_row_and_no_row():
    one = rows_of(256, 1, 3)
    for thr in THRESHOLDS:
        nb, cl = _lib.host_fp_neighbours(one, *thr), _lib.host_fp_cluster(one, *thr)
        assert nb["count"].tolist() == [1] and nb["offsets"].tolist() == [0, 1] and nb["list"].tolist() == [0]
        assert cl["n_clusters"] == 1 and cl["cluster"].tolist() == [0] and cl["centroid"].tolist() == [0] and cl["size"].tolist() == [1]
    pk = _lib.host_fp_pick_diverse(one, 3)
    same(pk, oracle_pick(one, 3), PK_KEYS)
    assert pk["n_picked"] == 1 and pk["picked"].tolist() == [0, -1, -1] and pk["pick_union"].tolist() == [0, 0, 0]
    zero = np.zeros((5, 512), np.uint8)
    nb, cl, pk = _lib.host_fp_neighbours(zero, 0, 1), _lib.host_fp_cluster(zero, 0, 1), _lib.host_fp_pick_diverse(zero, 3)
    same(nb, oracle_neighbours(zero, (0, 1)), NB_KEYS)
    same(cl, oracle_cluster(zero, (0, 1)), CL_KEYS)
    same(pk, oracle_pick(zero, 3), PK_KEYS)
    assert not nb["count"].any() and len(nb["list"]) == 0 and cl["n_clusters"] == 0 and (cl["cluster"] == -1).all()
    assert pk["n_picked"] == 0 and (pk["owner"] == -1).all() and (pk["picked"] == -1).all()
    none = np.zeros((0, 256), np.uint8)
    assert _lib.host_fp_cluster(none, 1, 2)["n_clusters"] == 0 and _lib.host_fp_pick_diverse(none, 4)["n_picked"] == 0
    assert len(_lib.host_fp_neighbours(none, 1, 2)["list"]) == 0


def test_pick_cases():
    rows = rows_of(256, 90, 5)
    rows[[3, 50]] = 0
    table = sims(rows)
    live = int(rows.any(-1).sum())
    # k = 0: nothing picked, nothing owned
    pk = _lib.host_fp_pick_diverse(rows, 0)
    same(pk, oracle_pick(rows, 0, table=table), PK_KEYS)
    assert pk["n_picked"] == 0 and len(pk["picked"]) == 0 and (pk["owner"] == -1).all()
    # k beyond the live rows: every live row is picked once
    pk = _lib.host_fp_pick_diverse(rows, 120)
    same(pk, oracle_pick(rows, 120, table=table), PK_KEYS)
    check_picks(rows, pk)
    assert pk["n_picked"] == live == 88 and sorted(pk["picked"][:live].tolist()) == np.nonzero(rows.any(-1))[0].tolist()
    # first given, and refused when it is not a live row or out of range
    pk = _lib.host_fp_pick_diverse(rows, 6, first=41)
    same(pk, oracle_pick(rows, 6, first=41, table=table), PK_KEYS)
    assert pk["picked"][0] == 41 and pk["pick_common"][0] == pk["pick_union"][0] == 0
    for bad in (3, 90, -2):
        with pytest.raises(_lib.GaudiError, match=r"\(-1\)"):
            _lib.host_fp_pick_diverse(rows, 6, first=bad)
    # seeds: one, seventy (a zero row among them), a seed equal to a batch row, and a threshold stop
    seeds70 = rows_of(256, 70, 6)
    seeds70[9] = 0
    seeds70[30] = rows[12]
    for seeds, k, thr in ((seeds70[:1], 9, None), (seeds70, 9, None), (seeds70, 120, MID), (seeds70, 120, (1, 1))):
        pk = _lib.host_fp_pick_diverse(rows, k, *(thr or (0, 0)), seeds=seeds)
        same(pk, oracle_pick(rows, k, thr, seeds=seeds, table=table), PK_KEYS)
        check_picks(rows, pk, thr, seeds)
        if thr is not None:
            assert 0 < pk["n_picked"] < live
            ok = rows.any(-1)
            assert all(Fraction(int(c), int(u)) >= Fraction(*thr) for c, u in zip(pk["owner_common"][ok], pk["owner_union"][ok]))
        if len(seeds) == 70:
            assert 12 not in pk["picked"].tolist() and pk["owner"][12] <= -2  # the seed's twin is covered at similarity 1 from the start
            assert pk["owner_common"][12] == pk["owner_union"][12]
    # without a pick the seeds own every live row
    pk = _lib.host_fp_pick_diverse(rows, 0, seeds=seeds70)
    assert (pk["owner"][rows.any(-1)] <= -2).all() and (pk["owner"][~rows.any(-1)] == -1).all()
    # all-255 rows: the largest totals there are
    full = np.full((4, 1024), 255, np.uint8)
    pk = _lib.host_fp_pick_diverse(full, 4, 1, 1)
    same(pk, oracle_pick(full, 4, (1, 1)), PK_KEYS)
    assert pk["n_picked"] == 1 and pk["owner"].tolist() == [0] * 4 and pk["owner_union"].tolist() == [255 * 1024] * 4
    assert _lib.host_fp_cluster(full, 1, 1)["size"][0] == 4


def test_capacity_protocol_and_refusals():
    lib = _lib.load_library()
    rows = rows_of(256, 40, 7)
    ref = _lib.host_fp_neighbours(rows, *MID)
    total = int(ref["offsets"][-1])
    u8, ip = rows.ctypes.data_as(_lib.U8P), (lambda a: a.ctypes.data_as(_lib.IP))
    count, offsets = np.zeros(40, np.int32), np.zeros(41, np.int64)
    op = offsets.ctypes.data_as(_lib.I64P)
    call = lambda cap, lst, n_bins=256, N=40, num=MID[0], den=MID[1]: lib.gaudi_host_fp_neighbours(  # noqa: E731
        n_bins, N, u8, num, den, ip(count), cap, op, lst)
    assert call(0, None) == 0 and np.array_equal(count, ref["count"]) and np.array_equal(offsets, ref["offsets"])
    count[:], offsets[:] = 0, 0
    small = np.full(total, -7, np.int32)
    assert call(total - 1, ip(small)) == _lib.E_CAPACITY  # too small: refused AFTER the counts and offsets are written
    assert np.array_equal(count, ref["count"]) and np.array_equal(offsets, ref["offsets"]) and (small == -7).all()
    exact = np.full(total + 1, -7, np.int32)
    assert call(total, ip(exact)) == 0 and np.array_equal(exact[:total], ref["list"]) and exact[total] == -7
    assert call(5, None) == -1 and call(-1, None) == -1
    for num, den in ((1, 0), (2, 1), (-1, 2), (1, 65537)):
        assert call(0, None, num=num, den=den) == -1
    assert call(0, None, num=65536, den=65536) == 0
    assert call(0, None, n_bins=128) == -1 and call(0, None, N=-1) == -1
    assert call(0, None, N=(1 << 20) + 1) == _lib.E_CAPACITY
    out = [np.zeros(40, np.int32) for _ in range(4)] + [np.zeros(1, np.int32)]
    assert lib.gaudi_host_fp_cluster(256, (1 << 20) + 1, u8, 1, 2, *map(ip, out)) == _lib.E_CAPACITY
    assert lib.gaudi_host_fp_cluster(256, 40, u8, 3, 2, *map(ip, out)) == -1
    pk = [np.zeros(40, np.int32) for _ in range(3)] + [np.zeros(1, np.int32)] + [np.zeros(40, np.int32) for _ in range(3)]
    assert lib.gaudi_host_fp_pick_diverse(256, 40, u8, 0, None, -1, 5, 0, 0, *map(ip, pk)) == 0 and pk[3][0] == 5
    assert lib.gaudi_host_fp_pick_diverse(256, 40, u8, 0, None, -1, 5, 1, 70000, *map(ip, pk)) == -1
    assert lib.gaudi_host_fp_pick_diverse(256, 40, u8, 0, None, -1, -1, 0, 0, *map(ip, pk)) == -1
    assert lib.gaudi_host_fp_pick_diverse(256, 40, u8, 3, None, -1, 5, 0, 0, *map(ip, pk)) == -1  # no resident library on the host


def test_declarations():
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    assert "#define GAUDI_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7 and _lib.load_library().gaudi_abi_version() == 7
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(_lib.EXPORTS[name][1]) == m.group(1).count(",") + 1, name
        assert header.index("(Entry points ADDED since") < header.index(name) < header.index("#define GAUDI_ABI_VERSION")
    for name in NEW[:3]:
        assert name in _lib._FP_EXPORTS and _lib.EXPORTS[name][1][1:] == _lib.EXPORTS[name.replace("gaudi_", "gaudi_host_")][1]
    assert _lib.EXPORTS["gaudi_fp_neighbours"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, _lib.U8P, C.c_int, C.c_int, _lib.IP,
                                                             C.c_int64, _lib.I64P, _lib.IP])
    assert "DESIGN.md section 8q" in header and re.search(r"\bint gaudi_fp_select_stages_get\(gaudi_handle\* h, double\* ms_out\);", header)
    assert _lib.EXPORTS["gaudi_fp_select_stages_get"] == (C.c_int, [C.c_void_p, _lib.DP])


def test_python_layer_on_a_host_engine(g32_rows):
    from gaudi_amd.similarity import Library, cluster, neighbours, pick_diverse
    eng = HostEngine()
    # threshold conversion: a float through limit_denominator(65536), a Fraction or a pair as given; the exact rational comes back
    assert _lib.fp_threshold(0.7) == (7, 10) and _lib.fp_threshold(Fraction(2, 3)) == (2, 3) and _lib.fp_threshold((14, 20)) == (14, 20)
    assert _lib.fp_threshold(1 / 3) == (1, 3) and _lib.fp_threshold(0) == (0, 1) and _lib.fp_threshold(1.0) == (1, 1)
    assert _lib.fp_threshold(0.123456789) == tuple(Fraction(0.123456789).limit_denominator(65536).as_integer_ratio())
    for bad in (1.5, -0.1, (3, 2), (1, 0), Fraction(1, 70001)):
        with pytest.raises(_lib.GaudiError, match="threshold"):
            _lib.fp_threshold(bad)
    rows = g32_rows[:120]
    raw = _lib.host_fp_cluster(rows, *MID)
    cl = cluster(rows, 0.7, engine=eng)
    assert cl["threshold"] == Fraction(7, 10) and cl["n_clusters"] == raw["n_clusters"] and cl["cluster"].dtype == np.int64
    assert np.array_equal(cl["cluster"], raw["cluster"]) and np.array_equal(cl["centroids"], raw["centroid"][:raw["n_clusters"]])
    assert np.array_equal(cl["sizes"], raw["size"][:raw["n_clusters"]]) and np.array_equal(cl["count"], raw["count"])
    assert set(cl) == {"cluster", "centroids", "sizes", "count", "n_clusters", "threshold"}
    nb = neighbours(rows, (14, 20), engine=eng)
    ref = _lib.host_fp_neighbours(rows, *MID)
    assert set(nb) == {"count", "offsets", "list", "threshold"} and nb["threshold"] == Fraction(7, 10)
    assert all(np.array_equal(nb[k], ref[k]) for k in NB_KEYS)
    pk = pick_diverse(rows, 10, engine=eng)
    raw = _lib.host_fp_pick_diverse(rows, 10)
    assert set(pk) == {"picked", "pick_similarity", "owner", "owner_similarity", "n_picked", "threshold"} and pk["threshold"] is None
    assert pk["picked"].dtype == np.int64 and pk["pick_similarity"].dtype == pk["owner_similarity"].dtype == np.float64
    assert np.array_equal(pk["picked"], raw["picked"]) and pk["n_picked"] == 10 and pk["pick_similarity"][0] == 0.0
    assert np.array_equal(pk["pick_similarity"][1:], raw["pick_common"][1:] / raw["pick_union"][1:])
    assert (pk["owner_similarity"][pk["picked"]] == 1.0).all() and np.array_equal(pk["owner"], raw["owner"])
    stop = pick_diverse(rows, 500, threshold=Fraction(7, 10), seeds=g32_rows[5:8], engine=eng)  # (seeds equal to batch rows own them)
    assert stop["threshold"] == Fraction(7, 10) and 0 < stop["n_picked"] == len(stop["picked"]) < 120
    assert (stop["owner_similarity"][rows.any(-1)] >= 0.7).all() and stop["owner"][5:8].tolist() == [-2, -3, -4]
    assert pick_diverse(rows, 3, first=17, engine=eng)["picked"][0] == 17
    with pytest.raises(ValueError, match="first"):
        pick_diverse(rows, 3, seeds=g32_rows[200:203], first=17, engine=eng)
    # a Library as seeds means the resident one: there is none without a device
    lib = Library.__new__(Library)
    lib.engine, lib.M, lib.n_bins = eng, 3, 1024
    eng._fp_library = lib
    with pytest.raises(_lib.GaudiError, match=r"gaudi_host_fp_pick_diverse failed \(-1\)"):
        pick_diverse(rows, 3, seeds=lib, engine=eng)
    other = Library.__new__(Library)
    other.engine, other.M, other.n_bins = HostEngine(), 3, 1024
    with pytest.raises(_lib.GaudiError, match="ITS engine"):
        pick_diverse(rows, 3, seeds=other, engine=eng)


def test_keywords_need_similarity_and_atoms():
    from gaudi_amd import generation_guidance
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    with pytest.raises(ValueError, match="similarity=True"):
        analyze_atoms_for_molecules([], cluster_threshold=0.7)
    for kw in (dict(cluster_threshold=0.7), dict(diverse=5)):
        with pytest.raises(ValueError, match="with_atoms"):
            generation_guidance._evaluate(None, None, None, None, None, 1.0, None, None, None, None, 1.0, similarity=True, **kw)
        with pytest.raises(ValueError, match="with_atoms"):
            generation_guidance._evaluate(None, None, None, None, None, 1.0, None, None, None, None, 1.0, with_atoms=True, **kw)


def test_distinct_rows_are_distinct():
    rows = distinct_rows()
    assert rows.shape == (432, 1024) and len(np.unique(rows, axis=0)) == 432 and rows.any(-1).all()
