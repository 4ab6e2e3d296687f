"""Shared by test_diversity_cpu.py and test_gpu_diversity.py: an oracle for neighbour lists, Butina clusters and MaxMin picks that
shares nothing with the C code (numpy for `common`, Python integers and fractions.Fraction for every comparison, a literal O(N^2)
neighbour set, a literal sort-and-walk, a literal picking loop), the rows the tests use, and an engine on the host twins."""
from fractions import Fraction

import numpy as np

from gaudi_amd import _lib
from tests.similarity_helpers import g32_fingerprints, numpy_common

MID = (7, 10)  # the in-between threshold: test_diversity_cpu.py asserts on the oracle alone that it makes g32 mean something
_CACHE = {}


def rows_of(n_bins, count, seed, perturb=True):
    """`count` rows from g32's real fingerprints, tiled (so rows repeat) and, where asked, every third row perturbed in a few bins
    (so near-duplicates sit next to exact ones)."""
    base = g32_fingerprints(2, n_bins)["fp"]
    rng = np.random.default_rng(seed)
    rows = np.array(base[(np.arange(count) * 5 + seed) % len(base)])
    if perturb:
        for r in range(0, count, 3):
            at = rng.integers(0, n_bins, 4)
            rows[r, at] = (rows[r, at].astype(np.int64) + rng.integers(0, 3, 4)).clip(0, 255)
    return rows


def distinct_rows(n_bins=1024):
    """One row per isomorphism class of g32, in fixture order: live and pairwise different."""
    key = ("distinct", n_bins)
    if key not in _CACHE:
        out = g32_fingerprints(2, n_bins)
        rows = np.array(out["fp"])[out["total"] > 0]
        rows = rows[np.sort(np.unique(rows, axis=0, return_index=True)[1])]
        rows.setflags(write=False)
        _CACHE[key] = rows
    return _CACHE[key]


def sims(a, b=None):
    """(similarity as a Fraction for every pair [Na][Nb] (0 where union = 0), totals of a, totals of b) in Python integers."""
    a = np.asarray(a)
    b = a if b is None else np.asarray(b)
    ta, tb = [int(t) for t in a.astype(np.int64).sum(-1)], [int(t) for t in b.astype(np.int64).sum(-1)]
    common = numpy_common(a, b) if len(a) and len(b) else np.zeros((len(a), len(b)), np.int64)
    out = []
    for i in range(len(a)):
        row = []
        for j in range(len(b)):
            c = int(common[i, j])
            u = ta[i] + tb[j] - c
            row.append((Fraction(c, u) if u > 0 else Fraction(0), c, u))
        out.append(row)
    return out, ta, tb


def oracle_neighbours(rows, thr, table=None):
    """-> dict(count, offsets, list) with the lists as a list of lists too (``lists``)."""
    thr = Fraction(*thr) if isinstance(thr, tuple) else Fraction(thr)
    s, t, _ = table or sims(rows)
    N = len(t)
    lists = [[j for j in range(N) if t[i] > 0 and t[j] > 0 and s[i][j][2] > 0 and s[i][j][0] >= thr] for i in range(N)]
    count = np.array([len(x) for x in lists], np.int32).reshape(N)
    offsets = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    return dict(count=count, offsets=offsets, list=np.array([j for x in lists for j in x], np.int32), lists=lists, total=t)


def oracle_cluster(rows, thr, table=None):
    nb = oracle_neighbours(rows, thr, table)
    N = len(nb["total"])
    order = sorted(range(N), key=lambda i: (-int(nb["count"][i]), i))
    cluster, centroid, size = np.full(N, -1, np.int32), np.full(N, -1, np.int32), np.zeros(N, np.int32)
    n = 0
    for i in order:
        if nb["total"][i] == 0 or cluster[i] >= 0:
            continue
        centroid[n] = i
        for j in nb["lists"][i]:
            if cluster[j] < 0:
                cluster[j] = n
                size[n] += 1
        n += 1
    return dict(cluster=cluster, centroid=centroid, size=size, count=nb["count"], n_clusters=n)


def oracle_pick(rows, k, thr=None, seeds=None, first=-1, table=None):
    """The literal MaxMin loop.  near(i) = (similarity, common, union, owner) or None."""
    thr = None if thr is None else Fraction(*thr) if isinstance(thr, tuple) else Fraction(thr)
    s, t, _ = table or sims(rows)
    N = len(t)
    live = [t[i] > 0 for i in range(N)]
    near = [None] * N
    if seeds is not None and len(seeds):
        ss, _, _ = sims(rows, seeds)
        for i in range(N):
            if not live[i]:
                continue
            for j in range(len(seeds)):  # the most similar seed, of equally similar ones the first
                if near[i] is None or ss[i][j][0] > near[i][0]:
                    near[i] = (ss[i][j][0], ss[i][j][1], ss[i][j][2], -2 - j)
    have_seeds = seeds is not None and len(seeds) > 0
    picked, pc, pu = np.full(k, -1, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
    chosen = set()
    n = 0
    for step in range(k):
        cand = [i for i in range(N) if live[i] and i not in chosen]
        if step == 0 and not have_seeds and first >= 0:
            cand = [i for i in cand if i == first]
        if not cand:
            break
        sim_of = lambda i: Fraction(0) if near[i] is None else near[i][0]  # noqa: E731
        p = min(cand, key=lambda i: (sim_of(i), i))
        if thr is not None and near[p] is not None and near[p][2] > 0 and near[p][0] >= thr:
            break
        picked[n], pc[n], pu[n] = p, (0 if near[p] is None else near[p][1]), (0 if near[p] is None else near[p][2])
        n += 1
        chosen.add(p)
        for i in range(N):
            if not live[i]:
                continue
            if i == p:
                near[i] = (Fraction(1), t[i], t[i], p)
            elif near[i] is None or s[i][p][0] > near[i][0]:
                near[i] = (s[i][p][0], s[i][p][1], s[i][p][2], p)
    owner = np.array([-1 if x is None else x[3] for x in near], np.int32).reshape(N)
    oc = np.array([0 if x is None else x[1] for x in near], np.int32).reshape(N)
    ou = np.array([0 if x is None else x[2] for x in near], np.int32).reshape(N)
    return dict(picked=picked, pick_common=pc, pick_union=pu, n_picked=n, owner=owner, owner_common=oc, owner_union=ou)


NB_KEYS = ("count", "offsets", "list")
CL_KEYS = ("cluster", "centroid", "size", "count", "n_clusters")
PK_KEYS = ("picked", "pick_common", "pick_union", "n_picked", "owner", "owner_common", "owner_union")


def same(got, ref, keys):
    """Every output exactly equal, dtypes included where both are arrays."""
    for k in keys:
        a, b = got[k], ref[k]
        if isinstance(b, np.ndarray):
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
        else:
            assert int(a) == int(b), (k, a, b)


class HostEngine:
    """What gaudi_amd.similarity asks of an engine for neighbours, clusters and picks, on the host twins (no resident library)."""

    def fp_neighbours(self, rows, num, den):
        return _lib.host_fp_neighbours(rows, num, den)

    def fp_cluster(self, rows, num, den):
        return _lib.host_fp_cluster(rows, num, den)

    def fp_pick_diverse(self, rows, k, num=0, den=0, seeds=None, first=-1, S=None):
        S = (0 if seeds is None else len(seeds)) if S is None else int(S)
        return _lib.fp_pick_call(_lib.load_library().gaudi_host_fp_pick_diverse, (), rows, S, seeds, first, k, num, den)
