#!/usr/bin/env python3
"""Rates of neighbour lists, Butina clusters and MaxMin picks (csrc/fp_select.inc) on rows built as tools/similarity_rate.py builds
its library: the real fingerprints of 1024 cata-condensed molecules of 11 rings at 1024 bins, tiled and perturbed in a few bins
per row.  Every figure is the median of --calls calls after one warm-up call; kernel times are HIP events by stage
(gaudi_fp_select_stages_get).

  neighbours   N = --rows: pairs/s of the COUNT pass and of COUNT + offsets + FILL, next to gaudi_fp_nearest at k = 1 on the same
               N x N pairs in the same run and to the v_sad_u8 issue bound (n_bins / 4 byte-quad instructions per pair on 1024
               SIMDs x 16 lanes per clock)
  cluster      the same N: the sort and the walk apart from the neighbour passes
  pick         N = --pick-rows (several): k = --picks rounds, time per round, bytes/s at N * n_bins bytes a round, next to
               fp_totals_kernel over the same rows in the same run (it reads every byte once), and the share of a dependent
               launch boundary (--boundary-us, 1.5 - 1.9 us on this part) in a round

The numbers go into DESIGN.md section 8q; there is no threshold on any of them.

    python tools/diversity_rate.py [--rows 65536] [--pick-rows 4096,16384,65536,262144] [--picks 256] [--threshold 0.7] [--calls 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)

from atoms_rate import cata_molecule  # noqa: E402


def medians(eng, fn, calls, stages=True):
    """-> (median wall seconds, median of every stage in ms, median summed kernel ms of the fingerprint log)."""
    fn()  # warm-up (workspaces)
    wall, rows, logged = [], [], []
    for _ in range(calls):
        eng.profile_reset(True)
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
        logged.append(eng.fp_profile_get()[1])
        rows.append(eng.fp_select_stages_get() if stages else {})
    eng.profile_reset(False)
    return float(np.median(wall)), {k: float(np.median([r[k] for r in rows])) for k in rows[0]}, float(np.median(logged))


def make_rows(base, M, rng, n_bins):
    rows = np.array(base[np.arange(M) % len(base)])
    at = rng.integers(0, n_bins, (M, 3))
    rows[np.arange(M)[:, None], at] = (rows[np.arange(M)[:, None], at].astype(np.int64) + rng.integers(0, 3, (M, 3))).clip(0, 255)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--pick-rows", default="4096,16384,65536,262144")
    ap.add_argument("--picks", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=0.7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--clock-mhz", type=float, default=2400.0)
    ap.add_argument("--boundary-us", type=float, default=1.7)
    a = ap.parse_args()
    from gaudi_amd import _lib
    from gaudi_amd.engine import Engine
    from gaudi_amd.gor2goa import rings_to_atoms
    from gaudi_amd.similarity import fingerprints
    rng = np.random.default_rng(0)
    B, n, n_bins = 1024, 11, 1024
    X = np.stack([cata_molecule(rng, n) for _ in range(B)])
    eng = Engine(0)
    recs = rings_to_atoms((X, np.zeros((B, n), np.int32), np.full(B, n, np.int32)), "cata", 0.1, place_hydrogens=True, engine=eng)
    base = fingerprints(recs, "cata", engine=eng)["fp"]
    num, den = _lib.fp_threshold(a.threshold)
    bound = 1024 * 16 * a.clock_mhz * 1e6 / (n_bins / 4)

    N = a.rows
    rows = make_rows(base, N, rng, n_bins)
    pairs = float(N) * N
    u8, ip = rows.ctypes.data_as(_lib.U8P), (lambda x: x.ctypes.data_as(_lib.IP))
    count, offsets = np.zeros(N, np.int32), np.zeros(N + 1, np.int64)

    def count_only(num=num, den=den):
        rc = eng.lib.gaudi_fp_neighbours(eng.h, n_bins, N, u8, num, den, ip(count), 0, offsets.ctypes.data_as(_lib.I64P), None)
        if rc != _lib.E_CAPACITY:  # (beyond 2^28 entries the counts and the 64-bit offsets are still written)
            eng._check(rc, "gaudi_fp_neighbours")
        return rc

    cw, cs, _ = medians(eng, count_only, a.calls)
    asked, entries_asked = f"{num}/{den}", int(offsets[N])
    # the lists and the clusters at the lowest of these thresholds whose lists fit 2^28 entries
    for t in (a.threshold, 0.8, 0.9, 0.95, 0.98, 1.0):
        num, den = _lib.fp_threshold(max(t, a.threshold))
        if count_only(num, den) == 0:
            break
    total = int(offsets[N])
    lst = np.zeros(max(total, 1), np.int32)

    def whole():
        eng._check(eng.lib.gaudi_fp_neighbours(eng.h, n_bins, N, u8, num, den, ip(count), total, offsets.ctypes.data_as(_lib.I64P),
                                               ip(lst)), "gaudi_fp_neighbours")

    ww, ws, _ = medians(eng, whole, a.calls)
    nw, _, nk = medians(eng, lambda: eng.fp_nearest(rows, rows, 1), a.calls, stages=False)
    both = ws["count"] + ws["offsets"] + ws["fill"]
    print(json.dumps(dict(metric="neighbours_pairs_per_s", rows=N, n_bins=n_bins, count_threshold=asked, count_entries=entries_asked,
                          threshold=f"{num}/{den}", entries=total,
                          live=int((count > 0).sum()), count_ms=round(cs["count"], 3), offsets_ms=round(cs["offsets"], 4),
                          count_pairs_per_s=round(pairs / (cs["count"] / 1e3), 1), count_call_s=round(cw, 4),
                          fill_ms=round(ws["fill"], 3), count_of_whole_ms=round(ws["count"], 3), whole_kernels_ms=round(both, 3),
                          whole_pairs_per_s=round(pairs / (both / 1e3), 1), whole_call_s=round(ww, 4),
                          nearest_k1_ms=round(nk, 3), nearest_k1_pairs_per_s=round(pairs / (nk / 1e3), 1), nearest_call_s=round(nw, 4),
                          count_over_nearest=round(cs["count"] / nk, 3), whole_over_nearest=round(both / nk, 3),
                          bound_pairs_per_s=round(bound, 1), clock_mhz=a.clock_mhz,
                          count_fraction_of_bound=round(pairs / (cs["count"] / 1e3) / bound, 4),
                          nearest_fraction_of_bound=round(pairs / (nk / 1e3) / bound, 4))))

    lw, ls, _ = medians(eng, lambda: eng.fp_cluster(rows, num, den), a.calls)
    cl = eng.fp_cluster(rows, num, den)
    print(json.dumps(dict(metric="cluster", rows=N, n_bins=n_bins, threshold=f"{num}/{den}", n_clusters=cl["n_clusters"],
                          largest=int(cl["size"].max()), singletons=int((cl["size"][:cl["n_clusters"]] == 1).sum()),
                          count_ms=round(ls["count"], 3), offsets_ms=round(ls["offsets"], 4), fill_ms=round(ls["fill"], 3),
                          sort_ms=round(ls["sort"], 4), walk_ms=round(ls["walk"], 4), call_s=round(lw, 4))))

    k = a.picks
    for M in [int(v) for v in a.pick_rows.split(",") if v]:
        prow = rows[:M] if M <= N else make_rows(base, M, rng, n_bins)
        pw, ps, _ = medians(eng, lambda: eng.fp_pick_diverse(prow, k), a.calls)
        out = eng.fp_pick_diverse(prow, k)
        per_round_us = ps["pick_rounds"] / out["n_picked"] * 1e3
        nbytes = float(M) * n_bins
        print(json.dumps(dict(metric="pick_round", rows=M, n_bins=n_bins, mib=round(nbytes / 2 ** 20, 1), picks=out["n_picked"],
                              rounds_ms=round(ps["pick_rounds"], 4), round_us=round(per_round_us, 3),
                              round_bytes_per_s=round(nbytes / (per_round_us / 1e6), 1), totals_us=round(ps["totals"] * 1e3, 3),
                              totals_bytes_per_s=round(nbytes / (ps["totals"] / 1e3), 1) if ps["totals"] > 0 else None,
                              round_over_totals=round(per_round_us / (ps["totals"] * 1e3), 3) if ps["totals"] > 0 else None,
                              boundary_us=a.boundary_us, boundary_share=round(a.boundary_us / per_round_us, 4),
                              setup_ms=round(ps["pick_setup"], 4), call_s=round(pw, 4))))
    eng.close()


if __name__ == "__main__":
    main()
