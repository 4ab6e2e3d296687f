#!/usr/bin/env python3
"""Rates of gaudi_amd.similarity (csrc/fp.inc): fingerprints per second at B = 1024 built cata-condensed molecules of 11 rings, and
pairs per second of the nearest-neighbour search at B = 1024 and B = 64 queries against a library of M = 2^18 rows of 1024 bins
-- real fingerprints, tiled and perturbed in a few bins per row -- once with the library resident on the device and once passed
in (the difference is the upload).  Per figure: the whole call as a user sees it and the kernels alone (HIP events), each the
median of --calls calls after one warm-up call.  The kernel time is set against the instruction bound: n_bins / 4 byte-quad
instructions per pair on 1024 SIMDs x 16 lanes per clock.  For context, the same search in numpy on the host with --threads
threads, on a slice of the library, scaled.  The numbers go into DESIGN.md section 8j; there is no threshold.

    python tools/similarity_rate.py [--rows 262144] [--calls 5] [--clock-mhz 2400]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)

from atoms_rate import cata_molecule  # noqa: E402


def median_call(eng, fn, calls):
    fn()  # warm-up (workspaces)
    wall, kernel = [], []
    for _ in range(calls):
        eng.profile_reset(True)
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
        n, ms = eng.fp_profile_get()
        assert n == 1
        kernel.append(ms)
    eng.profile_reset(False)
    return float(np.median(wall)), float(np.median(kernel))


def numpy_nearest_seconds(q, lib, threads):
    """Seconds of a k = 1 search of q against lib in numpy, the queries spread over `threads` threads."""
    tl = lib.sum(-1, dtype=np.int64)

    def one(rows):
        for row in rows:
            common = np.minimum(row[None, :], lib).sum(-1, dtype=np.int64)
            union = int(row.sum()) + tl - common
            (common / np.maximum(union, 1)).argmax()

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, np.array_split(q, threads)))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 18)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--clock-mhz", type=float, default=2400.0)
    a = ap.parse_args()
    from gaudi_amd.engine import Engine
    from gaudi_amd.gor2goa import rings_to_atoms
    from gaudi_amd.similarity import Library, fingerprints
    rng = np.random.default_rng(0)
    B, n, n_bins = 1024, 11, 1024
    X = np.stack([cata_molecule(rng, n) for _ in range(B)])
    eng = Engine(0)
    recs = rings_to_atoms((X, np.zeros((B, n), np.int32), np.full(B, n, np.int32)), "cata", 0.1, place_hydrogens=True, engine=eng)
    fp = fingerprints(recs, "cata", engine=eng)
    w, k = median_call(eng, lambda: fingerprints(recs, "cata", engine=eng), a.calls)
    print(json.dumps(dict(metric="fingerprints_per_s", input="cata, 11 rings, hydrogens placed", batch=B,
                          built=int((fp["status"] == 0).sum()), distinct_rows=len({r.tobytes() for r in fp["fp"]}),
                          call_median_s=round(w, 5), call_per_s=round(B / w, 1), kernel_median_ms=round(k, 4),
                          kernel_per_s=round(B / (k / 1e3), 1) if k > 0 else None)))
    M = a.rows
    lib = np.array(fp["fp"][np.arange(M) % B])
    at = rng.integers(0, n_bins, (M, 3))
    lib[np.arange(M)[:, None], at] = (lib[np.arange(M)[:, None], at].astype(np.int64) + rng.integers(0, 3, (M, 3))).clip(0, 255)
    bound_pairs_per_s = 1024 * 16 * a.clock_mhz * 1e6 / (n_bins / 4)
    res = Library(lib, engine=eng)
    for nq in (1024, 64):
        q = fp["fp"][:nq]
        rw, rk = median_call(eng, lambda: res.nearest(q, 1), a.calls)
        pw, pk = median_call(eng, lambda: eng.fp_nearest(q, lib, 1), a.calls)
        pairs = nq * M
        sub = lib[: max(1, M // 64)]
        host = numpy_nearest_seconds(q, sub, a.threads) * (M / len(sub))
        print(json.dumps(dict(metric="nearest_pairs_per_s", queries=nq, rows=M, n_bins=n_bins, k=1,
                              resident_call_s=round(rw, 5), resident_call_pairs_per_s=round(pairs / rw, 1),
                              passed_in_call_s=round(pw, 5), upload_s=round(pw - rw, 5),
                              kernel_median_ms=round(rk, 4), kernel_passed_in_median_ms=round(pk, 4),
                              kernel_pairs_per_s=round(pairs / (rk / 1e3), 1) if rk > 0 else None,
                              bound_pairs_per_s=round(bound_pairs_per_s, 1), clock_mhz=a.clock_mhz,
                              fraction_of_bound=round(pairs / (rk / 1e3) / bound_pairs_per_s, 4) if rk > 0 else None,
                              numpy_threads=a.threads, numpy_s_scaled=round(host, 3), numpy_pairs_per_s=round(pairs / host, 1))))
    res.close()
    eng.close()


if __name__ == "__main__":
    main()
