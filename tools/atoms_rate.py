#!/usr/bin/env python3
"""Molecules per second of gaudi_amd.gor2goa.rings_to_atoms (graph of rings -> graph of atoms, one launch per call) at B = 8192
cata-condensed molecules of 11 rings, with hydrogens placed and fingerprints.  Two figures: the whole call as a user sees it
(packing, copies to and from the device, the per-molecule records) and the kernel alone (HIP events around the launch).
One warm-up call, then --calls timed calls.  The number goes into DESIGN.md; there is no threshold.

    python tools/atoms_rate.py [--batch 8192] [--calls 5] [--plain]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)


def cata_molecule(rng, n, jitter=0.02):
    """Ring centres of a cata-condensed molecule: tree growth on a triangular lattice of spacing ~2.45 A, jittered, rotated."""
    dirs = [(1, 0), (0, 1), (-1, 1), (-1, 0), (0, -1), (1, -1)]
    occ = [(0, 0)]
    while len(occ) < n:
        a, d = occ[rng.integers(len(occ))], dirs[rng.integers(6)]
        c = (a[0] + d[0], a[1] + d[1])
        if c in occ or sum(((c[0] + e[0], c[1] + e[1]) in occ) for e in dirs) > 1:
            continue
        occ.append(c)
    occ = np.array(occ, np.float64)
    x = np.stack([occ[:, 0] + 0.5 * occ[:, 1], occ[:, 1] * np.sqrt(3) / 2, np.zeros(n)], 1) * rng.uniform(2.42, 2.48)
    x += rng.standard_normal(x.shape) * jitter
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return ((x - x.mean(0)) @ q).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--plain", action="store_true", help="no hydrogens, no fingerprints: the reference's gor2goa alone")
    a = ap.parse_args()
    from gaudi_amd.engine import Engine
    from gaudi_amd.gor2goa import rings_to_atoms
    rng = np.random.default_rng(0)
    B, n = a.batch, 11
    pool = [cata_molecule(rng, n) for _ in range(min(B, 512))]
    X = np.stack([pool[b % len(pool)] for b in range(B)])
    packed = (X, np.zeros((B, n), np.int32), np.full(B, n, np.int32))
    eng = Engine(0)
    kw = dict(place_hydrogens=not a.plain, fingerprint=not a.plain, engine=eng)
    recs = rings_to_atoms(packed, "cata", 0.1, **kw)  # warm-up (workspaces)
    built = sum(r["status"] == 0 for r in recs)
    eng.profile_reset(True)
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        rings_to_atoms(packed, "cata", 0.1, **kw)
        times.append(time.perf_counter() - t0)
    launches, ms = eng.atoms_profile_get()
    med = float(np.median(times))
    print(json.dumps(dict(metric="atoms_molecules_per_s", batch=B, rings=n, calls=a.calls, hydrogens=not a.plain,
                          fingerprint=not a.plain, built=built, distinct=len({r["fingerprint"] for r in recs}),
                          call_median_s=round(med, 5), call_molecules_per_s=round(B / med, 1), launches=launches,
                          kernel_ms_per_launch=round(ms / max(launches, 1), 4),
                          kernel_molecules_per_s=round(B * launches / (ms / 1e3), 1) if ms > 0 else None)))
    eng.close()


if __name__ == "__main__":
    main()
