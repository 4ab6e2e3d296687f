#!/usr/bin/env python3
"""Molecules per second of gaudi_amd.gor2goa.bond_orders (bond orders and formal charges from connectivity, one launch per call)
at B = 8192 cata-condensed molecules of 11 rings with their hydrogens placed (46 C + 28 H each), built by rings_to_atoms first.
Two figures: the whole call as a user sees it (packing, copies to and from the device, the per-molecule records) and the kernel
alone (HIP events around the launch).  One warm-up call, then --calls timed calls.  The number goes into DESIGN.md; there is no
threshold.

    python tools/bonds_rate.py [--batch 8192] [--calls 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from gaudi_amd.engine import Engine
    from gaudi_amd.gor2goa import bond_orders, rings_to_atoms
    rng = np.random.default_rng(0)
    B, n = a.batch, 11
    pool = [cata_molecule(rng, n) for _ in range(min(B, 512))]
    X = np.stack([pool[b % len(pool)] for b in range(B)])
    eng = Engine(0)
    recs = rings_to_atoms((X, np.zeros((B, n), np.int32), np.full(B, n, np.int32)), "cata", 0.1, place_hydrogens=True, engine=eng)
    out = bond_orders(recs, "cata", engine=eng)  # warm-up (workspaces)
    eng.profile_reset(True)
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        bond_orders(recs, "cata", engine=eng)
        times.append(time.perf_counter() - t0)
    launches, ms = eng.bonds_profile_get()
    med = float(np.median(times))
    print(json.dumps(dict(metric="bonds_molecules_per_s", batch=B, rings=n, calls=a.calls,
                          built=sum(r["status"] == 0 for r in recs), with_structure=sum(o["kekule_status"] == 0 for o in out),
                          charged=sum(o["n_charged"] > 0 for o in out), call_median_s=round(med, 5),
                          call_molecules_per_s=round(B / med, 1), launches=launches,
                          kernel_ms_per_launch=round(ms / max(launches, 1), 4),
                          kernel_molecules_per_s=round(B * launches / (ms / 1e3), 1) if ms > 0 else None)))
    eng.close()


if __name__ == "__main__":
    main()
