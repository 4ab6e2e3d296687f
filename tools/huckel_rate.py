#!/usr/bin/env python3
"""Rates of gaudi_huckel (csrc/huckel.inc): molecules per second for 4 096 copies of a 46-centre cata molecule (eleven rings in
a row: the 64-centre tier) and for 4 096 molecules drawn from the g32 fixture (the ones it solves, with a fixed seed: all three
tiers).  Per figure: the kernels alone from the profile counters (HIP events; one launch per tier present) and the whole call as
a user of Engine.huckel sees it (packed arrays in, fifteen arrays out), each the median of --calls calls after one warm-up call;
and the rotations per second the kernels made.  For context only, numpy.linalg.eigh in float64 on a 64th of the batch, scaled.
The numbers go into DESIGN.md section 8l; there is no threshold and no figure of an earlier revision to compare with.  No
hardware counter pass is made here: the line "not_measured" says what this run leaves open.

    python tools/huckel_rate.py [--calls 5] [--no-numpy]
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


def acene(rings):
    """A row of fused six-rings (cata): 4 * rings + 2 carbons, the hydrogens implied."""
    n = 4 * rings + 2
    top, bottom = list(range(0, 2 * rings + 1)), list(range(2 * rings + 1, n))
    bonds = [(a, a + 1) for a in top[:-1]] + [(a, a + 1) for a in bottom[:-1]] + [(top[2 * k], bottom[2 * k]) for k in range(rings + 1)]
    return np.full(n, 1, np.int32), np.array(bonds, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--molecules", type=int, default=4096)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    from gaudi_amd._lib import host_huckel
    from gaudi_amd.engine import Engine
    from gaudi_amd.huckel import c_huckel_tables
    from tests.bond_order_helpers import fixture, pack
    from tests.huckel_helpers import oracle
    tab = c_huckel_tables("hetro")
    fx = fixture()[1]
    solved = host_huckel(tab, *pack(fx))["status"] == 0
    good = [m for m in fx if solved[m["index"]]]
    rng = np.random.default_rng(0)
    eng = Engine(0)
    B = a.molecules
    for name, mols in (("acene46", [acene(11)] * B), ("g32_mix", [(good[k]["elem"], good[k]["bonds"]) for k in rng.integers(0, len(good), B)])):
        packed = pack(mols)
        run = lambda: eng.huckel(tab, *packed)  # noqa: E731
        out = run()  # warm-up (workspaces, the LDS attribute)
        wall, kernel, launches = [], [], 0
        for _ in range(a.calls):
            eng.profile_reset(True)
            t0 = time.perf_counter()
            run()
            wall.append(time.perf_counter() - t0)
            launches, ms = eng.huckel_profile_get()
            kernel.append(ms)
        eng.profile_reset(False)
        w, k = float(np.median(wall)), float(np.median(kernel))
        n = out["n_pi"].astype(np.int64)
        m = n + (n & 1)
        rotations = int((out["sweeps"] * (m - 1) * (m // 2)).sum())
        line = dict(metric="huckel_molecules_per_s", workload=name, molecules=B, launches_per_call=launches,
                    mean_pi_centres=round(float(n.mean()), 1), max_pi_centres=int(n.max()), mean_sweeps=round(float(out["sweeps"].mean()), 2),
                    statuses=np.bincount(out["status"], minlength=7).tolist(), rotations=rotations, kernel_median_ms=round(k, 4),
                    kernel_molecules_per_s=round(B / (k / 1e3), 1) if k > 0 else None,
                    kernel_rotations_per_s=round(rotations / (k / 1e3), 1) if k > 0 else None, call_median_s=round(w, 5),
                    call_molecules_per_s=round(B / w, 1), output_bytes=int(sum(v.nbytes for v in out.values())))
        if not a.no_numpy:
            part = mols[:max(1, B // 64)]
            t0 = time.perf_counter()
            for mol in part:
                oracle(mol)
            hosts = (time.perf_counter() - t0) * (B / len(part))
            line.update(numpy_molecules=len(part), numpy_s_scaled=round(hosts, 2), numpy_molecules_per_s=round(B / hosts, 1))
        print(json.dumps(line), flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, VALU utilisation, occupancy achieved): no counter pass in this run",
                                        "the 128-centre tier alone", "batches other than 4 096"])))
    eng.close()


if __name__ == "__main__":
    main()
