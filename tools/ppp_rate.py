#!/usr/bin/env python3
"""Rates of gaudi_ppp (csrc/ppp.inc): molecules per second for 4 096 copies of a 46-centre cata molecule (eleven rings in a row,
regular hexagons of side 1.40 A: the 64-centre tier) and for 4 096 molecules drawn from the g30 fixture (the closed-shell ones the
reference built, with a fixed seed).  Per figure: the kernels alone from the profile counters (HIP events; one launch per tier
present) and the whole call as a user of Engine.ppp sees it (packed arrays in, eighteen arrays out), each the median of --calls
calls after one warm-up call; and the mean SCF iterations and Jacobi sweeps per molecule.  The numbers go into DESIGN.md section
8m; there is no threshold and no figure of an earlier revision to compare with.  No hardware counter pass is made here: the line
"not_measured" says what this run leaves open.

    python tools/ppp_rate.py [--calls 5] [--molecules 4096]
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


def acene(rings, side=1.40):
    """A row of fused regular six-rings (cata): 4 * rings + 2 carbons in the plane, the hydrogens implied."""
    step = side * np.sqrt(3.0)
    index, xyz, bonds = {}, [], set()
    for k in range(rings):
        ring = []
        for j in range(6):
            t = np.deg2rad(30.0 + 60.0 * j)
            p = (k * step + side * np.cos(t), side * np.sin(t))
            key = (int(round(p[0] * 100)), int(round(p[1] * 100)))
            if key not in index:
                index[key] = len(xyz)
                xyz.append([p[0], p[1], 0.0])
            ring.append(index[key])
        bonds |= {tuple(sorted((ring[j], ring[(j + 1) % 6]))) for j in range(6)}
    return np.full(len(xyz), 1, np.int32), np.array(sorted(bonds), np.int32), np.array(xyz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--molecules", type=int, default=4096)
    a = ap.parse_args()
    from gaudi_amd._lib import host_ppp
    from gaudi_amd.engine import Engine
    from gaudi_amd.ppp import c_ppp_tables
    from tests.ppp_helpers import g30_molecules, pack
    tab = c_ppp_tables("hetro")
    fx = g30_molecules()
    status = host_ppp(tab, *pack(fx))["status"]
    good = [m for m, st in zip(fx, status) if st in (0, 1)]
    rng = np.random.default_rng(0)
    eng = Engine(0)
    B = a.molecules
    for name, mols in (("acene46", [acene(11)] * B), ("g30_mix", [good[k] for k in rng.integers(0, len(good), B)])):
        packed = pack(mols)
        run = lambda: eng.ppp(tab, *packed)  # noqa: E731
        out = run()  # warm-up (workspaces, the LDS attribute)
        wall, kernel, launches = [], [], 0
        for _ in range(a.calls):
            eng.profile_reset(True)
            t0 = time.perf_counter()
            run()
            wall.append(time.perf_counter() - t0)
            launches, ms = eng.ppp_profile_get()
            kernel.append(ms)
        eng.profile_reset(False)
        w, k = float(np.median(wall)), float(np.median(kernel))
        print(json.dumps(dict(metric="ppp_molecules_per_s", workload=name, molecules=B, launches_per_call=launches,
                              mean_pi_centres=round(float(out["n_pi"].mean()), 1), max_pi_centres=int(out["n_pi"].max()),
                              mean_iterations=round(float(out["iterations"].mean()), 2), max_iterations=int(out["iterations"].max()),
                              mean_sweeps=round(float(out["sweeps"].mean()), 2),
                              sweeps_per_iteration=round(float(out["sweeps"].sum()) / max(1, int(out["iterations"].sum())), 2),
                              statuses=np.bincount(out["status"], minlength=9).tolist(), kernel_median_ms=round(k, 4),
                              kernel_molecules_per_s=round(B / (k / 1e3), 1) if k > 0 else None, call_median_s=round(w, 5),
                              call_molecules_per_s=round(B / w, 1), output_bytes=int(sum(v.nbytes for v in out.values())))), flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, VALU utilisation, occupancy achieved): no counter pass in this run",
                                        "the 128-centre tier alone", "batches other than the one given", "the Ohno formula's rate"])))
    eng.close()


if __name__ == "__main__":
    main()
