#!/usr/bin/env python3
"""Rates of gaudi_ring_currents (csrc/ring_current.inc): molecules per second for 4 096 copies of a 46-centre cata molecule (eleven
rings in a row of regular hexagons: the 64-centre tier) and for 4 096 molecules drawn from golden g30 (the ones it solves, with a
fixed seed: all three tiers).  Per figure: the kernels alone from the profile counters (HIP events; one launch per tier present)
and the whole call as a user of Engine.ring_currents sees it (packed arrays in, fifteen arrays out), each the median of --calls
calls after one warm-up call; beside them gaudi_huckel's kernel time on the same batch, measured the same way -- the ring currents
run its diagonalisation and add the response, the rings and the small solve.  The numbers go into DESIGN.md section 8p; there is
no threshold and no figure of an earlier revision to compare with.  No hardware counter pass is made here: the line
"not_measured" says what this run leaves open.

    python tools/ring_current_rate.py [--calls 5]
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


def timed(eng, run, get, calls):
    """(median wall seconds, median kernel ms, launches per call) of ``calls`` calls after one warm-up."""
    run()
    wall, kernel, launches = [], [], 0
    for _ in range(calls):
        eng.profile_reset(True)
        t0 = time.perf_counter()
        run()
        wall.append(time.perf_counter() - t0)
        launches, ms = get()
        kernel.append(ms)
    eng.profile_reset(False)
    return float(np.median(wall)), float(np.median(kernel)), launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--molecules", type=int, default=4096)
    a = ap.parse_args()
    from gaudi_amd._lib import host_ring_currents
    from gaudi_amd.engine import Engine
    from gaudi_amd.huckel import c_huckel_tables
    from tests import ppp_helpers as pp
    from tests.ring_current_helpers import acene
    tab = c_huckel_tables("hetro")
    g30 = pp.g30_molecules()
    solved = host_ring_currents(tab, *pp.pack(g30), None)["status"] == 0
    good = [m for m, ok in zip(g30, solved) if ok]
    rng = np.random.default_rng(0)
    eng = Engine(0)
    B = a.molecules
    for name, mols in (("acene46", [acene(11)] * B), ("g30_mix", [good[k] for k in rng.integers(0, len(good), B)])):
        elem, na, bonds, nb, xyz = pp.pack(mols)
        out = eng.ring_currents(tab, elem, na, bonds, nb, xyz)
        w, k, launches = timed(eng, lambda: eng.ring_currents(tab, elem, na, bonds, nb, xyz), eng.ring_currents_profile_get, a.calls)
        hw, hk, _ = timed(eng, lambda: eng.huckel(tab, elem, na, bonds, nb), eng.huckel_profile_get, a.calls)
        n = out["n_pi"].astype(np.int64)
        print(json.dumps(dict(metric="ring_current_molecules_per_s", workload=name, molecules=B, launches_per_call=launches,
                              mean_pi_centres=round(float(n.mean()), 1), max_pi_centres=int(n.max()),
                              mean_rings=round(float(out["n_rings"].mean()), 2), mean_sweeps=round(float(out["sweeps"].mean()), 2),
                              statuses=np.bincount(out["status"], minlength=10).tolist(), kernel_median_ms=round(k, 4),
                              kernel_molecules_per_s=round(B / (k / 1e3), 1) if k > 0 else None, call_median_s=round(w, 5),
                              call_molecules_per_s=round(B / w, 1), huckel_kernel_median_ms=round(hk, 4),
                              kernel_ms_over_huckel=round(k / hk, 3) if hk > 0 else None, huckel_call_median_s=round(hw, 5),
                              output_bytes=int(sum(v.nbytes for v in out.values())))), flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, VALU utilisation, occupancy achieved): no counter pass in this run",
                                        "the 128-centre tier alone", "batches other than 4 096"])))
    eng.close()


if __name__ == "__main__":
    main()
