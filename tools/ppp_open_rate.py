#!/usr/bin/env python3
"""Rates of gaudi_ppp_open (csrc/ppp_open.inc) beside gaudi_ppp's from the same run: rows per second for 4 096 copies of the
46-centre acene (tools/ppp_rate.py's, the 64-centre tier) as a cation, and for 4 096 molecules drawn from the g30 fixture (the
closed-shell ones the reference built, a fixed seed) as neutral, cation and anion -- the batch gaudi_amd.ppp.ionization makes, three
rows per molecule in one call.  gaudi_ppp runs on the same molecules (neutral, closed shell) in the same process.  Per figure: the
kernels alone from the profile counters (HIP events; one launch per tier present), the median of --calls calls after one warm-up
call, the whole call as a user of the Engine sees it, the mean SCF iterations and Jacobi sweeps per row, and the kernel time per
Jacobi sweep -- the number that says whether an open-shell solve costs its sweeps and nothing measurable more.  The numbers go into
DESIGN.md section 8s; there is no threshold.  No hardware counter pass is made here: "not_measured" says what this run leaves open.

    python tools/ppp_open_rate.py [--calls 3] [--molecules 4096]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--molecules", type=int, default=4096)
    a = ap.parse_args()
    from gaudi_amd._lib import host_ppp
    from gaudi_amd.engine import Engine
    from gaudi_amd.ppp import c_ppp_tables
    from tests.ppp_helpers import g30_molecules, pack
    from tools.ppp_rate import acene
    tab = c_ppp_tables("hetro")
    fx = g30_molecules()
    status = host_ppp(tab, *pack(fx))["status"]
    good = [m for m, st in zip(fx, status) if st in (0, 1)]
    rng = np.random.default_rng(0)
    eng = Engine(0)
    B = a.molecules
    mix = [good[k] for k in rng.integers(0, len(good), B)]
    ones = np.ones(B, np.int32)
    jobs = (("acene46_cation", "ppp_open", pack([acene(11)] * B), ones, None),
            ("acene46_neutral", "ppp", pack([acene(11)] * B), None, None),
            ("g30_mix_neutral_cation_anion", "ppp_open", pack(mix * 3), np.concatenate([0 * ones, ones, -ones]), None),
            ("g30_mix_neutral", "ppp", pack(mix), None, None))
    for name, entry, packed, charge, mult in jobs:
        if entry == "ppp_open":
            run, get = (lambda: eng.ppp_open(tab, *packed, charge, mult)), eng.ppp_open_profile_get  # noqa: E731
        else:
            run, get = (lambda: eng.ppp(tab, *packed, charge)), eng.ppp_profile_get  # noqa: E731
        out = run()  # warm-up (workspaces, the LDS attribute)
        wall, kernel, launches = [], [], 0
        for _ in range(a.calls):
            eng.profile_reset(True)
            t0 = time.perf_counter()
            run()
            wall.append(time.perf_counter() - t0)
            launches, ms = get()
            kernel.append(ms)
        eng.profile_reset(False)
        w, k, rows = float(np.median(wall)), float(np.median(kernel)), len(out["status"])
        sweeps = int(out["sweeps"].sum())
        print(json.dumps(dict(metric="ppp_open_rows_per_s", workload=name, entry="gaudi_" + entry, rows=rows, launches_per_call=launches,
                              mean_pi_centres=round(float(out["n_pi"].mean()), 1), max_pi_centres=int(out["n_pi"].max()),
                              mean_iterations=round(float(out["iterations"].mean()), 2), max_iterations=int(out["iterations"].max()),
                              mean_sweeps=round(float(out["sweeps"].mean()), 2),
                              sweeps_per_iteration=round(sweeps / max(1, int(out["iterations"].sum())), 2),
                              statuses=np.bincount(out["status"], minlength=9).tolist(), kernel_median_ms=round(k, 4),
                              kernel_rows_per_s=round(rows / (k / 1e3), 1) if k > 0 else None,
                              kernel_ns_per_sweep=round(k * 1e6 / sweeps, 2) if sweeps else None, call_median_s=round(w, 5),
                              call_rows_per_s=round(rows / w, 1), output_bytes=int(sum(v.nbytes for v in out.values())))), flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, VALU and fp64 utilisation, occupancy achieved): no counter pass in this run",
                                        "the 128-centre tier alone", "triplet rows alone", "batches other than the one given",
                                        "the Ohno formula's rate"])))
    eng.close()


if __name__ == "__main__":
    main()
