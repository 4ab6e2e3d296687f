#!/usr/bin/env python3
"""Rates of gaudi_ppp_scf (csrc/ppp_scf.inc, Pulay's DIIS) beside gaudi_ppp_open's in the same process: 4 096 copies of the
46-centre acene (tools/ppp_rate.py's, the 64-centre tier) as a cation, and 4 096 molecules drawn from the g30 fixture (the
closed-shell ones the reference built, a fixed seed) as neutral, cation and anion -- the batch gaudi_amd.ppp.ionization makes.  Per
figure: the kernels alone from the profile counters (HIP events), the median of --calls calls after one warm-up call, the whole call
as a user of the Engine sees it, the mean SCF iterations and Jacobi sweeps per row, the kernel time per Jacobi sweep and per
iteration, and the rows each entry point leaves NOT_CONVERGED.  The last line says what the extra work of DIIS (the n^3 commutator,
the ring in global memory, the B matrix and the elimination) costs per iteration: the kernel time per iteration of gaudi_ppp_scf less
its sweeps at gaudi_ppp_open's time per sweep.  The numbers go into DESIGN.md section 8t; there is no threshold.  No hardware
counter pass is made here: "not_measured" says what this run leaves open.

    python tools/ppp_scf_rate.py [--calls 3] [--molecules 4096]
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
    workloads = (("acene46_cation", pack([acene(11)] * B), ones), ("g30_mix_neutral_cation_anion", pack(mix * 3), np.concatenate([0 * ones, ones, -ones])))
    seen = {}
    for name, packed, charge in workloads:
        for entry in ("ppp_open", "ppp_scf"):
            if entry == "ppp_open":
                run, get = (lambda: eng.ppp_open(tab, *packed, charge, None)), eng.ppp_open_profile_get  # noqa: E731
            else:
                run, get = (lambda: eng.ppp_scf(tab, *packed, charge, None)), eng.ppp_scf_profile_get  # noqa: E731
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
            sweeps, iterations = int(out["sweeps"].sum()), int(out["iterations"].sum())
            seen[name, entry] = dict(ns_per_sweep=k * 1e6 / sweeps, ns_per_iteration=k * 1e6 / iterations, sweeps_per_iteration=sweeps / iterations)
            rec = dict(metric="ppp_scf_rows_per_s", workload=name, entry="gaudi_" + entry, rows=rows, launches_per_call=launches,
                       mean_pi_centres=round(float(out["n_pi"].mean()), 1), max_pi_centres=int(out["n_pi"].max()),
                       mean_iterations=round(float(out["iterations"].mean()), 2), max_iterations=int(out["iterations"].max()),
                       mean_sweeps=round(float(out["sweeps"].mean()), 2), sweeps_per_iteration=round(sweeps / max(1, iterations), 2),
                       statuses=np.bincount(out["status"], minlength=9).tolist(), not_converged=int((out["status"] == 1).sum()),
                       kernel_median_ms=round(k, 4), kernel_rows_per_s=round(rows / (k / 1e3), 1) if k > 0 else None,
                       kernel_ns_per_sweep=round(k * 1e6 / sweeps, 2) if sweeps else None,
                       kernel_ns_per_iteration=round(k * 1e6 / iterations, 1) if iterations else None, call_median_s=round(w, 5),
                       call_rows_per_s=round(rows / w, 1))
            if entry == "ppp_scf":
                rec.update(mean_extrapolated=round(float(out["n_extrapolated"].mean()), 2), max_diis_error_ok=float(out["diis_error"][out["status"] == 0].max()))
            print(json.dumps(rec), flush=True)
        o, s = seen[name, "ppp_open"], seen[name, "ppp_scf"]
        print(json.dumps(dict(metric="ppp_scf_extra_ns_per_iteration", workload=name,
                              value=round(s["ns_per_iteration"] - s["sweeps_per_iteration"] * o["ns_per_sweep"], 1),
                              of_iteration=round(1.0 - s["sweeps_per_iteration"] * o["ns_per_sweep"] / s["ns_per_iteration"], 3),
                              note="kernel time per DIIS iteration less its sweeps at gaudi_ppp_open's time per sweep (which holds that entry's own Fock build and density)")),
              flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, VALU and fp64 utilisation, occupancy achieved): no counter pass in this run",
                                        "the 128-centre tier alone", "triplet rows alone", "histories other than 6", "batches other than the one given",
                                        "the Ohno formula's rate"])))
    eng.close()


if __name__ == "__main__":
    main()
