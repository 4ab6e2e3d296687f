#!/usr/bin/env python3
"""Rates of gaudi_reactivity (csrc/reactivity.inc): molecules per second and diagonalisations ("solves": a molecule's jobs and its
parent) per second for 4 096 copies of a 46-centre cata molecule (eleven rings in a row: the 64-centre tier, 136 solves each) and
for 4 096 molecules drawn from golden g30 (the ones it solves, with a fixed seed: all three tiers), and for the same acene at 64
molecules per call with one slice per molecule and with the number the entry point chooses.  Per figure: the kernels alone from
the profile counters (HIP events; one launch per tier present) and the whole call as a user of Engine.reactivity sees it (packed
arrays in, thirteen arrays out), each the median of --calls calls after one warm-up call; beside them gaudi_huckel's kernel time
on the same batch in the same run, measured the same way, and the ratio (kernel time per solve of this kernel) / (gaudi_huckel's
kernel time per molecule): a job runs gaudi_huckel's diagonalisation on a system one or two centres smaller.  The numbers go into
DESIGN.md section 8r; there is no threshold and no figure of an earlier revision to compare with.  No hardware counter pass is
made here: the line "not_measured" says what this run leaves open.

    python tools/reactivity_rate.py [--calls 3]
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
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--molecules", type=int, default=4096)
    ap.add_argument("--small", type=int, default=64)
    a = ap.parse_args()
    from gaudi_amd._lib import host_huckel
    from gaudi_amd.engine import Engine
    from gaudi_amd.huckel import c_huckel_tables
    from tests import ppp_helpers as pp
    from tests.bond_order_helpers import pack
    from tests.reactivity_helpers import acene
    tab = c_huckel_tables("hetro")
    g30 = [(m[0], m[1]) for m in pp.g30_molecules()]
    solved = host_huckel(tab, *pack(g30), None)["status"] == 0
    good = [m for m, ok in zip(g30, solved) if ok]
    rng = np.random.default_rng(0)
    eng = Engine(0)
    B = a.molecules
    cases = [("g30_mix", [good[k] for k in rng.integers(0, len(good), B)], 0), ("acene46", [acene(11)] * B, 0),
             ("acene46_small_unsliced", [acene(11)] * a.small, 1), ("acene46_small_chosen", [acene(11)] * a.small, 0)]
    for name, mols, slices in cases:
        elem, na, bonds, nb = pack(mols)
        n_mol = len(mols)
        out = eng.reactivity(tab, elem, na, bonds, nb, slices=slices)
        w, k, launches = timed(eng, lambda: eng.reactivity(tab, elem, na, bonds, nb, slices=slices), eng.reactivity_profile_get, a.calls)
        hw, hk, _ = timed(eng, lambda: eng.huckel(tab, elem, na, bonds, nb), eng.huckel_profile_get, a.calls)
        n = out["n_pi"].astype(np.int64)
        solves = int((out["n_jobs"].astype(np.int64) + (out["status"] == 0)).sum())
        per_solve_ms, huckel_per_mol_ms = k / solves, hk / n_mol
        print(json.dumps(dict(metric="reactivity_rate", workload=name, molecules=n_mol, slices_argument=slices, launches_per_call=launches,
                              mean_pi_centres=round(float(n.mean()), 1), max_pi_centres=int(n.max()), solves=solves,
                              mean_solves_per_molecule=round(solves / n_mol, 1), sweeps=int(out["sweeps"].sum()),
                              statuses=np.bincount(out["status"], minlength=7).tolist(), kernel_median_ms=round(k, 4),
                              kernel_molecules_per_s=round(n_mol / (k / 1e3), 1) if k > 0 else None,
                              kernel_solves_per_s=round(solves / (k / 1e3), 1) if k > 0 else None, call_median_s=round(w, 5),
                              call_molecules_per_s=round(n_mol / w, 1), call_solves_per_s=round(solves / w, 1),
                              huckel_kernel_median_ms=round(hk, 4), huckel_call_median_s=round(hw, 5),
                              kernel_ms_per_solve_over_huckel_ms_per_molecule=round(per_solve_ms / huckel_per_mol_ms, 3) if hk > 0 else None,
                              output_bytes=int(sum(v.nbytes for v in out.values())))), flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, VALU utilisation, occupancy achieved): no counter pass in this run",
                                        "the 128-centre tier alone", "batches other than 4 096 and 64", "slices other than 1 and the chosen number"])))
    eng.close()


if __name__ == "__main__":
    main()
