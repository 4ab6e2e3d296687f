#!/usr/bin/env python3
"""Rates of gaudi_substructure_search (csrc/sub.inc): (molecule, pattern) pairs per second for 1 024 and 16 384 molecules drawn
from the g32 fixture (the well-formed ones, with a fixed seed) against 1, 8 and 64 patterns (the named patterns of
tests/substructure_helpers.py, cycled), no flags.  Per figure: the kernel alone from the profile counters (HIP events) and the
whole call as a user of Engine.substructure_search sees it (packed arrays in, five arrays out: uploads, the launch, downloads),
each the median of --calls calls after one warm-up call; and the candidate tests per second the kernel made, which is what its
time follows.  For context only, networkx's subgraph monomorphisms on a 64th of the batch, scaled, for 1 and 8 patterns.  The
numbers go into DESIGN.md section 8k; there is no threshold, and no figure of an earlier revision to compare with.  No hardware
counter pass is made here: the line "not_measured" says what this run leaves open.  A counter pass is a run of its own with
nothing else traced, on one setting:

    python tools/substructure_rate.py [--calls 5] [--no-networkx]
    rocprofv3 --pmc SQ_WAVE_CYCLES SQ_INSTS_LDS ... -d DIR -- python tools/substructure_rate.py --only 16384 8 --calls 1 --no-networkx
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-networkx", action="store_true")
    ap.add_argument("--only", type=int, nargs=2, metavar=("B", "P"), help="one setting only: what a counter pass of its own runs")
    a = ap.parse_args()
    from gaudi_amd.engine import Engine
    from tests.bond_order_helpers import C, H, fixture, pack
    from tests.canonical_helpers import N_ELEMS
    from tests.substructure_helpers import NAMES, named_patterns, networkx_oracle, pack_patterns
    good = [m for m in fixture()[1] if m["special"] not in (5, 6, 7)]
    rng = np.random.default_rng(0)
    eng = Engine(0)
    base = named_patterns()
    for B in (1024, 16384) if a.only is None else (a.only[0],):
        mols = [good[k] for k in rng.integers(0, len(good), B)]
        packed = pack(mols)
        heavy = float(np.mean([(m["elem"] != H).sum() for m in mols]))
        for P in (1, 8, 64) if a.only is None else (a.only[1],):
            pats = [base[(k + 2) % len(base)] for k in range(P)]  # P = 1: benzene
            pp = pack_patterns(pats, 0)
            run = lambda: eng.substructure_search(N_ELEMS, H, C, *packed, *pp)  # noqa: E731
            out = run()  # warm-up (workspaces)
            wall, kernel = [], []
            for _ in range(a.calls):
                eng.profile_reset(True)
                t0 = time.perf_counter()
                run()
                wall.append(time.perf_counter() - t0)
                n, ms = eng.substructure_profile_get()
                assert n == 1
                kernel.append(ms)
            eng.profile_reset(False)
            w, k = float(np.median(wall)), float(np.median(kernel))
            pairs, steps = B * P, int(out["steps"].astype(np.int64).sum())
            line = dict(metric="substructure_pairs_per_s", molecules=B, patterns=P, pattern_names=[NAMES[(j + 2) % len(base)] for j in range(min(P, 8))],
                        mean_heavy_atoms=round(heavy, 1), statuses=np.bincount(out["status"].reshape(-1), minlength=6).tolist(),
                        cells_with_a_hit=int((out["count"] > 0).sum()), embeddings=int(out["count"].astype(np.int64).sum()),
                        candidate_tests=steps, kernel_median_ms=round(k, 4), kernel_pairs_per_s=round(pairs / (k / 1e3), 1) if k > 0 else None,
                        kernel_tests_per_s=round(steps / (k / 1e3), 1) if k > 0 else None, call_median_s=round(w, 5),
                        call_pairs_per_s=round(pairs / w, 1), output_bytes=int(sum(v.nbytes for v in out.values())))
            if not a.no_networkx and P <= 8:
                part = mols[:max(1, B // 64)]
                t0 = time.perf_counter()
                for m in part:
                    for pat in pats:
                        networkx_oracle((m["elem"], m["bonds"]), pat, 0)
                host = (time.perf_counter() - t0) * (B / len(part))
                line.update(networkx_molecules=len(part), networkx_s_scaled=round(host, 2), networkx_pairs_per_s=round(pairs / host, 1))
            print(json.dumps(line), flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, VALU utilisation, occupancy achieved): no counter pass in this run",
                                        "networkx at 64 patterns", "flag settings other than none", "patterns beyond the named ones"])))
    eng.close()


if __name__ == "__main__":
    main()
