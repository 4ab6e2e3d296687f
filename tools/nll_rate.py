#!/usr/bin/env python3
"""Molecules per second of GaudiModel.__call__ (the EDM's eval-mode NLL: both network passes in one launch) at B = 1024 cata
molecules of 11 rings, default widths.  One warm-up call, then --calls timed calls (each synchronises: the result is on the host).

    python tools/nll_rate.py [--batch 1024] [--calls 5]
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from gaudi_amd import synth
    from gaudi_amd.engine import Engine
    from gaudi_amd.models_edm import GaudiModel
    from gaudi_amd.sampling_edm import build_masks
    B = a.batch
    args = synth.edm_args(dataset="cata")
    eng = Engine(0)
    eng.load_edm(args, synth.synth_edm_state_dict(args, 1, seed=0))
    model = GaudiModel.from_engine(eng, args)
    nm3, em, N = build_masks(np.full(B, 11), 11, False)
    nm = nm3.reshape(B, N, 1)
    x = np.random.default_rng(0).standard_normal((B, N, 3)).astype(np.float32) * nm
    x = (x - x.sum(1, keepdims=True) / np.maximum(nm.sum(1, keepdims=True), 1) * nm).astype(np.float32)
    h = {"categorical": torch.from_numpy(nm.copy()), "integer": torch.zeros(0)}
    xt, nmt, emt = torch.from_numpy(x), torch.from_numpy(nm), torch.from_numpy(em.reshape(B, N * N))
    torch.manual_seed(0)
    model(xt, h, nmt, emt)  # warm-up (kernel attributes, workspaces)
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        nll = model(xt, h, nmt, emt)
        times.append(time.perf_counter() - t0)
    best, med = min(times), float(np.median(times))
    print(json.dumps(dict(metric="nll_molecules_per_s", batch=B, calls=a.calls, median_s=round(med, 5), best_s=round(best, 5),
                          molecules_per_s=round(B / med, 1), mean_nll=float(nll.mean()))))
    eng.close()


if __name__ == "__main__":
    main()
