#!/usr/bin/env python3
"""Molecules per second of chains on a time grid at the C3 shape (256 cata molecules of 11 rings, default widths, T = 1000):
unguided and gap-guided chains from the prior with n_steps = 1000 (through gaudi_sample: today's path), 1000 again through
gaudi_sample_grid (the unit grid: what the table walk costs), 500, 250, 100, and guided refinement of given molecules from
t_start = 500 / 250 (every step below t_start).  One warm-up call per row, then --calls timed calls; prints the median time
per call, per step, and the fixed part: time per call minus n_steps x the full chain's per-step time.

    python tools/grid_rate.py [--batch 256] [--calls 3] [--steps 1000 500 250 100]

Synthetic weights: the figures say what a chain COSTS, nothing about the quality of its molecules (stability rate, target
values) as a function of n_steps or t_start.
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--steps", type=int, nargs="*", default=[1000, 500, 250, 100])
    ap.add_argument("--t-start", type=int, nargs="*", default=[500, 250])
    a = ap.parse_args()
    from gaudi_amd import synth
    from gaudi_amd.engine import Engine
    from gaudi_amd.sampling_edm import build_masks, time_grid
    B, T = a.batch, 1000
    eargs, pargs = synth.edm_args(dataset="cata", diffusion_steps=T), synth.pred_args(dataset="cata")
    eng = Engine(0)
    eng.load_edm(eargs, synth.synth_edm_state_dict(eargs, 1, seed=0))
    eng.load_predictor(pargs, synth.synth_predictor_state_dict(pargs, 1, 5, seed=1))
    nm3, em, N = build_masks(np.full(B, 11), 11, False)
    nm, em = nm3.reshape(B, N), em.reshape(B, N, N)
    w = np.zeros(5, np.float32)
    w[1] = -1.0  # max_gap
    rng = np.random.default_rng(0)
    x0 = rng.standard_normal((B, N, 3)).astype(np.float32) * 2.0
    x0 = (x0 - x0.mean(1, keepdims=True)).astype(np.float32)
    oh0 = np.ones((B, N, 1), np.float32)

    def timed(**kw):
        eng.sample(nm, em, seed=1, std=1.0, **kw)  # warm-up
        ts = []
        for it in range(a.calls):
            t0 = time.perf_counter()
            eng.sample(nm, em, seed=2 + it, std=1.0, **kw)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    rows = []
    for guided in (False, True):
        g = dict(target_w=w, scale=0.6) if guided else {}
        full, lo, hi = timed(**g)
        per_step = full / T
        rows.append(dict(chain="guided" if guided else "unguided", entry="gaudi_sample", n_steps=T, s_per_call=full, best_s=lo, worst_s=hi))
        for n in a.steps:
            med, lo, hi = timed(grid=time_grid(T, n), **g)
            rows.append(dict(chain="guided" if guided else "unguided", entry="gaudi_sample_grid", n_steps=n, s_per_call=med, best_s=lo,
                             worst_s=hi, fixed_s=med - n * per_step))
        if guided:
            for t0_ in a.t_start:
                med, lo, hi = timed(grid=time_grid(T, t0_, t0_), start=(x0, oh0), **g)
                rows.append(dict(chain="guided refinement", entry="gaudi_sample_grid", t_start=t0_, n_steps=t0_, s_per_call=med, best_s=lo,
                                 worst_s=hi, fixed_s=med - t0_ * per_step))
    for r in rows:
        r["ms_per_step"] = round(1e3 * r["s_per_call"] / r["n_steps"], 4)
        r["molecules_per_s"] = round(B / r["s_per_call"], 1)
        for k in ("s_per_call", "best_s", "worst_s", "fixed_s"):
            if k in r:
                r[k] = round(r[k], 4)
        print(json.dumps(r))
    eng.close()


if __name__ == "__main__":
    main()
