#!/usr/bin/env python3
"""Molecules per second of the fused value-target family at the C3 shape (256 cata molecules of 11 rings, default widths,
T = 1000).  One warm-up call per row, then --calls timed calls, median per call:

  affine            gaudi_sample(target_w = max_gap, scale 0.6): the headline path (packed / wide launches allowed)
  affine_solo       the same through gaudi_sample_target (q = 0): one molecule per workgroup, what giving up shared workgroups costs
  value_fused       per-molecule value target (centres, one-sided terms, per-molecule scales) through gaudi_sample_target
  value_callback    the SAME target through gaudi_sample_cb (numpy gradient on the host, two launches per step)
  value_traced      value_fused with the guidance trace
  window_40         value_fused guided on 40 % of the chain (time indices 1..400) against the full chain
  sweep_one_call    8 scales x 128 molecules as ONE call of 1 024 molecules (generation_guidance.design_sweep's sampling call)
  sweep_eight_calls the same sweep as eight calls of 128 molecules

    python tools/target_rate.py [--batch 256] [--calls 3] [--T 1000]

Synthetic weights: the figures say what a chain COSTS, nothing about the quality of its molecules.
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
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--rows", nargs="*", default=None, help="only these rows")
    a = ap.parse_args()
    from gaudi_amd import synth
    from gaudi_amd.engine import Engine, host_target_seed
    from gaudi_amd.sampling_edm import build_masks
    B, T, K = a.batch, a.T, 5
    eargs, pargs = synth.edm_args(dataset="cata", diffusion_steps=T), synth.pred_args(dataset="cata")
    eng = Engine(0)
    eng.load_edm(eargs, synth.synth_edm_state_dict(eargs, 1, seed=0))
    eng.load_predictor(pargs, synth.synth_predictor_state_dict(pargs, 1, K, seed=1))

    def masks(n):
        nm3, em, N = build_masks(np.full(n, 11), 11, False)
        return nm3.reshape(n, N), em.reshape(n, N, N)

    nm, em = masks(B)
    w = np.zeros(K, np.float32)
    w[1] = -1.0  # max_gap
    rng = np.random.default_rng(0)

    def value_spec(n, scale=None):
        side = np.tile(np.array([0, 1, -1, 0, 1], np.int32), (n, 1))
        return dict(w=np.broadcast_to(w, (n, K)).copy(), q=rng.uniform(0.2, 1.5, (n, K)).astype(np.float32),
                    c=(0.5 * rng.standard_normal((n, K))).astype(np.float32), side=side,
                    scale=rng.uniform(0.2, 1.0, n).astype(np.float32) if scale is None else scale)

    spec = value_spec(B)

    def timed(fn):
        fn(1)  # warm-up
        ts = []
        for it in range(a.calls):
            t0 = time.perf_counter()
            fn(2 + it)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    scales = np.array([0.1, 0.2, 0.4, 0.6, 0.8, 1.0, 1.5, 2.0], np.float32)
    nm8, em8 = masks(128 * len(scales))
    nm1, em1 = masks(128)
    sweep = value_spec(128 * len(scales), np.repeat(scales, 128))
    part = [{k: v[128 * j:128 * (j + 1)] for k, v in sweep.items()} for j in range(len(scales))]

    def eight_calls(seed):
        for j in range(len(scales)):
            eng.sample_target(nm1, em1, part[j], seed=seed, sample_offset=128 * j)

    rows = dict(
        affine=(B, lambda s: eng.sample(nm, em, seed=s, target_w=w, scale=0.6)),
        affine_solo=(B, lambda s: eng.sample_target(nm, em, dict(w=w, scale=0.6), seed=s)),
        value_fused=(B, lambda s: eng.sample_target(nm, em, spec, seed=s)),
        value_callback=(B, lambda s: eng.sample_callback(nm, em, lambda p, t: host_target_seed(spec, p), seed=s, scale=1.0)),
        value_traced=(B, lambda s: eng.sample_target(nm, em, spec, seed=s, trace=True)),
        window_40=(B, lambda s: eng.sample_target(nm, em, dict(spec, window=(1, (4 * T) // 10)), seed=s)),
        sweep_one_call=(128 * len(scales), lambda s: eng.sample_target(nm8, em8, sweep, seed=s)),
        sweep_eight_calls=(128 * len(scales), eight_calls),
    )
    for name, (n, fn) in rows.items():
        if a.rows and name not in a.rows:
            continue
        med, lo, hi = timed(fn)
        print(json.dumps(dict(row=name, molecules=n, T=T, s_per_call=round(med, 4), best_s=round(lo, 4), worst_s=round(hi, 4),
                              ms_per_step=round(1e3 * med / T, 4), molecules_per_s=round(n / med, 1),
                              workgroups_x_slots=list(eng.last_launch_shape()))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
