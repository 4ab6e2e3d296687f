#!/usr/bin/env python3
"""Predictor training rate at B = 256 cata molecules of 11 rings, the reference defaults (nf 196, 12 layers, K 5):
the gradient call (Engine.predictor_loss_grad), a predict_noised call of the same batch, and a whole train_epoch step
(compute_loss in train mode, zero_grad, backward, AdamW(amsgrad) step, and the reload of the changed weights), with the
share of the step spent reloading (host repacking + upload).  One warm-up, then --calls timed repetitions of each.
Run under `rocprofv3 --kernel-trace --stats -- python tools/pred_train_rate.py` for the kernel split.

    python tools/pred_train_rate.py [--batch 256] [--calls 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime per process)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from gaudi_amd import cond_prediction as cp
    from gaudi_amd import synth
    from gaudi_amd.models_edm import get_cond_predictor_model, get_model
    from gaudi_amd.sampling_edm import build_masks
    B = a.batch
    eargs = synth.edm_args(dataset="cata")
    model, _, _ = get_model(eargs, state_dict=synth.synth_edm_state_dict(eargs, 1, seed=0))
    pargs = synth.pred_args(dataset="cata")
    psd = synth.synth_predictor_state_dict(pargs, 1, 5, seed=1)
    pred = get_cond_predictor_model(pargs, model=model, state_dict=psd)
    model.seed, model.sample_offset = 3, 0
    nm3, em, N = build_masks(np.full(B, 11), 11, False)
    nm = nm3.reshape(B, N)
    em = em.reshape(B, N, N)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((B, N, 3)).astype(np.float32) * nm[..., None]
    x = (x - x.sum(1, keepdims=True) / N * nm[..., None]).astype(np.float32)
    h = nm[..., None].copy()
    y = rng.standard_normal((B, 5)).astype(np.float32)
    ti = rng.integers(0, model.T + 1, B).astype(np.int32)
    eng = model.engine

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    t_grad = timed(lambda: eng.predictor_loss_grad(x, h, ti, nm, em, y, seed=3, sample_offset=0))
    t_fwd = timed(lambda: eng.predict_noised(x, h, ti, nm, em, seed=3, sample_offset=0))
    sd = {k: v.copy() for k, v in psd.items()}
    t_reload = timed(lambda: eng.load_predictor(pargs, sd))
    opt = torch.optim.AdamW(pred.parameters(), lr=6e-4, amsgrad=True, weight_decay=1e-12)

    class DS:
        std = np.ones(5, np.float32)

    class Loader(list):
        dataset = DS()

    loader = Loader([(x, nm, em.reshape(B, N * N), h, y)])
    torch.manual_seed(0)
    t_step = timed(lambda: cp.train_epoch(0, pred, model, loader, opt, None, None, None))
    print(json.dumps(dict(metric="pred_train_rate", batch=B, n_nodes=N, nf=196, n_layers=12, calls=a.calls,
                          grad_call_s=round(t_grad, 5), grad_molecules_per_s=round(B / t_grad, 1),
                          predict_noised_s=round(t_fwd, 5), reload_s=round(t_reload, 5), train_step_s=round(t_step, 5),
                          reload_share_of_step=round(t_reload / t_step, 3))))
    eng.close()


if __name__ == "__main__":
    main()
