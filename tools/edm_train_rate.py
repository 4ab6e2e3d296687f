#!/usr/bin/env python3
"""EDM training rate at B = 256 cata molecules of 11 rings, the reference defaults (nf 192, 9 layers): the gradient call
(Engine.edm_loss_grad), the forward-only call of the same batch, and the weight refresh after an optimizer step
(Engine.edm_set_train_weights: the torch-layout copy and its transposes, no repack of the sampler images), and a whole
train_epoch step through GaudiModel (compute_loss in train mode, zero_grad, backward, gradient_clipping, AdamW(amsgrad) step,
and the push of the changed weights), with the share of the step spent pushing.  One warm-up, then --calls timed repetitions
of each.  Run under `rocprofv3 --kernel-trace --stats -- python tools/edm_train_rate.py` for the
kernel split.

    python tools/edm_train_rate.py [--batch 256] [--calls 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from gaudi_amd import synth
    from gaudi_amd.engine import Engine
    from gaudi_amd.sampling_edm import build_masks
    B = a.batch
    eargs = synth.edm_args(dataset="cata")
    sd = synth.synth_edm_state_dict(eargs, 1, seed=0)
    eng = Engine(0)
    eng.load_edm(eargs, sd)
    nm3, em, N = build_masks(np.full(B, 11), 11, False)
    nm = nm3.reshape(B, N)
    em = em.reshape(B, N, N)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((B, N, 3)).astype(np.float32) * nm[:, :, None]
    x -= x.sum(1, keepdims=True) / nm.sum(1)[:, None, None] * nm[:, :, None]
    h = nm[:, :, None].astype(np.float32)
    t = rng.integers(0, int(eargs["diffusion_steps"]) + 1, B)

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    grad_s = timed(lambda: eng.edm_loss_grad(x, h, t, nm, em, seed=1, sample_offset=0))
    fwd_s = timed(lambda: eng.edm_loss_grad(x, h, t, nm, em, seed=1, sample_offset=0, grad=False))
    sd2 = {k: v + np.float32(1e-6) for k, v in sd.items()}
    set_s = timed(lambda: eng.edm_set_train_weights(sd2))
    eng.close()

    import torch
    from gaudi_amd import train_edm
    from gaudi_amd.models_edm import get_model
    model = get_model(eargs, state_dict=sd)[0]
    model.seed = 1
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, amsgrad=True, weight_decay=1e-12)
    q = train_edm.Queue(max_len=50)
    q.add(3000)
    tx, th, tnm, tem = (torch.from_numpy(v) for v in (x, h, nm[:, :, None].copy(), em))
    push = []

    def step():
        loss = train_edm.compute_loss(model, tx, th, tnm, tem)
        opt.zero_grad()
        loss.backward()
        train_edm.gradient_clipping(model, q)
        opt.step()
        t0 = time.perf_counter()
        model._sync()  # (what the next EDM call would do first)
        push.append(time.perf_counter() - t0)

    step_s = timed(step)
    push_s = float(np.median(push[1:]))
    model.engine.close()
    print(json.dumps(dict(batch=B, nodes=N, grad_call_ms=grad_s * 1e3, molecules_per_s=B / grad_s,
                          forward_only_ms=fwd_s * 1e3, set_train_weights_ms=set_s * 1e3, train_step_ms=step_s * 1e3,
                          weight_push_in_step_ms=push_s * 1e3, weight_push_share_of_step=push_s / step_s)))


if __name__ == "__main__":
    main()
