#!/usr/bin/env python3
"""sha256 of what every entry point that drives a reverse chain returns, one line per case: the bit-for-bit record a change to
the host code of the chain drivers (csrc/chain_host.inc) is checked with.  Run it on the library before the change and on the
library after it (GAUDI_LIB names the library, gaudi_amd/_lib.py) and compare the two listings: they must be identical.

    GAUDI_LIB=/path/to/libgaudi_hip.so python tools/chain_digest.py

Synthetic weights at the smallest widths the tiny kernels take (nf = 32, 2 layers; predictor nf = 36, 3 layers), T = 12, five
cata molecules of 3 to 6 rings padded to N = 6: masks, padding and unequal graphs all matter, and a case takes well under a
second.  The cases: gaudi_sample (unguided, guided, host noise, fix_noise, launches of 5 steps), gaudi_sample_grid (from the
prior on an uneven grid; from given molecules with z_t), gaudi_sample_target (a window narrower than the chain with a trace,
again with launches cut at its edges), the single steps and gaudi_decode, gaudi_sample_chain, and the three callback chains.
The guided and callback cases again under GAUDI_WAVES=4 and GAUDI_FORCE_GN=1 (two launches per guided step), one guided
request cut into sub-batches by GAUDI_MAX_WORKSPACE_MB=1, and one GAUDI_FAMILY_SPLIT=1 request of two buckets.  The knobs are
read once, by gaudi_create: every group runs in a fresh child process.
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 12
SIZES = [3, 6, 4, 5, 6]
GROUPS = {  # name -> (environment, which cases)
    "default": ({}, "all"),
    "waves4": (dict(GAUDI_WAVES="4"), "guided"),
    "force_gn": (dict(GAUDI_FORCE_GN="1"), "guided"),
    "workspace_1mb": (dict(GAUDI_MAX_WORKSPACE_MB="1"), "cut"),
    "family_split": (dict(GAUDI_FAMILY_SPLIT="1"), "split"),
}


def digest(out) -> str:
    """sha256 over every array of a call's result, in order (dtype, shape and bytes), and its NaN count."""
    import numpy as np
    h = hashlib.sha256()
    for a in out if isinstance(out, tuple) else (out,):
        if isinstance(a, dict):
            h.update(b"nan_count=%d;reprojected=%d;" % (a["nan_count"], a["reprojected"]))
            continue
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype}{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def tiny_engine(dataset="cata", widths=True, t=T, eseed=31, pseed=32):
    from gaudi_amd import synth
    from gaudi_amd.engine import Engine
    F = synth.num_node_features(dataset)
    over_e, over_p = (dict(nf=32, n_layers=2), dict(nf=36, n_layers=3)) if widths else ({}, {})
    eargs = synth.edm_args(dataset=dataset, diffusion_steps=t, **over_e)
    pargs = synth.pred_args(dataset=dataset, **over_p)
    eng = Engine(0)
    eng.load_edm(eargs, synth.synth_edm_state_dict(eargs, F, seed=eseed, amplify_coord=True))
    eng.load_predictor(pargs, synth.synth_predictor_state_dict(pargs, F, 5, seed=pseed, amplify_coord=True))
    return eng, F


def given_molecules(nm, F, seed):
    """Masked, mean-free coordinates and one ring type per live node."""
    import numpy as np
    B, N = nm.shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, N, 3)).astype(np.float32) * 2.0 * nm[:, :, None]
    x = (x - x.sum(1, keepdims=True) / np.maximum(nm.sum(1), 1)[:, None, None] * nm[:, :, None]).astype(np.float32)
    oh = np.zeros((B, N, F), np.float32)
    np.put_along_axis(oh, rng.integers(0, F, (B, N, 1)), 1.0, axis=2)
    return x, oh * nm[:, :, None]


def nonlinear_target_grad(pred, t):
    """dT/dpred of T = 0.5 * log(1 + p1^2) + 0.1 * tanh(p0) * p3 + t * p2: a target no target_w expresses."""
    import numpy as np
    th = np.tanh(pred[:, 0])
    g = np.zeros_like(pred)
    g[:, 0] = 0.1 * (1.0 - th * th) * pred[:, 3]
    g[:, 1] = pred[:, 1] / (1.0 + pred[:, 1] ** 2)
    g[:, 2] = pred.dtype.type(t)
    g[:, 3] = 0.1 * th
    return g


def direct_z_target_grad(nm):
    """(z_s, pred, t) -> (dT/dpred, direct dT/dz) of T = -pred[:, 1] + 0.05 * sum_live |x_n|^2 + 0.02 * sum_live z[:, :, 3]."""
    import numpy as np

    def grad(z, pred, t):
        gp = np.zeros_like(pred)
        gp[:, 1] = -1.0
        gz = np.zeros_like(z)
        gz[:, :, :3] = 0.1 * z[:, :, :3] * nm[:, :, None]
        gz[:, :, 3] = 0.02 * nm
        return gp, gz

    return grad


def run_group(group: str):
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from gaudi_amd.sampling_edm import build_masks

    which = GROUPS[group][1]

    def show(name, out):
        print(f"{group}/{name} {digest(out)}", flush=True)

    if which == "split":  # the shape of tests/test_gpu_grid.py::test_family_split_buckets_on_a_grid_from_given_molecules
        eng, F = tiny_engine("hetro", widths=False, t=8, eseed=21, pseed=22)
        rings = [3, 20, 6, 12]
        nm3, em, N = build_masks(rings, 20, True)
        nm, em = nm3.reshape(len(rings), N), em.reshape(len(rings), N, N)
        x0, oh0 = given_molecules(nm, F, 2)
        grid = np.array([6, 4, 1, 0], np.int32)
        w = np.array([3, 0, 1, 1, 0], np.float32)
        for name, kw in (("guided", dict(target_w=w, scale=0.6)), ("unguided", {})):
            out = eng.sample(nm, em, seed=5, grid=grid, start=(x0, oh0), return_z0=True, return_zt=True, **kw)
            print(f"# {group}/{name}: {out[2]['family_split_resident']} of {len(rings)} molecules on the resident kernels", flush=True)
            show(name, out)
        eng.close()
        return

    eng, F = tiny_engine()
    D = 3 + F
    w = np.array([0.5, -1.0, 0.25, 0.0, 1.0], np.float32)
    if which == "cut":
        B = 128
        nm3, em, N = build_masks([SIZES[b % len(SIZES)] for b in range(B)], max(SIZES), False)
        nm, em = nm3.reshape(B, N), em.reshape(B, N, N)
        eng.profile_reset(True)  # (T = 12 steps fit one launch: a launch per sub-batch)
        out = eng.sample(nm, em, seed=7, sample_offset=3, target_w=w, scale=0.6, return_z0=True)
        launches = eng.profile_get()[0]
        eng.profile_reset(False)
        print(f"# {group}/sample_guided: B = {B}, cut into {launches} sub-batches", flush=True)
        if launches < 2:
            raise SystemExit("the request was not cut: raise B")
        show("sample_guided", out)
        eng.close()
        return

    B = len(SIZES)
    nm3, em, N = build_masks(SIZES, max(SIZES), False)
    nm, em = nm3.reshape(B, N), em.reshape(B, N, N)
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((T + 2, B, N, D)).astype(np.float32)
    x0, oh0 = given_molecules(nm, F, 2)
    z = (rng.standard_normal((B, N, D)).astype(np.float32) * nm[:, :, None])
    z[:, :, :3] -= z[:, :, :3].sum(1, keepdims=True) / nm.sum(1)[:, None, None] * nm[:, :, None]
    eps = rng.standard_normal((B, N, D)).astype(np.float32)
    g = dict(target_w=w, scale=0.6)
    uneven = np.array([12, 9, 8, 3, 0], np.int32)
    short = np.array([7, 4, 1, 0], np.int32)
    spec = dict(w=np.array([0.0, -1.0, 0.5, 0.0, 0.0], np.float32), q=np.array([0.1, 0.0, 0.0, 0.2, 0.0], np.float32),
                c=np.array([0.0, 0.3, 0.0, -0.5, 0.0], np.float32), side=np.array([0, 0, 1, -1, 0], np.int32),
                scale=np.linspace(0.3, 0.9, B).astype(np.float32), window=(3, 9))
    everything = which == "all"

    if everything:
        show("sample_unguided", eng.sample(nm, em, seed=7, sample_offset=3, return_z0=True))
    show("sample_guided", eng.sample(nm, em, seed=7, sample_offset=3, return_z0=True, **g))
    if everything:
        show("sample_host_noise", eng.sample(nm, em, noise=noise, return_z0=True, **g))
        eng.set_steps_per_launch(5)
        show("sample_guided_5_steps_per_launch", eng.sample(nm, em, seed=7, sample_offset=3, return_z0=True, **g))
        eng.set_steps_per_launch(25)
        eng.set_fix_noise(True, 11)
        show("sample_fix_noise", eng.sample(nm, em, seed=7, return_z0=True, **g))
        show("sample_fix_noise_host_noise", eng.sample(nm, em, noise=noise[:, :1], return_z0=True))
        eng.set_fix_noise(False)
    show("grid_from_prior", eng.sample(nm, em, seed=8, grid=uneven, return_z0=True, **g))
    show("grid_from_given_zt", eng.sample(nm, em, seed=9, sample_offset=2, grid=short, start=(x0, oh0), return_z0=True, return_zt=True, **g))
    if everything:
        show("grid_from_given_zt_unguided", eng.sample(nm, em, seed=9, grid=short, start=(x0, oh0), return_z0=True, return_zt=True))
    show("target_window_trace", eng.sample_target(nm, em, spec, seed=10, sample_offset=1, return_z0=True, trace=True))
    eng.set_steps_per_launch(4)  # (the window holds 7 steps: launches are cut at its edges and inside it)
    show("target_window_trace_4_steps_per_launch", eng.sample_target(nm, em, spec, seed=10, sample_offset=1, return_z0=True, trace=True))
    eng.set_steps_per_launch(25)
    show("target_on_grid_from_given", eng.sample_target(nm, em, spec, seed=10, grid=uneven[1:], start=(x0, oh0), return_z0=True,
                                                        return_zt=True, trace=True))
    if everything:
        show("step", eng.step(4, z, nm, em, eps))
    show("step_guided", eng.step(4, z, nm, em, eps, **g))
    show("step_pair_guided", eng.step(2, z, nm, em, eps, t_idx=7, **g))
    show("step_target", eng.step_target(2, z, nm, em, eps, spec, t_idx=7, trace=True))
    if everything:
        show("decode", eng.decode(z, nm, em, eps))
        show("sample_chain", eng.sample_chain(nm, em, 3, seed=12, sample_offset=4))
        show("sample_chain_host_noise", eng.sample_chain(nm, em, 3, noise=noise))
    show("sample_cb", eng.sample_callback(nm, em, nonlinear_target_grad, seed=13, sample_offset=2, scale=0.6, return_z0=True))
    show("sample_cbz", eng.sample_callback(nm, em, direct_z_target_grad(nm), seed=13, scale=0.6, return_z0=True, with_z=True))
    show("sample_cb_host_noise", eng.sample_callback(nm, em, nonlinear_target_grad, noise=noise, scale=0.6, return_z0=True))
    show("sample_cb_grid_from_given", eng.sample_callback(nm, em, nonlinear_target_grad, seed=14, scale=0.6, grid=short, start=(x0, oh0),
                                                          return_z0=True, return_zt=True))
    show("sample_cbz_grid_from_prior", eng.sample_callback(nm, em, direct_z_target_grad(nm), seed=14, scale=0.6, grid=uneven,
                                                           return_z0=True, with_z=True))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=sorted(GROUPS), help="run one group in THIS process (what the parent starts per group)")
    a = ap.parse_args()
    if a.group:
        run_group(a.group)
        return
    for group, (env, _) in GROUPS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", group], env=dict(os.environ, **env), timeout=240)
        if r.returncode != 0:  # a fault or a refusal: start nothing more on the device
            raise SystemExit(f"group {group} ended with status {r.returncode}")


if __name__ == "__main__":
    main()
