"""Helpers of the time-grid tests (test_grid_cpu.py, test_gpu_grid.py): the tolerance rule for comparisons with the g28
fixtures, and the numpy composition of one reverse step for ANY pair s < t from the oracle's pieces."""
import os

import numpy as np

from tests.helpers import max_norm_err, rel_err

SPREAD_BAR = 5e-5


def g28_error(got, ref, spread):
    """-> (error, bound) under the rule for every comparison with g28: the suite's own metric and bar, rel_err < 1e-4, where
    the fixture's fp32-vs-float64 spread of that output is below 5e-5; otherwise twice that spread in max_norm_err (the rule
    of test_gpu_parity.py: test_tiny_chains_*).  The spread is the reference's own, read from the fixture."""
    spread = float(spread)
    if spread < SPREAD_BAR:
        return rel_err(got, ref), 1e-4
    return max_norm_err(got, ref), 2.0 * spread


def assert_g28(got, ref, spread, what):
    err, bound = g28_error(got, ref, spread)
    print(f"{what}: err {err:.3e} (bound {bound:.1e}, reference spread {float(spread):.2e})")
    assert err < bound, (what, err, bound)


def engine(eargs, esd, pargs=None, psd=None, **env):
    """An Engine created under the given environment knobs (they are read once, by gaudi_create)."""
    from gaudi_amd.engine import Engine
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        eng = Engine(0)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    eng.load_edm(eargs, esd)
    if pargs is not None:
        eng.load_predictor(pargs, psd)
    return eng


def oracle_step_pair(O, esd, eargs, gamma, s_idx, t_idx, z_t, node_mask, edge_mask, eps_raw, psd=None, pargs=None, target_w=None,
                     scale=1.0, target_z=None):
    """sample_p_zs_given_zt / sample_p_zs_given_zt_guidance (en_diffusion.py:807-935) for the pair (s_idx, t_idx), composed
    from oracle.edm_phi, oracle.predictor_grad and oracle.step_coefficients exactly as oracle.step_unguided / step_guided
    compose them for t_idx = s_idx + 1.  target_w: a weight vector, or a callable (pred, t) -> dT/dpred; target_z: a callable
    (z_s, pred, t) -> (dT/dpred, direct dT/dz)."""
    F32 = np.float32
    T = eargs["diffusion_steps"]
    B, N, D = z_t.shape
    nm = np.asarray(node_mask, F32).reshape(B, N, 1)
    z_t = np.asarray(z_t, F32)
    c = O.step_coefficients(gamma, s_idx, t_idx)
    t_val = F32(F32(t_idx) / F32(T))
    eps_hat = O.edm_phi(esd, eargs, z_t, t_val, nm, edge_mask)
    guided = target_w is not None or target_z is not None
    if guided:
        eps_hat = np.nan_to_num(eps_hat, nan=0.0, posinf=np.finfo(F32).max, neginf=np.finfo(F32).min)
    zs = z_t / c["alpha_ts"] - c["eps_coef"] * eps_hat + c["sigma"] * O._combined_noise(np.asarray(eps_raw, F32), nm)
    if guided:
        direct = None
        if target_z is not None:
            pred0 = O.predictor_forward(psd, pargs, zs, nm, edge_mask, t_val)
            gp, gz = target_z(zs, pred0, float(t_val))
            dpred = np.asarray(gp, F32).reshape(B, -1) * F32(scale)
            direct = np.asarray(gz, F32).reshape(B, N, D) * F32(scale) * nm
        elif callable(target_w):
            pred0 = O.predictor_forward(psd, pargs, zs, nm, edge_mask, t_val)
            dpred = np.asarray(target_w(pred0, float(t_val)), F32).reshape(B, -1) * F32(scale)
        else:
            dpred = np.broadcast_to(np.asarray(target_w, F32) * F32(scale), (B, len(target_w)))
        _, grad = O.predictor_grad(psd, pargs, zs, nm, edge_mask, t_val, dpred)
        if direct is not None:
            grad = grad + direct
        gnorm = np.sqrt((grad.reshape(B, -1) ** 2).sum(-1))
        clip = np.minimum(F32(10.0) / (gnorm + F32(1e-6)), F32(1.0))
        grad = grad * clip[:, None, None]
        grad = np.concatenate([O.remove_mean_with_mask(grad[:, :, :3], nm), grad[:, :, 3:]], axis=2)
        zs = zs - c["sigma"] * grad
    zs = np.concatenate([O.remove_mean_with_mask(zs[:, :, :3], nm), zs[:, :, 3:]], axis=2)
    if guided and np.isnan(zs).any():
        zs = np.nan_to_num(zs, nan=0.0, posinf=np.finfo(F32).max, neginf=np.finfo(F32).min)
    return zs
