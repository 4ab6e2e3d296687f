"""A numpy composition of the EDM's eval-mode NLL (en_diffusion.py:646-805, t0_always) around any phi: the yardstick the NLL
tests hold the fused launch and the reference fixture (golden g25) to."""
import json

import numpy as np
import torch

from gaudi_amd import synth
from oracle import gaudi_oracle as O

TERMS = ("kl_prior", "loss_t", "neg_log_constants", "loss_term_0", "delta_log_px", "error")
CASES = ("cata_tiny", "hetro_tiny", "cata_default", "hetro_large", "hetro_soft", "cata_se_tiny")


def case(g, name):
    """-> (edm args, state dict, inputs dict) of fixture case `name`."""
    cfg = json.loads(str(g[name + "_cfg"]))
    args = synth.edm_args(dataset=cfg["dataset"], **cfg["over"])
    F = synth.num_node_features(cfg["dataset"])
    sd = synth.synth_edm_state_dict(args, F, seed=cfg["wseed"], amplify_coord=cfg["amp"])
    inp = {k: g[f"{name}_{k}"] for k in ("x", "h", "node_mask", "edge_mask", "t_int", "noise")}
    return args, sd, inp


def noise_power(args):
    s = args["diffusion_noise_schedule"]
    return 0.0 if s == "cosine" else float(s.split("_")[1])


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _cdf(v):
    return 0.5 * (1.0 + torch.erf(torch.from_numpy(np.asarray(v, np.float64)) / np.sqrt(2.0)).numpy())


def nll_terms(args, gamma, x, h, node_mask, t_int, eps_raw, eps0_raw, phi):
    """phi(z [B,N,D] float32, t [B] float32) -> eps_hat.  Returns (nll [B], terms [B,6] in TERMS order), float64 except the
    network inputs, which are built in float32 as the device builds them."""
    B, N = x.shape[0], x.shape[1]
    T = int(args["diffusion_steps"])
    nv0, nv1 = (np.float32(v) for v in args["normalize_factors"][:2])
    nm = node_mask.reshape(B, N, 1).astype(np.float32)
    xh = np.concatenate([x / nv0, h / nv1 * nm], axis=2).astype(np.float32)
    e = O._combined_noise(eps_raw.astype(np.float32), nm)
    e0 = O._combined_noise(eps0_raw.astype(np.float32), nm)
    g = gamma.astype(np.float32)
    ti = np.asarray(t_int).reshape(B).astype(np.int64)
    g_t, g_s, g0, gT = g[ti], g[ti - 1], g[0], g[T]
    a_t, s_t = np.sqrt(_sig(-g_t)).astype(np.float32), np.sqrt(_sig(g_t)).astype(np.float32)
    a0, s0 = np.float32(np.sqrt(_sig(-g0))), np.float32(np.sqrt(_sig(g0)))
    zt = (a_t[:, None, None] * xh + s_t[:, None, None] * e).astype(np.float32)
    z0 = (a0 * xh + s0 * e0).astype(np.float32)
    ph_t = np.asarray(phi(zt, (ti / T).astype(np.float32)), np.float64)
    ph_0 = np.asarray(phi(z0, np.zeros(B, np.float32)), np.float64)
    error = ((e - ph_t) ** 2).sum((1, 2))
    loss_t = T * 0.5 * (np.exp(np.float64(g_t) - g_s) - 1.0) * error
    err0 = ((e0[:, :, :3] - ph_0[:, :, :3]) ** 2).sum((1, 2))
    c = z0[:, :, 3:].astype(np.float64) * nv1 - 1.0
    sc = np.float64(s0) * nv1
    lp = np.log(_cdf((c + 0.5) / sc) - _cdf((c - 0.5) / sc) + 1e-10)
    m = lp.max(2, keepdims=True)
    logz = np.log(np.exp(lp - m).sum(2, keepdims=True)) + m
    log_ph = ((lp - logz) * h * nm).sum((1, 2))
    loss0 = 0.5 * err0 - log_ph
    n = nm.reshape(B, N).astype(np.float64).sum(1)
    dof = (n - 1.0) * 3.0
    aT, sT = np.sqrt(_sig(-np.float64(gT))), np.sqrt(_sig(np.float64(gT)))
    mu_h = aT * xh[:, :, 3:].astype(np.float64)
    kl_h = ((np.log(1.0 / sT) + 0.5 * (sT ** 2 + mu_h ** 2) - 0.5) * nm).sum((1, 2))
    mu2 = ((aT * xh[:, :, :3].astype(np.float64)) ** 2).sum((1, 2))
    kl = dof * np.log(1.0 / sT) + 0.5 * (dof * sT ** 2 + mu2) - 0.5 * dof + kl_h
    nlc = -dof * (-0.5 * np.float64(g0) - 0.5 * np.log(2 * np.pi))
    dlp = -dof * np.log(np.float64(nv0))
    terms = np.stack([kl, loss_t, nlc, loss0, dlp, error], axis=1)
    return kl + loss_t + nlc + loss0 - dlp, terms


def check_close(got, ref, what, tol=1e-4):
    """|got - ref| <= tol * max(1, |ref|) element-wise."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = np.abs(got - ref) > tol * np.maximum(1.0, np.abs(ref))
    assert not bad.any(), f"{what}: {np.argwhere(bad)[:5].tolist()} got {got[bad][:5]} ref {ref[bad][:5]}"
