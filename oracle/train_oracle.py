"""TEST INFRASTRUCTURE ONLY (see oracle/__init__.py) -- torch restatement of the two training losses, differentiable in any dtype:
the EDM's train-mode loss per molecule (EnVariationalDiffusion.forward -> compute_loss with t0_always = False,
edm/equivariant_diffusion/en_diffusion.py:644-805) and the predictor's L1 loss on a noised molecule
(cond_prediction/train_cond_predictor.py:47-81).  ``torch.autograd.grad`` then yields every weight gradient: the yardstick
gaudi_edm_loss_grad and gaudi_predictor_loss_grad are held to at shapes no fixture stores.

The two networks are the formulas of oracle/gaudi_oracle.py (edm_phi, predictor_forward, sample_edm_t, _combined_noise, the gamma
table) written with torch tensors on the CPU; every function cites the reference file:line it follows.  As in the reference's
own float64 run (model.double()) three things stay float32 whatever ``dtype`` is: the gamma table (a float32 parameter, cast),
the time t_int / T (``t_int.float() / T``) and the sinusoid frequencies (neither a parameter nor a buffer)."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import gaudi_oracle as O


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def _lin(x, w, b=None):
    y = x @ w.T
    return y if b is None else y + b


def _silu(x):
    return x * torch.sigmoid(x)


def _remove_mean(x, nm):
    """edm/equivariant_diffusion/utils.py:33-44."""
    n = torch.clamp(nm.sum(1, keepdim=True), min=1)
    return x - x.sum(1, keepdim=True) / n * nm


def _noise(eps_raw, nm):
    """sample_combined_position_feature_noise (en_diffusion.py:937-956) from raw N(0, 1) draws [B,N,3+F]."""
    ex = _remove_mean(eps_raw[:, :, :3] * nm, nm)
    return torch.cat([ex, eps_raw[:, :, 3:] * nm], dim=2)


def _gamma(args, dtype):
    g = O.gamma_table(args["diffusion_noise_schedule"], int(args["diffusion_steps"]), args["diffusion_noise_precision"])
    return torch.from_numpy(g).to(dtype)  # float32 values (en_diffusion.py:191-218)


def _time(t_int, T, dtype):
    return torch.from_numpy(np.asarray(t_int, np.float32).reshape(-1) / np.float32(T)).to(dtype)


def _normalized(args, x, onehot, nm, dtype):
    """normalize (en_diffusion.py:384-404, norm_biases 0, no integer features) -> [x / nv0 | onehot / nv1 * mask]."""
    nv = args.get("normalize_factors", [1, 4, 10])
    return torch.cat([_t(x, dtype) / float(nv[0]), _t(onehot, dtype) / float(nv[1]) * nm], dim=2)


def _coord2diff(x, norm_constant):
    """egnn_new.py:394-400 on the dense edge set."""
    diff = x[:, :, None, :] - x[:, None, :, :]
    radial = (diff ** 2).sum(-1, keepdim=True)
    return radial, diff / (torch.sqrt(radial + 1e-8) + norm_constant)


def _sin(x, dtype):
    """SinusoidsEmbeddingNew.forward (egnn_new.py:387-391): the embedding is returned detached (:391), so no gradient reaches
    the coordinates through the edge attributes of a sin_embedding model."""
    e = torch.sqrt(x + 1e-8) * torch.from_numpy(O.sin_frequencies(np.float32)).to(dtype)
    return torch.cat([torch.sin(e), torch.cos(e)], dim=-1).detach()


def _edge_in(h, attr):
    B, N, H = h.shape
    return torch.cat([h[:, :, None, :].expand(B, N, N, H), h[:, None, :, :].expand(B, N, N, H), attr], dim=-1)


def edm_phi(w, cfg, z, t, nm, em, tanh_log=None):
    """EGNN_dynamics._forward (edm/egnn/models.py:83-152); w: {name: tensor}; nm [B,N,1]; em [B,N,N,1]; t [B]."""
    dtype = z.dtype
    B, N, _ = z.shape
    xh = z * nm
    x, h = xh[:, :, :3], xh[:, :, 3:]
    h = torch.cat([h, t.reshape(B, 1, 1).expand(B, N, 1)], dim=2)  # the time column is not masked (models.py:97-105)
    p = "dynamics.egnn."
    d0, _ = _coord2diff(x, 1.0)  # egnn_new.py:301
    sin = bool(cfg.get("sin_embedding", False))
    if sin:
        d0 = _sin(d0, dtype)
    h = _lin(h, w[p + "embedding.weight"], w[p + "embedding.bias"])
    x_in = x
    agg = cfg.get("aggregation_method", "sum")
    assert agg in ("sum", "mean")
    normf = float(cfg.get("normalization_factor", 1)) if agg == "sum" else float(N)  # egnn_new.py:403-421 (dense edge list)
    for l in range(int(cfg["n_layers"])):
        bp = f"{p}e_block_{l}."
        radial, cdiff = _coord2diff(x, float(cfg["norm_constant"]))  # egnn_new.py:216
        if sin:
            radial = _sin(radial, dtype)
        attr = torch.cat([radial, d0], dim=-1)
        for s in range(int(cfg.get("inv_sublayers", 1))):
            gp = f"{bp}gcl_{s}."
            m = _silu(_lin(_edge_in(h, attr), w[gp + "edge_mlp.0.weight"], w[gp + "edge_mlp.0.bias"]))
            m = _silu(_lin(m, w[gp + "edge_mlp.2.weight"], w[gp + "edge_mlp.2.bias"]))
            if cfg["attention"]:
                m = m * torch.sigmoid(_lin(m, w[gp + "att_mlp.0.weight"], w[gp + "att_mlp.0.bias"]))
            a = (m * em).sum(dim=2) / normf
            o = _silu(_lin(torch.cat([h, a], dim=-1), w[gp + "node_mlp.0.weight"], w[gp + "node_mlp.0.bias"]))
            h = (h + _lin(o, w[gp + "node_mlp.2.weight"], w[gp + "node_mlp.2.bias"])) * nm
        ep = f"{bp}gcl_equiv."
        c = _silu(_lin(_edge_in(h, attr), w[ep + "coord_mlp.0.weight"], w[ep + "coord_mlp.0.bias"]))
        c = _silu(_lin(c, w[ep + "coord_mlp.2.weight"], w[ep + "coord_mlp.2.bias"]))
        phi = _lin(c, w[ep + "coord_mlp.4.weight"])
        if cfg["tanh"]:
            th = torch.tanh(phi)
            if tanh_log is not None:
                tanh_log.append(th.detach())
            trans = cdiff * th * float(cfg["coords_range"])  # the raw argument (egnn_new.py:290)
        else:
            trans = cdiff * phi
        x = (x + (trans * em).sum(dim=2) / normf) * nm
        h = h * nm
    h = _lin(h, w[p + "embedding_out.weight"], w[p + "embedding_out.bias"]) * nm
    vel = _remove_mean((x - x_in) * nm, nm)
    return torch.cat([vel, h[:, :, :-1]], dim=2)  # the time column is dropped (models.py:132-134)


def predictor_forward(w, cfg, z, t, nm, em, tanh_log=None):
    """EGNN_predictor.forward (edm/egnn_predictor/models.py:433-457, gcl.py:225-316) -> pred [B,K]."""
    B, N, _ = z.shape
    x, h = z[:, :, :3] * nm, z[:, :, 3:] * nm
    h = torch.cat([h, t.reshape(B, 1, 1).expand(B, N, 1)], dim=2)
    d0 = ((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1, keepdim=True)  # models.py:452
    p = "egnn."
    h = _lin(h, w[p + "embedding.weight"], w[p + "embedding.bias"])
    L = int(cfg["n_layers"])
    R = float(cfg["coords_range"]) / L  # egnn_predictor/models.py:515
    for l in range(L):
        gp = f"{p}gcl_{l}."
        radial, cdiff = _coord2diff(x, 1.0)  # gcl.py:308-316
        m = _silu(_lin(_edge_in(h, torch.cat([radial, d0], dim=-1)), w[gp + "edge_mlp.0.weight"], w[gp + "edge_mlp.0.bias"]))
        m = _silu(_lin(m, w[gp + "edge_mlp.2.weight"], w[gp + "edge_mlp.2.bias"]))
        if cfg["attention"]:
            m = m * torch.sigmoid(_lin(m, w[gp + "att_mlp.0.weight"], w[gp + "att_mlp.0.bias"]))
        e = m * em
        phi = _lin(_silu(_lin(e, w[gp + "coord_mlp.0.weight"], w[gp + "coord_mlp.0.bias"])), w[gp + "coord_mlp.2.weight"])
        if cfg["tanh"]:
            th = torch.tanh(phi)
            if tanh_log is not None and l < L - 1:  # (the last layer's coordinates are never read)
                tanh_log.append(th.detach())
            tau = th * R
        else:
            tau = phi
        x_new = (x + (cdiff * tau * em).sum(dim=2)) * nm
        o = _silu(_lin(torch.cat([h, e.sum(dim=2)], dim=-1), w[gp + "node_mlp.0.weight"], w[gp + "node_mlp.0.bias"]))
        h = (h + _lin(o, w[gp + "node_mlp.2.weight"], w[gp + "node_mlp.2.bias"])) * nm
        x = x_new
    out = _lin(h, w[p + "embedding_out.weight"], w[p + "embedding_out.bias"]) * nm
    return out.mean(dim=1)  # over the padded N (models.py:457)


def _cdf(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _leaves(sd, prefix, dtype):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items() if k.startswith(prefix)}


def _grads(total, w, sd):
    names = list(w)
    got = torch.autograd.grad(total, [w[k] for k in names], allow_unused=True)
    out = {k: None for k in sd}
    for k, g in zip(names, got):
        out[k] = None if g is None else g.detach().numpy()
    return out


def edm_train(sd, args, x, onehot, t_int, node_mask, edge_mask, noise, loss_type="l2", weight=None, dtype=torch.float64,
              aux=None):
    """model.train(); loss = model(x, h, node_mask, edge_mask) under a fixed t_int and injected noise ->
    (loss [B], net [B,N,3+F], {name: d sum_b weight_b loss_b / d tensor, or None}); gamma.gamma and the buffer: None.
    aux (a dict): receives z_t and the tanh values of every coord_mlp."""
    assert loss_type in ("l2", "vlb")
    l2 = loss_type == "l2"
    B, N = np.asarray(x).shape[:2]
    T = int(args["diffusion_steps"])
    nv = args.get("normalize_factors", [1, 4, 10])
    nm = _t(node_mask, dtype).reshape(B, N, 1)
    em = _t(edge_mask, dtype).reshape(B, N, N, 1)
    w = _leaves(sd, "dynamics.", dtype)
    gamma = _gamma(args, dtype)
    ti = torch.as_tensor(np.asarray(t_int).reshape(B).astype(np.int64))
    xh = _normalized(args, x, onehot, nm, dtype)  # forward (:782)
    n_live = nm.reshape(B, N).sum(1)
    dof = (n_live - 1.0) * 3.0  # subspace_dimensionality (:379-382)
    dlp = torch.zeros(B, dtype=dtype) if l2 else -dof * math.log(float(nv[0]))  # (:386, 785-786)
    # compute_loss, t0_always = False (:644-775)
    g_t = gamma[ti].reshape(B, 1, 1)
    g_s = gamma[torch.clamp(ti - 1, min=0)].reshape(B, 1, 1)  # (s = -1 at t = 0 is never used, :663-665)
    alpha_t, sigma_t = torch.sqrt(torch.sigmoid(-g_t)), torch.sqrt(torch.sigmoid(g_t))
    eps = _noise(_t(noise, dtype), nm)
    z_t = alpha_t * xh + sigma_t * eps  # (:684)
    tanh_log = []
    net = edm_phi(w, args, z_t, _time(t_int, T, dtype), nm, em, tanh_log)  # (:689)
    D = xh.shape[2]
    denom = float(D * N) if l2 else 1.0  # compute_error (:507-515), in train mode with l2
    error = ((eps - net) ** 2).sum((1, 2)) / denom
    snr_w = torch.ones(B, dtype=dtype) if l2 else (torch.exp(-(g_s - g_t)) - 1.0).reshape(B)  # (:694-698)
    loss_gt0 = 0.5 * snr_w * error
    g_0 = gamma[0]
    nlc = torch.zeros(B, dtype=dtype) if l2 else -(dof * (-0.5 * g_0 - 0.5 * math.log(2 * math.pi)))  # (:517-531, 704-708)
    # kl_prior (:459-491, 90-129)
    g_T = gamma[T]
    a_T, s_T = torch.sqrt(torch.sigmoid(-g_T)), torch.sqrt(torch.sigmoid(g_T))
    mu = a_T * xh
    kl_h = ((torch.log(1.0 / s_T) + 0.5 * (s_T ** 2 + mu[:, :, 3:] ** 2) - 0.5) * nm).sum((1, 2))
    mu2 = (mu[:, :, :3] ** 2).sum((1, 2))
    kl = dof * torch.log(1.0 / s_T) + 0.5 * (dof * s_T ** 2 + mu2) - 0.5 * dof + kl_h
    # log_pxh_given_z0_without_constants on (z_t, gamma_t) (:568-642, 746-748), selected at t = 0
    log_px = -0.5 * ((eps[:, :, :3] - net[:, :, :3]) ** 2).sum((1, 2)) / denom
    sig_cat = sigma_t * float(nv[1])
    c = z_t[:, :, 3:] * float(nv[1]) - 1.0
    lp = torch.log(_cdf((c + 0.5) / sig_cat) - _cdf((c - 0.5) / sig_cat) + 1e-10)
    lp = lp - torch.logsumexp(lp, dim=2, keepdim=True)
    log_ph = (lp * (xh[:, :, 3:] * float(nv[1])) * nm).sum((1, 2))
    loss_0 = -(log_px + log_ph)
    t0 = (ti == 0).to(dtype)
    loss_t = loss_0 * t0 + (1.0 - t0) * loss_gt0  # (:750-755)
    est = loss_t if l2 else (T + 1) * loss_t  # (:757-762)
    loss = kl + est + nlc - dlp  # (:767, 803)
    wb = torch.ones(B, dtype=dtype) if weight is None else _t(weight, dtype).reshape(B)
    grads = _grads((wb * loss).sum(), w, sd)
    if aux is not None:
        aux["z_t"] = z_t.detach().numpy()
        aux["tanh"] = [t_.numpy() for t_ in tanh_log]
    return loss.detach().numpy(), net.detach().numpy(), grads


def pred_train(edm_args, pred_sd, pred_args, x, onehot, t_int, node_mask, edge_mask, y, noise, dtype=torch.float64, aux=None):
    """compute_loss + loss.backward() of the predictor (train_cond_predictor.py:64-81) under a fixed t_int and injected noise ->
    (loss, pred [B,K], {name: d loss / d tensor, or None where the tensor has no gradient path}); the noising is sample_edm_t
    (:47-61) on the EDM's schedule.  y = None: forward only, (None, pred, {})."""
    B, N = np.asarray(x).shape[:2]
    T = int(edm_args["diffusion_steps"])
    nm = _t(node_mask, dtype).reshape(B, N, 1)
    em = _t(edge_mask, dtype).reshape(B, N, N, 1)
    w = _leaves(pred_sd, "egnn.", dtype)
    gamma = _gamma(edm_args, dtype)
    ti = torch.as_tensor(np.asarray(t_int).reshape(B).astype(np.int64))
    g_t = gamma[ti].reshape(B, 1, 1)
    xh = _normalized(edm_args, x, onehot, nm, dtype)
    z_t = torch.sqrt(torch.sigmoid(-g_t)) * xh + torch.sqrt(torch.sigmoid(g_t)) * _noise(_t(noise, dtype), nm)
    tanh_log = []
    pred = predictor_forward(w, pred_args, z_t, _time(t_int, T, dtype), nm, em, tanh_log)
    if aux is not None:
        aux["z_t"] = z_t.detach().numpy()
        aux["tanh"] = [t_.numpy() for t_ in tanh_log]
    if y is None:
        return None, pred.detach().numpy(), {}
    loss = (pred - _t(y, dtype).reshape(pred.shape)).abs().mean()  # l1_loss, mean over B * K (:80)
    return float(loss.detach()), pred.detach().numpy(), _grads(loss, w, pred_sd)
