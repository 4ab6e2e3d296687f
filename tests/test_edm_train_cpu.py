"""EDM training, host side (no GPU): the name -> role table and the has-gradient rule gaudi_edm_loss_grad reads the denoiser
with (gaudi_host_edm_train_layout), its refusal of mis-shaped tensors, and the seed coefficients of the reverse pass
(gaudi_host_edm_seed_coef) against a numpy restatement of en_diffusion.py:507-515,694-767 in train mode."""
import ctypes as C

import numpy as np
import pytest

from gaudi_amd import _lib, synth
from gaudi_amd._lib import EdmConfig, FP, fptr

CONFIGS = [
    dict(dataset="cata", nf=32, n_layers=2),
    dict(dataset="hetro", nf=32, n_layers=2, attention=False, tanh=False, inv_sublayers=2),
    dict(dataset="cata", nf=32, n_layers=3, sin_embedding=True),
    dict(dataset="cata"),
]


def _cfg(a, F):
    return EdmConfig(F, int(a["nf"]), int(a["n_layers"]), int(a.get("inv_sublayers", 1)), int(bool(a["attention"])),
                     int(bool(a["tanh"])), float(a["coords_range"]), float(a["norm_constant"]), 1.0,
                     int(a["diffusion_steps"]), 2.0, 1e-5, (C.c_float * 3)(1.0, 4.0, 10.0),
                     int(bool(a.get("sin_embedding", False))))


def _layout(a, sd, with_wt=True):
    lib = _lib.load_library()
    F = synth.num_node_features(a["dataset"])
    names = list(sd)
    arrs = [np.ascontiguousarray(sd[k], np.float32) for k in names]
    n = len(names)
    L, S = int(a["n_layers"]), int(a.get("inv_sublayers", 1))
    off = np.full(4 + L * (10 * S + 5), -7, np.int32)
    has = np.full(n, -7, np.int32)
    total = sum(v.size for v in arrs)
    wt = np.zeros(total, np.float32) if with_wt else None
    rc = lib.gaudi_host_edm_train_layout(C.byref(_cfg(a, F)), n, (C.c_char_p * n)(*[k.encode() for k in names]),
                                         (FP * n)(*[fptr(v) for v in arrs]), (C.c_int64 * n)(*[v.size for v in arrs]),
                                         off.ctypes.data_as(_lib.IP), has.ctypes.data_as(_lib.IP), fptr(wt))
    return rc, names, arrs, off, has, wt


@pytest.mark.parametrize("over", CONFIGS)
def test_layout_table_and_gradient_rule(over):
    a = synth.edm_args(**over)
    F = synth.num_node_features(a["dataset"])
    sd = synth.synth_edm_state_dict(a, F, seed=1, gamma=np.zeros(int(a["diffusion_steps"]) + 1, np.float32))
    rc, names, arrs, off, has, wt = _layout(a, sd)
    assert rc == 0
    starts = np.cumsum([0] + [v.size for v in arrs])[:-1]
    start_of = dict(zip(names, starts))
    # every dynamics.egnn tensor has a role and a gradient path; gamma.gamma and buffer have neither
    for n, hflag in zip(names, has):
        assert hflag == (1 if n.startswith("dynamics.egnn.") else 0), n
    roles = {int(o) for o in off if o >= 0}
    assert roles == {int(start_of[n]) for n in names if n.startswith("dynamics.egnn.")}
    # head slots, and the transposes of the matrices
    p = "dynamics.egnn."
    assert off[0] == start_of[p + "embedding.weight"] and off[2] == start_of[p + "embedding_out.weight"]
    S = int(a.get("inv_sublayers", 1))
    att = bool(a["attention"])
    assert (off[4 + 4] >= 0) == att and (off[4 + 5] >= 0) == att  # att_mlp of block 0, gcl_0
    for n, v in zip(names, arrs):
        shp = sd[n].shape
        got = wt[start_of[n]:start_of[n] + v.size]
        if len(shp) == 2 and min(shp) > 1:
            assert np.array_equal(got, sd[n].T.reshape(-1)), n
        else:
            assert np.array_equal(got, v.reshape(-1)), n
    # the equivariant update's last layer (no bias) sits at slot 4 of gcl_equiv
    for l in range(int(a["n_layers"])):
        eq = 4 + l * (10 * S + 5) + 10 * S
        assert off[eq + 4] == start_of[f"{p}e_block_{l}.gcl_equiv.coord_mlp.4.weight"]


def test_mis_shaped_tensor_refused():
    a = synth.edm_args(dataset="cata", nf=32, n_layers=2)
    sd = synth.synth_edm_state_dict(a, 1, seed=1)
    k = "dynamics.egnn.e_block_1.gcl_0.edge_mlp.0.weight"
    sd[k] = sd[k][:, :-1].copy()
    rc, *_ = _layout(a, sd)
    assert rc != 0
    sd = synth.synth_edm_state_dict(synth.edm_args(dataset="cata", nf=32, n_layers=2, sin_embedding=True), 1, seed=1)
    rc, *_ = _layout(a, sd)  # sin_embedding weights (24 edge features) for a config without it
    assert rc != 0


def _ref_coef(loss_type, t, T, D, N, snr_w, w):
    """d loss_b / d net = c (net - eps) from en_diffusion.py:507-515 (compute_error), 694-700 (SNR weight), 585-599 (x part of
    log p(x | z_0)), 750-762 (selection and the (T+1) estimator weight), differentiated by hand."""
    l2 = loss_type == 0
    denom = D * N if l2 else 1.0
    if t > 0:
        weight = 1.0 if l2 else snr_w
        c = 0.5 * weight * 2.0 / denom
        c = c if l2 else (T + 1) * c
        return w * c, w * c
    c = 0.5 * 2.0 / denom  # -log p(x | z_0) = 0.5 error_x
    c = c if l2 else (T + 1) * c
    return w * c, 0.0


def test_seed_coefficients():
    lib = _lib.load_library()
    rng = np.random.default_rng(0)
    T, D, N, B = 50, 4, 11, 16
    t = rng.integers(0, T + 1, B).astype(np.int32)
    t[0], t[1] = 0, T
    snr = rng.uniform(0.1, 5.0, B).astype(np.float32)
    w = rng.uniform(-2.0, 2.0, B).astype(np.float32)
    for lt in (0, 1):
        for weight in (None, w):
            out = np.zeros((B, 2), np.float32)
            rc = lib.gaudi_host_edm_seed_coef(lt, B, T, D, N, t.ctypes.data_as(_lib.IP), fptr(snr), fptr(weight), fptr(out))
            assert rc == 0
            ww = np.ones(B, np.float32) if weight is None else weight
            ref = np.array([_ref_coef(lt, int(t[b]), T, D, N, float(snr[b]), float(ww[b])) for b in range(B)])
            np.testing.assert_allclose(out, ref, rtol=1e-6, atol=0)
            assert np.all(out[t == 0, 1] == 0)
    out = np.zeros((B, 2), np.float32)
    assert lib.gaudi_host_edm_seed_coef(2, B, T, D, N, t.ctypes.data_as(_lib.IP), fptr(snr), None, fptr(out)) != 0


@pytest.mark.parametrize("name", ["init_att", "init_plain"])
def test_fresh_init_matches_reference(golden, name):
    """get_model without a checkpoint: the reference's modules' draws after torch.manual_seed(0), bit for bit (g27)."""
    import json

    import torch

    from gaudi_amd.models_edm import init_edm_state_dict
    g = golden("g27_edm_train")
    a = synth.edm_args(dataset="cata", **json.loads(str(g[name + "_cfg"])))
    torch.manual_seed(0)
    sd = init_edm_state_dict(a, 1)
    keys = [k for k in json.loads(str(g[name + "_keys"])) if k != "gamma.gamma"]
    assert set(sd) == set(keys)
    for k in keys:
        assert np.array_equal(sd[k], g[f"{name}:{k}"]), k


def test_queue_and_gradient_clipping_vs_torch():
    """train_edm.Queue / gradient_clipping (edm/utils.py:31-70) against torch's clip_grad_norm_ and a numpy history."""
    import torch

    from gaudi_amd.train_edm import Queue, gradient_clipping

    class Flow:
        def __init__(self, ps):
            self.ps = ps

        def parameters(self):
            return iter(self.ps)

    q = Queue(max_len=3)
    q.add(3000)
    hist = [3000.0]
    rng = np.random.default_rng(1)
    for scale in (10.0, 5000.0, 1.0, 2.0, 7.0):
        ps = [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(5)),
              torch.nn.Parameter(torch.zeros(2), requires_grad=False)]
        for p in ps[:2]:
            p.grad = torch.from_numpy(rng.standard_normal(p.shape).astype(np.float32) * scale)
        ref = [p.grad.clone() for p in ps[:2]]
        allowed = 1.5 * np.mean(q.items) + 2 * np.std(q.items)
        norm = float(np.sqrt(sum(float((r.double() ** 2).sum()) for r in ref)))
        gn = gradient_clipping(Flow(ps), q)
        assert abs(float(gn) - norm) <= 1e-5 * norm
        hist.insert(0, allowed if float(gn) > allowed else float(gn))
        hist = hist[:3]
        assert q.items == hist
        coef = min(1.0, allowed / (norm + 1e-6))  # torch's clip_coef
        for p, r in zip(ps[:2], ref):
            np.testing.assert_allclose(p.grad.numpy(), r.numpy() * coef, rtol=1e-5, atol=0)
    assert len(q) == 3
