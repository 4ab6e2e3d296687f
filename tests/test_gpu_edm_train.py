"""EDM training on the GPU (gaudi_edm_loss_grad: the train-mode loss per molecule and its weight gradient through a separate
fp32 reverse pass): against the reference's own model.train() / backward() (golden g27), and by its own properties --
determinism, batch additivity, the per-molecule weights, rotation invariance, central differences, the stale-image reload
after gaudi_edm_set_train_weights, and the refusals."""
import json

import numpy as np
import pytest

from gaudi_amd import synth
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
FILES = {"cata_mixed": "g27_edm_grad", "cata_t0": "g27_edm_grad", "cata_vlb": "g27_edm_grad",
         "hetro_500_T": "g27_edm_grad_hetro", "plain_mean": "g27_edm_grad_hetro", "cata_sin": "g27_edm_grad_hetro",
         "cata_default": "g27_edm_grad_default"}


def _proj_summary(g, seed):
    """tools/make_golden.py:_proj_summary."""
    g = np.asarray(g, np.float64).reshape(-1)
    r = np.random.Generator(np.random.Philox(key=seed))
    proj = r.standard_normal((8, g.size))
    idx = r.integers(0, g.size, 64)
    return np.concatenate([[g.sum(), (g * g).sum()], proj @ g, g[idx]])


def _case(golden, name):
    g = golden(FILES[name])
    cfg = json.loads(str(g[name + "_cfg"]))
    args = synth.edm_args(dataset=cfg["dataset"], **cfg["over"])
    F = synth.num_node_features(cfg["dataset"])
    sd = synth.synth_edm_state_dict(args, F, seed=cfg["wseed"], amplify_coord=cfg["amp"])
    inp = {k: g[f"{name}_{k}"] for k in ("x", "h", "node_mask", "edge_mask", "t_int", "noise")}
    B, N = inp["x"].shape[0], inp["x"].shape[1]
    inp["node_mask"] = inp["node_mask"].reshape(B, N)
    inp["edge_mask"] = inp["edge_mask"].reshape(B, N, N)
    return g, args, sd, inp


def _engine(args, sd):
    from gaudi_amd.engine import Engine
    eng = Engine(0)
    eng.load_edm(args, sd)
    return eng


def _call(eng, args, inp, sl=slice(None), **kw):
    kw.setdefault("noise", inp["noise"][sl])
    kw.setdefault("loss_type", args.get("diffusion_loss_type", "l2"))
    return eng.edm_loss_grad(inp["x"][sl], inp["h"][sl], inp["t_int"][sl], inp["node_mask"][sl], inp["edge_mask"][sl], **kw)


@pytest.mark.parametrize("name", list(FILES))
def test_loss_and_gradients_vs_reference(golden, name):
    g, args, sd, inp = _case(golden, name)
    eng = _engine(args, sd)
    try:
        loss, net, grads = _call(eng, args, inp)
        ref_loss = g[name + "_loss"]
        # sin_embedding: sinusoids of up to 429 sqrt(r) turn the fp32 rounding of r into ~1e-4 rad of phase; the bounds
        # there are twice the fp32 reference's own spread from the float64 one (at least the common bounds)
        sin = bool(args.get("sin_embedding"))
        ltol = max(1e-5, 2 * float(np.max(np.abs(ref_loss - g[name + "_loss64"]) / np.abs(g[name + "_loss64"])))) if sin else 1e-5
        assert np.all(np.abs(loss - ref_loss) <= ltol * np.abs(ref_loss)), (loss, ref_loss)
        params = json.loads(str(g[name + "_params"]))
        nograd = set(json.loads(str(g[name + "_nograd"])))
        assert nograd == {"gamma.gamma"}
        if sin:  # the fp32 reference's own spread from the exact gradient, over the case (test_gpu_round6's rule)
            spread = max(rel_err(g[f"{name}_grad32:{n}"], g[f"{name}_grad:{n}"]) for n in params if n not in nograd)
        for n in params:
            if n in nograd:
                continue
            assert grads[n] is not None, n
            if name == "cata_default":
                got, ref = _proj_summary(grads[n], 2790 + params.index(n)), g[f"{name}_gsum:{n}"]
            else:
                got, ref = grads[n], g[f"{name}_grad:{n}"]
            tol = max(TOL, 2 * spread) if sin else TOL
            assert rel_err(got, ref) < tol, (n, rel_err(got, ref), tol)
        assert all(v is None for n, v in grads.items() if not n.startswith("dynamics."))  # buffer (and gamma.gamma)
        F = eng.F
        assert np.all(grads["dynamics.egnn.embedding_out.weight"][F] == 0)  # the time column of h_final is dropped
        ntol = max(TOL, 2 * rel_err(g[name + "_net32"], g[name + "_net"])) if sin else TOL
        assert rel_err(net, g[name + "_net"]) < ntol
        # net is phi of the z_t the call built
        eng_phi = eng.phi(g[name + "_zt"], inp["t_int"].astype(np.float32) / float(args["diffusion_steps"]),
                          inp["node_mask"], inp["edge_mask"])
        assert rel_err(net, eng_phi) < ntol
    finally:
        eng.close()


def test_deterministic_additive_weighted(golden):
    """Two calls are bit-identical; g(A u B) = g(A) + g(B); weight w gives sum_b w_b g_b; forward-only gives the same loss."""
    g, args, sd, inp = _case(golden, "cata_mixed")
    eng = _engine(args, sd)
    try:
        l0, n0, g0 = _call(eng, args, inp)
        l1, n1, g1 = _call(eng, args, inp)
        assert np.array_equal(l0, l1) and np.array_equal(n0, n1)
        assert all(np.array_equal(g0[k], g1[k]) for k in g0 if g0[k] is not None)
        lf, nf, gf = _call(eng, args, inp, grad=False)
        assert np.array_equal(lf, l0) and np.array_equal(nf, n0) and gf == {}
        B = inp["x"].shape[0]
        parts = [_call(eng, args, inp, slice(b, b + 1))[2] for b in range(B)]
        la, _, ga = _call(eng, args, inp, slice(0, 2))
        lb, _, gb = _call(eng, args, inp, slice(2, B))
        assert np.array_equal(np.concatenate([la, lb]), l0)
        w = np.array([0.5, -1.0, 2.0, 0.0, 1.5], np.float32)
        _, _, gw = _call(eng, args, inp, weight=w)
        for k, v in g0.items():
            if v is None:
                continue
            assert rel_err(ga[k] + gb[k], v) < TOL, k
            ref = sum(np.float64(w[b]) * parts[b][k] for b in range(B))
            assert rel_err(gw[k], ref) < TOL, k
    finally:
        eng.close()


def test_rotation_invariance(golden):
    """Rotating x and the noise's position columns rotates net and leaves the loss and every weight gradient unchanged."""
    g, args, sd, inp = _case(golden, "cata_mixed")
    eng = _engine(args, sd)
    try:
        l0, n0, g0 = _call(eng, args, inp)
        q, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((3, 3)))
        R = q.astype(np.float32)
        rot = dict(inp, x=(inp["x"] @ R).astype(np.float32))
        nz = inp["noise"].copy()
        nz[:, :, :3] = nz[:, :, :3] @ R
        l1, n1, g1 = _call(eng, args, rot, noise=nz)
        assert rel_err(l1, l0) < TOL
        assert rel_err(n1[:, :, :3], n0[:, :, :3] @ R) < TOL
        for k, v in g0.items():
            if v is not None:
                assert rel_err(g1[k], v) < 1e-3, (k, rel_err(g1[k], v))
    finally:
        eng.close()


def test_central_differences(golden):
    """Four scalars against forward-only calls (float64 composition of the fp32 losses)."""
    g, args, sd, inp = _case(golden, "cata_mixed")
    eng = _engine(args, sd)
    try:
        _, _, g0 = _call(eng, args, inp)
        for name, idx in [("dynamics.egnn.embedding.weight", (3, 1)),
                          ("dynamics.egnn.e_block_1.gcl_0.edge_mlp.2.weight", (5, 7)),
                          ("dynamics.egnn.e_block_0.gcl_equiv.coord_mlp.4.weight", (0, 3)),
                          ("dynamics.egnn.e_block_1.gcl_0.node_mlp.0.bias", (4,))]:
            vals = []
            h = 1e-2 * max(abs(float(sd[name][idx])), 1.0)
            for sgn in (1, -1):
                sd2 = {k: v.copy() for k, v in sd.items()}
                sd2[name][idx] += sgn * h
                eng.edm_set_train_weights(sd2)
                vals.append(np.float64(_call(eng, args, inp, grad=False)[0]).sum())
            fd = (vals[0] - vals[1]) / (2 * h)
            got = float(g0[name][idx])
            assert abs(fd - got) <= 2e-2 * max(abs(fd), abs(got)) + 5e-5, (name, fd, got)
        eng.edm_set_train_weights(sd)
    finally:
        eng.close()


def test_set_train_weights_and_stale_sampler(golden):
    """After gaudi_edm_set_train_weights the training call sees the new weights; the C entry points of the sampler refuse
    (GAUDI_E_STATE) until gaudi_load_edm runs; the Engine reloads on its own, and its phi and sample then equal those of a
    fresh Engine loaded with the same weights, bit for bit."""
    from gaudi_amd import _lib
    g, args, sd, inp = _case(golden, "cata_mixed")
    rng = np.random.default_rng(7)
    sd2 = {k: (v + 0.05 * rng.standard_normal(v.shape).astype(np.float32) if k.startswith("dynamics.") else v)
           for k, v in sd.items()}
    eng, fresh = _engine(args, sd), _engine(args, sd2)
    try:
        eng.edm_set_train_weights(sd2)
        la, na, ga = _call(eng, args, inp)
        lb, nb, gb = _call(fresh, args, inp)
        assert np.array_equal(la, lb) and np.array_equal(na, nb)
        assert all(np.array_equal(ga[k], gb[k]) for k in ga if ga[k] is not None)
        B, N, D = g["cata_mixed_zt"].shape
        z = np.ascontiguousarray(g["cata_mixed_zt"], np.float32)
        t = np.full(B, 0.5, np.float32)
        nm = np.ascontiguousarray(inp["node_mask"], np.float32)
        em = np.ascontiguousarray(inp["edge_mask"], np.float32)
        out = np.empty_like(z)
        rc = eng.lib.gaudi_phi(eng.h, B, N, _lib.fptr(z), _lib.fptr(t), _lib.fptr(nm), _lib.fptr(em), _lib.fptr(out))
        assert rc != 0 and b"gaudi_load_edm" in eng.lib.gaudi_last_error(eng.h)
        assert np.array_equal(eng.phi(z, t, nm, em), fresh.phi(z, t, nm, em))
        T = int(args["diffusion_steps"])
        noise = np.random.default_rng(3).standard_normal((T + 2, B, N, D)).astype(np.float32)
        xa, ha, _ = eng.sample(nm, em, noise=noise)
        xb, hb, _ = fresh.sample(nm, em, noise=noise)
        assert np.array_equal(xa, xb) and np.array_equal(ha, hb)
    finally:
        eng.close()
        fresh.close()


def test_refusals(golden):
    from gaudi_amd._lib import GaudiError
    g, args, sd, inp = _case(golden, "cata_mixed")
    eng = _engine(args, sd)
    try:
        with pytest.raises(GaudiError, match="l2"):
            _call(eng, args, inp, loss_type="x")
        bad = dict(inp, t_int=np.where(np.arange(len(inp["t_int"])) == 1, int(args["diffusion_steps"]) + 1, inp["t_int"]))
        with pytest.raises(GaudiError, match="outside"):
            _call(eng, args, bad)
        with pytest.raises(GaudiError, match="outside"):
            _call(eng, args, dict(inp, t_int=np.full_like(inp["t_int"], -1)))
        N = 129
        nm = np.ones((1, N), np.float32)
        em = np.ones((1, N, N), np.float32)
        x = np.zeros((1, N, 3), np.float32)
        h = np.zeros((1, N, eng.F), np.float32)
        h[:, :, 0] = 1
        with pytest.raises(GaudiError, match="128"):
            eng.edm_loss_grad(x, h, [1], nm, em)
        with pytest.raises(GaudiError):
            eng.edm_set_train_weights({k: v for k, v in list(sd.items())[::-1]})
    finally:
        eng.close()


def test_philox_noise_stream(golden):
    """Without injected noise the call draws Philox draw 0 of (seed, sample_offset + b): the same as injecting those draws."""
    g, args, sd, inp = _case(golden, "cata_mixed")
    eng = _engine(args, sd)
    try:
        B, N, D = inp["noise"].shape
        raw = eng.philox_normal(11, 7, B, N * D, 0, 1)
        nz = np.ascontiguousarray(np.asarray(raw, np.float32).reshape(-1)[:B * N * D].reshape(B, N, D))
        la, na, ga = _call(eng, args, inp, noise=None, seed=11, sample_offset=7)
        lb, nb, gb = _call(eng, args, inp, noise=nz)
        assert np.array_equal(la, lb) and np.array_equal(na, nb)
        assert all(np.array_equal(ga[k], gb[k]) for k in ga if ga[k] is not None)
    finally:
        eng.close()


def test_chunked_call_bit_identical(golden, monkeypatch):
    """A batch cut into several scratch chunks (a full one and a short last one): loss and net are the same bits as in one
    chunk; the gradients agree to summation order (the reduction splits each chunk's rows over four waves, so the order
    depends on the chunk size, while a wrong chunk offset would mix up whole tensors)."""
    g, args, sd, inp = _case(golden, "hetro_500_T")
    eng = _engine(args, sd)
    try:
        l0, n0, g0 = _call(eng, args, inp)
        monkeypatch.setenv("GAUDI_EDM_TRAIN_SCRATCH_KB", "600")  # ~1.5 molecules of N = 20 at nf 32: chunks of 1
        l1, n1, g1 = _call(eng, args, inp)
        monkeypatch.setenv("GAUDI_EDM_TRAIN_SCRATCH_KB", "1200")  # chunks of 3 then 1
        l2, n2, g2 = _call(eng, args, inp)
        for l, n_, gg in ((l1, n1, g1), (l2, n2, g2)):
            assert np.array_equal(l, l0) and np.array_equal(n_, n0)
            for k, v in g0.items():
                if v is not None:
                    assert rel_err(gg[k], v) < TOL, k
    finally:
        eng.close()


# ---- the torch-facing layer: GaudiModel in train mode, train_edm.train_epoch / val_epoch

def _model(args, sd):
    from gaudi_amd.models_edm import get_model
    return get_model(args, state_dict=sd)[0]


def _fixed_t(monkeypatch, t_int, T):
    import torch
    orig = torch.randint

    def fake(low, high, size, *a, **kw):
        if (low, high) == (0, T + 1):
            return torch.from_numpy(np.asarray(t_int, np.int64).reshape(size))
        return orig(low, high, size, *a, **kw)

    monkeypatch.setattr(torch, "randint", fake)


def test_model_train_forward_and_backward(golden, monkeypatch):
    """model.train(); loss = model(...): the per-molecule loss, whose backward through loss.mean(0), loss.sum() and a weighted
    sum gives G / B, G and sum_b w_b g_b; the names are the reference's; gamma.gamma keeps .grad None."""
    import torch
    g, args, sd, inp = _case(golden, "cata_mixed")
    model = _model(args, sd)
    try:
        assert model.training is False  # (starts in eval mode, unlike an nn.Module)
        model.train()
        names = [k for k, _ in model.named_parameters()]
        assert names == json.loads(str(g["cata_mixed_params"]))
        assert list(model.state_dict()) == json.loads(str(g["cata_mixed_state_keys"]))
        B, N = inp["x"].shape[0], inp["x"].shape[1]
        _fixed_t(monkeypatch, inp["t_int"], int(args["diffusion_steps"]))
        model.injected_noise = inp["noise"][None]
        ref_l, _, ref_g = _call(model.engine, args, inp)
        w = np.array([0.5, -1.0, 2.0, 0.0, 1.5], np.float32)
        _, _, ref_w = _call(model.engine, args, inp, weight=w)
        hd = {"categorical": torch.from_numpy(inp["h"]), "integer": torch.zeros(0)}
        args_in = (torch.from_numpy(inp["x"]), hd, torch.from_numpy(inp["node_mask"]),
                   torch.from_numpy(inp["edge_mask"]).view(B, N * N))
        for how, scale, ref in (("mean", 1.0 / B, ref_g), ("sum", 1.0, ref_g), ("weighted", None, ref_w)):
            for p in model.parameters():
                p.grad = None
            loss = model(*args_in)
            assert np.array_equal(loss.detach().numpy(), ref_l)
            red = loss.mean(0) if how == "mean" else (loss.sum() if how == "sum" else (loss * torch.from_numpy(w)).sum())
            red.backward()
            for k, p in model.named_parameters():
                if k == "gamma.gamma":
                    assert p.grad is None
                    continue
                want = ref[k] if scale is None else ref[k] * np.float32(scale)
                assert rel_err(p.grad.numpy(), want) < TOL, (how, k)
    finally:
        model.engine.close()


def test_train_epoch_vs_reference_then_eval(golden, monkeypatch):
    """Two train_epoch iterations (gradient_clipping with the Queue seeded at 3000, AdamW amsgrad) match the reference's
    losses and grad norms (g27_edm_train); val_epoch afterwards runs the eval-mode NLL; eval NLL and sample() on the trained
    handle (stale images reloaded) equal those of a fresh model built from state_dict(), bit for bit."""
    import torch
    from gaudi_amd import train_edm
    from gaudi_amd.models_edm import GaudiError
    g = golden("g27_edm_train")
    cfg = json.loads(str(g["train_cfg"]))
    args = synth.edm_args(dataset=cfg["dataset"], **cfg["over"])
    sd = synth.synth_edm_state_dict(args, 1, seed=cfg["wseed"], amplify_coord=cfg["amp"])
    model = _model(args, sd)
    fresh = None
    try:
        opt = torch.optim.AdamW(model.parameters(), lr=cfg["lr"], amsgrad=True, weight_decay=1e-12)
        q = train_edm.Queue(max_len=50)
        q.add(3000)
        x, h, nm, em = g["train_x"], g["train_h"], g["train_node_mask"], g["train_edge_mask"]
        B, N = x.shape[0], x.shape[1]
        loader = [(x, nm.reshape(B, N), em.reshape(B, N, N), h, None)]
        losses, norms = [], []
        for it in range(2):
            _fixed_t(monkeypatch, g["train_t_int"][it], cfg["T"])
            model.injected_noise = g["train_noise"][it][None]
            lo, gn = train_edm.train_epoch(it, model, loader, opt, {"clip_grad": True}, None, q)
            losses += lo
            norms += gn
        np.testing.assert_allclose(losses, g["train_loss"], rtol=1e-5)
        np.testing.assert_allclose(norms, g["train_grad_norm"], rtol=1e-5)
        for k, p in model.named_parameters():
            if k.startswith("dynamics."):
                assert rel_err(p.detach().numpy(), g["train_w:" + k]) < TOL, k
        monkeypatch.undo()
        model.injected_noise = None
        model.seed, model.sample_offset = 5, 0
        torch.manual_seed(3)
        v = train_edm.val_epoch("val", 0, model, None, None, loader, {})
        assert model.training is False and np.isfinite(v)
        fresh = _model(args, {k: t.numpy() for k, t in model.state_dict().items()})
        fresh.seed, fresh.sample_offset = 5, 0
        torch.manual_seed(3)
        assert train_edm.val_epoch("val", 0, fresh, None, None, loader, {}) == v
        noise = np.random.default_rng(3).standard_normal((cfg["T"] + 2, B, N, 4)).astype(np.float32)
        nm2, em2 = nm.reshape(B, N), em.reshape(B, N, N)
        xa, ha, _ = model.engine.sample(nm2, em2, noise=noise)
        xb, hb, _ = fresh.engine.sample(nm2, em2, noise=noise)
        assert np.array_equal(xa, xb) and np.array_equal(ha, hb)
        model.train()
        hd = {"categorical": torch.from_numpy(h), "integer": torch.zeros(0)}
        with pytest.raises(GaudiError, match="context"):
            model(torch.from_numpy(x), hd, torch.from_numpy(nm), torch.from_numpy(em), context=torch.zeros(1))
    finally:
        model.engine.close()
        if fresh is not None:
            fresh.engine.close()


def test_model_refuses_unknown_loss_type(golden):
    from gaudi_amd.models_edm import GaudiError
    g, args, sd, inp = _case(golden, "cata_mixed")
    model = _model(dict(args, diffusion_loss_type="nll"), sd)
    try:
        with pytest.raises(GaudiError, match="l2"):
            model.train()
    finally:
        model.engine.close()
