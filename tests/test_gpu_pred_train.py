"""GPU tests of predictor training (gaudi_predictor_loss_grad / Engine.predictor_loss_grad / CondPredictor training):
gradients against the reference's compute_loss + loss.backward() (g26), the forward it shares with predict_noised,
determinism, batch additivity, rotation invariance, central differences and two AdamW steps of train_epoch."""
import json

import numpy as np
import pytest

from tests.helpers import TINY, edm_from_cfg, pred_from_cfg, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _proj_summary(g, seed):
    """tools/make_golden.py:_proj_summary."""
    g = np.asarray(g, np.float64).reshape(-1)
    r = np.random.Generator(np.random.Philox(key=seed))
    proj = r.standard_normal((8, g.size))
    idx = r.integers(0, g.size, 64)
    return np.concatenate([[g.sum(), (g * g).sum()], proj @ g, g[idx]])


def _fixture(golden, name):
    return golden({"hetro": "g26_pred_grad_hetro", "plain": "g26_pred_grad_plain"}.get(name, "g26_pred_grad"))


def _models(cfg):
    from gaudi_amd.models_edm import get_cond_predictor_model, get_model
    eargs, esd = edm_from_cfg(dict(dataset=cfg["dataset"], over=TINY, wseed=cfg["eseed"], amp=False))
    pargs, psd = pred_from_cfg(dict(dataset=cfg["dataset"], over=cfg["over"], wseed=cfg["pseed"], amp=True))
    model, _, _ = get_model(eargs, state_dict=esd)
    pred = get_cond_predictor_model(pargs, model=model, state_dict=psd)
    return model, pred, pargs, psd


def _inputs(g, name):
    return tuple(g[f"{name}_{k}"] for k in ("x", "h", "node_mask", "edge_mask"))


def _masks2(nm, em):
    B, N = nm.shape[0], nm.shape[1]
    return nm.reshape(B, N), em.reshape(B, N, N)


@pytest.mark.parametrize("name", ["cata", "hetro", "plain", "full"])
def test_gradients_vs_reference(golden, name):
    g = _fixture(golden, name)
    cfg = json.loads(str(g[name + "_cfg"]))
    model, pred, _, _ = _models(cfg)
    x, h, nm, em = _inputs(g, name)
    nm2, em2 = _masks2(nm, em)
    names = cfg["names"]
    for tag in cfg["tags"]:
        k = f"{name}_{tag}"
        loss, p, grads = model.engine.predictor_loss_grad(x, h, g[k + "_t_int"], nm2, em2, g[k + "_y"], noise=g[k + "_eps"])
        assert abs(loss - float(g[k + "_loss"])) <= 1e-5 * abs(float(g[k + "_loss"])), (tag, loss, g[k + "_loss"])
        nograd = set(json.loads(str(g[k + "_nograd"])))
        assert {n for n, v in grads.items() if v is None} == nograd, tag
        assert set(grads) == set(names)
        for n in names:
            if n in nograd:
                continue
            if name == "full":
                got = _proj_summary(grads[n], 2650 + names.index(n))
                ref = g[f"{k}_sum.{n}"]
                assert rel_err(got, ref) < TOL, (tag, n, rel_err(got, ref))
            else:
                assert rel_err(grads[n], g[f"{k}_g.{n}"]) < TOL, (tag, n, rel_err(grads[n], g[f"{k}_g.{n}"]))
    model.engine.close()


def test_same_forward_deterministic_and_additive(golden):
    """pred equals predict_noised's (same launch); two calls are bit-identical; |A u B| g(A u B) = |A| g(A) + |B| g(B)."""
    gc, gh = golden("g26_pred_grad"), golden("g26_pred_grad_hetro")
    cfg = json.loads(str(gh["hetro_cfg"]))
    model, pred, _, _ = _models(cfg)
    x, h, nm, em = _inputs(gh, "hetro")
    nm2, em2 = _masks2(nm, em)
    k = "hetro_tT"
    ti, y, eps = gh[k + "_t_int"], gh[k + "_y"], gh[k + "_eps"]
    loss, p, g1 = model.engine.predictor_loss_grad(x, h, ti, nm2, em2, y, noise=eps)
    _, p_ref = model.engine.predict_noised(x, h, ti, nm2, em2, noise=eps)
    assert np.array_equal(p, p_ref)
    _, p2, g2 = model.engine.predictor_loss_grad(x, h, ti, nm2, em2, y, noise=eps)
    assert np.array_equal(p, p2)
    for n in g1:
        assert (g1[n] is None) == (g2[n] is None)
        if g1[n] is not None:
            assert np.array_equal(g1[n], g2[n]), n
    # additivity: A = the largest hetero molecule (many edge tiles) + one more, B = the rest
    B = x.shape[0]
    live = nm2.sum(1)
    a = sorted(np.argsort(-live)[:2].tolist())
    b = [i for i in range(B) if i not in a]
    parts = []
    for idx in (a, b):
        _, _, gp = model.engine.predictor_loss_grad(x[idx], h[idx], ti[idx], nm2[idx], em2[idx], y[idx], noise=eps[idx])
        parts.append(gp)
    for n in g1:
        if g1[n] is None:
            assert parts[0][n] is None and parts[1][n] is None
            continue
        comb = (len(a) * parts[0][n].astype(np.float64) + len(b) * parts[1][n].astype(np.float64)) / B
        scale = max(np.abs(g1[n]).max(), 1e-30)
        assert np.abs(comb - g1[n]).max() <= 1e-5 * scale, n
    model.engine.close()
    del gc


def test_rotation_invariance(golden):
    g = golden("g26_pred_grad")
    cfg = json.loads(str(g["cata_cfg"]))
    model, pred, _, _ = _models(cfg)
    x, h, nm, em = _inputs(g, "cata")
    nm2, em2 = _masks2(nm, em)
    k = "cata_tmix"
    ti, y, eps = g[k + "_t_int"], g[k + "_y"], g[k + "_eps"]
    _, _, g0 = model.engine.predictor_loss_grad(x, h, ti, nm2, em2, y, noise=eps)
    q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))
    q = q.astype(np.float32)
    xr = (x @ q.T).astype(np.float32)
    er = eps.copy()
    er[:, :, :3] = eps[:, :, :3] @ q.T
    _, _, g1 = model.engine.predictor_loss_grad(xr, h, ti, nm2, em2, y, noise=er)
    for n in g0:
        if g0[n] is not None:
            assert rel_err(g1[n], g0[n]) < TOL, (n, rel_err(g1[n], g0[n]))
    model.engine.close()


def test_central_differences(golden):
    """A few scalars against the loss through predict_noised (the forward of the same launch)."""
    g = golden("g26_pred_grad")
    cfg = json.loads(str(g["cata_cfg"]))
    model, pred, pargs, psd = _models(cfg)
    x, h, nm, em = _inputs(g, "cata")
    nm2, em2 = _masks2(nm, em)
    k = "cata_tmix"
    ti, y, eps = g[k + "_t_int"], g[k + "_y"], g[k + "_eps"]
    _, _, grads = model.engine.predictor_loss_grad(x, h, ti, nm2, em2, y, noise=eps)
    picks = [("egnn.gcl_0.att_mlp.0.bias", (0,)), ("egnn.embedding.weight", (3, 1)), ("egnn.embedding_out.bias", (2,)),
             ("egnn.gcl_1.coord_mlp.0.weight", (5, 7))]
    for n, ix in picks:
        hstep = 1e-2 * max(1.0, abs(float(psd[n][ix])))
        vals = []
        for s in (1, -1):
            sd = {kk: v.copy() for kk, v in psd.items()}
            sd[n][ix] += s * hstep
            model.engine.load_predictor(pargs, sd)
            _, p = model.engine.predict_noised(x, h, ti, nm2, em2, noise=eps)
            vals.append(np.abs(p.astype(np.float64) - y).mean())
        fd = (vals[0] - vals[1]) / (2 * hstep)
        an = float(grads[n][ix])
        assert abs(fd - an) <= 2e-2 * max(abs(an), 1e-3), (n, fd, an)
    model.engine.close()


def test_train_epoch_adamw_two_steps(golden):
    import torch
    from gaudi_amd import cond_prediction as cp
    from gaudi_amd.models_edm import get_cond_predictor_model, get_model
    g = golden("g26_pred_grad")
    cfg = json.loads(str(g["cata_cfg"]))
    model, pred, pargs, psd = _models(cfg)
    model.seed, model.sample_offset = 11, 0  # the noise is injected; next_stream must not draw from the patched randint
    x, h, nm, em = _inputs(g, "cata")
    nm2, em2 = _masks2(nm, em)
    B = x.shape[0]
    opt = torch.optim.AdamW(pred.parameters(), lr=float(g["adam_lr"]), amsgrad=True, weight_decay=1e-12)
    names = dict(pred.named_parameters())
    assert set(names) == set(psd)
    losses = []
    randint0 = torch.randint
    try:
        for step in range(2):
            ti = g[f"adam_{step}_t_int"]
            torch.randint = lambda low, high, size, device=None, **kw: torch.from_numpy(ti.reshape(B, 1).astype(np.int64))
            pred.train()
            loss, _ = cp.compute_loss(pred, x, h, nm, em, g["adam_y"], model, None, noise=g[f"adam_{step}_eps"])
            opt.zero_grad()
            loss.backward()
            assert names["egnn.gcl_2.coord_mlp.0.weight"].grad is None
            assert names["egnn.gcl_1.coord_mlp.0.weight"].grad is not None
            opt.step()
            losses.append(loss.item())
    finally:
        torch.randint = randint0
    ref = g["adam_losses"]
    assert np.allclose(losses, ref, rtol=1e-5, atol=0), (losses, ref)
    # the trained handle and a fresh engine loaded with state_dict() compute the same numbers
    ti = g["cata_tmix_t_int"]
    _, p_trained = model.engine.predict_noised(x, h, ti, nm2, em2, noise=g["cata_tmix_eps"])
    eargs, esd = edm_from_cfg(dict(dataset="cata", over=TINY, wseed=cfg["eseed"], amp=False))
    m2, _, _ = get_model(eargs, state_dict=esd)
    get_cond_predictor_model(pargs, model=m2, state_dict={k: v.numpy() for k, v in pred.state_dict().items()})
    _, p_fresh = m2.engine.predict_noised(x, h, ti, nm2, em2, noise=g["cata_tmix_eps"])
    assert np.array_equal(p_trained, p_fresh)
    m2.engine.close()
    model.engine.close()


def test_train_epoch_lowers_loss_and_refusals(golden):
    import torch
    from gaudi_amd import cond_prediction as cp
    from gaudi_amd._lib import GaudiError
    g = golden("g26_pred_grad")
    cfg = json.loads(str(g["cata_cfg"]))
    model, pred, _, _ = _models(cfg)
    model.seed, model.sample_offset = 7, 0
    x, h, nm, em = _inputs(g, "cata")
    B = x.shape[0]
    y = g["adam_y"]

    class DS:
        std = np.ones(5, np.float32)

    class Loader(list):
        dataset = DS()

    torch.manual_seed(0)
    opt = torch.optim.AdamW(pred.parameters(), lr=1e-3, amsgrad=True, weight_decay=1e-12)
    loader = Loader([(x, nm[..., 0], em.reshape(B, -1), h, y)] * 4)
    first = cp.train_epoch(0, pred, model, loader, opt, None, None, None)
    for e in range(1, 5):
        last = cp.train_epoch(e, pred, model, loader, opt, None, None, None)
    assert np.mean(last) < np.mean(first)
    # refusal: more nodes than the training kernels take
    N = 130
    nmb = np.zeros((1, N), np.float32)
    nmb[0, :3] = 1
    emb = (nmb[:, :, None] * nmb[:, None, :] * (1 - np.eye(N, dtype=np.float32))).astype(np.float32)
    with pytest.raises(GaudiError, match="128 nodes"):
        model.engine.predictor_loss_grad(np.zeros((1, N, 3), np.float32), np.zeros((1, N, 1), np.float32), [5], nmb, emb,
                                         np.zeros((1, 5), np.float32), noise=np.zeros((1, N, 4), np.float32))
    model.engine.close()


@pytest.mark.parametrize("env", [dict(GAUDI_WAVES=4), dict(GAUDI_FORCE_GN=1), dict(GAUDI_EDGE_MATH="fp32")])
def test_every_kernel_family(golden, monkeypatch, env):
    """The gradient runs on its own kernels whatever family the forward launch takes (4-wave, V4G / V8G node buffers in
    global memory, fp32 edge math): every family is supported, and each matches the reference."""
    from gaudi_amd.engine import Engine
    g = golden("g26_pred_grad")
    cfg = json.loads(str(g["cata_cfg"]))
    eargs, esd = edm_from_cfg(dict(dataset="cata", over=TINY, wseed=cfg["eseed"], amp=False))
    pargs, psd = pred_from_cfg(dict(dataset="cata", over=cfg["over"], wseed=cfg["pseed"], amp=True))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    eng = Engine(0)  # the knobs are read once, by gaudi_create
    for k in env:
        monkeypatch.delenv(k)
    eng.load_edm(eargs, esd)
    eng.load_predictor(pargs, psd)
    x, h, nm, em = _inputs(g, "cata")
    nm2, em2 = _masks2(nm, em)
    for tag in cfg["tags"]:
        k = f"cata_{tag}"
        loss, p, grads = eng.predictor_loss_grad(x, h, g[k + "_t_int"], nm2, em2, g[k + "_y"], noise=g[k + "_eps"])
        _, p_ref = eng.predict_noised(x, h, g[k + "_t_int"], nm2, em2, noise=g[k + "_eps"])
        assert np.array_equal(p, p_ref)
        assert abs(loss - float(g[k + "_loss"])) <= 1e-5 * abs(float(g[k + "_loss"])), (tag, loss)
        for n, v in grads.items():
            if v is not None:
                assert rel_err(v, g[f"{k}_g.{n}"]) < TOL, (tag, n)
    eng.close()


def test_val_epoch_after_train_epoch_is_forward_only(golden, monkeypatch):
    """train_epoch leaves the predictor in train mode; val_epoch switches it back (eval_cond_predictor.py:35) and runs
    the forward-only path, as does compute_loss after eval()."""
    import torch
    from gaudi_amd import cond_prediction as cp
    g = golden("g26_pred_grad")
    cfg = json.loads(str(g["cata_cfg"]))
    model, pred, _, _ = _models(cfg)
    model.seed, model.sample_offset = 5, 0
    x, h, nm, em = _inputs(g, "cata")
    B = x.shape[0]

    class DS:
        std = np.ones(5, np.float32)

    class Loader(list):
        dataset = DS()

    loader = Loader([(x, nm[..., 0], em.reshape(B, -1), h, g["adam_y"])])
    opt = torch.optim.AdamW(pred.parameters(), lr=1e-3, amsgrad=True, weight_decay=1e-12)
    cp.train_epoch(0, pred, model, loader, opt, None, None, None)
    assert pred.training

    def refuse(*a, **kw):
        raise AssertionError("the reverse pass ran during evaluation")

    monkeypatch.setattr(model.engine, "predictor_loss_grad", refuse)
    cp.val_epoch("val", pred, model, loader, None, None)
    assert not pred.training
    loss, _ = cp.compute_loss(pred, x, h, nm, em, g["adam_y"], model, None, t_fix=500)
    assert not loss.requires_grad
    pred.train()
    assert pred.training and not pred.eval().training
    model.engine.close()
