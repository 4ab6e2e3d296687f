"""oracle/train_oracle.py (the torch restatement of the two training losses, differentiated by autograd) against the reference's
own numbers -- every case of golden g27 (EDM: model.double(), loss.sum().backward(); its float32 loss) and g26 (predictor: the
float32 compute_loss + backward) -- and, for every case of tests/train_shapes.py, the conditions that make the GPU comparison
of tests/test_gpu_train_shapes.py meaningful.  Those involve the oracle alone, so they are checked here, without a device.

Bars: 1e-9 where the fixture holds float64 from the float64 run (loss64, net, the default case's projection records), 1e-6
(rel_err) for float64 gradients stored as float32, 1e-4 where the fixture is the reference's float32 run."""
import json

import numpy as np
import pytest
import torch

from gaudi_amd import synth
from oracle import train_oracle as TO
from tests import train_shapes as TS
from tests.helpers import TINY, edm_from_cfg, pred_from_cfg, rel_err

G27 = {"cata_mixed": "g27_edm_grad", "cata_t0": "g27_edm_grad", "cata_vlb": "g27_edm_grad",
       "hetro_500_T": "g27_edm_grad_hetro", "plain_mean": "g27_edm_grad_hetro", "cata_sin": "g27_edm_grad_hetro",
       "cata_default": "g27_edm_grad_default"}
G26 = {"cata": "g26_pred_grad", "hetro": "g26_pred_grad_hetro", "plain": "g26_pred_grad_plain", "full": "g26_pred_grad"}


def _proj_summary(g, seed):
    """tools/make_golden.py:_proj_summary."""
    g = np.asarray(g, np.float64).reshape(-1)
    r = np.random.Generator(np.random.Philox(key=seed))
    proj = r.standard_normal((8, g.size))
    idx = r.integers(0, g.size, 64)
    return np.concatenate([[g.sum(), (g * g).sum()], proj @ g, g[idx]])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize("name", list(G27))
def test_edm_oracle_vs_reference(golden, name):
    g = golden(G27[name])
    cfg = json.loads(str(g[name + "_cfg"]))
    args = synth.edm_args(dataset=cfg["dataset"], **cfg["over"])
    sd = synth.synth_edm_state_dict(args, synth.num_node_features(cfg["dataset"]), seed=cfg["wseed"], amplify_coord=cfg["amp"])
    x, h, t_int, noise = (g[f"{name}_{k}"] for k in ("x", "h", "t_int", "noise"))
    B, N = x.shape[:2]
    nm, em = g[name + "_node_mask"].reshape(B, N), g[name + "_edge_mask"].reshape(B, N, N)
    lt = args.get("diffusion_loss_type", "l2")
    aux = {}
    loss, net, grads = TO.edm_train(sd, args, x, h, t_int, nm, em, noise, loss_type=lt, aux=aux)
    assert _rel(loss, g[name + "_loss64"]) < 1e-9, (loss, g[name + "_loss64"])
    assert rel_err(net, g[name + "_net"]) < 1e-9
    assert rel_err(aux["z_t"], g[name + "_zt"]) < 1e-6  # (stored as float32)
    params = json.loads(str(g[name + "_params"]))
    nograd = set(json.loads(str(g[name + "_nograd"])))
    assert nograd == {"gamma.gamma"}  # (not in the synthetic state dict: the table is rebuilt from the schedule's name)
    assert {k for k, v in grads.items() if v is None} == {"buffer"} and set(grads) == set(sd)
    for pi, n in enumerate(params):
        if n in nograd:
            continue
        if name == "cata_default":  # float64 records of the float64 run
            err = rel_err(_proj_summary(grads[n], 2790 + pi), g[f"{name}_gsum:{n}"])
            assert err < 1e-9, (n, err)
        else:  # float64 gradients stored as float32
            err = rel_err(grads[n], g[f"{name}_grad:{n}"])
            assert err < 1e-6, (n, err)
    # the reference's float32 run: its loss everywhere; net and gradients where the fixture keeps them (sin_embedding)
    loss32, net32, grads32 = TO.edm_train(sd, args, x, h, t_int, nm, em, noise, loss_type=lt, dtype=torch.float32)
    assert _rel(loss32, g[name + "_loss"]) < 1e-4, (loss32, g[name + "_loss"])
    if name + "_net32" in g:
        # sinusoids of up to 429 sqrt(r) turn one float32 rounding of r into ~1e-4 rad of phase: two float32 runs agree no
        # better than either does with the exact one, which is what tests/test_gpu_edm_train.py's rule allows the kernels
        spread = max(rel_err(g[f"{name}_grad32:{n}"], g[f"{name}_grad:{n}"]) for n in params if n not in nograd)
        tol = max(1e-4, 2 * spread)
        assert rel_err(net32, g[name + "_net32"]) < max(1e-4, 2 * rel_err(g[name + "_net32"], g[name + "_net"]))
        for n in params:
            if n not in nograd:
                assert rel_err(grads32[n], g[f"{name}_grad32:{n}"]) < tol, (n, rel_err(grads32[n], g[f"{name}_grad32:{n}"]), tol)


@pytest.mark.parametrize("name", list(G26))
def test_pred_oracle_vs_reference(golden, name):
    """g26 is the reference's float32 run throughout: both precisions of the oracle are held to it at 1e-4 (loss: 1e-5, the bar
    the kernels get)."""
    g = golden(G26[name])
    cfg = json.loads(str(g[name + "_cfg"]))
    eargs, _ = edm_from_cfg(dict(dataset=cfg["dataset"], over=TINY, wseed=cfg["eseed"], amp=False))
    pargs, psd = pred_from_cfg(dict(dataset=cfg["dataset"], over=cfg["over"], wseed=cfg["pseed"], amp=True))
    x, h = g[name + "_x"], g[name + "_h"]
    B, N = x.shape[:2]
    nm, em = g[name + "_node_mask"].reshape(B, N), g[name + "_edge_mask"].reshape(B, N, N)
    names = cfg["names"]
    for tag in cfg["tags"]:
        k = f"{name}_{tag}"
        nograd = set(json.loads(str(g[k + "_nograd"])))
        for dtype in (torch.float64, torch.float32):
            loss, pred, grads = TO.pred_train(eargs, psd, pargs, x, h, g[k + "_t_int"], nm, em, g[k + "_y"], g[k + "_eps"],
                                              dtype=dtype)
            assert abs(loss - float(g[k + "_loss"])) <= 1e-5 * abs(float(g[k + "_loss"])), (tag, dtype, loss, g[k + "_loss"])
            assert {n for n, v in grads.items() if v is None} == nograd and set(grads) == set(names), (tag, dtype)
            for n in names:
                if n in nograd:
                    continue
                if name == "full":
                    got, ref = _proj_summary(grads[n], 2650 + names.index(n)), g[f"{k}_sum.{n}"]
                else:
                    got, ref = grads[n], g[f"{k}_g.{n}"]
                assert rel_err(got, ref) < 1e-4, (tag, dtype, n, rel_err(got, ref))


# ---- the GPU cases: what the oracle alone can say about them

SPREAD_MAX = 5e-5  # (leaves the kernels' bar at 1e-4 = twice the oracle's own float32 error)
ZERO_WITHOUT_EDGES = ("edge_mlp.", "att_mlp.", "coord_mlp.")


@pytest.mark.parametrize("name", list(TS.BY_NAME))
def test_gpu_case_is_meaningful(name):
    case = TS.BY_NAME[name]
    ref = TS.reference(name)
    worst = max(ref.spread, key=ref.spread.get)
    print(f"{name}: spread {ref.spread[worst]:.2e} ({worst}) loss {np.asarray(ref.loss).reshape(-1)[:4]}")
    # spread
    sin = bool(case.edm.get("sin_embedding")) and case.net == "edm"
    if not sin:
        assert ref.spread[worst] <= SPREAD_MAX, (worst, ref.spread[worst])
    # live gradients
    assert np.all(np.isfinite(ref.loss)) and np.all(np.isfinite(ref.out))
    sd = TS.models(case)[1 if case.net == "edm" else 3]
    assert set(ref.grads) == set(sd)
    live = 0
    for n, v in ref.grads.items():
        if v is None:
            continue
        if case.no_edges and any(s in n for s in ZERO_WITHOUT_EDGES):
            assert not np.any(v), n  # no live edge: exact zeros, in the oracle too
        else:
            assert np.abs(v).max() > 0, n
            live += 1
    assert live >= 4
    L = case.pred["n_layers"]
    none = {n for n, v in ref.grads.items() if v is None}
    if case.net == "pred":
        assert none == {n for n in sd if n.startswith(f"egnn.gcl_{L - 1}.coord_mlp.")}
    else:
        assert none == {"buffer"}
    # no saturated coordinate head
    em = TS.inputs(case)["edge_mask"].astype(bool)
    for th in ref.tanh:
        if em.any():
            assert np.mean(np.abs(th[..., 0][em]) > 0.999) < 0.5
    # the predictor's L1 sign margin
    if case.net == "pred":
        assert np.all(np.abs(ref.out - ref.y) >= 1e-2 * np.maximum(1.0, np.abs(ref.out)))
        assert np.array_equal(np.sign(ref.out32 - ref.y), np.sign(ref.out - ref.y))


def test_case_table_reaches_what_it_claims():
    """The arithmetic the shapes were chosen by (csrc/train_device.h: mm_rows stages 16 rows per round on 256 threads;
    pt_outer_kernel gives each of four waves per = ceil(R / 16) * 4 rows)."""
    c = TS.BY_NAME
    assert c["edm_n16"].N ** 2 == 256 and c["edm_n17"].N ** 2 == 289 and c["edm_n128"].N ** 2 == 16384
    assert c["edm_n16"].N * len(c["edm_n16"].live) == 16 and (c["edm_n17"].N * len(c["edm_n17"].live)) % 16 == 2
    assert c["edm_n33"].N % 16 == 1
    per = -(-33 // 16) * 4
    assert [max(0, min(per, 33 - w * per)) for w in range(4)] == [12, 12, 9, 0]
    assert c["pred_nmax"].N == c["pred_nmax_l1"].N == TS.PRED_NMAX
    assert len(c["edm_rows"].live) * 400 == 25600 and len(c["edm_n128"].live) * 16384 == 32768
    assert c["edm_h256"].edm["nf"] == 256 and 250 % 32 == 26 and c["pred_h20_hetro"].pred["nf"] == 20
    for name in ("edm_chunks", "pred_chunks"):
        assert len(c[name].live) == 5 and TS.chunk_of(c[name], TS.knob_kb(c[name], 2)) == 2
        assert TS.chunk_of(c[name], 1 << 20) == 5  # the default, 1 GiB: one chunk
