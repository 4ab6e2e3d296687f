#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE (read-only, /root/reference) on CPU.

Runs only in the build container (the GPU box has no /root/reference).  Nothing from the
reference is copied: it is imported, fed seeded synthetic weights (gaudi_amd.synth) and
injected noise, and only numeric inputs/outputs are stored.  Recipe = SURVEY.md Appendix A.

    python tools/make_golden.py            # rewrites every fixture
"""
import copy
import json
import os
import sys
from unittest.mock import MagicMock

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
for m in ["rdkit", "rdkit.Chem", "rdkit.Chem.Draw", "rdkit.Chem.rdmolops", "rdkit.Chem.rdchem",
          "rdkit.Chem.AllChem", "imageio", "torch.utils.tensorboard"]:
    sys.modules[m] = MagicMock()

import torch  # noqa: E402

import models_edm  # noqa: E402  (reference)
import sampling_edm as ref_sampling  # noqa: E402  (reference)
from cond_prediction.train_cond_predictor import get_cond_predictor_model  # noqa: E402
from cond_prediction.prediction_args import PredictionArgs  # noqa: E402
from utils.args_edm import Args_EDM  # noqa: E402
from utils.helpers import switch_grad_off  # noqa: E402

from gaudi_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)
torch.set_num_threads(8)
META = dict(torch=torch.__version__, numpy=np.__version__, threads=torch.get_num_threads())


class FakeDataset:
    def __init__(self, F, K):
        self.num_node_features = F
        self.num_targets = K
        self.mean = torch.zeros(K)
        self.std = torch.ones(K)


class FakeLoader:
    def __init__(self, F, K):
        self.dataset = FakeDataset(F, K)


class InjectNoise:
    """Replace torch.randn by a queue of pre-drawn tensors (call order: x-noise then h-noise)."""

    def __init__(self, eps_list, dtype=None):
        # eps_list: list of [B,N,3+F] arrays, one per sample_combined_position_feature_noise call
        self.q = []
        for e in eps_list:
            e = torch.from_numpy(np.ascontiguousarray(e))
            if dtype is not None:
                e = e.to(dtype)
            self.q.append(e[:, :, :3].contiguous())
            self.q.append(e[:, :, 3:].contiguous())
        self.orig = None

    def __enter__(self):
        self.orig = torch.randn

        def fake(size, device=None, **kw):
            t = self.q.pop(0)
            assert tuple(t.shape) == tuple(size), (t.shape, size)
            return t.clone()

        torch.randn = fake
        return self

    def __exit__(self, *a):
        torch.randn = self.orig
        assert not self.q, f"{len(self.q)} injected tensors unused"


def build_ref_edm(dataset, sd_np, **over):
    a = Args_EDM().parse_args([])
    a.device = torch.device("cpu")
    a.dp = False
    a.restore = None
    a.dataset = dataset
    for k, v in over.items():
        setattr(a, k, v)
    F = synth.num_node_features(dataset)
    model, _, prop = models_edm.get_model(a, FakeLoader(F, 5), only_norm=True)
    full = model.state_dict()
    for k, v in sd_np.items():
        assert k in full and tuple(full[k].shape) == v.shape, k
        full[k] = torch.from_numpy(v.copy())
    model.load_state_dict(full)
    switch_grad_off([model])
    return a, model


def build_ref_pred(dataset, sd_np, K=5, **over):
    a = PredictionArgs().parse_args([])
    a.device = torch.device("cpu")
    a.dp = False
    a.restore = None
    a.dataset = dataset
    for k, v in over.items():
        setattr(a, k, v)
    F = synth.num_node_features(dataset)
    pred = get_cond_predictor_model(a, FakeDataset(F, K))
    full = pred.state_dict()
    assert set(full.keys()) == set(sd_np.keys()), set(full.keys()) ^ set(sd_np.keys())
    pred.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()})
    switch_grad_off([pred])
    return a, pred


def masks(dataset, nodesxsample, max_nodes):
    """Reference mask construction, run through the reference's own code by calling
    sample_guidance / sample_pos_edm with a recording fake model."""
    rec = {}

    class Rec:
        def sample(self, B, n_nodes, node_mask, edge_mask, std=1.0):
            rec.update(node_mask=node_mask.numpy().copy(), edge_mask=edge_mask.numpy().copy())
            x = torch.zeros(B, n_nodes, 3)
            return x, {"categorical": torch.zeros(B, n_nodes, 1)}

        def sample_guidance(self, B, tf, node_mask, edge_mask, scale, fix_noise=False, std=1.0):
            rec.update(node_mask=node_mask.numpy().copy(), edge_mask=edge_mask.numpy().copy())
            x = torch.zeros(B, node_mask.shape[1], 3)
            return x, {"categorical": torch.zeros(B, node_mask.shape[1], 1)}

    class A:
        pass

    a = A()
    a.device = torch.device("cpu")
    a.dataset = dataset
    a.max_nodes = max_nodes
    n = torch.tensor(nodesxsample).long()
    if max_nodes is None:
        ref_sampling.sample_guidance(a, Rec(), None, n)
    else:
        ref_sampling.sample_pos_edm(a, Rec(), n)
    return rec["node_mask"], rec["edge_mask"]


def rng_noise(seed, shape):
    return np.random.Generator(np.random.Philox(key=seed)).standard_normal(shape).astype(np.float32)


def save(name, **arrs):
    arrs["meta"] = np.array(json.dumps(META))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


# --------------------------------------------------------------------------------------
def g1_schedule():
    out = {}
    for T in (50, 1000):
        sd = synth.synth_edm_state_dict(synth.edm_args(nf=8, n_layers=1), 1, seed=0)
        a, model = build_ref_edm("cata", sd, nf=8, n_layers=1, diffusion_steps=T)
        gamma = model.gamma.gamma.numpy().copy()
        out[f"gamma_T{T}"] = gamma
        rows = []
        for s in ([0, 1, T // 2, T - 2, T - 1]):
            st = torch.full((1, 1), s) / T
            tt = (torch.full((1, 1), s) + 1) / T
            gs, gt = model.gamma(st), model.gamma(tt)
            zt = torch.zeros(1, 1, 1)
            s2, s_ts, a_ts = model.sigma_and_alpha_t_given_s(gt, gs, zt)
            sig_s, sig_t = model.sigma(gs, zt), model.sigma(gt, zt)
            rows.append([s, a_ts.item(), s2.item(), (s2 / a_ts / sig_t).item(), (s_ts * sig_s / sig_t).item(),
                         sig_s.item(), sig_t.item(), tt.item()])
        out[f"coef_T{T}"] = np.array(rows, dtype=np.float64)
    save("g1_schedule", **out)


def g2_masks():
    out = {}
    nm, em = masks("cata", [4, 11, 7, 1], 11)
    out["cata_n"] = np.array([4, 11, 7, 1])
    out["cata_node_mask"], out["cata_edge_mask"] = nm, em
    nm, em = masks("hetro", [3, 5, 10, 7], 10)
    out["hetro_pos_n"] = np.array([3, 5, 10, 7])
    out["hetro_pos_node_mask"], out["hetro_pos_edge_mask"] = nm, em
    nm, em = masks("hetro", [3, 5, 9, 7], None)  # sample_guidance pads to batch max (9 -> N=18)
    out["hetro_guid_n"] = np.array([3, 5, 9, 7])
    out["hetro_guid_node_mask"], out["hetro_guid_edge_mask"] = nm, em
    nm, em = masks("cata", [6, 8, 8], None)
    out["cata_guid_n"] = np.array([6, 8, 8])
    out["cata_guid_node_mask"], out["cata_guid_edge_mask"] = nm, em
    save("g2_masks", **out)


TINY = dict(nf=32, n_layers=2)
TINY_P = dict(nf=36, n_layers=3)  # 36: not a multiple of 16 -> exercises feature padding


def case_inputs(dataset, nodes, max_nodes, seed, guidance_pad=False):
    nm, em = masks(dataset, nodes, None if guidance_pad else max_nodes)
    B, N, _ = nm.shape
    F = synth.num_node_features(dataset)
    z = rng_noise(seed, (B, N, 3 + F)) * nm
    z[:, :, :3] -= (z[:, :, :3].sum(1, keepdims=True) / np.maximum(nm.sum(1, keepdims=True), 1)) * nm
    return nm, em, z.astype(np.float32)


def g3_phi():
    out = {}
    cases = [
        ("cata_tiny", "cata", [4, 11, 7, 1, 11], 11, TINY, False),
        ("cata_tiny_amp", "cata", [4, 11, 7, 2, 11], 11, TINY, True),
        ("hetro_tiny_amp", "hetro", [3, 5, 10, 7], 10, TINY, True),
        ("cata_tiny_sub2_amp", "cata", [5, 9, 11], 11, dict(nf=32, n_layers=2, inv_sublayers=2,
                                                            normalization_factor=3.0, norm_constant=0.5), True),
        ("cata_full", "cata", [11, 8, 11], 11, dict(nf=192, n_layers=9), False),
        ("hetro_full_amp", "hetro", [10, 6], 10, dict(nf=192, n_layers=9), True),
    ]
    for i, (name, ds, nodes, mx, over, amp) in enumerate(cases):
        F = synth.num_node_features(ds)
        args = synth.edm_args(dataset=ds, **over)
        sd = synth.synth_edm_state_dict(args, F, seed=100 + i, amplify_coord=amp)
        a, model = build_ref_edm(ds, sd, **over)
        nm, em, z = case_inputs(ds, nodes, mx, seed=200 + i)
        B = z.shape[0]
        t = np.linspace(0.05, 0.95, B).astype(np.float32).reshape(B, 1)
        with torch.no_grad():
            eps = model.phi(torch.from_numpy(z), torch.from_numpy(t), torch.from_numpy(nm),
                            torch.from_numpy(em), None).numpy()
        out[name + "_cfg"] = np.array(json.dumps(dict(dataset=ds, over=over, amp=amp, wseed=100 + i)))
        out[name + "_z"], out[name + "_t"] = z, t
        out[name + "_node_mask"], out[name + "_edge_mask"] = nm, em
        out[name + "_eps"] = eps
    save("g3_phi", **out)


TARGETS = {
    "gap": lambda pred, prop: -pred[:, 1],
    "opv": lambda pred, prop: (lambda u: u[:, 3] + u[:, 2] + 3 * u[:, 0])(pred * prop["std"] + prop["mean"]),
}


def g4_predictor():
    out = {}
    cases = [
        ("cata_tiny_amp", "cata", [4, 11, 7, 1, 11], 11, TINY_P, True, False),
        ("hetro_tiny_amp", "hetro", [3, 5, 9, 7], None, TINY_P, True, True),
        ("cata_full", "cata", [11, 9], 11, dict(nf=196, n_layers=12), False, False),
        ("hetro_full_amp", "hetro", [10, 4], 10, dict(nf=196, n_layers=12), True, False),
    ]
    prop = dict(mean=torch.tensor([0.3, -1.0, 0.5, 2.0, 0.1]), std=torch.tensor([1.5, 0.7, 2.0, 0.9, 1.1]))
    for i, (name, ds, nodes, mx, over, amp, gpad) in enumerate(cases):
        F = synth.num_node_features(ds)
        pargs = synth.pred_args(dataset=ds, **over)
        sd = synth.synth_predictor_state_dict(pargs, F, 5, seed=300 + i, amplify_coord=amp)
        a, pred = build_ref_pred(ds, sd, **over)
        nm, em, z = case_inputs(ds, nodes, mx, seed=400 + i, guidance_pad=gpad)
        B = z.shape[0]
        t = np.full((B, 1), 0.37, np.float32)
        zt = torch.from_numpy(z).requires_grad_()
        p = pred(zt, torch.from_numpy(nm), torch.from_numpy(em), torch.from_numpy(t))
        out[name + "_pred"] = p.detach().numpy()
        for tn, tf in TARGETS.items():
            energy = (0.6 * tf(p, prop)).sum()
            g = torch.autograd.grad(energy, zt, retain_graph=True)[0]
            out[f"{name}_grad_{tn}"] = g.numpy()
        out[name + "_cfg"] = np.array(json.dumps(dict(dataset=ds, over=over, amp=amp, wseed=300 + i)))
        out[name + "_z"], out[name + "_t"] = z, t
        out[name + "_node_mask"], out[name + "_edge_mask"] = nm, em
    out["prop_mean"], out["prop_std"] = prop["mean"].numpy(), prop["std"].numpy()
    out["scale"] = np.float32(0.6)
    save("g4_predictor", **out)


def g5_steps():
    """Teacher-forced reverse steps (unguided + guided) at several t, tiny configs."""
    out = {}
    T = 1000
    for ci, (name, ds, nodes) in enumerate([("cata", "cata", [4, 11, 7, 11]), ("hetro", "hetro", [3, 9, 6])]):
        F = synth.num_node_features(ds)
        eargs = synth.edm_args(dataset=ds, **TINY)
        esd = synth.synth_edm_state_dict(eargs, F, seed=500 + ci, amplify_coord=True)
        a, model = build_ref_edm(ds, esd, **TINY)
        pargs = synth.pred_args(dataset=ds, **TINY_P)
        psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=510 + ci, amplify_coord=True)
        pa, pred = build_ref_pred(ds, psd, **TINY_P)
        nm, em, z = case_inputs(ds, nodes, None, seed=520 + ci, guidance_pad=True)
        B, N, D = z.shape
        tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)

        def tf_gap(_in, _nm, _em, _t):
            return -pred(_in, _nm, _em, _t)[:, 1]

        out[f"{name}_z"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = z, nm, em
        for s in (0, 1, 500, 998, 999):
            eps = rng_noise(600 + 10 * ci + s % 7, (B, N, D))
            st = torch.full((B, 1), s) / T
            tt = (torch.full((B, 1), s) + 1) / T
            with InjectNoise([eps]), torch.no_grad():
                zs = model.sample_p_zs_given_zt(st, tt, torch.from_numpy(z), tnm, tem, None).numpy()
            out[f"{name}_s{s}_eps"] = eps
            out[f"{name}_s{s}_zs_unguided"] = zs
            for scale in (0.6, 400.0):  # 400: forces the ||g||>10 clip branch
                with InjectNoise([eps]), torch.no_grad():
                    zg = model.sample_p_zs_given_zt_guidance(st, tt, torch.from_numpy(z), tnm, tem, tf_gap,
                                                             scale).numpy()
                out[f"{name}_s{s}_zs_guided_scale{scale}"] = zg
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=500 + ci, pseed=510 + ci, T=T)))
    save("g5_steps", **out)


def g6_decode():
    out = {}
    for ci, (name, ds, nodes) in enumerate([("cata", "cata", [4, 11, 7]), ("hetro", "hetro", [3, 9, 6])]):
        F = synth.num_node_features(ds)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **TINY), F, seed=700 + ci, amplify_coord=True)
        a, model = build_ref_edm(ds, esd, **TINY)
        nm, em, z = case_inputs(ds, nodes, None, seed=720 + ci, guidance_pad=True)
        eps = rng_noise(730 + ci, z.shape)
        with InjectNoise([eps]), torch.no_grad():
            x, h = model.sample_p_xh_given_z0(torch.from_numpy(z), torch.from_numpy(nm), torch.from_numpy(em), None)
        out[f"{name}_z"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"], out[f"{name}_eps"] = z, nm, em, eps
        out[f"{name}_x"], out[f"{name}_h"] = x.numpy(), h["categorical"].numpy().astype(np.float32)
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=700 + ci)))
    save("g6_decode", **out)


def g7_end_to_end():
    """C1: cata, 4 rings padded to 11, B=8, T=50, unguided, default architecture and default
    init (+ tiny guided T=50 variants).  Entry points: the reference's sample_pos_edm /
    sample_guidance with torch.randn injected."""
    out = {}
    # --- C1 (full default architecture, default init, std=1.0)
    T = 50
    over = dict(diffusion_steps=T)
    eargs = synth.edm_args(**over)
    esd = synth.synth_edm_state_dict(eargs, 1, seed=0)
    a, model = build_ref_edm("cata", esd, **over)
    a.max_nodes = 11
    B, N, D = 8, 11, 4
    noise = rng_noise(1, (T + 2, B, N, D))
    with InjectNoise(list(noise)):
        x, h, nm, em = ref_sampling.sample_pos_edm(a, model, torch.tensor([4] * B), std=1.0)
    out["c1_noise"], out["c1_x"], out["c1_h"] = noise, x.numpy(), h.numpy().astype(np.float32)
    out["c1_node_mask"], out["c1_edge_mask"] = nm.numpy(), em.numpy()
    out["c1_cfg"] = np.array(json.dumps(dict(dataset="cata", T=T, eseed=0, nodes=[4] * B, std=1.0)))

    # --- tiny guided / unguided chains, amplified coordinate heads, T=50
    for ci, (name, ds, nodes, amp) in enumerate([("cata_tiny", "cata", [6, 8, 8, 3], False),
                                                 ("hetro_tiny", "hetro", [3, 5, 4], False),
                                                 ("cata_tiny_amp", "cata", [6, 8, 8, 3], True)]):
        F = synth.num_node_features(ds)
        over = dict(diffusion_steps=T, **TINY)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=800 + ci, amplify_coord=amp)
        a, model = build_ref_edm(ds, esd, **over)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=810 + ci,
                                               amplify_coord=amp)
        pa, pred = build_ref_pred(ds, psd, **TINY_P)

        def tf_gap(_in, _nm, _em, _t):
            return -pred(_in, _nm, _em, _t)[:, 1]

        n = torch.tensor(nodes)
        Nn = max(nodes) * (2 if ds != "cata" else 1)
        noise = rng_noise(820 + ci, (T + 2, len(nodes), Nn, 3 + F))
        with InjectNoise(list(noise)):
            x, h, nm, em = ref_sampling.sample_guidance(a, model, tf_gap, n, scale=0.6, std=1.0)
        out[f"{name}_noise"] = noise
        out[f"{name}_x_guided"], out[f"{name}_h_guided"] = x.numpy(), h.numpy().astype(np.float32)
        out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = nm.numpy(), em.numpy()
        a.max_nodes = max(nodes)
        with InjectNoise(list(noise)):
            x, h, nm2, em2 = ref_sampling.sample_pos_edm(a, model, n, std=0.7)
        assert np.array_equal(nm2.numpy(), nm.numpy())
        out[f"{name}_x_unguided"], out[f"{name}_h_unguided"] = x.numpy(), h.numpy().astype(np.float32)
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, T=T, eseed=800 + ci, pseed=810 + ci,
                                                      nodes=nodes, amp=amp)))
    save("g7_end_to_end", **out)


def g9_sample_chain():
    """EnVariationalDiffusion.sample_chain (keep_frames trajectory capture), tiny config, injected noise."""
    out = {}
    T, K = 50, 10
    for ci, (name, ds, nodes) in enumerate([("cata", "cata", [6, 8]), ("hetro", "hetro", [3, 5])]):
        F = synth.num_node_features(ds)
        over = dict(diffusion_steps=T, **TINY)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=900 + ci)
        a, model = build_ref_edm(ds, esd, **over)
        nm, em = masks(ds, nodes, None)
        B, N, _ = nm.shape
        noise = rng_noise(920 + ci, (T + 2, B, N, 3 + F))
        with InjectNoise(list(noise)):
            chain = model.sample_chain(B, N, torch.from_numpy(nm), torch.from_numpy(em), None, keep_frames=K, std=0.7)
        out[f"{name}_noise"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = noise, nm, em
        out[f"{name}_chain"] = chain.numpy()
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, T=T, K=K, eseed=900 + ci, nodes=nodes, amp=False, std=0.7)))
    save("g9_sample_chain", **out)


def nonlinear_target_torch(pred, t):
    """Golden nonlinear, time-dependent target (numpy twin with its analytic gradient: tests/helpers.py)."""
    return 0.5 * torch.log1p(pred[:, 1] ** 2) + 0.1 * torch.tanh(pred[:, 0]) * pred[:, 3] + t * pred[:, 2]


def g10_nonlinear_target():
    """Guidance with a target that is NOT linear in the predictor outputs: teacher-forced steps and a T=50 chain
    through the reference's sample_guidance (autograd through the closure, en_diffusion.py:899-903)."""
    out = {}
    ds, nodes = "hetro", [3, 5, 4]
    F = synth.num_node_features(ds)
    T = 1000
    esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **TINY), F, seed=900, amplify_coord=True)
    a, model = build_ref_edm(ds, esd, **TINY)
    psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=910, amplify_coord=True)
    pa, pred = build_ref_pred(ds, psd, **TINY_P)

    def tf(_in, _nm, _em, _t):
        return nonlinear_target_torch(pred(_in, _nm, _em, _t), _t.reshape(-1))

    nm, em, z = case_inputs(ds, nodes, None, seed=920, guidance_pad=True)
    B, N, D = z.shape
    tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
    out["z"], out["node_mask"], out["edge_mask"] = z, nm, em
    for s in (0, 500, 999):
        eps = rng_noise(930 + s % 7, (B, N, D))
        st = torch.full((B, 1), s) / T
        tt = (torch.full((B, 1), s) + 1) / T
        out[f"s{s}_eps"] = eps
        for scale in (0.6, 400.0):
            with InjectNoise([eps]), torch.no_grad():
                zg = model.sample_p_zs_given_zt_guidance(st, tt, torch.from_numpy(z), tnm, tem, tf, scale).numpy()
            out[f"s{s}_zs_scale{scale}"] = zg
    out["cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=900, pseed=910, T=T, nodes=nodes)))
    # chain, T=50
    Tc = 50
    over = dict(diffusion_steps=Tc, **TINY)
    esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=940, amplify_coord=False)
    a, model = build_ref_edm(ds, esd, **over)
    psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=950, amplify_coord=False)
    pa, pred = build_ref_pred(ds, psd, **TINY_P)
    noise = rng_noise(960, (Tc + 2, len(nodes), 2 * max(nodes), 3 + F))
    with InjectNoise(list(noise)):
        x, h, nm, em = ref_sampling.sample_guidance(a, model, tf, torch.tensor(nodes), scale=0.6, std=1.0)
    out["chain_noise"], out["chain_x"], out["chain_h"] = noise, x.numpy(), h.numpy().astype(np.float32)
    out["chain_node_mask"], out["chain_edge_mask"] = nm.numpy(), em.numpy()
    out["chain_cfg"] = np.array(json.dumps(dict(dataset=ds, T=Tc, eseed=940, pseed=950, nodes=nodes)))
    save("g10_nonlinear_target", **out)


def _rand_rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def synth_cata_molecule(rng, n, tree_prob, jitter, zjit):
    """Ring centres on a triangular lattice (spacing ~2.45): tree-like growth gives cata-condensed shapes, allowing
    lattice neighbours gives cycles (peri shapes, 60-degree triplets) -- a mix of stable / unstable molecules."""
    dirs = [(1, 0), (0, 1), (-1, 1), (-1, 0), (0, -1), (1, -1)]
    occ = [(0, 0)]
    tries = 0
    while len(occ) < n and tries < 1000:
        tries += 1
        a = occ[rng.integers(len(occ))]
        d = dirs[rng.integers(6)]
        c = (a[0] + d[0], a[1] + d[1])
        if c in occ:
            continue
        nb = sum(((c[0] + e[0], c[1] + e[1]) in occ) for e in dirs)
        if nb > 1 and rng.random() < tree_prob:
            continue
        occ.append(c)
    occ = np.array(occ, np.float64)
    d = rng.uniform(2.40, 2.50)
    xy = np.stack([occ[:, 0] + 0.5 * occ[:, 1], occ[:, 1] * np.sqrt(3) / 2], 1) * d
    x = np.concatenate([xy, np.zeros((len(occ), 1))], 1)
    x += rng.standard_normal(x.shape) * jitter
    x[:, 2] += rng.standard_normal(len(occ)) * zjit
    x = (x - x.mean(0)) @ _rand_rot(rng)
    return x.astype(np.float32)


def synth_hetro_molecule(rng, n, tables, jitter, corrupt):
    """Tree growth in the plane: bonded-distance windows and 3-ring angle windows of the reference's tables pick the
    bond length / direction, then jitter.  Orientation nodes (type '.') are appended; `corrupt` breaks them."""
    R = len(tables["rings"]["hetro"]) - 1
    lo, hi, a3 = tables["dist_lo"]["hetro"], tables["dist_hi"]["hetro"], tables["a3"]["hetro"]
    w = np.array([6, 1, 1, 1, 1, 1, 1, 1, 0.3, 1, 0.5])
    types = [int(rng.choice(R, p=w / w.sum()))]
    pos = [np.zeros(2)]
    heading = [rng.uniform(0, 2 * np.pi)]  # direction towards the parent (or arbitrary for the root)
    tries = 0
    while len(pos) < n and tries < 2000:
        tries += 1
        p = int(rng.integers(len(pos)))
        t = int(rng.choice(R, p=w / w.sum()))
        if hi[types[p]][t] <= 0:
            continue
        d = rng.uniform(lo[types[p]][t], hi[types[p]][t])
        wins = a3[types[p]] or [[120.0, 120.0]]
        win = wins[rng.integers(len(wins))]
        ang = np.deg2rad(rng.uniform(win[0], win[1])) * rng.choice([-1, 1])
        th = heading[p] + ang
        c = pos[p] + d * np.array([np.cos(th), np.sin(th)])
        if min(np.linalg.norm(c - q) for q in pos) < 1.3 and rng.random() < 0.9:
            continue
        pos.append(c)
        types.append(t)
        heading.append(th + np.pi)
    k = len(pos)
    x = np.concatenate([np.array(pos), np.zeros((k, 1))], 1)
    x += rng.standard_normal(x.shape) * jitter
    orient = x + rng.standard_normal(x.shape) * 0.5
    x = np.concatenate([x, orient], 0)
    x = (x - x.mean(0)) @ _rand_rot(rng)
    ty = np.array(types + [R] * k, np.int64)
    if corrupt == 1:
        ty[k + rng.integers(k)] = 0          # an orientation slot holds a real ring type
    elif corrupt == 2:
        ty[rng.integers(k)] = R              # a ring slot holds the orientation type
    return x.astype(np.float32), ty


def synth_hetro_fused(rng, n, tables, jitter):
    """A cata-condensed hetero molecule that could exist: ring templates grown edge to edge, only carbon-carbon edges are shared and
    no atom belongs to three rings, so the atoms gor2goa merges coincide (before the jitter) and the result does not depend on the
    order of the rings.  (synth_hetro_molecule above draws orientation nodes at random: fine for the stability check, but gor2goa
    gives a merged atom the element of the lower-index ring, and on such input its result changes with the ring order.)
    -> (x [2k,3] rings then orientation nodes, types [2k], fused pairs as a set of (i, j), i < j)."""
    G, names = tables["goa"], tables["rings"]["hetro"]
    R = len(names) - 1
    tm = [np.array(G["templates"][G["ring_template"][s]], np.float64) for s in names[:R]]
    el = [G["ring_atoms"][s] for s in names[:R]]
    w = np.array([6, 1, 1, 1, 1, 1, 1, 1, 0.3, 1, 0.5])
    rot = lambda a: np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    cc_edges = lambda t: [k for k in range(len(el[t])) if el[t][k] == "C" and el[t][(k + 1) % len(el[t])] == "C"]
    t0 = int(rng.choice(R, p=w / w.sum()))
    a0 = rng.uniform(0, 2 * np.pi)
    rings = [dict(t=t0, c=np.zeros(2), ang=a0, v=tm[t0] @ rot(a0).T, used=set())]
    pairs = set()
    tries = 0
    while len(rings) < n and tries < 4000:
        tries += 1
        p = int(rng.integers(len(rings)))
        P = rings[p]
        free = [k for k in cc_edges(P["t"]) if k not in P["used"] and (k + 1) % len(P["v"]) not in P["used"]]
        if not free:
            continue
        k = free[rng.integers(len(free))]
        A, B = P["v"][k], P["v"][(k + 1) % len(P["v"])]
        t = int(rng.choice(R, p=w / w.sum()))
        m = cc_edges(t)[rng.integers(len(cc_edges(t)))]
        a, b = tm[t][m], tm[t][(m + 1) % len(tm[t])]
        best = None
        for src, dst in (((a, b), (B, A)), ((a, b), (A, B))):
            ang = np.arctan2(*(dst[1] - dst[0])[::-1]) - np.arctan2(*(src[1] - src[0])[::-1])
            c = dst[0] - rot(ang) @ src[0]
            if np.linalg.norm(c - P["c"]) > np.linalg.norm((A + B) / 2 - P["c"]) + 0.3:
                best = (ang, c)
        if best is None:
            continue
        ang, c = best
        v = tm[t] @ rot(ang).T + c
        if any(np.linalg.norm(c - q["c"]) < 3.4 for i, q in enumerate(rings) if i != p):
            continue
        if any(np.linalg.norm(v[:, None] - q["v"][None], axis=-1).min() < 1.1 for i, q in enumerate(rings) if i != p):
            continue
        P["used"] |= {k, (k + 1) % len(P["v"])}
        rings.append(dict(t=t, c=c, ang=ang, v=v, used={m, (m + 1) % len(v)}))
        pairs.add((p, len(rings) - 1))
    k = len(rings)
    cen = np.array([q["c"] for q in rings])
    # the orientation node: on the template's +x axis (where the hetero atom sits); the centre itself for Bn / Cbd
    ori = np.array([q["c"] + (0 if names[q["t"]] in G["no_orientation"] else 1.3) * np.array([np.cos(q["ang"]), np.sin(q["ang"])])
                    for q in rings])
    x = np.concatenate([np.concatenate([cen, ori]), np.zeros((2 * k, 1))], 1)
    x += rng.standard_normal(x.shape) * jitter
    x = (x - x.mean(0)) @ _rand_rot(rng)
    return x.astype(np.float32), np.array([q["t"] for q in rings] + [R] * k, np.int64), pairs


def g11_stability():
    """Graph-of-rings stability check (analyze/analyze.py:50-100) on seeded synthetic molecules + a few degenerate
    ones; stores the reference's flags, distance matrix, adjacency and the sorted 3-ring / 4-ring angle lists."""
    from analyze import analyze as ref_an
    from utils import helpers as ref_h
    tables = json.load(open(os.path.join(ROOT, "gaudi_amd", "data", "ring_tables.json")))
    rng = np.random.default_rng(1100)
    out = {}
    for ds in ("cata", "hetro"):
        mols = []
        if ds == "cata":
            for i in range(260):
                n = int(rng.integers(1, 12))
                jit = [0.0, 0.01, 0.03, 0.08, 0.2][i % 5]
                zj = [0.0, 0.02, 0.3, 0.8][(i // 5) % 4]
                x = synth_cata_molecule(rng, n, tree_prob=[1.0, 0.9, 0.5][i % 3], jitter=jit, zjit=zj)
                mols.append((x, np.zeros(len(x), np.int64)))
            # degenerate: two far-apart fragments, two coincident rings, an exactly straight chain
            mols.append((np.array([[0, 0, 0], [2.45, 0, 0], [9, 0, 0], [11.45, 0, 0]], np.float32), np.zeros(4, np.int64)))
            mols.append((np.array([[0, 0, 0], [2.45, 0, 0], [2.45, 0.1, 0]], np.float32), np.zeros(3, np.int64)))
            mols.append((np.array([[2.45 * i, 0, 0] for i in range(5)], np.float32), np.zeros(5, np.int64)))
        else:
            for i in range(260):
                n = int(rng.integers(2, 11))
                x, ty = synth_hetro_molecule(rng, n, tables, jitter=[0.0, 0.01, 0.03, 0.1][i % 4],
                                             corrupt=[0, 0, 0, 0, 0, 0, 1, 2][i % 8])
                mols.append((x, ty))
        M = len(mols)
        NM = max(len(x) for x, _ in mols)
        X = np.zeros((M, NM, 3), np.float32)
        TY = -np.ones((M, NM), np.int64)
        NN = np.zeros(M, np.int64)
        FL = np.zeros((M, 5), np.uint8)
        DIST = np.zeros((M, NM, NM), np.float32)
        ADJ = np.zeros((M, NM, NM), np.float32)
        A3 = np.full((M, 128), np.nan, np.float32)
        A3T = -np.ones((M, 128), np.int64)
        A4 = np.full((M, 256), np.nan, np.float32)
        CNT = np.zeros((M, 2), np.int64)
        for m, (x, ty) in enumerate(mols):
            k = len(x)
            X[m, :k], TY[m, :k], NN[m] = x, ty, k
            res = ref_an.check_stability(torch.from_numpy(x.copy()), torch.from_numpy(ty.copy()), dataset=ds)
            FL[m] = [res[key] for key in ("orientation_nodes", "dist_stable", "connected", "angels3", "angels4")]
            nr = k if ds == "cata" else k // 2
            if res["orientation_nodes"]:
                dist, adj = ref_h.positions2adj(torch.from_numpy(x[None, :nr].copy()), torch.from_numpy(ty[None, :nr].copy()),
                                                0.1, dataset=ds)
                DIST[m, :nr, :nr], ADJ[m, :nr, :nr] = dist[0].numpy(), adj[0].numpy()
                if res["connected"]:
                    a3, a4 = ref_an.get_angels(torch.from_numpy(x[None, :nr].copy()), torch.from_numpy(ty[None, :nr].copy()),
                                               adj, dataset=ds)
                    rl = tables["rings"][ds]
                    pairs = [(rl.index(sym), float(a)) for sym, a in a3]
                    for i, (t, a) in enumerate(pairs):
                        A3T[m, i], A3[m, i] = t, a
                    for i, a in enumerate(float(a) for _, a in a4):
                        A4[m, i] = a
                    CNT[m] = len(a3), len(a4)
        out.update({f"{ds}_x": X, f"{ds}_types": TY, f"{ds}_n": NN, f"{ds}_flags": FL, f"{ds}_dist": DIST,
                    f"{ds}_adj": ADJ, f"{ds}_a3": A3, f"{ds}_a3_type": A3T, f"{ds}_a4": A4, f"{ds}_counts": CNT})
        print(ds, "flag rates", FL.mean(0), "all-stable", FL.all(1).mean())
    save("g11_stability", **out)


def g12_ring_count_sampler():
    """DistributionRings (models_edm.py:21-58): seeded draws and log-probabilities of the reference."""
    out = {}
    for ds in ("cata", "hetro"):
        d = models_edm.DistributionRings(ds)
        torch.manual_seed(1234)
        s = d.sample(2000)
        out[f"{ds}_sample"] = s.numpy()
        out[f"{ds}_log_prob"] = d.log_prob(s[:64]).numpy()
        out[f"{ds}_n_nodes"] = d.n_nodes.numpy()
        out[f"{ds}_prob"] = d.prob.numpy()
    save("g12_ring_count_sampler", **out)


def g13_noised_predictor():
    """sample_edm_t + compute_loss (cond_prediction/train_cond_predictor.py:47-81): forward-noised inputs, predictor
    outputs at the noise level and the per-target absolute errors, for fixed and per-sample t."""
    from cond_prediction import train_cond_predictor as tcp
    out = {}
    for ci, (name, ds, nodes) in enumerate([("cata", "cata", [4, 11, 7, 1, 11]), ("hetro", "hetro", [3, 9, 6, 10])]):
        F = synth.num_node_features(ds)
        eargs = synth.edm_args(dataset=ds, **TINY)
        esd = synth.synth_edm_state_dict(eargs, F, seed=1300 + ci)
        a, model = build_ref_edm(ds, esd, **TINY)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=1310 + ci, amplify_coord=True)
        pa, pred = build_ref_pred(ds, psd, **TINY_P)
        nm, em, z = case_inputs(ds, nodes, None, seed=1320 + ci, guidance_pad=(ds != "cata"))
        B, N, D = z.shape
        rng = np.random.default_rng(1330 + ci)
        x = (z[:, :, :3] * 3.0).astype(np.float32)                      # un-normalised, masked, mean-free positions
        cls = rng.integers(0, F, (B, N))
        h = (np.eye(F, dtype=np.float32)[cls] * nm).astype(np.float32)   # one-hot ring types
        y = rng.standard_normal((B, 5)).astype(np.float32)
        out[f"{name}_x"], out[f"{name}_h"], out[f"{name}_y"] = x, h, y
        out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = nm, em
        tx, th, tnm, tem = (torch.from_numpy(v) for v in (x, h, nm, em))
        T = a.diffusion_steps
        for tag, t_int in (("t0", np.zeros(B)), ("t500", np.full(B, 500.0)), ("tT", np.full(B, float(T))),
                           ("tmix", rng.integers(0, T + 1, B).astype(np.float64))):
            eps = rng_noise(1340 + ci + len(tag), (B, N, D))
            t = torch.from_numpy((t_int / T).astype(np.float32)).view(B, 1)
            with InjectNoise([eps]), torch.no_grad():
                zt = tcp.sample_edm_t(tx, th, model, t, tnm)
                p = pred(zt, tnm, tem.view(B, N * N), t)
            out[f"{name}_{tag}_t_int"] = t_int.astype(np.int32)
            out[f"{name}_{tag}_eps"], out[f"{name}_{tag}_zt"], out[f"{name}_{tag}_pred"] = eps, zt.numpy(), p.numpy()
            if tag == "t500":   # the whole compute_loss with t_fix (same noise -> same z_t)
                with InjectNoise([eps]), torch.no_grad():
                    loss, err = tcp.compute_loss(pred, tx, th, tnm, tem, torch.from_numpy(y), model, a, t_fix=500)
                out[f"{name}_t500_loss"], out[f"{name}_t500_err"] = np.float32(loss.item()), err.numpy()
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=1300 + ci, pseed=1310 + ci, T=T)))
    save("g13_noised_predictor", **out)


def g14_long_chains():
    """T = 1000 chains at the DEFAULT architectures (the bench's C2 / C3 weights: EDM seed 0, predictor seed 1), B = 8,
    N = 11, injected noise regenerated from a seed (checksummed).  Unguided final (x, h); guided final (x, h) plus the
    reference's own (z_t, z_s) at 26 points of its trajectory for teacher-forced step parity along the real chain."""
    out = {}
    T = 1000
    nodes = [11, 11, 11, 7, 4, 11, 9, 11]
    B, N, D = len(nodes), 11, 4
    over = dict(diffusion_steps=T)
    esd = synth.synth_edm_state_dict(synth.edm_args(**over), 1, seed=0)
    a, model = build_ref_edm("cata", esd, **over)
    psd = synth.synth_predictor_state_dict(synth.pred_args(), 1, 5, seed=1)
    pa, pred = build_ref_pred("cata", psd)
    noise = rng_noise(1400, (T + 2, B, N, D))
    out["noise_seed"] = np.int64(1400)
    out["noise_checksum"] = np.array([np.float64(noise.astype(np.float64).sum()), np.float64(np.abs(noise).astype(np.float64).sum()),
                                      np.float64(noise[17, 3, 5, 2]), np.float64(noise[T + 1, 7, 10, 3])])
    a.max_nodes = N
    import time
    t0 = time.time()
    with InjectNoise(list(noise)):
        x, h, nm, em = ref_sampling.sample_pos_edm(a, model, torch.tensor(nodes), std=1.0)
    print(f"g14 unguided T=1000: {time.time() - t0:.0f} s")
    out["unguided_x"], out["unguided_h"] = x.numpy(), h.numpy().astype(np.float32)
    out["node_mask"], out["edge_mask"] = nm.numpy(), em.numpy()

    def tf_gap(_in, _nm, _em, _t):
        return -pred(_in, _nm, _em, _t)[:, 1]

    pts = [999, 990, 950, 900, 850, 800, 750, 700, 650, 600, 550, 500, 450, 400, 350, 300, 250, 200, 150, 100, 50, 25, 10, 5, 1, 0]
    rec = {}
    orig = model.sample_p_zs_given_zt_guidance

    def wrapped(s, t, zt, node_mask, edge_mask, target_function, scale, fix_noise=False):
        zs = orig(s, t, zt, node_mask, edge_mask, target_function, scale, fix_noise=fix_noise)
        si = int(round(float(s[0, 0]) * T))
        if si in pts:
            rec[si] = (zt.detach().numpy().copy(), zs.detach().numpy().copy())
        return zs

    model.sample_p_zs_given_zt_guidance = wrapped
    t0 = time.time()
    with InjectNoise(list(noise)):
        x, h, nm2, em2 = ref_sampling.sample_guidance(a, model, tf_gap, torch.tensor(nodes), scale=0.6, std=1.0)
    print(f"g14 guided T=1000: {time.time() - t0:.0f} s")
    model.sample_p_zs_given_zt_guidance = orig
    assert np.array_equal(nm2.numpy(), nm.numpy()) and sorted(rec) == sorted(pts)
    out["guided_x"], out["guided_h"] = x.numpy(), h.numpy().astype(np.float32)
    # the reference's OWN rounding sensitivity on exactly these chains: the same model and noise in float64
    model.double()
    pred.double()
    with InjectNoise(list(noise), torch.float64):
        x64, _, _, _ = ref_sampling.sample_pos_edm(a, model, torch.tensor(nodes), std=1.0)
    with InjectNoise(list(noise), torch.float64):
        xg64, _, _, _ = ref_sampling.sample_guidance(a, model, tf_gap, torch.tensor(nodes), scale=0.6, std=1.0)
    out["unguided_x_fp64"], out["guided_x_fp64"] = x64.numpy(), xg64.numpy()
    mx = lambda p, q: float(np.abs(p.astype(np.float64) - q.astype(np.float64)).max() / np.abs(q).max())
    out["spread_unguided"] = np.float64(mx(out["unguided_x"], out["unguided_x_fp64"]))
    out["spread_guided"] = np.float64(mx(out["guided_x"], out["guided_x_fp64"]))
    print("g14 reference fp32-vs-fp64 spread: unguided %.2e guided %.2e" % (out["spread_unguided"], out["spread_guided"]))
    out["traj_s"] = np.array(pts, np.int32)
    out["traj_zt"] = np.stack([rec[s][0] for s in pts])
    out["traj_zs"] = np.stack([rec[s][1] for s in pts])
    out["cfg"] = np.array(json.dumps(dict(dataset="cata", T=T, eseed=0, pseed=1, nodes=nodes, scale=0.6, std=1.0)))
    save("g14_long_chains", **out)


def g15_nan_scrub():
    """NaN handling of the reverse steps (edm/egnn/models.py:138-141, en_diffusion.py:881,933-934): a NaN planted in the
    last block's coordinate head makes phi's velocity NaN (scrubbed to 0 inside phi); a NaN planted in the predictor's
    readout makes the guidance gradient NaN (z_s scrubbed to 0 at the end of the guided step)."""
    out = {}
    T = 1000
    ds, nodes = "cata", [4, 11, 7, 11]
    F = 1
    eargs = synth.edm_args(dataset=ds, **TINY)
    esd = synth.synth_edm_state_dict(eargs, F, seed=1500, amplify_coord=True)
    pargs = synth.pred_args(dataset=ds, **TINY_P)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=1510, amplify_coord=True)
    nm, em, z = case_inputs(ds, nodes, None, seed=1520, guidance_pad=True)
    B, N, D = z.shape
    tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
    out["z"], out["node_mask"], out["edge_mask"] = z, nm, em
    esd_bad = {k: v.copy() for k, v in esd.items()}
    key_e = "dynamics.egnn.e_block_1.gcl_equiv.coord_mlp.4.weight"
    esd_bad[key_e][0, 3] = np.nan
    psd_bad = {k: v.copy() for k, v in psd.items()}
    key_p = "egnn.embedding_out.weight"
    psd_bad[key_p][1, 5] = np.nan
    out["edm_poison_key"], out["edm_poison_idx"] = np.array(key_e), np.array([0, 3])
    out["pred_poison_key"], out["pred_poison_idx"] = np.array(key_p), np.array([1, 5])
    a, model_bad = build_ref_edm(ds, esd_bad, **TINY)
    a2, model_ok = build_ref_edm(ds, esd, **TINY)
    pa, pred_ok = build_ref_pred(ds, psd, **TINY_P)
    pb, pred_bad = build_ref_pred(ds, psd_bad, **TINY_P)
    import contextlib, io
    for s in (999, 500, 0):
        eps = rng_noise(1530 + s % 7, (B, N, D))
        st = torch.full((B, 1), s) / T
        tt = (torch.full((B, 1), s) + 1) / T
        out[f"s{s}_eps"] = eps
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            e = model_bad.phi(torch.from_numpy(z), tt, tnm, tem, None).numpy()
            with InjectNoise([eps]):
                zu = model_bad.sample_p_zs_given_zt(st, tt, torch.from_numpy(z), tnm, tem, None).numpy()
            with InjectNoise([eps]):
                zg = model_bad.sample_p_zs_given_zt_guidance(
                    st, tt, torch.from_numpy(z), tnm, tem, lambda i, n, m, t: -pred_ok(i, n, m, t)[:, 1], 0.6).numpy()
            with InjectNoise([eps]):
                zp = model_ok.sample_p_zs_given_zt_guidance(
                    st, tt, torch.from_numpy(z), tnm, tem, lambda i, n, m, t: -pred_bad(i, n, m, t)[:, 1], 0.6).numpy()
        assert np.isfinite(e).all() and np.isfinite(zu).all() and np.isfinite(zg).all() and np.isfinite(zp).all()
        out[f"s{s}_phi_edm_poisoned"] = e
        out[f"s{s}_zs_unguided_edm_poisoned"] = zu
        out[f"s{s}_zs_guided_edm_poisoned"] = zg
        out[f"s{s}_zs_guided_pred_poisoned"] = zp
    out["cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=1500, pseed=1510, T=T, nodes=nodes)))
    save("g15_nan_scrub", **out)


def g17_nan_in_edge_gemm_matrix():
    """NaN planted in a matrix of the EDGE-level GEMMs (edge_mlp.2.weight of an EDM GCL; edge_mlp.2.weight and
    coord_mlp.0.weight of a predictor layer) -- the matrices the default kernels stream as three bf16 pieces.  The EDM's
    h output is NaN (only the velocity is scrubbed, edm/egnn/models.py:138-141), the guided step zeroes eps_hat
    (en_diffusion.py:881) and stays finite; a poisoned predictor gives a NaN gradient and z_s is scrubbed to zeros (:933-934)."""
    out = {}
    T = 1000
    ds, nodes = "cata", [4, 11, 7, 11]
    F = 1
    eargs = synth.edm_args(dataset=ds, **TINY)
    esd = synth.synth_edm_state_dict(eargs, F, seed=1700, amplify_coord=True)
    pargs = synth.pred_args(dataset=ds, **TINY_P)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=1710, amplify_coord=True)
    nm, em, z = case_inputs(ds, nodes, None, seed=1720, guidance_pad=True)
    B, N, D = z.shape
    tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
    out["z"], out["node_mask"], out["edge_mask"] = z, nm, em
    poison = dict(edm=("dynamics.egnn.e_block_1.gcl_0.edge_mlp.2.weight", [5, 17]),
                  pred_w2=("egnn.gcl_1.edge_mlp.2.weight", [30, 2]),
                  pred_wc1=("egnn.gcl_0.coord_mlp.0.weight", [7, 33]))
    bad = {}
    for name, (key, idx) in poison.items():
        src = esd if name == "edm" else psd
        d = {k: v.copy() for k, v in src.items()}
        d[key][tuple(idx)] = np.nan
        bad[name] = d
        out[f"{name}_key"], out[f"{name}_idx"] = np.array(key), np.array(idx)
    a, model_bad = build_ref_edm(ds, bad["edm"], **TINY)
    a2, model_ok = build_ref_edm(ds, esd, **TINY)
    pa, pred_ok = build_ref_pred(ds, psd, **TINY_P)
    preds_bad = {k: build_ref_pred(ds, bad[k], **TINY_P)[1] for k in ("pred_w2", "pred_wc1")}
    import contextlib, io
    for s in (999, 500, 0):
        eps = rng_noise(1730 + s % 7, (B, N, D))
        st = torch.full((B, 1), s) / T
        tt = (torch.full((B, 1), s) + 1) / T
        out[f"s{s}_eps"] = eps
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            e = model_bad.phi(torch.from_numpy(z), tt, tnm, tem, None).numpy()
            with InjectNoise([eps]):
                zg = model_bad.sample_p_zs_given_zt_guidance(
                    st, tt, torch.from_numpy(z), tnm, tem, lambda i, n, m, t: -pred_ok(i, n, m, t)[:, 1], 0.6).numpy()
            zp = {}
            for k, pb in preds_bad.items():
                with InjectNoise([eps]):
                    zp[k] = model_ok.sample_p_zs_given_zt_guidance(
                        st, tt, torch.from_numpy(z), tnm, tem, lambda i, n, m, t, pb=pb: -pb(i, n, m, t)[:, 1], 0.6).numpy()
        assert np.isfinite(e[:, :, :3]).all() and np.isnan(e[:, :, 3:][nm[:, :, 0] != 0]).all()
        assert np.isfinite(zg).all() and all(np.isfinite(v).all() for v in zp.values())
        out[f"s{s}_phi_edm_poisoned"] = e
        out[f"s{s}_zs_guided_edm_poisoned"] = zg
        for k, v in zp.items():
            out[f"s{s}_zs_guided_{k}_poisoned"] = v
    out["cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=1700, pseed=1710, T=T, nodes=nodes)))
    save("g17_nan_edge_matrix", **out)


def g18_large_molecules():
    """Molecules beyond the LDS limit of the library's resident kernels: hetero 20 rings (N = 40 graph nodes with the
    orientation nodes: BASELINE config 4's "ring count 6-20" read literally; sampling_edm.py:172-209 has no cap) and a
    14-ring one in the same batch, DEFAULT architectures: phi, predictor + input gradient, one teacher-forced guided step."""
    out = {}
    T = 1000
    ds, nodes = "hetro", [20, 14]
    F = synth.num_node_features(ds)
    eargs = synth.edm_args(dataset=ds)
    esd = synth.synth_edm_state_dict(eargs, F, seed=1800, amplify_coord=True)
    pargs = synth.pred_args(dataset=ds)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=1810, amplify_coord=True)
    a, model = build_ref_edm(ds, esd)
    pa, pred = build_ref_pred(ds, psd)
    nm, em, z = case_inputs(ds, nodes, None, seed=1820, guidance_pad=True)
    B, N, D = z.shape
    assert N == 40
    tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
    out["z"], out["node_mask"], out["edge_mask"] = z, nm, em
    s = 600
    st = torch.full((B, 1), s) / T
    tt = (torch.full((B, 1), s) + 1) / T
    eps = rng_noise(1830, (B, N, D))
    out["eps"] = eps
    with torch.no_grad():
        out["phi"] = model.phi(torch.from_numpy(z), tt, tnm, tem, None).numpy()
    zt = torch.from_numpy(z).requires_grad_()
    p = pred(zt, tnm, tem, tt)
    out["pred"] = p.detach().numpy()
    out["grad_gap"] = torch.autograd.grad((0.6 * -p[:, 1]).sum(), zt)[0].numpy()
    with InjectNoise([eps]), torch.no_grad():
        out["zs_unguided"] = model.sample_p_zs_given_zt(st, tt, torch.from_numpy(z), tnm, tem, None).numpy()
    with InjectNoise([eps]), torch.no_grad():
        out["zs_guided"] = model.sample_p_zs_given_zt_guidance(st, tt, torch.from_numpy(z), tnm, tem,
                                                               lambda i, n, m, t: -pred(i, n, m, t)[:, 1], 0.6).numpy()
    out["cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=1800, pseed=1810, T=T, s=s, nodes=nodes)))
    save("g18_large_molecules", **out)


def g19_amplified_default_steps():
    """Reference-held anchor for the ill-conditioned case: DEFAULT architectures with amplified coordinate heads (cata C3
    shape and hetero C4 shape), teacher-forced unguided / guided steps at s = 999, 400, 0 -- run by the reference in fp32 AND
    in float64 (model.double()), so that a kernel can be held to 1e-4 against the reference's own float64 result where
    the two fp32 evaluations differ from each other by about that much."""
    out = {}
    T = 1000
    for ci, (name, ds, nodes) in enumerate([("cata", "cata", [11, 11, 7, 11, 4, 9]), ("hetro", "hetro", [10, 3, 7, 5])]):
        F = synth.num_node_features(ds)
        eargs = synth.edm_args(dataset=ds)
        esd = synth.synth_edm_state_dict(eargs, F, seed=1900 + ci, amplify_coord=True)
        pargs = synth.pred_args(dataset=ds)
        psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=1910 + ci, amplify_coord=True)
        a, model = build_ref_edm(ds, esd)
        pa, pred = build_ref_pred(ds, psd)
        nm, em, z = case_inputs(ds, nodes, None, seed=1920 + ci, guidance_pad=True)
        B, N, D = z.shape
        tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
        wv = torch.tensor([0., -1., 0., 0., 0.] if ds == "cata" else [3., 0., 1., 1., 0.])
        out[f"{name}_z"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"], out[f"{name}_w"] = z, nm, em, wv.numpy()
        for dt, tag in ((torch.float32, "fp32"), (torch.float64, "fp64")):
            if dt == torch.float64:
                model.double()
                pred.double()
            zt_, nm_, em_ = torch.from_numpy(z).to(dt), tnm.to(dt), tem.to(dt)
            tf = lambda i, n, m, t: (pred(i, n, m, t) * wv.to(dt)).sum(-1)
            for s in (999, 400, 0):
                eps = rng_noise(1930 + 10 * ci + s % 7, (B, N, D))
                st = (torch.full((B, 1), s) / T).to(dt)
                tt = ((torch.full((B, 1), s) + 1) / T).to(dt)
                out[f"{name}_s{s}_eps"] = eps
                with InjectNoise([eps], dt), torch.no_grad():
                    out[f"{name}_s{s}_zs_unguided_{tag}"] = model.sample_p_zs_given_zt(st, tt, zt_, nm_, em_, None).numpy()
                with InjectNoise([eps], dt), torch.no_grad():
                    out[f"{name}_s{s}_zs_guided_{tag}"] = model.sample_p_zs_given_zt_guidance(st, tt, zt_, nm_, em_, tf, 0.6).numpy()
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=1900 + ci, pseed=1910 + ci, T=T, nodes=nodes)))
    save("g19_amplified_default_steps", **out)


def g16_fix_noise():
    """fix_noise=True (en_diffusion.py:562-566,972-978,1022-1028): ONE raw draw [1,N,3+F] per call is broadcast over the
    batch and masked / mean-centred per molecule.  Tiny config, T = 50, unguided and guided."""
    out = {}
    T = 50
    ds, nodes = "cata", [6, 8, 8, 3]
    F = 1
    over = dict(diffusion_steps=T, **TINY)
    esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=1600)
    a, model = build_ref_edm(ds, esd, **over)
    psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=1610)
    pa, pred = build_ref_pred(ds, psd, **TINY_P)
    nm, em = masks(ds, nodes, None)
    B, N, _ = nm.shape
    noise = rng_noise(1620, (T + 2, 1, N, 3 + F))
    tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
    with InjectNoise(list(noise)):
        x, h = model.sample(B, N, tnm, tem, fix_noise=True, std=0.7)
    out["x_unguided"], out["h_unguided"] = x.numpy(), h["categorical"].numpy().astype(np.float32)
    with InjectNoise(list(noise)):
        x, h = model.sample_guidance(B, lambda i, n, m, t: -pred(i, n, m, t)[:, 1], tnm, tem, scale=0.6, fix_noise=True, std=1.0)
    out["x_guided"], out["h_guided"] = x.numpy(), h["categorical"].numpy().astype(np.float32)
    out["noise"], out["node_mask"], out["edge_mask"] = noise, nm, em
    out["cfg"] = np.array(json.dumps(dict(dataset=ds, T=T, eseed=1600, pseed=1610, nodes=nodes, amp=False)))
    save("g16_fix_noise", **out)


def g20_cosine_and_mean():
    """The two EDM modes SURVEY 2 allowed to refuse and VERDICT r3 asked to accept: diffusion_noise_schedule='cosine'
    (en_diffusion.py:64-81,196-197) and aggregation_method='mean' (egnn_new.py:403-421: the norm counts EVERY edge of the dense
    list, masked or not, i.e. the padded node count N).  gamma / coefficient tables, phi with 'mean', and guided T=50 chains
    with both switched on, tiny configs, injected noise."""
    out = {}
    for T in (50, 1000):
        sd = synth.synth_edm_state_dict(synth.edm_args(nf=8, n_layers=1), 1, seed=0)
        # (the reference refuses 'cosine' with the default normalize_factors [3, 4, 10]: sigma_0 = 0.041 is too large for a
        # one-hot scaled by 1/4, en_diffusion.py:336-349 -- a cosine model needs smaller ones)
        a, model = build_ref_edm("cata", sd, nf=8, n_layers=1, diffusion_steps=T, diffusion_noise_schedule="cosine",
                                 normalize_factors=[1, 2, 2])
        out[f"gamma_T{T}"] = model.gamma.gamma.numpy().copy()
        rows = []
        for s in ([0, 1, T // 2, T - 2, T - 1]):
            st = torch.full((1, 1), s) / T
            tt = (torch.full((1, 1), s) + 1) / T
            gs, gt = model.gamma(st), model.gamma(tt)
            zt = torch.zeros(1, 1, 1)
            s2, s_ts, a_ts = model.sigma_and_alpha_t_given_s(gt, gs, zt)
            sig_s, sig_t = model.sigma(gs, zt), model.sigma(gt, zt)
            rows.append([s, a_ts.item(), s2.item(), (s2 / a_ts / sig_t).item(), (s_ts * sig_s / sig_t).item(),
                         sig_s.item(), sig_t.item(), tt.item()])
        out[f"coef_T{T}"] = np.array(rows, dtype=np.float64)
    T = 50
    for ci, (name, ds, nodes, mx) in enumerate([("cata", "cata", [4, 11, 7, 2, 11], 11), ("hetro", "hetro", [3, 5, 10, 7], 10)]):
        F = synth.num_node_features(ds)
        over = dict(diffusion_steps=T, aggregation_method="mean", diffusion_noise_schedule="cosine", normalize_factors=[1, 2, 2], **TINY)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=2000 + ci, amplify_coord=True)
        a, model = build_ref_edm(ds, esd, **over)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=2010 + ci, amplify_coord=True)
        pa, pred = build_ref_pred(ds, psd, **TINY_P)
        nm, em, z = case_inputs(ds, nodes, mx, seed=2020 + ci)
        B = z.shape[0]
        t = np.linspace(0.05, 0.95, B).astype(np.float32).reshape(B, 1)
        with torch.no_grad():
            eps = model.phi(torch.from_numpy(z), torch.from_numpy(t), torch.from_numpy(nm), torch.from_numpy(em), None).numpy()
        out[f"{name}_z"], out[f"{name}_t"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = z, t, nm, em
        out[f"{name}_eps"] = eps

        # the chains run on DEFAULT-init weights (a free-running chain through amplified heads is not a 1e-4 comparison:
        # BASELINE.md section 2), the phi cases above on amplified ones
        esd_c = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=2040 + ci)
        a_c, model_c = build_ref_edm(ds, esd_c, **over)
        psd_c = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=2050 + ci)
        pa_c, pred_c = build_ref_pred(ds, psd_c, **TINY_P)

        def tf_gap(_in, _nm, _em, _t):
            return -pred_c(_in, _nm, _em, _t)[:, 1]

        n = torch.tensor(nodes)
        Nn = max(nodes) * (2 if ds != "cata" else 1)
        noise = rng_noise(2030 + ci, (T + 2, len(nodes), Nn, 3 + F))
        with InjectNoise(list(noise)):
            x, h, nm2, em2 = ref_sampling.sample_guidance(a_c, model_c, tf_gap, n, scale=0.6, std=1.0)
        out[f"{name}_noise"], out[f"{name}_x_guided"], out[f"{name}_h_guided"] = noise, x.numpy(), h.numpy().astype(np.float32)
        out[f"{name}_chain_node_mask"], out[f"{name}_chain_edge_mask"] = nm2.numpy(), em2.numpy()
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, T=T, eseed=2000 + ci, pseed=2010 + ci, chain_eseed=2040 + ci,
                                                      chain_pseed=2050 + ci, nodes=nodes, amp=True,
                                                      over=dict(TINY, aggregation_method="mean", diffusion_noise_schedule="cosine",
                                                                normalize_factors=[1, 2, 2]))))
    save("g20_cosine_and_mean", **out)


def g22_sin_embedding():
    """`sin_embedding=True` (utils/args_edm.py:33, models_edm.py:78; egnn_new.py:269-273,302-303,217-218,378-391): the two scalar
    edge features r, d0 become 2 x 12 sinusoids of their square roots, the first Linear of every edge / coordinate MLP takes
    2 H + 24 inputs.  phi (tiny widths, amplified heads, cata and hetro; default widths, default init), a teacher-forced
    unguided and guided step at the default widths, run by the reference in fp32 AND float64 (the highest frequency multiplies
    sqrt(r) by 429: the embedding is ill-conditioned in fp32 by construction -- the float64 run says by how much)."""
    out = {}
    from edm.egnn.egnn_new import SinusoidsEmbeddingNew
    out["frequencies"] = SinusoidsEmbeddingNew().frequencies.numpy().copy()
    for ci, (name, ds, nodes, mx, over) in enumerate([("cata_tiny", "cata", [4, 11, 7, 2, 11], 11, dict(TINY)),
                                                      ("hetro_tiny", "hetro", [3, 5, 10, 7], 10, dict(TINY)),
                                                      ("cata_default", "cata", [11, 9, 11], 11, {})]):
        F = synth.num_node_features(ds)
        T = 1000
        over = dict(over, sin_embedding=True, diffusion_steps=T)
        amp = "tiny" in name
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=2200 + ci, amplify_coord=amp)
        a, model = build_ref_edm(ds, esd, **over)
        nm, em, z = case_inputs(ds, nodes, mx, seed=2220 + ci)
        B = z.shape[0]
        t = np.linspace(0.05, 0.95, B).astype(np.float32).reshape(B, 1)
        with torch.no_grad():
            eps = model.phi(torch.from_numpy(z), torch.from_numpy(t), torch.from_numpy(nm), torch.from_numpy(em), None).numpy()
            m64 = copy.deepcopy(model).double()
            eps64 = m64.phi(torch.from_numpy(z).double(), torch.from_numpy(t).double(), torch.from_numpy(nm).double(),
                            torch.from_numpy(em).double(), None).numpy()
        out[f"{name}_z"], out[f"{name}_t"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = z, t, nm, em
        out[f"{name}_eps"], out[f"{name}_eps64"] = eps, eps64
        cfgd = dict(dataset=ds, T=T, eseed=2200 + ci, nodes=nodes, amp=amp, over={k: v for k, v in over.items() if k != "diffusion_steps"})
        if name == "cata_default":
            psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds), F, 5, seed=2210 + ci)
            pa, pred = build_ref_pred(ds, psd)

            def tf_gap(_in, _nm, _em, _t):
                return -pred(_in, _nm, _em, _t)[:, 1]

            eps_n = rng_noise(2230 + ci, z.shape)
            for sidx in (999, 400, 0):
                s_t = torch.full((B, 1), sidx / T)
                t_t = torch.full((B, 1), (sidx + 1) / T)
                with InjectNoise([eps_n]):
                    zs_u = model.sample_p_zs_given_zt(s_t, t_t, torch.from_numpy(z), torch.from_numpy(nm), torch.from_numpy(em), None)
                with InjectNoise([eps_n]):
                    zs_g = model.sample_p_zs_given_zt_guidance(s_t, t_t, torch.from_numpy(z), torch.from_numpy(nm), torch.from_numpy(em),
                                                               tf_gap, 0.6)
                out[f"{name}_zs_unguided_s{sidx}"], out[f"{name}_zs_guided_s{sidx}"] = zs_u.numpy(), zs_g.detach().numpy()
            out[f"{name}_step_noise"] = eps_n
            cfgd["pseed"] = 2210 + ci
        out[f"{name}_cfg"] = np.array(json.dumps(cfgd))
    save("g22_sin_embedding", **out)


def g23_attention_tanh_flags():
    """`--attention False` / `--tanh False` (utils/args_edm.py:29-30, cond_prediction/prediction_args.py:44-45; egnn_new.py:53-57,117-125,
    egnn_predictor/gcl.py): the edge gate and the tanh bound of the coordinate update are constructor switches of BOTH networks.
    Every combination other than the default (True, True), on both networks at once: phi, predictor + input gradient, a
    teacher-forced unguided and guided step -- tiny widths (amplified heads, cata and hetro) and the default widths (cata)."""
    out = {}
    T = 1000
    cases = []
    for att, th in ((False, True), (True, False), (False, False)):
        tag = f"att{int(att)}_tanh{int(th)}"
        cases.append((f"cata_tiny_{tag}", "cata", [4, 11, 7, 2, 11], 11, dict(TINY), dict(TINY_P), True, att, th))
        cases.append((f"hetro_tiny_{tag}", "hetro", [3, 5, 10, 7], 10, dict(TINY), dict(TINY_P), True, att, th))
    cases.append(("cata_default_att0_tanh0", "cata", [11, 9, 11], 11, {}, {}, False, False, False))
    for ci, (name, ds, nodes, mx, over_e, over_p, amp, att, th) in enumerate(cases):
        F = synth.num_node_features(ds)
        over_e = dict(over_e, attention=att, tanh=th, diffusion_steps=T)
        over_p = dict(over_p, attention=att, tanh=th)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over_e), F, seed=2300 + ci, amplify_coord=amp)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **over_p), F, 5, seed=2350 + ci, amplify_coord=amp)
        a, model = build_ref_edm(ds, esd, **over_e)
        pa, pred = build_ref_pred(ds, psd, **over_p)
        assert ("dynamics.egnn.e_block_0.gcl_0.att_mlp.0.weight" in esd) == att
        nm, em, z = case_inputs(ds, nodes, mx, seed=2320 + ci)
        B = z.shape[0]
        t = np.linspace(0.05, 0.95, B).astype(np.float32).reshape(B, 1)
        tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
        with torch.no_grad():
            out[f"{name}_eps"] = model.phi(torch.from_numpy(z), torch.from_numpy(t), tnm, tem, None).numpy()
        zt = torch.from_numpy(z).requires_grad_()
        p = pred(zt, tnm, tem, torch.from_numpy(t))
        out[f"{name}_pred"] = p.detach().numpy()
        out[f"{name}_grad_gap"] = torch.autograd.grad((0.6 * -p[:, 1]).sum(), zt)[0].numpy()

        def tf_gap(_in, _nm, _em, _t):
            return -pred(_in, _nm, _em, _t)[:, 1]

        s = 400
        eps_n = rng_noise(2340 + ci, z.shape)
        s_t, t_t = torch.full((B, 1), s / T), torch.full((B, 1), (s + 1) / T)
        with InjectNoise([eps_n]), torch.no_grad():
            out[f"{name}_zs_unguided"] = model.sample_p_zs_given_zt(s_t, t_t, torch.from_numpy(z), tnm, tem, None).numpy()
        with InjectNoise([eps_n]):
            out[f"{name}_zs_guided"] = model.sample_p_zs_given_zt_guidance(s_t, t_t, torch.from_numpy(z), tnm, tem, tf_gap, 0.6).detach().numpy()
        out[f"{name}_z"], out[f"{name}_t"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"], out[f"{name}_step_noise"] = z, t, nm, em, eps_n
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, T=T, s=s, eseed=2300 + ci, pseed=2350 + ci, amp=amp,
                                                      over_e={k: v for k, v in over_e.items() if k != "diffusion_steps"}, over_p=over_p)))
    out["names"] = np.array(json.dumps([c[0] for c in cases]))
    save("g23_attention_tanh_flags", **out)


def g24_scalar_hyperparameters():
    """Every scalar hyper-parameter of the path away from its default at once (utils/args_edm.py, prediction_args.py):
    diffusion_noise_schedule 'polynomial_3' with diffusion_noise_precision 1e-4 (en_diffusion.py:47-61,191-218), normalize_factors
    [2, 3, 5] (:384-415), coords_range 7 (denoiser, egnn_new.py:290) and 4 (predictor, egnn_predictor/models.py:515), norm_constant 2,
    normalization_factor 2, inv_sublayers 2: gamma / coefficient tables, phi, predictor + gradient (amplified heads), and a guided
    T = 50 chain through sample_guidance on default-init weights, injected noise."""
    out = {}
    sched = dict(diffusion_noise_schedule="polynomial_3", diffusion_noise_precision=1e-4, normalize_factors=[2, 3, 5])
    for T in (50, 1000):
        sd = synth.synth_edm_state_dict(synth.edm_args(nf=8, n_layers=1), 1, seed=0)
        a, model = build_ref_edm("cata", sd, nf=8, n_layers=1, diffusion_steps=T, **sched)
        out[f"gamma_T{T}"] = model.gamma.gamma.numpy().copy()
        rows = []
        for s in ([0, 1, T // 2, T - 2, T - 1]):
            st = torch.full((1, 1), s) / T
            tt = (torch.full((1, 1), s) + 1) / T
            gs, gt = model.gamma(st), model.gamma(tt)
            zt = torch.zeros(1, 1, 1)
            s2, s_ts, a_ts = model.sigma_and_alpha_t_given_s(gt, gs, zt)
            sig_s, sig_t = model.sigma(gs, zt), model.sigma(gt, zt)
            rows.append([s, a_ts.item(), s2.item(), (s2 / a_ts / sig_t).item(), (s_ts * sig_s / sig_t).item(),
                         sig_s.item(), sig_t.item(), tt.item()])
        out[f"coef_T{T}"] = np.array(rows, dtype=np.float64)
    T = 50
    arch_e = dict(nf=32, n_layers=2, inv_sublayers=2, coords_range=7.0, norm_constant=2.0, normalization_factor=2.0)
    arch_p = dict(TINY_P, coords_range=4.0)
    for ci, (name, ds, nodes, mx) in enumerate([("cata", "cata", [4, 11, 7, 2, 11], 11), ("hetro", "hetro", [3, 5, 10, 7], 10)]):
        F = synth.num_node_features(ds)
        over = dict(diffusion_steps=T, **sched, **arch_e)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=2400 + ci, amplify_coord=True)
        a, model = build_ref_edm(ds, esd, **over)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **arch_p), F, 5, seed=2410 + ci, amplify_coord=True)
        pa, pred = build_ref_pred(ds, psd, **arch_p)
        nm, em, z = case_inputs(ds, nodes, mx, seed=2420 + ci)
        B = z.shape[0]
        t = np.linspace(0.05, 0.95, B).astype(np.float32).reshape(B, 1)
        tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
        with torch.no_grad():
            out[f"{name}_eps"] = model.phi(torch.from_numpy(z), torch.from_numpy(t), tnm, tem, None).numpy()
        zt = torch.from_numpy(z).requires_grad_()
        p = pred(zt, tnm, tem, torch.from_numpy(t))
        out[f"{name}_pred"] = p.detach().numpy()
        out[f"{name}_grad_gap"] = torch.autograd.grad((0.6 * -p[:, 1]).sum(), zt)[0].numpy()
        out[f"{name}_z"], out[f"{name}_t"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = z, t, nm, em

        esd_c = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=2440 + ci)
        a_c, model_c = build_ref_edm(ds, esd_c, **over)
        psd_c = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **arch_p), F, 5, seed=2450 + ci)
        pa_c, pred_c = build_ref_pred(ds, psd_c, **arch_p)

        def tf_gap(_in, _nm, _em, _t):
            return -pred_c(_in, _nm, _em, _t)[:, 1]

        n = torch.tensor(nodes)
        Nn = max(nodes) * (2 if ds != "cata" else 1)
        noise = rng_noise(2430 + ci, (T + 2, len(nodes), Nn, 3 + F))
        with InjectNoise(list(noise)):
            x, h, nm2, em2 = ref_sampling.sample_guidance(a_c, model_c, tf_gap, n, scale=0.6, std=1.0)
        out[f"{name}_noise"], out[f"{name}_x_guided"], out[f"{name}_h_guided"] = noise, x.numpy(), h.numpy().astype(np.float32)
        out[f"{name}_chain_node_mask"], out[f"{name}_chain_edge_mask"] = nm2.numpy(), em2.numpy()
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, T=T, eseed=2400 + ci, pseed=2410 + ci, chain_eseed=2440 + ci,
                                                      chain_pseed=2450 + ci, nodes=nodes, over_e=dict(sched, **arch_e), over_p=arch_p)))
    save("g24_scalar_hyperparameters", **out)


def direct_z_target_torch(z, pred, nm):
    """-pred[:, 1] + 0.05 * sum over live nodes of |x_n|^2 + 0.02 * sum of the first feature column: depends on z through the
    predictor AND directly (numpy twin: tests/helpers.direct_z_target_grad)."""
    return -pred[:, 1] + 0.05 * ((z[:, :, :3] ** 2) * nm).sum((1, 2)) + 0.02 * (z[:, :, 3] * nm[:, :, 0]).sum(1)


def g21_direct_z_target():
    """sample_guidance with a closure that depends on z outside the predictor too (the reference differentiates any function
    of z_s, en_diffusion.py:899-903): tiny configs, T = 50, default-init weights, injected noise."""
    out = {}
    T = 50
    for ci, (name, ds, nodes) in enumerate([("cata", "cata", [6, 8, 8, 3]), ("hetro", "hetro", [3, 5, 4])]):
        F = synth.num_node_features(ds)
        over = dict(diffusion_steps=T, **TINY)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=2100 + ci)
        a, model = build_ref_edm(ds, esd, **over)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=2110 + ci)
        pa, pred = build_ref_pred(ds, psd, **TINY_P)

        def tf(_in, _nm, _em, _t):
            return direct_z_target_torch(_in, pred(_in, _nm, _em, _t), _nm)

        n = torch.tensor(nodes)
        Nn = max(nodes) * (2 if ds != "cata" else 1)
        noise = rng_noise(2120 + ci, (T + 2, len(nodes), Nn, 3 + F))
        with InjectNoise(list(noise)):
            x, h, nm, em = ref_sampling.sample_guidance(a, model, tf, n, scale=0.6, std=1.0)
        out[f"{name}_noise"], out[f"{name}_x"], out[f"{name}_h"] = noise, x.numpy(), h.numpy().astype(np.float32)
        out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = nm.numpy(), em.numpy()
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, T=T, eseed=2100 + ci, pseed=2110 + ci, nodes=nodes, amp=False)))
    save("g21_direct_z_target", **out)


def g25_nll():
    """The EDM's eval-mode negative log-likelihood (EnVariationalDiffusion.forward, en_diffusion.py:646-805 with t0_always): the
    reference's model(x, h, node_mask, edge_mask) in eval() driven by a fixed t_int (torch.randint patched) and InjectNoise([eps,
    eps_0]); the six terms recomputed with the reference's own methods from the values its two phi passes saw, and phi at both
    passes.  Cases: tiny cata / hetero (mixed sizes, t_int including 1 and T), the default widths on the C3 weights, a
    g18-like N = 40 hetero batch (V8G), a schedule whose categorical term is NOT saturated, and sin_embedding."""
    out = {}
    cases = [  # name, dataset, nodes, max_nodes, over, weight seed, amplify
        ("cata_tiny", "cata", [4, 11, 7, 2, 11], 11, dict(TINY, diffusion_steps=50), 2500, True),
        ("hetro_tiny", "hetro", [3, 9, 6, 10], None, dict(TINY, diffusion_steps=50), 2501, True),
        ("cata_default", "cata", [11, 9, 11, 7, 11, 4], 11, {}, 0, False),
        ("hetro_large", "hetro", [20, 14], None, {}, 2503, False),
        ("hetro_soft", "hetro", [5, 8, 10], None, dict(TINY, diffusion_steps=50, diffusion_noise_precision=9e-4,
                                                          normalize_factors=[3, 4, 1]), 2504, False),
        ("cata_se_tiny", "cata", [4, 11, 7, 2, 11], 11, dict(TINY, diffusion_steps=50, sin_embedding=True), 2505, False),
    ]
    for ci, (name, ds, nodes, mx, over, wseed, amp) in enumerate(cases):
        F = synth.num_node_features(ds)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=wseed, amplify_coord=amp)
        a, model = build_ref_edm(ds, esd, **over)
        model.eval()
        nm, em, z = case_inputs(ds, nodes, mx, seed=2520 + ci, guidance_pad=mx is None)
        B, N, D = z.shape
        if name == "hetro_large":
            assert N == 40
        T = a.diffusion_steps
        rng = np.random.default_rng(2530 + ci)
        x = (z[:, :, :3] * 3.0).astype(np.float32)                      # un-normalised, masked, mean-free positions
        h = (np.eye(F, dtype=np.float32)[rng.integers(0, F, (B, N))] * nm).astype(np.float32)
        t_int = rng.integers(1, T + 1, B)
        t_int[0], t_int[-1] = 1, T
        eps, eps0 = rng_noise(2540 + ci, (B, N, D)), rng_noise(2550 + ci, (B, N, D))
        tx, th, tnm, tem = (torch.from_numpy(v) for v in (x, h, nm, em))
        hd = {"categorical": th, "integer": torch.zeros(0)}
        rec = {"phi": [], "noise": []}
        phi0, noise0, randint0 = model.phi, model.sample_combined_position_feature_noise, torch.randint

        def phi_rec(zz, tt, *rest):
            o = phi0(zz, tt, *rest)
            rec["phi"].append((zz.clone(), tt.clone(), o.clone()))
            return o

        def noise_rec(*args, **kw):
            o = noise0(*args, **kw)
            rec["noise"].append(o.clone())
            return o

        def randint_fixed(low, high, size, device=None, **kw):
            assert (low, high, tuple(size)) == (1, T + 1, (B, 1)), (low, high, size)
            return torch.from_numpy(t_int.reshape(B, 1)).long()

        model.phi, model.sample_combined_position_feature_noise = phi_rec, noise_rec
        torch.randint = randint_fixed
        try:
            with InjectNoise([eps, eps0]), torch.no_grad():
                nll = model(tx, hd, tnm, tem.view(B, N * N))
        finally:
            torch.randint = randint0
            del model.phi, model.sample_combined_position_feature_noise
        assert len(rec["phi"]) == 2 and len(rec["noise"]) == 2
        (zt, tt, net_t), (z0, t0, net_0) = rec["phi"]
        e_t, e_0 = rec["noise"]
        with torch.no_grad():  # the six terms, by the reference's own methods on what its passes saw
            xn, hn, dlp = model.normalize(tx, hd, tnm)
            xh = torch.cat([xn, hn["categorical"], hn["integer"]], dim=2)
            ti = torch.from_numpy(t_int.reshape(B, 1)).float()
            g_t = model.inflate_batch_array(model.gamma(ti / T), xn)
            g_s = model.inflate_batch_array(model.gamma((ti - 1) / T), xn)
            g_0 = model.inflate_batch_array(model.gamma(torch.zeros(B, 1)), xn)
            error = model.compute_error(net_t, g_t, e_t)
            snr = (model.SNR(g_s - g_t) - 1).squeeze(1).squeeze(1)
            loss_t = T * (0.5 * snr * error)
            nlc = -model.log_constants_p_x_given_z0(xn, tnm)
            kl = model.kl_prior(xh, tnm)
            lpxh = model.log_pxh_given_z0_without_constants(xn, hn, z0, g_0, e_0, net_0, tnm)
            lpx = -0.5 * model.compute_error(net_0[:, :, :3], g_0, e_0[:, :, :3])
            total = kl + loss_t + nlc - lpxh - dlp
        assert torch.allclose(total, nll, rtol=1e-5, atol=1e-5), (total, nll)
        log_ph = (lpxh - lpx).numpy()
        if name == "hetro_soft":
            assert np.abs(log_ph).max() > 1e-3, log_ph
        else:
            out[name + "_log_ph_max"] = np.float32(np.abs(log_ph).max())
        out[name + "_cfg"] = np.array(json.dumps(dict(dataset=ds, over=over, wseed=wseed, amp=amp, nodes=nodes, T=T)))
        out[name + "_x"], out[name + "_h"], out[name + "_node_mask"], out[name + "_edge_mask"] = x, h, nm, em
        out[name + "_t_int"] = t_int.astype(np.int32)
        out[name + "_noise"] = np.stack([eps, eps0])
        out[name + "_nll"] = nll.numpy()
        out[name + "_terms"] = torch.stack([kl, loss_t, nlc, -lpxh, dlp, error], dim=1).numpy()
        out[name + "_snr_weight"] = snr.numpy()
        out[name + "_log_ph"] = log_ph
        out[name + "_zt"], out[name + "_z0"] = zt.numpy(), z0.numpy()
        out[name + "_phi_t"], out[name + "_phi_0"] = net_t.numpy(), net_0.numpy()
        print(f"g25 {name}: nll {nll.numpy()} max|log p(h|z0)| {np.abs(log_ph).max():.3g}")
    save("g25_nll", **out)


def _proj_summary(g, seed):
    """Compact record of a large gradient tensor: sum, sum of squares, 8 fixed random projections, 64 sampled entries
    (tests/test_gpu_pred_train.py:_proj_summary recomputes the same from the device gradient)."""
    g = np.asarray(g, np.float64).reshape(-1)
    r = np.random.Generator(np.random.Philox(key=seed))
    proj = r.standard_normal((8, g.size))
    idx = r.integers(0, g.size, 64)
    return np.concatenate([[g.sum(), (g * g).sum()], proj @ g, g[idx]]).astype(np.float64)


def g26_pred_grad():
    """compute_loss + loss.backward() of the predictor (cond_prediction/train_cond_predictor.py:64-81, 84-125) under injected
    noise: the full gradient of every tensor (None -> listed in *_nograd), the loss, for tiny cata / hetro predictors with
    attention and tanh on, one case with both off, t = 0, 500, T and mixed; two AdamW(amsgrad) steps of train_epoch on the
    tiny cata case; and one default-width case (nf 196, 2 layers) stored as per-tensor summaries."""
    from cond_prediction import train_cond_predictor as tcp
    out = {}
    cases = [  # name, dataset, nodes, predictor overrides, t tags
        ("cata", "cata", [4, 11, 7, 1, 11], dict(TINY_P, attention=True, tanh=True), ("t0", "tmix")),
        ("hetro", "hetro", [3, 9, 6, 10, 20], dict(TINY_P, attention=True, tanh=True), ("t500", "tT")),
        ("plain", "cata", [5, 11, 8], dict(TINY_P, attention=False, tanh=False), ("tmix",)),
        ("full", "cata", [11, 9, 11], dict(nf=196, n_layers=2), ("tmix",)),
    ]
    for ci, (name, ds, nodes, over, tags) in enumerate(cases):
        F = synth.num_node_features(ds)
        eargs = synth.edm_args(dataset=ds, **TINY)
        esd = synth.synth_edm_state_dict(eargs, F, seed=2600 + ci)
        a, model = build_ref_edm(ds, esd, **TINY)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **over), F, 5, seed=2610 + ci, amplify_coord=True)
        pa, pred = build_ref_pred(ds, psd, **over)
        for prm in pred.parameters():
            prm.requires_grad_(True)
        nm, em, z = case_inputs(ds, nodes, None, seed=2620 + ci, guidance_pad=(ds != "cata"))
        B, N, D = z.shape
        rng = np.random.default_rng(2630 + ci)
        x = (z[:, :, :3] * 3.0).astype(np.float32)
        cls = rng.integers(0, F, (B, N))
        h = (np.eye(F, dtype=np.float32)[cls] * nm).astype(np.float32)
        out[f"{name}_x"], out[f"{name}_h"] = x, h
        out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = nm, em
        tx, th, tnm, tem = (torch.from_numpy(v) for v in (x, h, nm, em))
        T = a.diffusion_steps
        names = list(pred.state_dict().keys())
        for tag in tags:
            t_int = dict(t0=np.zeros(B), t500=np.full(B, 500.0), tT=np.full(B, float(T)),
                         tmix=rng.integers(0, T + 1, B).astype(np.float64))[tag]
            eps = rng_noise(2640 + 10 * ci + len(tag), (B, N, D))
            t = torch.from_numpy((t_int / T).astype(np.float32)).view(B, 1)
            with InjectNoise([eps]), torch.no_grad():
                p0 = pred(tcp.sample_edm_t(tx, th, model, t, tnm), tnm, tem.view(B, N * N), t).numpy()
            sgn = np.where(rng.random(p0.shape) < 0.5, -1.0, 1.0)
            y = (p0 + sgn * (0.5 + rng.random(p0.shape))).astype(np.float32)
            randint0 = torch.randint
            torch.randint = lambda low, high, size, device=None, **kw: torch.from_numpy(t_int.reshape(B, 1)).long()
            try:
                pred.zero_grad(set_to_none=True)
                with InjectNoise([eps]):
                    loss, _ = tcp.compute_loss(pred, tx, th, tnm, tem, torch.from_numpy(y), model, a)
                loss.backward()
            finally:
                torch.randint = randint0
            k = f"{name}_{tag}"
            out[k + "_t_int"], out[k + "_eps"], out[k + "_y"] = t_int.astype(np.int32), eps, y
            out[k + "_loss"] = np.float32(loss.item())
            nograd = [n for n, prm in pred.named_parameters() if prm.grad is None]
            out[k + "_nograd"] = np.array(json.dumps(nograd))
            for n, prm in pred.named_parameters():
                if prm.grad is None:
                    continue
                if name == "full":
                    out[f"{k}_sum.{n}"] = _proj_summary(prm.grad.numpy(), 2650 + names.index(n))
                else:
                    out[f"{k}_g.{n}"] = prm.grad.numpy()
        if name == "cata":  # two steps of train_epoch's loop: zero_grad, backward, AdamW(amsgrad) step
            pred.load_state_dict({kk: torch.from_numpy(v.copy()) for kk, v in psd.items()})
            opt = torch.optim.AdamW(pred.parameters(), lr=pa.lr, amsgrad=True, weight_decay=1e-12)
            y = torch.from_numpy(rng.standard_normal((B, 5)).astype(np.float32))
            losses = []
            for step in range(2):
                t_int = rng.integers(0, T + 1, B).astype(np.float64)
                eps = rng_noise(2690 + step, (B, N, D))
                randint0 = torch.randint
                torch.randint = lambda low, high, size, device=None, **kw: torch.from_numpy(t_int.reshape(B, 1)).long()
                try:
                    with InjectNoise([eps]):
                        loss, _ = tcp.compute_loss(pred, tx, th, tnm, tem, y, model, a)
                finally:
                    torch.randint = randint0
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(loss.item())
                out[f"adam_{step}_t_int"], out[f"adam_{step}_eps"] = t_int.astype(np.int32), eps
            out["adam_y"], out["adam_losses"], out["adam_lr"] = y.numpy(), np.array(losses, np.float32), np.float32(pa.lr)
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, over=over, eseed=2600 + ci, pseed=2610 + ci, T=T,
                                                      tags=list(tags), names=names)))
        print(f"g26 {name}: N {N} losses {[float(out[f'{name}_{tg}_loss']) for tg in tags]}")
    save("g26_pred_grad", **{k: v for k, v in out.items() if not k.startswith(("hetro_", "plain_"))})
    save("g26_pred_grad_hetro", **{k: v for k, v in out.items() if k.startswith("hetro_")})
    save("g26_pred_grad_plain", **{k: v for k, v in out.items() if k.startswith("plain_")})


def g27_edm_grad():
    """EDM training, in float64: model.train(); loss = model(x, h, node_mask, edge_mask) (the per-molecule loss of compute_loss with
    t0_always = False, en_diffusion.py:644-805, before train_edm.py's .mean(0)); loss.sum().backward() under a fixed t_int
    (torch.randint patched) and InjectNoise([eps]).  Gradients are switched on for dynamics.* only (gamma.gamma keeps
    requires_grad=False).  Per case: per-molecule losses, net, the full gradients (tiny widths) or _proj_summary records
    (default widths), the no-grad list, and the parameter / state-dict key lists.  One file per group, as g26."""
    groups = {
        "g27_edm_grad": [  # name, dataset, nodes, max_nodes, over, weight seed, amplify, t_int rule
            ("cata_mixed", "cata", [4, 11, 7, 2, 11], 11, dict(TINY, diffusion_steps=50), 2700, True, "mixed"),
            ("cata_t0", "cata", [4, 11, 7, 2, 11], 11, dict(TINY, diffusion_steps=50), 2701, True, "zero"),
            ("cata_vlb", "cata", [4, 11, 7, 2, 11], 11, dict(TINY, diffusion_steps=50, diffusion_loss_type="vlb"), 2702, True,
             "mixed"),
        ],
        "g27_edm_grad_hetro": [
            ("hetro_500_T", "hetro", [3, 9, 6, 20], None, dict(TINY), 2703, True, "500_T"),
            ("plain_mean", "hetro", [5, 8, 10], None, dict(TINY, diffusion_steps=50, attention=False, tanh=False,
                                                          inv_sublayers=2, aggregation_method="mean", norm_constant=0.5,
                                                          coords_range=7.0), 2704, True, "mixed"),
            ("cata_sin", "cata", [4, 11, 7, 2, 11], 11, dict(TINY, diffusion_steps=50, sin_embedding=True), 2705, True,
             "mixed"),
        ],
        "g27_edm_grad_default": [
            ("cata_default", "cata", [11, 11, 11], 11, {}, 2706, False, "mixed"),
        ],
    }
    for fname, cases in groups.items():
        out = {}
        for ci, (name, ds, nodes, mx, over, wseed, amp, trule) in enumerate(cases):
            F = synth.num_node_features(ds)
            esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=wseed, amplify_coord=amp)
            a, model = build_ref_edm(ds, esd, **over)
            model.double()  # float64: the yardstick is the exact gradient, not one fp32 summation order
            for k, prm in model.named_parameters():
                prm.requires_grad_(k.startswith("dynamics."))
            model.train()
            nm, em, z = case_inputs(ds, nodes, mx, seed=wseed + 20, guidance_pad=mx is None)
            B, N, D = z.shape
            T = a.diffusion_steps
            rng = np.random.default_rng(wseed + 30)
            x = (z[:, :, :3] * 3.0).astype(np.float32)
            h = (np.eye(F, dtype=np.float32)[rng.integers(0, F, (B, N))] * nm).astype(np.float32)
            if trule == "zero":
                t_int = np.zeros(B, np.int64)
            elif trule == "500_T":
                t_int = np.array([min(500, T), T] * B)[:B]
            else:
                t_int = rng.integers(0, T + 1, B)
                t_int[0], t_int[-1] = 0, T
            eps = rng_noise(wseed + 40, (B, N, D))
            tx, th, tnm, tem = (torch.from_numpy(v).double() for v in (x, h, nm, em))
            hd = {"categorical": th, "integer": torch.zeros(0, dtype=torch.float64)}
            rec = []
            phi0, randint0 = model.phi, torch.randint

            def phi_rec(zz, tt, *rest):
                o = phi0(zz, tt, *rest)
                rec.append((zz.detach().clone(), tt.detach().clone(), o.detach().clone()))
                return o

            def randint_fixed(low, high, size, device=None, **kw):
                assert (low, high, tuple(size)) == (0, T + 1, (B, 1)), (low, high, size)
                return torch.from_numpy(t_int.reshape(B, 1)).long()

            model.phi = phi_rec
            torch.randint = randint_fixed
            try:
                with InjectNoise([eps], dtype=torch.float64):
                    loss = model(tx, hd, tnm, tem.view(B, N * N))
            finally:
                torch.randint = randint0
                del model.phi
            loss.sum().backward()
            assert len(rec) == 1
            # the per-molecule loss as the fp32 reference computes it (log p(h | z_0) at t = 0 is a difference of nearly equal
            # Phi values: the recorded loss is the fp32 one, the gradients the exact ones)
            _, m32 = build_ref_edm(ds, esd, **over)
            for k, prm in m32.named_parameters():
                prm.requires_grad_(k.startswith("dynamics."))
            m32.train()
            rec32 = []
            phi32 = m32.phi
            m32.phi = lambda zz, tt, *rest: rec32.append(phi32(zz, tt, *rest)) or rec32[-1]
            torch.randint = randint_fixed
            try:
                with InjectNoise([eps]):
                    loss32 = m32(*(torch.from_numpy(v) for v in (x,)), {"categorical": torch.from_numpy(h),
                                                                         "integer": torch.zeros(0)},
                                 torch.from_numpy(nm), torch.from_numpy(em).view(B, N * N))
            finally:
                torch.randint = randint0
                del m32.phi
            if over.get("sin_embedding"):  # the fp32 reference's own spread from the exact values (the tests' bound)
                loss32.sum().backward()
                out[name + "_net32"] = rec32[0].detach().numpy()
                for k, prm in m32.named_parameters():
                    if prm.grad is not None:
                        out[name + "_grad32:" + k] = prm.grad.numpy()
            loss32 = loss32.detach()
            zt, _, net = rec[0]
            names = [k for k, _ in model.named_parameters()]
            nograd = [k for k, prm in model.named_parameters() if prm.grad is None]
            out[name + "_cfg"] = np.array(json.dumps(dict(dataset=ds, over=over, wseed=wseed, amp=amp, nodes=nodes, T=T)))
            out[name + "_x"], out[name + "_h"], out[name + "_node_mask"], out[name + "_edge_mask"] = x, h, nm, em
            out[name + "_t_int"] = t_int.astype(np.int32)
            out[name + "_noise"] = eps
            out[name + "_loss"] = loss32.numpy()
            out[name + "_loss64"] = loss.detach().numpy()
            out[name + "_zt"], out[name + "_net"] = zt.numpy().astype(np.float32), net.numpy()
            out[name + "_params"] = np.array(json.dumps(names))
            out[name + "_state_keys"] = np.array(json.dumps(list(model.state_dict().keys())))
            out[name + "_nograd"] = np.array(json.dumps(nograd))
            for pi, (k, prm) in enumerate(model.named_parameters()):
                if prm.grad is None:
                    continue
                g = prm.grad.numpy()
                if name == "cata_default":
                    out[name + "_gsum:" + k] = _proj_summary(g, 2790 + pi)
                else:
                    out[name + "_grad:" + k] = g.astype(np.float32)
            print(f"g27 {name}: loss {loss.detach().numpy()} t {t_int} nograd {nograd}")
        save(fname, **out)


def g27_edm_train():
    """EDM training loop and initialisation (g27_edm_train): two iterations of train_edm.py:52-94 on the tiny cata case --
    compute_loss in train mode, zero_grad, backward, edm/utils.py gradient_clipping with the Queue seeded with 3000
    (train_edm.py:155-156), AdamW(lr, amsgrad=True, weight_decay=1e-12) (:152-154) -- with t_int and the noise fixed per
    iteration: losses, grad norms and the trained dynamics.* weights.  And the reference's fresh state dict after
    torch.manual_seed(0) (get_model without restore) for a tiny config with attention and one with two sub-layers."""
    import train_edm as ref_train
    from edm.utils import Queue as RQueue, gradient_clipping as rclip
    out = {}
    ds, nodes, over, wseed = "cata", [4, 11, 7, 2, 11], dict(TINY, diffusion_steps=50), 2710
    F = synth.num_node_features(ds)
    esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=wseed, amplify_coord=True)
    a, model = build_ref_edm(ds, esd, **over)
    for k, prm in model.named_parameters():
        prm.requires_grad_(k.startswith("dynamics."))
    nm, em, z = case_inputs(ds, nodes, 11, seed=wseed + 20)
    B, N, D = z.shape
    T = a.diffusion_steps
    rng = np.random.default_rng(wseed + 30)
    x = (z[:, :, :3] * 3.0).astype(np.float32)
    h = (np.eye(F, dtype=np.float32)[rng.integers(0, F, (B, N))] * nm).astype(np.float32)
    optim = torch.optim.AdamW(model.parameters(), lr=a.lr, amsgrad=True, weight_decay=1e-12)
    q = RQueue(max_len=50)
    q.add(3000)
    losses, norms, ts, epss = [], [], [], []
    randint0 = torch.randint
    for it in range(2):
        t_int = rng.integers(0, T + 1, B)
        eps = rng_noise(wseed + 40 + it, (B, N, D))

        def randint_fixed(low, high, size, device=None, **kw):
            assert (low, high, tuple(size)) == (0, T + 1, (B, 1)), (low, high, size)
            return torch.from_numpy(t_int.reshape(B, 1)).long()

        model.train()
        torch.randint = randint_fixed
        try:
            with InjectNoise([eps]):
                loss = ref_train.compute_loss(model, torch.from_numpy(x), torch.from_numpy(h), torch.from_numpy(nm),
                                              torch.from_numpy(em))
        finally:
            torch.randint = randint0
        optim.zero_grad()
        loss.backward()
        gn = rclip(model, q)
        optim.step()
        losses.append(loss.item())
        norms.append(float(gn))
        ts.append(t_int.astype(np.int32))
        epss.append(eps)
    out["train_cfg"] = np.array(json.dumps(dict(dataset=ds, over=over, wseed=wseed, amp=True, nodes=nodes, T=T, lr=a.lr)))
    out["train_x"], out["train_h"], out["train_node_mask"], out["train_edge_mask"] = x, h, nm, em
    out["train_t_int"], out["train_noise"] = np.stack(ts), np.stack(epss)
    out["train_loss"], out["train_grad_norm"] = np.array(losses), np.array(norms)
    for k, v in model.state_dict().items():
        if k.startswith("dynamics."):
            out["train_w:" + k] = v.numpy()
    for name, o in (("init_att", dict(TINY)), ("init_plain", dict(TINY, attention=False, inv_sublayers=2,
                                                                         sin_embedding=True))):
        ra = Args_EDM().parse_args([])
        ra.device, ra.dp, ra.restore, ra.dataset = torch.device("cpu"), False, None, "cata"
        for k, v in o.items():
            setattr(ra, k, v)
        torch.manual_seed(0)
        m, _, _ = models_edm.get_model(ra, FakeLoader(1, 5), only_norm=True)
        out[name + "_cfg"] = np.array(json.dumps(o))
        out[name + "_keys"] = np.array(json.dumps(list(m.state_dict().keys())))
        for k, v in m.state_dict().items():
            out[name + ":" + k] = v.numpy()
    print(f"g27_edm_train: losses {losses} grad norms {norms}")
    save("g27_edm_train", **out)


G28_PAIRS = [(1000, 998), (1000, 990), (1000, 950), (500, 498), (500, 490), (500, 450), (2, 0), (10, 0), (50, 0), (1000, 0)]


def _spread(a32, a64):
    return np.float64(np.abs(a32.astype(np.float64) - a64).max() / max(np.abs(a64).max(), 1e-30))


def _g28_time_grid(t_start, n_steps):
    """gaudi_amd.sampling_edm.time_grid, restated so the fixture does not depend on the code under test."""
    return [int((2 * t_start * (n_steps - k) + n_steps) // (2 * n_steps)) for k in range(n_steps + 1)]


def _g28_chain(model, T, grid, z, tnm, tem, noise, dt, tf=None, scale=0.0):
    """The reference's sample / sample_guidance loop (en_diffusion.py:982-1067) over the pairs of a time grid instead of
    t = s + 1: its own sample_p_zs_given_zt[_guidance](s, t), then sample_p_xh_given_z0 and the CoG re-projection.  noise
    [T+2,B,N,D] is keyed by time index: the step that lands on s draws row T - s, the decode row T + 1."""
    B = z.shape[0]
    eps = [noise[T - s] for s in grid[1:]] + [noise[T + 1]]
    with InjectNoise(eps, dt), torch.no_grad():
        for t_i, s_i in zip(grid[:-1], grid[1:]):
            st = (torch.full((B, 1), s_i) / T).to(dt)
            tt = (torch.full((B, 1), t_i) / T).to(dt)
            if tf is None:
                z = model.sample_p_zs_given_zt(st, tt, z, tnm, tem, None)
            else:
                z = model.sample_p_zs_given_zt_guidance(st, tt, z, tnm, tem, tf, scale)
        x, h = model.sample_p_xh_given_z0(z, tnm, tem, None)
        if torch.sum(x, dim=1, keepdim=True).abs().max().item() > 5e-2:
            x = x - x.sum(1, keepdim=True) / tnm.sum(1, keepdim=True) * tnm  # remove_mean_with_mask (utils.py:33-44)
    return x.numpy(), h["categorical"].numpy().astype(np.float32)


def g28_grid():
    """Chains on a time grid (gaudi_sample_grid): the reference's step functions take ANY pair s < t (en_diffusion.py:807-935);
    only its loops fix t = s + 1.  g28_grid_steps: the scalars of G28_PAIRS for both schedules, and teacher-forced unguided /
    guided steps for those pairs (tiny cata and hetro widths, default widths).  g28_grid_chains: T = 50 chains on
    time_grid(50, 10) and time_grid(50, 7) from the prior, and refinement chains from given molecules noised to t_start = 20
    by sample_edm_t, in 20 and 5 steps.  Every output is computed by the fp32 reference and by the reference in float64;
    *_spread is the max-norm distance of the two.  (Chain noise seeds 2875..: with 2870.. the reference's own spread of ONE
    non-amplified guided chain on the uneven grid was 1.3e-4 -- a chain that close to a branch of its own says nothing about
    a port; milder inputs instead of a wider bound.)"""
    from cond_prediction.train_cond_predictor import sample_edm_t
    out = {}
    T = 1000
    out["pairs"] = np.array(G28_PAIRS, np.int32)
    for sched, over in (("polynomial_2", {}), ("cosine", dict(diffusion_noise_schedule="cosine", normalize_factors=[1, 2, 2]))):
        sd = synth.synth_edm_state_dict(synth.edm_args(nf=8, n_layers=1), 1, seed=0)
        a, model = build_ref_edm("cata", sd, nf=8, n_layers=1, diffusion_steps=T, **over)
        rows = []
        for t_i, s_i in G28_PAIRS:
            st, tt = torch.full((1, 1), s_i) / T, torch.full((1, 1), t_i) / T
            gs, gt = model.gamma(st), model.gamma(tt)
            zt = torch.zeros(1, 1, 1)
            s2, s_ts, a_ts = model.sigma_and_alpha_t_given_s(gt, gs, zt)
            sig_s, sig_t = model.sigma(gs, zt), model.sigma(gt, zt)
            rows.append([t_i, s_i, a_ts.item(), (s2 / a_ts / sig_t).item(), (s_ts * sig_s / sig_t).item(), tt.item()])
        out[f"coef_{sched}"] = np.array(rows, dtype=np.float64)  # t, s, alpha_t|s, sigma2_t|s / alpha_t|s / sigma_t, sigma, t / T
    cases = [("cata", "cata", [4, 11, 7, 11], TINY, TINY_P, True), ("hetro", "hetro", [3, 9, 6], TINY, TINY_P, True),
             ("cata_full", "cata", [11, 8], dict(nf=192, n_layers=9), dict(nf=196, n_layers=12), False)]
    for ci, (name, ds, nodes, eo, po, amp) in enumerate(cases):
        F = synth.num_node_features(ds)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **eo), F, seed=2800 + ci, amplify_coord=amp)
        a, model = build_ref_edm(ds, esd, **eo)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **po), F, 5, seed=2810 + ci, amplify_coord=amp)
        pa, pred = build_ref_pred(ds, psd, **po)
        nm, em, z = case_inputs(ds, nodes, None, seed=2820 + ci, guidance_pad=True)
        B, N, D = z.shape

        def tf_gap(_in, _nm, _em, _t):
            return -pred(_in, _nm, _em, _t)[:, 1]

        out[f"{name}_z"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = z, nm, em
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=2800 + ci, pseed=2810 + ci, T=T, amp=amp, eover=eo, pover=po)))
        res = {}
        for dt, tag in ((torch.float32, "fp32"), (torch.float64, "fp64")):
            if dt == torch.float64:
                model.double()
                pred.double()
            tnm, tem, tz = torch.from_numpy(nm).to(dt), torch.from_numpy(em).to(dt), torch.from_numpy(z).to(dt)
            for t_i, s_i in G28_PAIRS:
                eps = rng_noise(2830 + 10 * ci + s_i % 7, (B, N, D))
                st, tt = (torch.full((B, 1), s_i) / T).to(dt), (torch.full((B, 1), t_i) / T).to(dt)
                with InjectNoise([eps], dt), torch.no_grad():
                    res[(tag, t_i, s_i, "unguided")] = model.sample_p_zs_given_zt(st, tt, tz, tnm, tem, None).numpy()
                for scale in (0.6, 400.0):
                    with InjectNoise([eps], dt), torch.no_grad():
                        res[(tag, t_i, s_i, f"guided_scale{scale}")] = model.sample_p_zs_given_zt_guidance(
                            st, tt, tz, tnm, tem, tf_gap, scale).numpy()
                out[f"{name}_t{t_i}_s{s_i}_eps"] = eps
        for (tag, t_i, s_i, kind), v in res.items():
            if tag == "fp32":
                out[f"{name}_t{t_i}_s{s_i}_zs_{kind}"] = v
                out[f"{name}_t{t_i}_s{s_i}_zs_{kind}_spread"] = _spread(v, res[("fp64", t_i, s_i, kind)])
        worst = max(float(v) for k, v in out.items() if k.startswith(name) and k.endswith("_spread"))
        over_bar = [k for k, v in out.items() if k.startswith(name) and k.endswith("_spread") and float(v) >= 5e-5]
        print(f"g28 steps {name}: worst fp32-vs-fp64 spread {worst:.2e}; at or above 5e-5: {over_bar}")
    save("g28_grid_steps", **out)

    out = {}
    T = 50
    for ci, (name, ds, nodes, amp) in enumerate([("cata_tiny", "cata", [6, 8, 8, 3], False), ("hetro_tiny", "hetro", [3, 5, 4], False),
                                                 ("cata_tiny_amp", "cata", [6, 8, 8, 3], True)]):
        F = synth.num_node_features(ds)
        over = dict(diffusion_steps=T, **TINY)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=2850 + ci, amplify_coord=amp)
        a, model = build_ref_edm(ds, esd, **over)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, 5, seed=2860 + ci, amplify_coord=amp)
        pa, pred = build_ref_pred(ds, psd, **TINY_P)

        def tf_gap(_in, _nm, _em, _t):
            return -pred(_in, _nm, _em, _t)[:, 1]

        nm, em = masks(ds, nodes, None)
        B, N = nm.shape[0], nm.shape[1]
        D = 3 + F
        noise = rng_noise(2875 + ci, (T + 2, B, N, D))
        # given molecules for the refinement: masked, mean-free coordinates of a few Angstrom and a ring type per node
        rng = np.random.default_rng(2880 + ci)
        x0 = (rng.standard_normal((B, N, 3)) * 2.5).astype(np.float32) * nm
        x0 = (x0 - x0.sum(1, keepdims=True) / np.maximum(nm.sum(1, keepdims=True), 1) * nm).astype(np.float32)
        oh0 = np.zeros((B, N, F), np.float32)
        np.put_along_axis(oh0, rng.integers(0, F, (B, N, 1)), 1.0, axis=2)
        oh0 *= nm
        out[f"{name}_noise"], out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = noise, nm, em
        out[f"{name}_x0"], out[f"{name}_onehot0"] = x0, oh0
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, T=T, eseed=2850 + ci, pseed=2860 + ci, nodes=nodes, amp=amp,
                                                      std_unguided=0.7, std_guided=1.0, scale=0.6, t_start=20)))
        res = {}
        for dt, tag in ((torch.float32, "fp32"), (torch.float64, "fp64")):
            if dt == torch.float64:
                model.double()
                pred.double()
            tnm, tem = torch.from_numpy(nm).to(dt), torch.from_numpy(em).to(dt)
            for n_steps in (10, 7):
                grid = _g28_time_grid(T, n_steps)
                out[f"{name}_grid{n_steps}"] = np.array(grid, np.int32)
                for kind, std, tf, scale in (("unguided", 0.7, None, 0.0), ("guided", 1.0, tf_gap, 0.6)):
                    with InjectNoise([noise[0]], dt):
                        zT = model.sample_combined_position_feature_noise(B, N, tnm, std)
                    res[(tag, f"prior{n_steps}_{kind}")] = _g28_chain(model, T, grid, zT, tnm, tem, noise, dt, tf, scale)
            with InjectNoise([noise[0]], dt), torch.no_grad():
                tt = (torch.full((B, 1), 20) / T).to(dt)
                zt = sample_edm_t(torch.from_numpy(x0).to(dt), torch.from_numpy(oh0).to(dt), model, tt, tnm)
            res[(tag, "zt20")] = (zt.numpy(),)
            for n_steps in (20, 5):
                grid = _g28_time_grid(20, n_steps)
                out[f"{name}_refine_grid{n_steps}"] = np.array(grid, np.int32)
                for kind, tf, scale in (("unguided", None, 0.0), ("guided", tf_gap, 0.6)):
                    res[(tag, f"refine{n_steps}_{kind}")] = _g28_chain(model, T, grid, zt, tnm, tem, noise, dt, tf, scale)
        for (tag, key), v in res.items():
            if tag != "fp32":
                continue
            v64 = res[("fp64", key)]
            if key == "zt20":
                out[f"{name}_zt20"], out[f"{name}_zt20_spread"] = v[0], _spread(v[0], v64[0])
                continue
            out[f"{name}_{key}_x"], out[f"{name}_{key}_h"] = v
            out[f"{name}_{key}_x_spread"] = _spread(v[0], v64[0])
            out[f"{name}_{key}_h_equal_fp64"] = np.array(np.array_equal(v[1], v64[1]))
        for k, v in out.items():
            if k.startswith(name + "_") and k.endswith("_spread"):
                print(f"g28 chains {k}: {float(v):.2e}")
    save("g28_grid_chains", **out)


def _g29_params(seed, B, K, scale_lo, scale_hi):
    """Per-molecule value-target parameters (models_edm.ValueTarget): every side occurs, scales spread over [lo, hi]."""
    rng = np.random.default_rng(seed)
    w = (0.5 * rng.standard_normal((B, K))).astype(np.float32)
    q = rng.uniform(0.2, 1.5, (B, K)).astype(np.float32)
    c = (0.5 * rng.standard_normal((B, K))).astype(np.float32)
    side = rng.integers(-1, 2, (B, K)).astype(np.int32)
    side[:, :3] = np.array([0, 1, -1], np.int32)  # (each form in every molecule, whatever the draw)
    scale = np.exp(rng.uniform(np.log(scale_lo), np.log(scale_hi), B)).astype(np.float32)
    return dict(w=w, q=q, c=c, side=side, scale=scale)


def _g29_closure(pred, par):
    """The value-target family as a closure the reference differentiates: per-molecule tensors, the per-molecule scale folded
    in (the reference call runs with scale = 1)."""
    w, q, c, scale = (torch.from_numpy(par[k]) for k in ("w", "q", "c", "scale"))
    side = torch.from_numpy(par["side"])

    def tf(_in, _nm, _em, _t):
        p = pred(_in, _nm, _em, _t)
        d = p - c
        a = torch.where(side == 0, d, torch.where(side > 0, d.clamp(min=0), d.clamp(max=0)))
        return scale * ((w * p).sum(1) + (q * a * a).sum(1))

    return tf


def g29_value_target():
    """Value-seeking targets with per-molecule parameters (aim at a value, upper and lower bounds, per-molecule strength):
    teacher-forced steps through the reference's sample_p_zs_given_zt_guidance at the tiny and the default widths, and T = 50
    chains through its sample_guidance at the tiny cata / hetero widths of g7, injected noise."""
    out = {}
    K, T = 5, 1000
    for tag, ds, nodes, over, over_p, eseed, pseed in (("tiny", "hetro", [3, 5, 4], TINY, TINY_P, 2900, 2910),
                                                       ("default", "cata", [11, 7], {}, {}, 2901, 2911)):
        F = synth.num_node_features(ds)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=eseed, amplify_coord=True)
        a, model = build_ref_edm(ds, esd, **over)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **over_p), F, K, seed=pseed, amplify_coord=True)
        pa, pred = build_ref_pred(ds, psd, **over_p)
        nm, em, z = case_inputs(ds, nodes, None, seed=2920, guidance_pad=True)
        B, N, D = z.shape
        tnm, tem = torch.from_numpy(nm), torch.from_numpy(em)
        out[f"{tag}_z"], out[f"{tag}_node_mask"], out[f"{tag}_edge_mask"] = z, nm, em
        steps = (0, 500, 999) if tag == "tiny" else (500,)
        for strength, (lo, hi) in (("weak", (0.2, 1.0)), ("strong", (100.0, 600.0))):  # strong: the clip branch
            par = _g29_params(2930 + (strength == "strong"), B, K, lo, hi)
            for k, v in par.items():
                out[f"{tag}_{strength}_{k}"] = v
            tf = _g29_closure(pred, par)
            for s in steps:
                eps = rng_noise(2940 + s % 7, (B, N, D))
                st = torch.full((B, 1), s) / T
                tt = (torch.full((B, 1), s) + 1) / T
                out[f"{tag}_s{s}_eps"] = eps
                with InjectNoise([eps]), torch.no_grad():
                    zg = model.sample_p_zs_given_zt_guidance(st, tt, torch.from_numpy(z), tnm, tem, tf, 1.0).numpy()
                out[f"{tag}_{strength}_s{s}_zs"] = zg
        out[f"{tag}_cfg"] = np.array(json.dumps(dict(dataset=ds, eseed=eseed, pseed=pseed, T=T, nodes=nodes, steps=list(steps), amp=True)))
    Tc = 50
    for ci, (name, ds, nodes) in enumerate([("cata_chain", "cata", [6, 8, 8, 3]), ("hetro_chain", "hetro", [3, 5, 4])]):
        F = synth.num_node_features(ds)
        over = dict(diffusion_steps=Tc, **TINY)
        esd = synth.synth_edm_state_dict(synth.edm_args(dataset=ds, **over), F, seed=2950 + ci, amplify_coord=False)
        a, model = build_ref_edm(ds, esd, **over)
        psd = synth.synth_predictor_state_dict(synth.pred_args(dataset=ds, **TINY_P), F, K, seed=2960 + ci, amplify_coord=False)
        pa, pred = build_ref_pred(ds, psd, **TINY_P)
        par = _g29_params(2970 + ci, len(nodes), K, 0.2, 1.0)
        Nn = max(nodes) * (2 if ds != "cata" else 1)
        noise = rng_noise(2980 + ci, (Tc + 2, len(nodes), Nn, 3 + F))
        with InjectNoise(list(noise)):
            x, h, nm, em = ref_sampling.sample_guidance(a, model, _g29_closure(pred, par), torch.tensor(nodes), scale=1.0, std=1.0)
        for k, v in par.items():
            out[f"{name}_{k}"] = v
        out[f"{name}_noise"], out[f"{name}_x"], out[f"{name}_h"] = noise, x.numpy(), h.numpy().astype(np.float32)
        out[f"{name}_node_mask"], out[f"{name}_edge_mask"] = nm.numpy(), em.numpy()
        out[f"{name}_cfg"] = np.array(json.dumps(dict(dataset=ds, T=Tc, eseed=2950 + ci, pseed=2960 + ci, nodes=nodes, amp=False)))
    save("g29_value_target", **out)


def _g30_graph(types, bonds, names):
    import networkx as nx
    g = nx.Graph()
    for i, t in enumerate(types):
        g.add_node(i, el=names[int(t)])
    g.add_edges_from((int(a), int(b)) for a, b in bonds)
    return g


def _g30_same(g1, g2):
    import networkx as nx
    return nx.is_isomorphic(g1, g2, node_match=lambda a, b: a["el"] == b["el"])


def g30_gor2goa():
    """Graph of rings -> graph of atoms (data/gor2goa.py:133-261) on seeded synthetic molecules, a few inputs the reference raises
    on and the capacity edge.  Per molecule: the inputs, `threw`, the reference's atom types, sorted bond list and atom positions
    (the pairwise distance matrix is a function of those: the tests form it in float64; stored as a matrix it would not fit a
    committed file), `stable` (check_stability, all flags), `iso_class` (exact isomorphism with element match over the whole set),
    `dist_spread` and a twin: the same molecule with its rings permuted, rotated and reflected, and the twin's own class.

    Tie filter: the discrete result of gor2goa flips on exact ties (argmin, the > 0 masks), which no implementation can be held
    to.  Every candidate is re-run on 8 copies perturbed at relative 2^-23 and on its twin; it is dropped when the atom types or
    the bond set change (copies) or the result is not isomorphic (twin).  At most 10 % may be dropped.  dist_spread = the
    largest change of the distance matrix over the 8 copies."""
    from analyze import analyze as ref_an
    from data.aromatic_dataloader import ATOMS_LIST
    from data.gor2goa import gor2goa
    tables = json.load(open(os.path.join(ROOT, "gaudi_amd", "data", "ring_tables.json")))
    rng = np.random.default_rng(3000)
    DOT = len(tables["rings"]["hetro"]) - 1
    # (dataset, x, types, kind); kind 0 = synthetic, 1 = special (kept whatever the filters say about ties), 2 = a special whose
    # result depends on the ring order by construction: its twin is rotated and reflected but keeps the order
    cands = []
    for i in range(84):
        n = 1 + i % 11
        x = synth_cata_molecule(rng, n, tree_prob=[1.0, 1.0, 0.5][i % 3], jitter=[0.01, 0.03][i % 2], zjit=[0.0, 0.02][(i // 2) % 2])
        cands.append(("cata", x, np.zeros(len(x), np.int64), 0))
    from utils import helpers as ref_h
    n_rejected = 0
    for i in range(84):
        while True:  # geometry check, not a tie filter: the grown molecule must have the fused pairs it was grown with
            x, ty, pairs = synth_hetro_fused(rng, 2 + i % 9, tables, jitter=[0.01, 0.03][i % 2])
            k = len(x) // 2
            _, adj = ref_h.positions2adj(torch.from_numpy(x[None, :k].copy()), torch.from_numpy(ty[None, :k].copy()), 0.1, dataset="hetro")
            if {(int(a), int(b)) for a, b in zip(*np.triu(adj[0].numpy()).nonzero())} == pairs and k >= 2:
                break
            n_rejected += 1
        cands.append(("hetro", x, ty, 0))
    print(f"g30: {n_rejected} grown hetero molecules re-drawn (a fused pair outside the reference's distance windows)")
    f32 = lambda a: np.array(a, np.float32)
    pair = f32([[-1.225, 0.02, 0], [1.225, -0.02, 0.01]])
    specials = [
        ("cata", f32([[0.3, -0.2, 0.1]]), [0]),                                             # a single ring
        ("cata", pair, [0, 0]),                                                             # a pair
        ("cata", f32([[2.45 * (k - 15.5), 0.013 * np.sin(1.7 * k), 0.009 * np.cos(2.3 * k)] for k in range(32)]), [0] * 32),  # capacity edge
        ("cata", f32([[0, 0, 0], [2.45, 0.03, 0], [9, 0.1, 0], [11.45, 0.05, 0.02]]), [0] * 4),  # two far-apart pairs: builds
        ("cata", f32([[0, 0, 0], [2.45, 0.03, 0], [9, 0.1, 0]]), [0] * 3),                  # a pair and a lone ring: raises
        ("hetro", f32([[0, 0, 0], [2.45, 0.03, 0], [0.1, 0.5, 0], [2.5, 0.6, 0]]), [0, DOT, DOT, DOT]),  # "." as a ring: raises
        ("hetro", f32([[0, 0, 0], [0.4, 0.3, 0]]), [DOT, DOT]),                             # "." as the only ring: raises
        ("hetro", f32([[0, 0, 0], [2.45, 0.03, 0], [4.9, -0.02, 0], [0.1, 0.5, 0], [2.5, 0.6, 0]]), [0, 0, 0, DOT, DOT]),  # odd node count
        ("hetro", f32([[0.5, 0.2, 0]]), [DOT]),                                             # one orientation node, no ring: raises
    ]
    for ds, x, ty in specials:
        cands.append((ds, x, np.array(ty, np.int64), 1))
    # pyridine (ring 0) and benzene fused across the N-C edge: each merged atom has a different element on the two rings, and
    # gor2goa gives it ring i's (i < j) -- one N, where ring j's element would give none.  The grown molecules share C-C edges only.
    hn = tables["rings"]["hetro"]
    cands.append(("hetro", f32([[0.01, -0.02, 0], [2.077, 1.199, 0.015], [1.31, 0.02, 0], [2.09, 1.21, 0]]),
                  np.array([hn.index("Pd"), hn.index("Bn"), DOT, DOT], np.int64), 2))

    def run(ds, x, ty):
        try:
            a, t, b = gor2goa(torch.from_numpy(np.ascontiguousarray(x, np.float32).copy()), torch.from_numpy(ty.copy()), ds)
        except Exception:
            return None
        return a.numpy().astype(np.float64), t.numpy().astype(np.int64), sorted((int(p), int(q)) for p, q in b)

    def pdist(a):
        return np.sqrt(((a[:, None] - a[None]) ** 2).sum(-1))

    kept, dropped = [], {"cata": 0, "hetro": 0}
    for ds, x, ty, kind in cands:
        names = ATOMS_LIST[ds]
        res = run(ds, x, ty)
        rec = dict(ds=ds, x=x, ty=ty, threw=res is None, spread=0.0)
        # the twin: rings permuted (orientation nodes along with them), then a random rotation and a reflection
        n = len(x)
        nr = n if ds == "cata" else n // 2
        perm = rng.permutation(nr) if kind != 2 else np.arange(nr)
        full = np.concatenate([perm, nr + perm, np.arange(2 * nr, n)]) if ds != "cata" else perm
        Q = _rand_rot(rng)
        Q[:, 0] *= -1.0 if np.linalg.det(Q) > 0 else 1.0  # det -1: a reflection is in
        rec["tx"], rec["tty"] = (x[full].astype(np.float64) @ Q).astype(np.float32), ty[full]
        if res is not None:
            atoms, types, bonds = res
            ok = True
            d0 = pdist(atoms)
            for k in range(8):
                xp = (x.astype(np.float64) * (1.0 + rng.uniform(-1, 1, x.shape) * 2.0 ** -23)).astype(np.float32)
                rp = run(ds, xp, ty)
                if rp is None or not np.array_equal(rp[1], types) or rp[2] != bonds:
                    ok = False
                    break
                rec["spread"] = max(rec["spread"], float(np.abs(pdist(rp[0]) - d0).max()))
            rt = run(ds, rec["tx"], rec["tty"])
            if ok and (rt is None or not _g30_same(_g30_graph(types, bonds, names), _g30_graph(rt[1], rt[2], names))):
                ok = False
            if not ok:
                if kind >= 1:
                    raise RuntimeError("a special molecule of g30 sits on a tie: move it")
                dropped[ds] += 1
                continue
            rec.update(atoms=atoms, types=types, bonds=np.array(bonds, np.int64).reshape(-1, 2), twin=rt)
            st = ref_an.check_stability(torch.from_numpy(x.copy()), torch.from_numpy(ty.copy()), dataset=ds)
            rec["stable"] = all(bool(st[k]) for k in ("orientation_nodes", "dist_stable", "connected", "angels3", "angels4"))
        else:
            rec.update(atoms=np.zeros((0, 2)), types=np.zeros(0, np.int64), bonds=np.zeros((0, 2), np.int64), twin=None, stable=False)
        kept.append(rec)
    total = len(cands)
    n_drop = sum(dropped.values())
    print(f"g30: dropped {n_drop} of {total} candidates on ties ({dropped}); cap {total // 10}")
    assert n_drop * 10 <= total, "tie filter dropped more than 10 %"

    # classes under exact isomorphism, originals and twins together
    reps, cls, tcls = [], [], []
    def classify(ds, types, bonds):
        g = _g30_graph(types, bonds, ATOMS_LIST[ds])
        sig = (g.number_of_nodes(), g.number_of_edges(), tuple(sorted(ATOMS_LIST[ds][int(t)] for t in types)),
               tuple(sorted(d for _, d in g.degree())))
        for k, (s2, g2) in enumerate(reps):
            if s2 == sig and _g30_same(g, g2):
                return k
        reps.append((sig, g))
        return len(reps) - 1
    for r in kept:
        cls.append(-1 if r["threw"] else classify(r["ds"], r["types"], r["bonds"]))
    for r in kept:
        tcls.append(-1 if r["twin"] is None else classify(r["ds"], r["twin"][1], r["twin"][2]))
    M = len(kept)
    NM = max(len(r["x"]) for r in kept)
    X = np.zeros((M, NM, 3), np.float32)
    TX = np.zeros((M, NM, 3), np.float32)
    TY = np.zeros((M, NM), np.int8)
    TTY = np.zeros((M, NM), np.int8)
    for m, r in enumerate(kept):
        k = len(r["x"])
        X[m, :k], TX[m, :k], TY[m, :k], TTY[m, :k] = r["x"], r["tx"], r["ty"], r["tty"]
    aoff = np.concatenate([[0], np.cumsum([len(r["types"]) for r in kept])]).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum([len(r["bonds"]) for r in kept])]).astype(np.int64)
    n_stable_cata = sum(r["stable"] and r["ds"] == "cata" for r in kept)
    print(f"g30: {M} molecules kept, {sum(r['threw'] for r in kept)} raise, {len(reps)} isomorphism classes, "
          f"{n_stable_cata} stable cata, largest dist_spread {max(r['spread'] for r in kept):.2e}")
    save("g30_gor2goa", x=X, types=TY, n=np.array([len(r["x"]) for r in kept], np.int32),
         hetro=np.array([r["ds"] == "hetro" for r in kept]), threw=np.array([r["threw"] for r in kept]),
         stable=np.array([r["stable"] for r in kept]), atom_off=aoff, bond_off=boff,
         ref_atoms=np.concatenate([r["atoms"] for r in kept]).astype(np.float64),
         ref_types=np.concatenate([r["types"] for r in kept]).astype(np.int8),
         ref_bonds=np.concatenate([r["bonds"] for r in kept]).astype(np.int16),
         iso_class=np.array(cls, np.int32), dist_spread=np.array([r["spread"] for r in kept], np.float64),
         twin_x=TX, twin_types=TTY, twin_iso_class=np.array(tcls, np.int32))


def _g31_hexes(centres, r=1.40):
    """Carbon skeleton of fused regular hexagons (pointy top) around the given 2-D centres: shared corners once."""
    pts = []
    for cx, cy in centres:
        for k in range(6):
            p = (cx + r * np.cos(np.pi / 6 + k * np.pi / 3), cy + r * np.sin(np.pi / 6 + k * np.pi / 3))
            if not any(abs(p[0] - q[0]) + abs(p[1] - q[1]) < 1e-6 for q in pts):
                pts.append(p)
    return np.array(pts)


def g31_goa2gor():
    """Graph of atoms -> graph of rings: the reference's own get_connectivity_matrix / get_rings / get_rings_adj (through xyz files
    and load_xyz) and AromaticDataset.get_all on the atoms g30's molecules were built into, plus hand-written specials.

    Inputs: every non-raising molecule of g30, its reference atoms lifted to 3-D (z = 0), template H (parked at the origin) dropped,
    under its own seeded rotation and translation, coordinates rounded to float32 values (stored as float32: the size limit of a
    committed fixture; the reference reads them back exactly from `repr`-precision xyz files).  Recorded per molecule: the inputs,
    `threw`, `expect` (specials: the status the kernel must give, else -1), the rings in ascending order of their sorted atom tuples
    (`g30_index`: the g30 molecule it was built from, else -1; atom sets, types, float64 centres, the float32 x of get_rings, orientation candidates as atom indices -- the reference returns
    the atoms' own coordinates, asserted here; -1 = the centre), the ring adjacency, `basis_ok` (networkx's minimum cycle basis
    equals the set of chordless cycles of 4..6 atoms and their number is E - V + C) and `margin` (smallest |distance - cutoff| over
    heavy pairs).  For 8 hetero and 4 cata molecules: the tensors of AromaticDataset.get_all with normalize=True.
    Tie filter: margin < 1e-9 is dropped, at most 10 %.  Prints the rate of the reference's get_rings path on this CPU."""
    import random
    import tempfile
    import time
    import networkx as nx
    import pandas as pd
    from data import aromatic_dataloader as adl
    from data.mol import load_xyz
    from utils.const import __COV_RADII__
    from utils.molgraph import get_connectivity_matrix, get_edges
    from utils.ring_graph import get_rings, get_rings_adj
    g30 = np.load(os.path.join(OUT, "g30_gor2goa.npz"))
    rng = np.random.default_rng(3100)
    cands = []  # (dataset, symbols, xyz float64 of float32 values, use_h, expect)

    def place(xy_or_xyz):
        p = np.asarray(xy_or_xyz, np.float64)
        if p.shape[1] == 2:
            p = np.concatenate([p, np.zeros((len(p), 1))], 1)
        return ((p @ _rand_rot(rng)) + rng.uniform(-4, 4, 3)).astype(np.float32).astype(np.float64)

    for m in range(len(g30["n"])):
        if g30["threw"][m]:
            continue
        ds = "hetro" if g30["hetro"][m] else "cata"
        a0, a1 = g30["atom_off"][m], g30["atom_off"][m + 1]
        ty, xy = g30["ref_types"][a0:a1], g30["ref_atoms"][a0:a1]
        keep = ty != adl.ATOMS_LIST[ds].index("H")
        cands.append((ds, [adl.ATOMS_LIST[ds][t] for t in ty[keep]], place(xy[keep]), False, -1))
    g30_of = [m for m in range(len(g30["n"])) if not g30["threw"][m]]
    n_g30 = len(cands)
    OK, NO_RINGS, BAD_TYPE, NOT_A_BASIS, OVERFLOW = range(5)
    d = 1.40 * np.sqrt(3.0)
    ring = lambda n, r, ph=0.0: np.array([[r * np.cos(ph + 2 * np.pi * k / n), r * np.sin(ph + 2 * np.pi * k / n)] for k in range(n)])
    hexa = ring(6, 1.40)
    cata_sp = lambda pts, expect, sym=None: cands.append(("cata", sym or ["C"] * len(pts), place(pts), False, expect))
    cata_sp(hexa, OK)                                                                       # benzene
    cata_sp(np.concatenate([hexa, ring(6, 2.49)]), OK, ["C"] * 6 + ["H"] * 6)               # benzene with its hydrogens
    cands.append(("hetro", ["C"] * 4, place(ring(4, 1.03)), False, OK))                     # a single Cbd ring
    db = ["C", "C", "B", "C", "C", "B"]
    hc = ring(6, 2.49)[[0, 1, 3, 4]]
    cands.append(("hetro", db + ["H"] * 4, place(np.concatenate([hexa, hc])), True, OK))    # Db: H on the carbons only
    cands.append(("hetro", db + ["H"] * 6, place(np.concatenate([hexa, hc, ring(6, 2.59)[[2, 5]]])), True, OK))  # DhDb: H on both B
    cata_sp(_g31_hexes([(0, 0), (d, 0), (d / 2, 1.5 * 1.40), (d / 2, -1.5 * 1.40)]), OK)    # pyrene: three rings meet at an atom
    cata_sp(np.concatenate([hexa, _g31_hexes([(10, 0), (10 + d, 0)])]), OK)                 # two molecules in one record
    cata_sp([[1.21 * k, 0.7 * (k % 2)] for k in range(5)], NO_RINGS)                        # a chain
    cands.append(("hetro", ["C"] * 5, place(ring(5, 1.2)), False, BAD_TYPE))                # an all-carbon five-ring
    cata_sp(ring(7, 1.613), NOT_A_BASIS)                                                    # a 7-ring
    cata_sp(_g31_hexes([(d * k, 0) for k in range(32)]), OK)                                # the capacity edge
    cata_sp(_g31_hexes([(d * k, 0) for k in range(33)]), OVERFLOW)                          # one ring beyond it

    def reference(ds, sym, xyz, use_h, tmp, name):
        path = os.path.join(tmp, name + ".xyz")
        with open(path, "w") as f:
            f.write(f"{len(sym)}\n\n")
            for s_, p in zip(sym, xyz.tolist()):
                f.write(f"{s_} {p[0]!r} {p[1]!r} {p[2]!r}\n")
        mol = load_xyz(path)
        assert all(a.x == p[0] and a.y == p[1] and a.z == p[2] for a, p in zip(mol.atoms, xyz.tolist()))
        con = get_connectivity_matrix(mol.atoms, skip_hydrogen=not use_h)
        g = nx.Graph(get_edges(con))
        heavy = [i for i, s_ in enumerate(sym) if s_ != "H"]
        gh = nx.Graph()
        gh.add_nodes_from(heavy)
        gh.add_edges_from((i, j) for i, j in get_edges(con) if sym[i] != "H" and sym[j] != "H")
        basis = {frozenset(c) for c in nx.minimum_cycle_basis(gh)}
        short = {frozenset(c) for c in nx.chordless_cycles(gh, length_bound=6) if len(c) >= 4}
        cyclo = gh.number_of_edges() - gh.number_of_nodes() + nx.number_connected_components(gh)
        basis_ok = basis == short and len(short) == cyclo
        margin = np.inf
        for a in range(len(heavy)):
            for b_ in range(a + 1, len(heavy)):
                i, j = heavy[a], heavy[b_]
                cut = (__COV_RADII__[sym[i]] + __COV_RADII__[sym[j]]) * 1.3
                margin = min(margin, abs(float(np.sqrt(((xyz[i] - xyz[j]) ** 2).sum())) - cut))
        rec = dict(basis_ok=basis_ok, margin=margin, threw=False, rings=[])
        try:
            knots = get_rings(mol.atoms, g)
            adj = get_rings_adj(knots).numpy()
            x32 = torch.tensor([k.get_coord() for k in knots], dtype=adl.DTYPE).numpy().reshape(-1, 3)
            types = [adl.RINGS_LIST[ds].index(k.cycle_type) for k in knots]
        except Exception:
            rec["threw"] = True
            return rec
        order = sorted(range(len(knots)), key=lambda r: tuple(sorted(a.index for a in knots[r].atoms)))
        for r in order:
            k = knots[r]
            idx = sorted(a.index for a in k.atoms)
            oi = []
            for o in k.orientation:
                hit = [i for i in idx if [xyz[i][0], xyz[i][1], xyz[i][2]] == list(o)]
                if hit:
                    assert len(hit) == 1 and sym[hit[0]] != "C"
                    oi.append(hit[0])
                else:
                    assert list(o) == k.get_coord()
                    oi.append(-1)
            rec["rings"].append(dict(atoms=idx, type=types[r], centre=k.get_coord(), x32=x32[r], orient=oi))
        rec["adj"] = adj[np.ix_(order, order)].astype(np.uint8)
        return rec

    kept, n_drop = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        t_ref, n_ref = 0.0, 0
        for m, (ds, sym, xyz, use_h, expect) in enumerate(cands):
            rec = reference(ds, sym, xyz, use_h, tmp, f"m{m}")
            if rec["margin"] < 1e-9:
                if expect >= 0:
                    raise RuntimeError("a special molecule of g31 sits on a tie: move it")
                n_drop += 1
                continue
            if m < n_g30:  # the rate of the reference's path (get_mol + get_rings + get_rings_adj), file already written
                t0 = time.perf_counter()
                try:
                    mol = load_xyz(os.path.join(tmp, f"m{m}.xyz"))
                    kn = get_rings(mol.atoms, nx.Graph(get_edges(get_connectivity_matrix(mol.atoms, skip_hydrogen=True))))
                    get_rings_adj(kn)
                except Exception:
                    pass
                t_ref += time.perf_counter() - t0
                n_ref += 1
            rec.update(ds=ds, sym=sym, xyz=xyz, use_h=use_h, expect=expect, name=f"m{m}", g30=g30_of[m] if m < n_g30 else -1)
            kept.append(rec)
        print(f"g31: dropped {n_drop} of {len(cands)} candidates on ties; cap {len(cands) // 10}")
        assert n_drop * 10 <= len(cands), "tie filter dropped more than 10 %"
        print(f"g31: reference get_rings path on this CPU: {n_ref / t_ref:.1f} molecules/s over {n_ref} molecules")
        good = [r for r in kept if r["basis_ok"] and not r["threw"] and r["expect"] <= 0 and r["rings"]]
        n_ok = sum(r["basis_ok"] and not r["threw"] for r in kept)
        n_ok_h = sum(r["basis_ok"] and not r["threw"] and r["ds"] == "hetro" for r in kept)
        n_nb = sum(not r["basis_ok"] for r in kept)
        print(f"g31: {len(kept)} molecules kept, {n_ok} with basis_ok ({n_ok_h} hetero), {n_nb} without, "
              f"{sum(r['threw'] for r in kept)} raise, smallest margin {min(r['margin'] for r in kept):.2e}")
        assert n_ok >= 100 and n_ok_h >= 40 and n_nb >= 5

        # AromaticDataset.get_all on a subset, normalize=True, two targets
        out = {}
        for ds, want, MN in (("hetro", 8, 10), ("cata", 4, 11)):
            sub = [r for r in good if r["ds"] == ds and not r["use_h"] and 2 <= len(r["rings"]) <= MN]
            sub = sub[:: max(1, len(sub) // want)][:want]
            assert len(sub) == want
            tg = np.random.default_rng(3101).normal(2.0, 1.5, (want, 2)).astype(np.float32)
            df = pd.DataFrame(dict(molecule=[r["name"] for r in sub], n_rings=[len(r["rings"]) for r in sub], gap=tg[:, 0], ip=tg[:, 1]))

            class A:
                pass
            args = A()
            args.rings_graph, args.normalize, args.max_nodes, args.dataset, args.target_features = True, True, MN, ds, "gap,ip"
            args.sample_rate, args.df_train, args.df_val = 1, df, df
            old = adl.get_paths
            adl.get_paths = lambda a: (None, tmp)
            try:
                dset = adl.AromaticDataset(args, "train")
                random.seed(31)
                rows = [dset[i] for i in range(want)]
            finally:
                adl.get_paths = old
            out[ds] = dict(idx=np.array([kept.index(r) for r in sub], np.int32), max_nodes=MN, targets=tg,
                           mean=dset.mean.numpy(), std=dset.std.numpy(),
                           x=np.stack([r[0].numpy() for r in rows]).astype(np.float32), node_mask=np.stack([r[1].numpy() for r in rows]).astype(np.float32),
                           edge_mask=np.stack([r[2].numpy() for r in rows]).astype(np.float32),
                           node_features=np.stack([r[3].numpy() for r in rows]).astype(np.float32), y=np.stack([r[4].numpy() for r in rows]).astype(np.float32))

    aoff = np.concatenate([[0], np.cumsum([len(r["sym"]) for r in kept])]).astype(np.int32)
    roff = np.concatenate([[0], np.cumsum([len(r["rings"]) for r in kept])]).astype(np.int32)
    joff = np.concatenate([[0], np.cumsum([len(r["rings"]) ** 2 for r in kept])]).astype(np.int32)
    rings = [q for r in kept for q in r["rings"]]
    ra = np.full((len(rings), 6), -1, np.int16)
    ro = np.full((len(rings), 2), -2, np.int16)  # -2: no such candidate, -1: the centre
    for i, q in enumerate(rings):
        ra[i, :len(q["atoms"])] = q["atoms"]
        assert 1 <= len(q["orient"]) <= 2
        ro[i, :len(q["orient"])] = q["orient"]
    arrs = dict(
        hetro=np.array([r["ds"] == "hetro" for r in kept]), use_h=np.array([r["use_h"] for r in kept]),
        expect=np.array([r["expect"] for r in kept], np.int8), g30_index=np.array([r["g30"] for r in kept], np.int16), threw=np.array([r["threw"] for r in kept]),
        basis_ok=np.array([r["basis_ok"] for r in kept]), margin=np.array([r["margin"] for r in kept], np.float32),
        atom_off=aoff, xyz=np.concatenate([r["xyz"] for r in kept]).astype(np.float32),
        elem=np.concatenate([[adl.ATOMS_LIST[r["ds"]].index(s_) for s_ in r["sym"]] for r in kept]).astype(np.int8),
        ring_off=roff, ring_atoms=ra, ring_type=np.array([q["type"] for q in rings], np.int8),
        centre=np.array([q["centre"] for q in rings], np.float64), x32=np.array([q["x32"] for q in rings], np.float32),
        orient=ro, adj_off=joff, adj=np.concatenate([r["adj"].reshape(-1) for r in kept if r["rings"]]).astype(np.uint8),
        ref_rate=np.array(n_ref / t_ref))
    for ds, o in out.items():
        for k, v in o.items():
            arrs[f"ga_{ds}_{k}"] = np.asarray(v)
    save("g31_goa2gor", **arrs)
    size, cap = os.path.getsize(os.path.join(OUT, "g31_goa2gor.npz")), os.path.getsize(os.path.join(OUT, "g30_gor2goa.npz"))
    assert size <= cap, f"g31 is {size} bytes, g30 {cap}"


def _g32_h_rule(types, bonds, C, H):
    """build_molecule_aromatic's hydrogens (data/gor2goa.py:288-293): one H on every carbon with exactly two bonds, appended."""
    types = [int(t) for t in types]
    bonds = [(int(a), int(b)) for a, b in bonds]
    deg = np.zeros(len(types), int)
    for a, b in bonds:
        deg[a] += 1
        deg[b] += 1
    for a in range(len(deg)):
        if types[a] == C and deg[a] == 2:
            bonds.append((a, len(types)))
            types.append(H)
    return np.array(types, np.int64), np.array(bonds, np.int64).reshape(-1, 2)


def _g32_acene(k, C):
    """Carbon skeleton of a linear acene of k rings: 4 k + 2 atoms, 5 k + 1 bonds."""
    top = list(range(0, 2 * k + 1))
    bot = list(range(2 * k + 1, 4 * k + 2))
    bonds = [(top[i], top[i + 1]) for i in range(2 * k)] + [(bot[i], bot[i + 1]) for i in range(2 * k)]
    bonds += [(top[2 * i], bot[2 * i]) for i in range(k + 1)]
    return [C] * (4 * k + 2), bonds


def g32_bond_orders():
    """Bond orders and formal charges from connectivity (data/xyz2mol.py:538-634, AC2BO, as rdkit_valid calls it: charge 0).
    Candidates: every built molecule of g30 with build_molecule_aromatic's H rule applied; for each hetero one of at most 40 atoms
    six mutants with 1-3 heavy atoms re-elemented among C, B, N, O, S; specials built at the atom level.  Elements are indices
    into ATOMS_LIST["hetro"] for every molecule (ATOMS_LIST["cata"] is its prefix).  Stored per molecule: elements, bonds,
    ref_ran (the reference can take the input at all), ref_valid (AC2BO under the identity: every atom's bond-order sum is one of
    its allowed valences and the formal charges sum to zero, sys.exit = invalid; and the bond graph is connected, rdkit_valid's
    fragment condition), ref_stable (the identity and two seeded relabellings agree), ref_cumulated (some labelling's VALID
    structure gives an atom two or more added bonds), min_charged (exhaustive search over the options table below with networkx
    maximum-cardinality matching, up to 6 charged atoms, -1: none), odd_cycle (the selected subgraph of the first minimum
    solution is not bipartite), special (the status a special is there for, -1 otherwise), g30 (index into g30, -1 otherwise).
    The options table: per (element, sigma degree 0..4) the (added bonds, charge) pairs of every allowed valence v >= degree
    with v - degree <= 1, from the reference's valence lists and charge function, the neutral one first."""
    import itertools
    import time
    import networkx as nx
    from data import xyz2mol as X
    from data.aromatic_dataloader import ATOMS_LIST
    names = list(ATOMS_LIST["hetro"])
    assert list(ATOMS_LIST["cata"]) == names[:2]
    H, C = names.index("H"), names.index("C")
    Z = [X.int_atom(e) for e in names]
    table = [[sorted(([v - d, int(X.get_atomic_charge(z, X.atomic_valence_electrons[z], v))] for v in X.atomic_valence[z] if 0 <= v - d <= 1),
                     key=lambda o: (abs(o[1]), o[0])) for d in range(5)] for z in Z]
    g30 = np.load(os.path.join(OUT, "g30_gor2goa.npz"))
    rng = np.random.default_rng(3200)

    def ref_choices(types, bonds):
        deg = np.bincount(bonds.reshape(-1), minlength=len(types))
        return sum(len([v for v in X.atomic_valence[Z[t]] if v >= d]) >= 2 for t, d in zip(types, deg))

    def ref_verdict(types, bonds, perm):
        n = len(types)
        AC = np.zeros((n, n), int)
        for a, b in bonds:
            AC[perm[a], perm[b]] = AC[perm[b], perm[a]] = 1
        atoms = [0] * n
        for a in range(n):
            atoms[perm[a]] = Z[types[a]]
        try:
            BO, _ = X.AC2BO(AC, atoms, 0)
        except SystemExit:
            return False, False
        val = BO.sum(1)
        ok = all(int(v) in X.atomic_valence[z] for v, z in zip(val, atoms))
        q = sum(X.get_atomic_charge(z, X.atomic_valence_electrons[z], int(v)) for v, z in zip(val, atoms))
        valid = bool(ok and q == 0)
        return valid, valid and bool((BO - AC).sum(1).max() >= 2)

    def own_search(types, bonds):
        n = len(types)
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from((int(a), int(b)) for a, b in bonds)
        if n == 0 or not nx.is_connected(g):
            return -1, False
        deg = np.bincount(bonds.reshape(-1), minlength=n) if len(bonds) else np.zeros(n, int)
        opts = [table[t][d] if d < 5 else [] for t, d in zip(types, deg)]
        if any(not o for o in opts):
            return -1, False
        flex = [a for a in range(n) if len(opts[a]) == 2]
        base_q = sum(o[0][1] for o in opts)
        forced = sum(o[0][1] != 0 for o in opts)
        for t in range(0, 7 - forced):
            for sub in itertools.combinations(flex, t):
                if base_q + sum(opts[a][1][1] for a in sub) != 0:
                    continue
                S = [a for a in range(n) if opts[a][1 if a in sub else 0][0] == 1]
                if len(S) % 2:
                    continue
                h = g.subgraph(S)
                if 2 * len(nx.max_weight_matching(h, maxcardinality=True)) == len(S):
                    return forced + t, not nx.is_bipartite(h)
        return -1, False

    cands = []  # (types, bonds, kind, special status, g30 index)
    built = [m for m in range(len(g30["n"])) if not g30["threw"][m]]
    n_skipped = n_mut = 0
    for m in built:
        ty = g30["ref_types"][g30["atom_off"][m]:g30["atom_off"][m + 1]].astype(np.int64)
        bo = g30["ref_bonds"][g30["bond_off"][m]:g30["bond_off"][m + 1]].astype(np.int64)
        cands.append((*_g32_h_rule(ty, bo, C, H), 0, -1, m))
        if not g30["hetro"][m] or len(cands[-1][0]) > 40:
            continue
        heavy = np.flatnonzero(ty != H)
        for _ in range(6):  # (three leave no molecule that needs two charge pairs)
            n_mut += 1
            t2 = ty.copy()
            for a in rng.choice(heavy, size=int(rng.integers(1, 4)), replace=False):
                t2[a] = names.index("CBNOS"[int(rng.integers(5))])
            t2, b2 = _g32_h_rule(t2, bo, C, H)
            if ref_choices(t2, b2) > 9:
                n_skipped += 1
                continue
            cands.append((t2, b2, 1, -1, -1))
    print(f"g32: {n_skipped} of {n_mut} mutants skipped (more than 9 atoms with a choice of valence); cap 12 %")
    assert n_skipped * 100 <= 12 * n_mut
    ring6 = [(i, (i + 1) % 6) for i in range(6)]
    sp = lambda t, b, st=-1, h=True: cands.append((*(_g32_h_rule(t, b, C, H) if h else (np.array(t, np.int64), np.array(b, np.int64).reshape(-1, 2))), 2, st, -1))
    sp([C] * 6, ring6, 0)                                                   # benzene
    sp(*_g32_acene(16, C), 0)                                               # 66 carbons: more heavy atoms than lanes
    sp(*_g32_acene(47, C), 0)                                               # 190 carbons: the capacity edge
    sp(*_g32_acene(48, C), 6)                                               # 194: OVERFLOW
    t47, b47 = _g32_acene(47, C)
    t47[1] = names.index("O")                                               # a CH carbon -> O: an odd remainder
    sp(t47, b47, 1)
    sp([C] * 12, ring6 + [(6 + i, 6 + j) for i, j in ring6], 3)             # two benzenes, not connected
    sp([C] + [H] * 5, [(0, k) for k in range(1, 6)], 4, h=False)            # a carbon with five bonds
    sp([C] * 6 + [H] * 6, ring6[:5] + [(5, 12)] + [(k, 6 + k) for k in range(6)], 5, h=False)  # a bond index equal to n_atoms
    sp([], [], 7, h=False)                                                  # an empty molecule

    recs = []
    t0 = time.time()
    for types, bonds, kind, special, gi in cands:
        n = len(types)
        ran = special not in (5, 6, 7)
        rec = dict(types=types, bonds=bonds, kind=kind, special=special, g30=gi, ran=ran, valid=False, stable=True, cumulated=False,
                   minq=-1, odd=False)
        if ran:
            g = nx.Graph()
            g.add_nodes_from(range(n))
            g.add_edges_from((int(a), int(b)) for a, b in bonds)
            verdicts = [ref_verdict(types, bonds, p) for p in [np.arange(n), rng.permutation(n), rng.permutation(n)]]
            rec["valid"] = verdicts[0][0] and nx.is_connected(g)
            rec["stable"] = len({v for v, _ in verdicts}) == 1
            rec["cumulated"] = any(c for _, c in verdicts)
            rec["minq"], rec["odd"] = own_search(types, bonds)
        recs.append(rec)
    print(f"g32: reference and search over {len(recs)} molecules in {time.time() - t0:.0f} s")
    for kind, label in ((0, "g30"), (1, "mutants")):
        sel = [r for r in recs if r["kind"] == kind]
        exc = sum((not r["stable"]) or r["cumulated"] for r in sel)
        print(f"g32: {label}: {len(sel)} kept, {exc} outside the verdict comparison (unstable or cumulated)")
    exc = sum((not r["stable"]) or r["cumulated"] or not r["ran"] for r in recs)
    print(f"g32: {exc} of {len(recs)} molecules outside the verdict comparison; cap 5 %")
    assert exc * 100 <= 5 * len(recs)
    counts = {k: sum(r["minq"] == k for r in recs) for k in range(-1, 7)}
    n_odd = sum(r["odd"] for r in recs)
    print(f"g32: min_charged counts {counts} (-1 includes the specials without a structure), odd_cycle {n_odd}")
    agree = sum((0 <= r["minq"] <= 4) == r["valid"] for r in recs if r["stable"] and not r["cumulated"] and r["ran"])
    print(f"g32: the rule agrees with the reference's verdict on {agree} of {len(recs) - exc} compared molecules")
    assert counts[0] >= 100 and counts[2] >= 10 and counts[4] >= 1 and counts[-1] >= 50 and n_odd >= 10
    aoff = np.concatenate([[0], np.cumsum([len(r["types"]) for r in recs])]).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum([len(r["bonds"]) for r in recs])]).astype(np.int64)
    tn = np.array([[len(table[e][d]) for d in range(5)] for e in range(len(names))], np.int8)
    to = np.zeros((len(names), 5, 2, 2), np.int8)
    for e in range(len(names)):
        for d in range(5):
            for k, o in enumerate(table[e][d]):
                to[e, d, k] = o
    col = lambda key, dt: np.array([r[key] for r in recs], dt)
    save("g32_bond_orders", elem=np.concatenate([r["types"] for r in recs]).astype(np.int8),
         bonds=np.concatenate([r["bonds"] for r in recs]).astype(np.int16), atom_off=aoff, bond_off=boff,
         kind=col("kind", np.int8), special=col("special", np.int8), g30=col("g30", np.int32), ref_ran=col("ran", bool),
         ref_valid=col("valid", bool), ref_stable=col("stable", bool), ref_cumulated=col("cumulated", bool),
         min_charged=col("minq", np.int8), odd_cycle=col("odd", bool), table_n=tn, table_opt=to,
         elements=np.array(json.dumps(names)))
    size, cap = os.path.getsize(os.path.join(OUT, "g32_bond_orders.npz")), os.path.getsize(os.path.join(OUT, "g30_gor2goa.npz"))
    assert size <= cap, f"g32 is {size} bytes, g30 {cap}"


def g8_checkpoint_roundtrip():
    """The reference's own loader must accept checkpoints written by gaudi_amd.synth.write_checkpoint
    (args.txt + model.pt, with and without the ``module.`` prefix).  Stores nothing but a marker."""
    import tempfile
    from utils.helpers import get_edm_args

    for dp in (True, False):
        with tempfile.TemporaryDirectory() as d:
            args = synth.edm_args(dp=dp, **TINY)
            sd = synth.synth_edm_state_dict(args, 1, seed=5)
            a0, m0 = build_ref_edm("cata", sd, **TINY)
            sd["gamma.gamma"] = m0.gamma.gamma.numpy().copy()
            synth.write_checkpoint(d, args, sd)
            a = get_edm_args(d)
            a.device = torch.device("cpu")
            model, _, _ = models_edm.get_model(a, FakeLoader(1, 5), only_norm=True)
            got = model.state_dict()
            pre = "module." if dp else ""
            for k, v in sd.items():
                assert np.array_equal(got[pre + k].numpy(), v), k
    print("g8: reference loader accepts synth checkpoints (dp=True/False)")


if __name__ == "__main__":
    fns = dict(g1=g1_schedule, g2=g2_masks, g3=g3_phi, g4=g4_predictor, g5=g5_steps, g6=g6_decode,
               g7=g7_end_to_end, g8=g8_checkpoint_roundtrip, g9=g9_sample_chain, g10=g10_nonlinear_target, g11=g11_stability, g12=g12_ring_count_sampler, g13=g13_noised_predictor, g14=g14_long_chains, g15=g15_nan_scrub, g16=g16_fix_noise, g17=g17_nan_in_edge_gemm_matrix, g18=g18_large_molecules, g19=g19_amplified_default_steps, g20=g20_cosine_and_mean, g21=g21_direct_z_target, g22=g22_sin_embedding, g23=g23_attention_tanh_flags, g24=g24_scalar_hyperparameters, g25=g25_nll, g26=g26_pred_grad, g27=g27_edm_grad, g27t=g27_edm_train, g28=g28_grid, g29=g29_value_target, g30=g30_gor2goa, g31=g31_goa2gor)
    fns["g30_gor2goa"] = g30_gor2goa  # (also under its full name)
    fns["g31_goa2gor"] = g31_goa2gor
    fns["g32"] = fns["g32_bond_orders"] = g32_bond_orders
    which = sys.argv[1:] or [k for k in fns if k not in ("g30_gor2goa", "g31_goa2gor", "g32_bond_orders")]
    for w in which:
        fns[w]()
