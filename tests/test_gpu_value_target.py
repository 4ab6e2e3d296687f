"""GPU tests of the fused value-target family (gaudi_sample_target / gaudi_step_target): per-molecule value-seeking and
one-sided targets, a guidance window and a guidance trace in one launch sequence, against the split-step callback path
(bit for bit), the reference (g29), the affine path, and across kernel families and launch shapes."""
import json
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest

from gaudi_amd import synth
from tests.helpers import TINY, TINY_P, cfg_of, edm_from_cfg, pred_from_cfg, rel_err
from tests.value_target_helpers import numpy_seed

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(eargs, esd, pargs, psd, **env):
    from gaudi_amd.engine import Engine
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        eng = Engine(0)  # the knobs are read once, by gaudi_create
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    eng.load_edm(eargs, esd)
    eng.load_predictor(pargs, psd)
    return eng


def _tiny(golden, name, **env):
    """The T = 50 tiny-width case of g7 -> (engine, node_mask, edge_mask, noise, T)."""
    g = golden("g7_end_to_end")
    cfg = cfg_of(g, name)
    base = dict(dataset=cfg["dataset"], amp=cfg["amp"])
    eargs, esd = edm_from_cfg(dict(base, over=TINY, wseed=cfg["eseed"]), diffusion_steps=cfg["T"])
    pargs, psd = pred_from_cfg(dict(base, over=TINY_P, wseed=cfg["pseed"]))
    return _engine(eargs, esd, pargs, psd, **env), g[name + "_node_mask"], g[name + "_edge_mask"], g[name + "_noise"], cfg["T"]


def _params(seed, B, scale=(0.2, 2.0)):
    """Per-molecule random parameters; every side occurs in every molecule."""
    rng = np.random.default_rng(seed)
    side = rng.integers(-1, 2, (B, K)).astype(np.int32)
    side[:, :3] = np.array([0, 1, -1], np.int32)
    return dict(w=(0.5 * rng.standard_normal((B, K))).astype(np.float32), q=rng.uniform(0.2, 1.5, (B, K)).astype(np.float32),
                c=(0.5 * rng.standard_normal((B, K))).astype(np.float32), side=side,
                scale=np.exp(rng.uniform(np.log(scale[0]), np.log(scale[1]), B)).astype(np.float32))


def _grad(spec, window=None, T=None, seen=None):
    """The callback twin of a spec: the numpy float32 seed (scale inside, so the callback path runs with scale = 1.0); zeros
    outside a window (t = time index / T of the step)."""
    def grad(pred, t):
        if seen is not None:
            seen.append(pred.copy())
        if window is not None:
            ti = int(round(float(t) * T))
            if not window[0] <= ti <= window[1]:
                return np.zeros_like(pred)
        zero = np.zeros(K, np.float32)  # an absent array: w = q = c = side = 0, scale = 1, as the library reads the spec
        return numpy_seed(spec.get("w", zero), spec.get("q", zero), spec.get("c", zero), spec.get("side", zero.astype(np.int32)),
                          spec.get("scale", np.float32(1.0)), pred)
    return grad


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. the callback path
@pytest.mark.parametrize("name", ["cata_tiny", "hetro_tiny"])
def test_fused_value_target_equals_callback_path_bit_for_bit(golden, name):
    eng, nm, em, noise, T = _tiny(golden, name)
    B = nm.shape[0]
    spec = _params(11, B)
    xa, ha, _, za = eng.sample_target(nm, em, spec, noise=noise, return_z0=True)
    assert eng.last_launch_shape() == (B, nm.shape[1])  # one molecule per workgroup (the callback path is unpacked too)
    xb, hb, _, zb = eng.sample_callback(nm, em, _grad(spec), noise=noise, scale=1.0, return_z0=True)
    assert np.array_equal(xa, xb) and np.array_equal(ha, hb) and np.array_equal(za, zb)
    assert np.isfinite(xa).all()
    xu, _, _ = eng.sample(nm, em, noise=noise, target_w=np.zeros(K, np.float32), scale=1.0)
    assert not np.array_equal(xa, xu), "the target must have moved the chain"
    # Philox noise + sample_offset go through the same plumbing
    xa, ha, _, za = eng.sample_target(nm, em, spec, seed=5, sample_offset=3, return_z0=True)
    xb, hb, _, zb = eng.sample_callback(nm, em, _grad(spec), seed=5, sample_offset=3, scale=1.0, return_z0=True)
    assert np.array_equal(xa, xb) and np.array_equal(ha, hb) and np.array_equal(za, zb)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. the reference (g29)
def _spec_of(g, prefix):
    return {k: g[f"{prefix}_{k}"] for k in ("w", "q", "c", "side", "scale")}


@pytest.mark.parametrize("tag", ["tiny", "default"])
def test_g29_steps_vs_reference(golden, tag):
    g = golden("g29_value_target")
    cfg = json.loads(str(g[tag + "_cfg"]))
    over, over_p = (TINY, TINY_P) if tag == "tiny" else ({}, {})
    eargs, esd = edm_from_cfg(dict(dataset=cfg["dataset"], over=over, wseed=cfg["eseed"], amp=True), diffusion_steps=cfg["T"])
    pargs, psd = pred_from_cfg(dict(dataset=cfg["dataset"], over=over_p, wseed=cfg["pseed"], amp=True))
    eng = _engine(eargs, esd, pargs, psd)
    z, nm, em = g[tag + "_z"], g[tag + "_node_mask"], g[tag + "_edge_mask"]
    clip = []
    for strength in ("weak", "strong"):
        spec = _spec_of(g, f"{tag}_{strength}")
        for s in cfg["steps"]:
            zs, tr = eng.step_target(s, z, nm, em, g[f"{tag}_s{s}_eps"], spec, trace=True)
            err = rel_err(zs, g[f"{tag}_{strength}_s{s}_zs"])
            print(f"g29 {tag} {strength} s={s}: rel_err {err:.3e}")
            assert err < TOL, (strength, s, err)
            clip.append(tr[:, K + 1])
    clip = np.concatenate(clip)
    assert (clip < 1).any() and (clip == 1).any(), "the fixture must exercise both branches of the clip"
    eng.close()


@pytest.mark.parametrize("name", ["cata_chain", "hetro_chain"])
def test_g29_chains_vs_reference(golden, name):
    from gaudi_amd import sampling_edm
    from gaudi_amd.models_edm import ValueTarget, get_cond_predictor_model, get_model
    g = golden("g29_value_target")
    cfg = cfg_of(g, name)
    base = dict(dataset=cfg["dataset"], amp=cfg["amp"])
    eargs, esd = edm_from_cfg(dict(base, over=TINY, wseed=cfg["eseed"]), diffusion_steps=cfg["T"])
    pargs, psd = pred_from_cfg(dict(base, over=TINY_P, wseed=cfg["pseed"]))
    spec = _spec_of(g, name)
    eng = _engine(eargs, esd, pargs, psd)
    x, h, _ = eng.sample_target(g[name + "_node_mask"], g[name + "_edge_mask"], spec, noise=g[name + "_noise"])
    err = rel_err(x, g[name + "_x"])
    print(f"g29 {name}: rel_err {err:.3e}")
    assert err < TOL
    assert np.array_equal(h, g[name + "_h"])
    eng.close()
    # ... and through the reference-shaped entry point with a ValueTarget (the call's scale multiplies the target's own)
    model, _, _ = get_model(eargs, state_dict=esd)
    pred = get_cond_predictor_model(pargs, model=model, state_dict=psd)
    model.injected_noise = g[name + "_noise"]
    model.trace_guidance = True
    target = ValueTarget(pred, spec["w"], spec["q"], spec["c"], spec["side"], spec["scale"] * np.float32(2.0))
    args = types.SimpleNamespace(device="cuda", dataset=cfg["dataset"], max_nodes=max(cfg["nodes"]))
    x2, h2, nm2, em2 = sampling_edm.sample_guidance(args, model, target, cfg["nodes"], scale=0.5)
    assert np.array_equal(x2.numpy(), x) and np.array_equal(h2.numpy(), h)
    assert model.last_trace.shape == (cfg["T"], len(cfg["nodes"]), K + 2) and np.isfinite(model.last_trace).all()
    # the target object is callable with the reference's closure signature (get_target_function_values / design)
    zt = np.concatenate([x2.numpy(), h2.numpy()], axis=2).astype(np.float32)
    val = target(zt, nm2, em2, np.zeros((len(cfg["nodes"]), 1), np.float32))
    B, N = zt.shape[0], zt.shape[1]
    p = model.engine.predictor_fwd(zt, 0.0, nm2.numpy().reshape(B, N), em2.numpy().reshape(B, N, N))
    assert rel_err(np.asarray(val), target.value(p)) < TOL
    model.engine.close()


# ------------------------------------------------------------------------------------------------ 3. the affine path
def test_zero_curvature_shared_arrays_equal_the_affine_path(golden):
    eng, nm, em, noise, T = _tiny(golden, "hetro_tiny")
    w = np.array([3, 0, 1, 1, 0], np.float32)
    x0, h0, _, z0 = eng.sample(nm, em, noise=noise, target_w=w, scale=0.6, return_z0=True)
    for spec in (dict(w=w, scale=0.6), dict(w=w, q=np.zeros(K, np.float32), c=np.ones(K, np.float32), side=np.ones(K, np.int32), scale=0.6)):
        x1, h1, _, z1 = eng.sample_target(nm, em, spec, noise=noise, return_z0=True)
        assert np.array_equal(x0, x1) and np.array_equal(h0, h1) and np.array_equal(z0, z1)
    x0, h0, _ = eng.sample(nm, em, seed=9, sample_offset=2, target_w=w, scale=0.6, grid=[T, 30, 11, 4, 0])
    x1, h1, _ = eng.sample_target(nm, em, dict(w=w, scale=0.6), seed=9, sample_offset=2, grid=[T, 30, 11, 4, 0])
    assert np.array_equal(x0, x1) and np.array_equal(h0, h1)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. sweep invariance
def test_molecule_of_a_mixed_call_equals_the_uniform_call_with_its_parameters(golden):
    eng, nm, em, noise, T = _tiny(golden, "cata_tiny")
    B = nm.shape[0]
    spec = _params(12, B)
    xm, hm, _, zm = eng.sample_target(nm, em, spec, seed=7, sample_offset=40, return_z0=True)
    for i in range(B):
        uni = {k: v[i] for k, v in spec.items()}  # [K] arrays and one scale: everyone gets molecule i's parameters
        xu, hu, _, zu = eng.sample_target(nm, em, uni, seed=7, sample_offset=40, return_z0=True)
        assert np.array_equal(xm[i], xu[i]) and np.array_equal(hm[i], hu[i]) and np.array_equal(zm[i], zu[i]), i
    assert not np.array_equal(zm[0], eng.sample_target(nm, em, {k: v[1] for k, v in spec.items()}, seed=7, sample_offset=40,
                                                       return_z0=True)[3][0]), "the parameters must matter"
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. launch shapes and kernel families
@pytest.mark.parametrize("dataset,rings", [("hetro", [3, 10, 4, 3, 5, 7, 3, 6, 4, 9, 3, 4, 8, 5, 3, 3]),
                                           ("cata", [4, 11, 3, 5, 2, 6, 3, 4, 1, 7, 5, 2])])
def test_value_targets_keep_one_molecule_per_workgroup_where_affine_calls_pack(dataset, rings):
    """A shared workgroup has ONE readout and ONE seed; the per-component forms are not built for this family, so the call
    falls back to one molecule per workgroup -- asserted by the launch shape -- and GAUDI_PACK changes nothing, bit for bit."""
    from gaudi_amd.sampling_edm import build_masks
    hetero = dataset == "hetro"
    F = synth.num_node_features(dataset)
    nm3, em_flat, N = build_masks(np.asarray(rings), max(rings), hetero)
    B = len(rings)
    nm, em = nm3.reshape(B, N), em_flat.reshape(B, N, N)
    T = 9
    eargs, pargs = synth.edm_args(diffusion_steps=T, dataset=dataset, **TINY), synth.pred_args(dataset=dataset, **TINY_P)
    esd = synth.synth_edm_state_dict(eargs, F, seed=51, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=52, amplify_coord=True)
    spec = _params(13, B)
    outs = []
    for pack in (1, 0):
        eng = _engine(eargs, esd, pargs, psd, GAUDI_PACK=pack)
        eng.sample(nm, em, seed=3, sample_offset=5, target_w=spec["w"][0], scale=0.6)
        assert (eng.last_launch_shape()[0] < B) == bool(pack)  # the affine call of the same batch does share workgroups
        o = eng.sample_target(nm, em, spec, seed=3, sample_offset=5, return_z0=True)
        assert eng.last_launch_shape() == (B, N) and eng.kernel_variant()[1] == 8
        outs.append((o[0], o[1], o[3]))
        if not pack:
            ref = eng.sample_callback(nm, em, _grad(spec), seed=3, sample_offset=5, scale=1.0, return_z0=True)
            assert _same(outs[-1], (ref[0], ref[1], ref[3]))
        eng.close()
    assert _same(*outs)


def test_value_targets_do_not_form_wide_groups():
    from oracle import gaudi_oracle as O
    T = 6
    eargs, pargs = synth.edm_args(diffusion_steps=T), synth.pred_args()
    esd = synth.synth_edm_state_dict(eargs, 1, seed=51)
    psd = synth.synth_predictor_state_dict(pargs, 1, 5, seed=52)
    nm, em = O.build_masks([11, 11, 11, 9], 11, False)
    nm, em = nm.reshape(4, 11), em.reshape(4, 11, 11)
    spec = _params(14, 4)
    res = []
    for env in ({"GAUDI_PAIRS": 0}, {"GAUDI_PAIRS": 2, "GAUDI_WIDE_FULL": 0}, {"GAUDI_PAIRS": 2}):
        eng = _engine(eargs, esd, pargs, psd, **env)
        x, h, _, z0 = eng.sample_target(nm, em, spec, seed=4, return_z0=True)
        assert eng.last_launch_shape() == (4, 11) and eng.node_buffers_form() == 0, (env, eng.last_launch_shape())
        res.append((x, h, z0))
        if env["GAUDI_PAIRS"] == 0:
            ref = eng.sample_callback(nm, em, _grad(spec), seed=4, scale=1.0, return_z0=True)
            assert _same(res[0], (ref[0], ref[1], ref[3]))
        eng.close()
    assert _same(res[0], res[1]) and _same(res[0], res[2])


@pytest.mark.parametrize("env", [{"GAUDI_WAVES": 4}, {"GAUDI_FORCE_GN": 1}, {"GAUDI_FORCE_GN8": 1}, {"GAUDI_EDGE_MATH": "fp32"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_every_kernel_family_equals_its_own_callback_path(golden, env):
    eng, nm, em, noise, T = _tiny(golden, "cata_tiny", **env)
    B = nm.shape[0]
    spec = dict(_params(15, B), window=(5, 40))
    a = eng.sample_target(nm, em, spec, noise=noise, return_z0=True)
    fam = (eng.kernel_variant()[1], eng.edge_math()[1], eng.node_buffers_global())
    b = eng.sample_callback(nm, em, _grad(spec, (5, 40), T), noise=noise, scale=1.0, return_z0=True)
    assert fam == (eng.kernel_variant()[1], eng.edge_math()[1], eng.node_buffers_global())
    if "GAUDI_WAVES" in env or "GAUDI_FORCE_GN" in env:
        assert fam[0] == 4
    if "GAUDI_FORCE_GN" in env or "GAUDI_FORCE_GN8" in env:
        assert fam[2]
    if "GAUDI_EDGE_MATH" in env:
        assert fam[1] == 0
    assert _same((a[0], a[1], a[3]), (b[0], b[1], b[3]))
    eng.close()


@pytest.mark.parametrize("nf", [32, 64])
def test_sin_embedding_handle_equals_its_callback_path(nf):
    """nf = 32: the fused sin_embedding kernel; nf = 64: no fused instantiation, a guided step is two launches (and a step
    outside the window one: the denoiser-only kernel finishes it)."""
    from oracle import gaudi_oracle as O
    T, ds = 8, "hetro"
    F = synth.num_node_features(ds)
    eargs = synth.edm_args(dataset=ds, diffusion_steps=T, sin_embedding=True, nf=nf, n_layers=2)
    pargs = synth.pred_args(dataset=ds, **TINY_P)
    esd = synth.synth_edm_state_dict(eargs, F, seed=71)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=72)
    nm3, em_flat = O.build_masks([3, 5, 4], 5, True)
    B, N = nm3.shape[0], nm3.shape[1]
    nm, em = nm3.reshape(B, N), em_flat.reshape(B, N, N)
    eng = _engine(eargs, esd, pargs, psd)
    spec = dict(_params(16, B), window=(2, 6))
    a = eng.sample_target(nm, em, spec, seed=2, return_z0=True, trace=True)
    seen = []
    b = eng.sample_callback(nm, em, _grad(spec, (2, 6), T, seen), seed=2, scale=1.0, return_z0=True)
    assert eng.kernel_variant()[1] == 4
    assert _same((a[0], a[1], a[3]), (b[0], b[1], b[3]))
    tr = a[4]
    on = np.array([2 <= T - k <= 6 for k in range(T)])
    assert np.array_equal(tr[on][:, :, :K], np.stack(seen)[on]) and not tr[~on].any()
    eng.close()


def test_sub_batches_scatter_parameters_and_trace_by_request_index(golden, monkeypatch):
    """A request cut into sub-batches (here: a 1 MiB workspace, two molecules per cut) stages each cut's parameter rows and
    scatters its trace rows by the molecule's index in the request: same bits as the uncut call and as the callback path."""
    from gaudi_amd.sampling_edm import build_masks
    rings = [3, 10, 4, 3, 5, 7, 3, 6, 4, 9]
    F = synth.num_node_features("hetro")
    nm3, em_flat, N = build_masks(np.asarray(rings), max(rings), True)
    B = len(rings)
    nm, em = nm3.reshape(B, N), em_flat.reshape(B, N, N)
    T = 9
    eargs, pargs = synth.edm_args(diffusion_steps=T, dataset="hetro", **TINY), synth.pred_args(dataset="hetro", **TINY_P)
    esd = synth.synth_edm_state_dict(eargs, F, seed=51, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=52, amplify_coord=True)
    eng = _engine(eargs, esd, pargs, psd)
    spec = dict(_params(18, B), window=(2, 8))
    whole = eng.sample_target(nm, em, spec, seed=3, sample_offset=5, return_z0=True, trace=True)
    assert eng.last_launch_shape() == (B, N)
    monkeypatch.setenv("GAUDI_MAX_WORKSPACE_MB", "1")  # (read per call)
    cut = eng.sample_target(nm, em, spec, seed=3, sample_offset=5, return_z0=True, trace=True)
    assert eng.last_launch_shape()[0] < B, "the request must have been cut"
    monkeypatch.delenv("GAUDI_MAX_WORKSPACE_MB")
    assert _same((whole[0], whole[1], whole[3], whole[4]), (cut[0], cut[1], cut[3], cut[4]))
    seen = []
    ref = eng.sample_callback(nm, em, _grad(spec, (2, 8), T, seen), seed=3, sample_offset=5, scale=1.0, return_z0=True)
    assert _same((cut[0], cut[1], cut[3]), (ref[0], ref[1], ref[3]))
    on = np.array([2 <= T - k <= 8 for k in range(T)])
    assert np.array_equal(cut[4][on][:, :, :K], np.stack(seen)[on]) and not cut[4][~on].any()
    eng.close()


def test_beyond_the_resident_limit_every_molecule_runs_v8g():
    """A padded N beyond the resident kernels' LDS limit (hetero, 20 rings = 40 graph nodes, default widths): the affine call
    with GAUDI_FAMILY_SPLIT=1 sorts the small molecules into a packed resident bucket; a value target does not (that bucket
    is packed) -- every molecule runs alone on the V8G kernels, bit-equal to the callback path."""
    from gaudi_amd.sampling_edm import build_masks
    rings = [20, 3, 4]
    F = synth.num_node_features("hetro")
    nm3, em_flat, N = build_masks(np.asarray(rings), max(rings), True)
    B = len(rings)
    nm, em = nm3.reshape(B, N), em_flat.reshape(B, N, N)
    T = 3
    eargs, pargs = synth.edm_args(diffusion_steps=T, dataset="hetro"), synth.pred_args(dataset="hetro")
    esd = synth.synth_edm_state_dict(eargs, F, seed=61)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=62)
    eng = _engine(eargs, esd, pargs, psd, GAUDI_FAMILY_SPLIT=1)
    spec = _params(19, B)
    a = eng.sample_target(nm, em, spec, seed=6, return_z0=True)
    assert a[2]["family_split_resident"] == 0 and eng.last_launch_shape() == (B, N)
    assert eng.kernel_variant()[1] == 8 and eng.node_buffers_global()
    b = eng.sample_callback(nm, em, _grad(spec), seed=6, scale=1.0, return_z0=True)
    assert _same((a[0], a[1], a[3]), (b[0], b[1], b[3]))
    eng.sample(nm, em, seed=6, target_w=spec["w"][0], scale=0.6)
    assert eng.family_split() > 0  # the affine call of the same batch does split
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. window
def test_window_equals_a_callback_that_returns_zeros_outside_it(golden):
    eng, nm, em, noise, T = _tiny(golden, "hetro_tiny")
    B = nm.shape[0]
    win = (1, 20)
    spec = dict(_params(17, B), window=win)
    xa, ha, _, za, tr = eng.sample_target(nm, em, spec, noise=noise, return_z0=True, trace=True)
    xb, hb, _, zb = eng.sample_callback(nm, em, _grad(spec, win, T), noise=noise, scale=1.0, return_z0=True)
    assert np.array_equal(xa, xb) and np.array_equal(ha, hb) and np.array_equal(za, zb)
    # trace row k belongs to the step from time index T - k
    assert tr.shape == (T, B, K + 2)
    assert not tr[: T - 20].any() and (tr[T - 20:, :, K + 1] > 0).all()
    full = eng.sample_target(nm, em, dict(spec, window=None), noise=noise, return_z0=True)
    assert not np.array_equal(full[3], za)
    from gaudi_amd._lib import GaudiError
    for bad in ((0, 20), (5, T + 1), (21, 20)):
        with pytest.raises(GaudiError, match="window"):
            eng.sample_target(nm, em, dict(spec, window=bad), noise=noise)
    with pytest.raises(GaudiError, match="side"):
        eng.sample_target(nm, em, dict(spec, side=np.full(K, 2, np.int32)), noise=noise)
    with pytest.raises(GaudiError, match="finite"):
        eng.sample_target(nm, em, dict(spec, c=np.full(K, np.nan, np.float32)), noise=noise)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. trace
def _ulp_diff(a, b):
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_trace_against_the_callback_path_and_the_clip_formula(golden):
    eng, nm, em, noise, T = _tiny(golden, "cata_tiny")
    B = nm.shape[0]
    # where the predictions go without guidance: the one-sided terms get their centres at the median of that trace, so
    # each of them is on for part of the chain and off for the rest
    tr0 = eng.sample_target(nm, em, dict(scale=0.0), noise=noise, trace=True)[3]
    side = np.tile(np.array([1, -1, 0, 1, -1], np.int32), (B, 1))
    spec = dict(q=np.ones((B, K), np.float32), c=np.median(tr0[:, :, :K], axis=0).astype(np.float32), side=side,
                scale=np.array([1e-3, 0.05, 30.0, 3000.0], np.float32)[:B])
    seen = []
    xa, ha, _, tr = eng.sample_target(nm, em, spec, noise=noise, trace=True)
    xb, hb, _ = eng.sample_callback(nm, em, _grad(spec, seen=seen), noise=noise, scale=1.0)
    assert np.array_equal(xa, xb) and np.array_equal(ha, hb)
    pred, norm, clip = tr[:, :, :K], tr[:, :, K], tr[:, :, K + 1]
    assert np.array_equal(pred.view(np.uint32), np.stack(seen).view(np.uint32))  # what the callback was handed, step by step
    want = np.minimum(np.float32(1), np.float32(10) / (norm + np.float32(1e-6))).astype(np.float32)
    assert _ulp_diff(clip, want).max() <= 4
    assert (clip < 1).any() and (clip == 1).any(), "the scales must span clipped and unclipped steps"
    d = pred - spec["c"][None]
    for k in (0, 1, 3, 4):
        active = d[:, :, k] > 0 if side[0, k] > 0 else d[:, :, k] < 0
        assert active.any() and (~active).any(), f"one-sided term {k} never switches"
    eng.close()


def test_step_trace_norm_against_predictor_grad(golden):
    from oracle import gaudi_oracle as O
    g = golden("g29_value_target")
    cfg = json.loads(str(g["tiny_cfg"]))
    eargs, esd = edm_from_cfg(dict(dataset=cfg["dataset"], over=TINY, wseed=cfg["eseed"], amp=True), diffusion_steps=cfg["T"])
    pargs, psd = pred_from_cfg(dict(dataset=cfg["dataset"], over=TINY_P, wseed=cfg["pseed"], amp=True))
    eng = _engine(eargs, esd, pargs, psd)
    z, nm3, em = g["tiny_z"], g["tiny_node_mask"], g["tiny_edge_mask"]
    B, N, D = z.shape
    nm = nm3.reshape(B, N)
    s, T = 500, cfg["T"]
    eps = g[f"tiny_s{s}_eps"]
    spec = _spec_of(g, "tiny_weak")
    _, tr = eng.step_target(s, z, nm, em, eps, spec, trace=True)
    # z_s before guidance, rebuilt from phi, the step table and the injected noise (en_diffusion.py:843-852, 897)
    a_ts, c_eps, sigma, t = eng.step_coefficients()[s]
    zs = z / a_ts - c_eps * eng.phi(z, t, nm, em) + sigma * O._combined_noise(eps, nm3)
    p = eng.predictor_fwd(zs, t, nm, em)
    seed = numpy_seed(spec["w"], spec["q"], spec["c"], spec["side"], spec["scale"], p)
    _, grad = eng.predictor_grad(zs, t, nm, em, seed)
    norm = np.sqrt((grad.astype(np.float64) ** 2).sum((1, 2)))
    assert rel_err(tr[:, :K], p) < TOL
    assert rel_err(tr[:, K], norm) < TOL
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. sharding
def test_two_ranks_per_sample_parameters(tmp_path):
    """world_size = 2 (gloo rendezvous, both ranks on this GPU): a mixed-parameter batch through
    sample_sharded(per_sample=...) equals the unsharded call bit for bit."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker_value_target.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    errs = "".join(open(tmp_path / f).read() for f in sorted(os.listdir(tmp_path)) if f.startswith("err"))
    assert r.returncode == 0, errs + r.stderr[-1500:]
    ref = np.load(tmp_path / "unsharded.npz")
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert (int(r0["lo"]), int(r0["hi"]), int(r1["lo"]), int(r1["hi"])) == (0, 6, 6, 11)
    assert np.array_equal(r0["x"], r1["x"]) and np.array_equal(r0["h"], r1["h"])
    assert np.array_equal(r0["x"], ref["x"]) and np.array_equal(r0["h"], ref["h"])
    assert np.isfinite(ref["x"]).all()
    assert not np.array_equal(ref["x"], ref["x_uniform"]), "the per-molecule parameters must matter"


# ------------------------------------------------------------------------------------------------ 9. design_sweep
def test_design_sweep_returns_each_setting_as_its_own_call_would(golden, capsys):
    """One sampling call for three settings (two scales of a shared target, one other ValueTarget): the dict of setting j holds
    molecules j * batch_size .. and equals, bit for bit, what sample_guidance gives for that setting alone at the same seed and
    the sample offset of its first molecule; its target values are that setting's target on its own molecules."""
    from gaudi_amd import generation_guidance as gg
    from gaudi_amd import sampling_edm
    from gaudi_amd.models_edm import ValueTarget, get_cond_predictor_model, get_model
    g = golden("g7_end_to_end")
    cfg = cfg_of(g, "cata_tiny")
    eargs, esd = edm_from_cfg(dict(dataset="cata", amp=cfg["amp"], over=TINY, wseed=cfg["eseed"]), diffusion_steps=cfg["T"])
    pargs, psd = pred_from_cfg(dict(dataset="cata", amp=cfg["amp"], over=TINY_P, wseed=cfg["pseed"]))
    model, _, _ = get_model(eargs, state_dict=esd)
    pred = get_cond_predictor_model(pargs, model=model, state_dict=psd)
    bs, n_nodes = 3, 7
    args = types.SimpleNamespace(device="cuda", dataset="cata", max_nodes=11, batch_size=bs)
    base = ValueTarget(pred, weights=np.array([0, -1, 0, 0, 0], np.float32), curvature=np.array([0.5, 0, 0, 1, 0], np.float32),
                       center=np.array([0.3, 0, 0, -0.2, 0], np.float32), side=np.array([0, 0, 0, 1, 0], np.int32), scale=0.5)
    other = ValueTarget(pred, curvature=np.full(K, 0.7, np.float32), center=np.linspace(-1, 1, K).astype(np.float32),
                        side=np.array([1, -1, 0, 1, -1], np.int32), scale=1.5)
    settings = [0.3, 2.0, other]
    model.seed, model.sample_offset = 7, 0
    out = gg.design_sweep(args, model, pred, settings, None, None, n_nodes, target=base, scale=0.8)
    assert len(out) == 3 and model.sample_offset == 3 * bs
    for j, st in enumerate(settings):
        tgt, mult = (st, 1.0) if isinstance(st, ValueTarget) else (base, st)
        model.seed, model.sample_offset = 7, j * bs
        x, h, nm, em = sampling_edm.sample_guidance(args, model, tgt, np.full(bs, n_nodes), scale=0.8 * mult)
        d = out[j]
        assert np.array_equal(np.asarray(d["x"]), x.numpy()) and np.array_equal(np.asarray(d["one_hot"]), h.numpy()), j
        assert np.asarray(d["x"]).shape[0] == bs and len(d["stability"]["molecule_stable_bool"]) == bs
        vals = np.asarray(gg.get_target_function_values(x, h, tgt, nm, em, model))
        assert rel_err(np.asarray(d["target_function_values"]), vals) < TOL, j
    assert not np.array_equal(np.asarray(out[0]["x"]), np.asarray(out[1]["x"])), "the scale must matter"
    # refusals: per-molecule arrays, a non-scalar scale, windows that differ, scales without a target
    with pytest.raises(ValueError, match=r"\[K\]"):
        gg.design_sweep(args, model, pred, [ValueTarget(pred, weights=np.zeros((bs, K), np.float32))], None, None, n_nodes)
    with pytest.raises(ValueError, match="scalar scale"):
        gg.design_sweep(args, model, pred, [ValueTarget(pred, weights=np.zeros(K, np.float32), scale=np.ones(bs, np.float32))], None,
                        None, n_nodes)
    with pytest.raises(ValueError, match="window"):
        gg.design_sweep(args, model, pred, [base, ValueTarget(pred, weights=np.zeros(K, np.float32), window=(1, 20))], None, None,
                        n_nodes)
    with pytest.raises(ValueError, match="target="):
        gg.design_sweep(args, model, pred, [0.5], None, None, n_nodes)
    model.engine.close()
