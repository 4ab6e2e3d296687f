"""Value-seeking targets without a device: the host twin of the seed the kernels compute (gaudi_host_target_seed) against the
numpy float32 expression, ValueTarget against the formula and torch.autograd, the refusals, per-sample sharding, and the
numpy oracle driven by the host twin against the reference's own guided steps and chains (g29)."""
import ctypes as C
import json

import numpy as np
import pytest

from gaudi_amd import _lib
from gaudi_amd._lib import GaudiError
from gaudi_amd.engine import host_target_seed, target_spec
from tests.helpers import TINY, TINY_P, cfg_of, edm_from_cfg, pred_from_cfg, rel_err
from tests.value_target_helpers import numpy_seed

TOL = 1e-4
K = 5


def random_params(seed, B, per_mol=True):
    rng = np.random.default_rng(seed)
    shp = (B, K) if per_mol else (K,)
    return dict(w=rng.standard_normal(shp).astype(np.float32), q=rng.uniform(-1, 2, shp).astype(np.float32),
                c=rng.standard_normal(shp).astype(np.float32), side=rng.integers(-1, 2, shp).astype(np.int32),
                scale=rng.uniform(0.1, 3, B).astype(np.float32) if per_mol else np.float32(0.7))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("per_mol", [True, False])
def test_host_seed_equals_the_numpy_expression_bit_for_bit(per_mol):
    B = 257
    par = random_params(1, B, per_mol)
    rng = np.random.default_rng(2)
    p = (3 * rng.standard_normal((B, K))).astype(np.float32)
    p[rng.random((B, K)) < 0.05] = np.nan
    p[0] = par["c"][0] if per_mol else par["c"]  # d = 0 exactly: both hinges inactive
    got = host_target_seed(par, p)
    want = numpy_seed(par["w"], par["q"], par["c"], par["side"], par["scale"], p)
    sd = np.broadcast_to(par["side"], p.shape)
    assert (sd == 1).any() and (sd == -1).any() and (sd == 0).any() and np.isnan(p).any()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)  # a NaN prediction: NaN through a value term, 0 through a hinge
    assert (nan.sum() < np.isnan(p).sum()) and same_bits(got[~nan], want[~nan])


def test_mixed_shared_and_per_molecule_arrays():
    B = 6
    per, shared = random_params(3, B, True), random_params(4, B, False)
    spec = dict(w=shared["w"], q=per["q"], c=per["c"], side=shared["side"], scale=per["scale"])
    p = np.random.default_rng(5).standard_normal((B, K)).astype(np.float32)
    assert same_bits(host_target_seed(spec, p), numpy_seed(spec["w"], spec["q"], spec["c"], spec["side"], spec["scale"], p))
    # absent arrays: w = q = c = side = 0, scale = 1
    assert same_bits(host_target_seed(dict(w=shared["w"]), p), np.broadcast_to(shared["w"], p.shape))


def test_value_target_call_and_autograd():
    import torch

    from gaudi_amd.models_edm import ValueTarget
    B = 9
    par = random_params(6, B, True)
    p = np.random.default_rng(7).standard_normal((B, K)).astype(np.float32)

    class FakePredictor:
        def __call__(self, xh, nm, em, t):
            return torch.from_numpy(p)

    vt = ValueTarget(FakePredictor(), par["w"], par["q"], par["c"], par["side"], par["scale"])
    val = vt(None, None, None, None)
    pt = torch.from_numpy(p).requires_grad_(True)
    side = torch.from_numpy(par["side"])
    d = pt - torch.from_numpy(par["c"])
    a = torch.where(side == 0, d, torch.where(side > 0, d.clamp(min=0), d.clamp(max=0)))
    formula = (torch.from_numpy(par["w"]) * pt).sum(1) + (torch.from_numpy(par["q"]) * a * a).sum(1)
    np.testing.assert_allclose(np.asarray(val), formula.detach().numpy(), rtol=1e-6, atol=1e-6)
    (g,) = torch.autograd.grad((torch.from_numpy(par["scale"]) * formula).sum(), pt)
    # float32 rounding of the autograd side: a few operations in another order (2 q a against (q + q) a is exact)
    np.testing.assert_allclose(vt.grad(p), g.numpy(), rtol=4 * np.finfo(np.float32).eps, atol=1e-7)
    # the call's scale multiplies the target's own
    assert same_bits(vt.spec(0.5)["scale"], par["scale"] * np.float32(0.5))
    # a ValueTarget is accepted where a spec dict is; anything else that is not a dict is refused
    assert same_bits(host_target_seed(vt, p), vt.grad(p))
    with pytest.raises(GaudiError, match="dict"):
        host_target_seed(object(), p)


def test_from_physical_round_trip():
    from gaudi_amd.models_edm import PropertyNorm, ValueTarget
    rng = np.random.default_rng(8)
    mean, std = rng.standard_normal(K).astype(np.float32), rng.uniform(0.5, 2, K).astype(np.float32)
    prop = PropertyNorm(mean, std)
    w, q, c = (rng.standard_normal(K).astype(np.float32) for _ in range(3))
    side = np.array([0, 1, -1, 0, 1], np.int32)
    vt = ValueTarget.from_physical(None, prop, weights=w, curvature=q, center=c, side=side, scale=0.6, window=(1, 20))
    np.testing.assert_allclose(prop.unnormalize(vt.center), c, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(vt.curvature / (std * std), q, rtol=1e-6)
    np.testing.assert_allclose(vt.weights / std, w, rtol=1e-6)
    assert np.array_equal(vt.side, side) and vt.window == (1, 20)
    # the physical target and the normalised one have the same value up to the dropped constant w . mean
    P = rng.standard_normal((4, K)).astype(np.float32) * 2
    d = P - c
    a = np.where(side == 0, d, np.where(side > 0, np.maximum(d, 0), np.minimum(d, 0)))
    phys = (w * P).sum(1) + (q * a * a).sum(1)
    np.testing.assert_allclose(vt.value(prop.normalize(P)) + (w * mean).sum(), phys, rtol=1e-4, atol=1e-4)


def test_refusals():
    lib = _lib.load_library()
    B = 3
    p = np.zeros((B, K), np.float32)
    out = np.zeros_like(p)

    def rc(spec, k=K):
        cs, keep = target_spec(spec, B, k)
        return lib.gaudi_host_target_seed(C.byref(cs), B, K, _lib.fptr(p), _lib.fptr(out))

    assert rc(dict(w=np.ones(K, np.float32))) == 0
    assert rc(dict(w=np.ones(4, np.float32)), k=4) != 0  # K mismatch
    assert rc(dict(side=np.array([0, 2, 0, 0, 0], np.int32))) != 0
    assert rc(dict(side=np.full((B, K), -2, np.int32))) != 0
    for name in ("w", "q", "c"):
        bad = np.zeros((B, K), np.float32)
        bad[2, 4] = np.inf
        assert rc({name: bad}) != 0, name
    assert rc(dict(scale=np.array([1, np.nan, 1], np.float32))) != 0
    with pytest.raises(GaudiError, match="side"):
        host_target_seed(dict(side=np.array([0, 3, 0, 0, 0])), p)
    with pytest.raises(GaudiError, match=r"\[K\]"):
        target_spec(dict(w=np.ones((B + 1, K), np.float32)), B, K)
    with pytest.raises(GaudiError, match="side"):
        target_spec(dict(side=np.full(K, 0.5)), B, K)
    with pytest.raises(GaudiError, match="scale"):
        target_spec(dict(scale=np.ones(B + 1, np.float32)), B, K)
    with pytest.raises(GaudiError, match="unknown"):
        target_spec(dict(weights=np.ones(K)), B, K)
    # a 1-d scale is per molecule and needs B entries ([0.6] with B = 3 would be read past its end); a number is shared
    with pytest.raises(GaudiError, match="scale"):
        target_spec(dict(scale=[0.6]), B, K)
    assert target_spec(dict(scale=0.6), B, K)[0].scale_per_mol == 0 and target_spec(dict(scale=[0.6]), 1, K)[0].scale_per_mol == 1
    # NOT covered here: the window refusals (outside 1..T, empty).  T belongs to a loaded denoiser, and the device-free
    # gaudi_host_target_seed has none to check a window against; tests/test_gpu_value_target.py
    # (test_window_equals_a_callback_that_returns_zeros_outside_it) exercises them through gaudi_sample_target.


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sample_sharded_slices_per_sample_arrays_by_global_index(world):
    from gaudi_amd.dist import sample_sharded, shard_bounds
    B, N = 7, 4  # uneven over 2 and 3 ranks
    nm = np.ones((B, N), np.float32)
    em = np.ones((B, N, N), np.float32)
    per = dict(c=np.arange(B * K, dtype=np.float32).reshape(B, K), scale=np.arange(B, dtype=np.float32))
    seen = []

    def fake(nm_s, em_s, offset, per_sample=None):
        seen.append((offset, per_sample))
        return np.full((len(nm_s), N, 3), offset, np.float32), np.zeros((len(nm_s), N, 1), np.float32)

    got = np.zeros(B, bool)
    for rank in range(world):
        lo, hi, x, h = sample_sharded(fake, nm, em, rank, world, per_sample=per)
        assert (lo, hi) == shard_bounds(B, rank, world)
        off, ps = seen[-1]
        assert off == lo and set(ps) == {"c", "scale"}
        assert np.array_equal(ps["c"], per["c"][lo:hi]) and np.array_equal(ps["scale"], per["scale"][lo:hi])
        got[lo:hi] = True
    assert got.all()
    with pytest.raises(ValueError, match="whole batch"):
        sample_sharded(fake, nm, em, 0, world, per_sample=dict(c=np.zeros((B - 1, K), np.float32)))


def _spec_of(g, prefix):
    return {k: g[f"{prefix}_{k}"] for k in ("w", "q", "c", "side", "scale")}


def test_oracle_with_the_host_twin_reproduces_g29(golden):
    """Pins the fixture and the formula before a GPU is involved: the numpy oracle, handed the host twin as its dT/dpred
    callable (scale = 1: the per-molecule scale is inside the seed, as it is inside the reference's closure), against the
    reference's sample_p_zs_given_zt_guidance and sample_guidance."""
    from oracle import gaudi_oracle as O
    g = golden("g29_value_target")
    cfg = json.loads(str(g["tiny_cfg"]))
    eargs, esd = edm_from_cfg(dict(dataset=cfg["dataset"], over=TINY, wseed=cfg["eseed"], amp=True), diffusion_steps=cfg["T"])
    pargs, psd = pred_from_cfg(dict(dataset=cfg["dataset"], over=TINY_P, wseed=cfg["pseed"], amp=True))
    gamma = O.gamma_table("polynomial_2", cfg["T"], 1e-5)
    z, nm, em = g["tiny_z"], g["tiny_node_mask"], g["tiny_edge_mask"]
    clipped = False
    for strength in ("weak", "strong"):
        spec = _spec_of(g, f"tiny_{strength}")
        for s in cfg["steps"]:
            zg, aux = O.step_guided(esd, eargs, psd, pargs, gamma, s, z, nm, em, g[f"tiny_s{s}_eps"],
                                    lambda p, t: host_target_seed(spec, p), 1.0, return_aux=True)
            assert rel_err(zg, g[f"tiny_{strength}_s{s}_zs"]) < TOL, (strength, s)
            clipped = clipped or bool((aux["gnorm"] > 10).any())
    assert clipped, "the strong scales must exercise the clip"
    for name in ("cata_chain", "hetro_chain"):
        cfg = cfg_of(g, name)
        base = dict(dataset=cfg["dataset"], amp=cfg["amp"])
        eargs, esd = edm_from_cfg(dict(base, over=TINY, wseed=cfg["eseed"]), diffusion_steps=cfg["T"])
        pargs, psd = pred_from_cfg(dict(base, over=TINY_P, wseed=cfg["pseed"]))
        spec = _spec_of(g, name)
        x, h, _ = O.sample(esd, eargs, g[name + "_node_mask"], g[name + "_edge_mask"], g[name + "_noise"], std=1.0, pred_sd=psd,
                           pcfg=pargs, target_w=lambda p, t: host_target_seed(spec, p), scale=1.0)
        assert rel_err(x, g[name + "_x"]) < TOL, name
        assert np.array_equal(h, g[name + "_h"]), name
