"""The device noise stream (csrc/device_common.h: philox_normal4) on the GPU at the keys production uses: 62-bit seeds, global
sample indices that cross 2^32 inside the batch, N * D = 2 mod 4 (a partial last quad), draws up to 1001.

a. Engine.philox_normal against the float64 reference of tests/noise_helpers.py on every entry of KEYS and EXTREMES, on
   |dev - z| / max(1, r) (an angle error times the radius plus a relative error of the radius).  The bar is noise_helpers.BAR =
   8.24e-7: twice what the numpy twin measures against the same reference on the CPU (tests/test_philox_cpu.py) -- the device's
   logf / sincosf / sqrtf are another library's, each good to an ulp or two of fp32, under the same error model.
   Measured on an MI355X over the same 83209 values: 4.14e-7 (plain maximum 1.55e-6); the largest radius comes out as
   5.7681071 against 5.7681075.
b. Every entry point that draws inside its kernel, called with seed / sample_offset, against the same call with noise= built from
   Engine.philox_normal of the same key in the layout the entry point documents: bit for bit, every output array.
c. One unguided and one guided chain drawn on the device against oracle.gaudi_oracle.sample in float64 fed normal_f64's draws:
   the in-kernel stream tied to the published generator through nothing the device computed."""
import numpy as np
import pytest

from gaudi_amd import synth
from gaudi_amd.sampling_edm import build_masks
from tests import noise_helpers as H
from tests.grid_helpers import engine
from tests.helpers import TINY, TINY_P, direct_z_target_grad, nonlinear_target_grad

pytestmark = pytest.mark.gpu

S, O = H.S62, H.CARRY  # the batch straddles the carry: molecules 0, 1 below 2^32, the rest above
W = np.array([0.5, -1.0, 0.25, 0.0, 1.0], np.float32)
SCALE = 0.6
K = 5
HETERO = [3, 5, 4, 3, 2, 5, 3, 4, 5]  # rings; N * D = 10 * 15 = 150 = 2 mod 4, masked slots in every molecule but three
CATA = [6, 8, 8, 3, 11, 5, 7]


# ------------------------------------------------------------------------------------------------ a. the stand-alone stream
@pytest.fixture(scope="module")
def bare():
    from gaudi_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def test_stream_against_float64_reference(bare):
    worst_s = worst_p = 0.0
    for key in H.all_keys():
        dev = bare.philox_normal(*key)
        z, r = H.normal_f64(*key)
        assert dev.shape == z.shape and np.isfinite(dev).all(), key
        s, p = H.scaled_error(dev, z, r)
        print(f"{key}: scaled {s:.3e} plain {p:.3e}")
        worst_s, worst_p = max(worst_s, s), max(worst_p, p)
    print(f"device vs float64: scaled {worst_s:.4e}, plain {worst_p:.4e} (bar {H.BAR:.2e}; the numpy twin: {H.TWIN_SCALED:.2e})")
    assert worst_s < H.BAR


def test_stream_sharding_identities_bit_for_bit(bare):
    carry, past, wide = bare.philox_normal(*H.KEY_CARRY), bare.philox_normal(*H.KEY_PAST), bare.philox_normal(*H.KEY_212)
    assert np.array_equal(carry[:, 2:], past)
    assert np.array_equal(carry, wide[:, :, :210])
    seed, off, B, n, d0, nd = H.KEY_CARRY
    for other in (bare.philox_normal(seed ^ (1 << 40), off, B, n, d0, nd), bare.philox_normal(seed, off + (1 << 40), B, n, d0, nd),
                  bare.philox_normal(seed, off, B, n, d0 + nd, nd)):
        assert np.all(other != carry)
    for b in range(B):  # every sample alone, every draw alone
        for d in range(nd):
            assert np.array_equal(bare.philox_normal(seed, off + b, 1, n, d0 + d, 1)[0, 0], carry[d, b]), (b, d)
    seed, off, B, n, d0, nd = next(k for k in H.KEYS if k[1] == -2)
    wrap = bare.philox_normal(seed, off, B, n, d0, nd)
    assert np.array_equal(wrap[:, 2:], bare.philox_normal(seed, 0, 2, n, d0, nd))


def test_second_trip_of_the_grid_stride_loop_equals_pieces(bare):
    seed, off, B, n, d0, nd = H.KEY_LARGE
    assert B * n * nd > 65536 and (B * n * nd) % 65536 and B * n <= 65536
    whole = bare.philox_normal(*H.KEY_LARGE)
    for d in range(nd):
        assert np.array_equal(bare.philox_normal(seed, off, B, n, d0 + d, 1)[0], whole[d]), d
    for b in range(B):
        assert np.array_equal(bare.philox_normal(seed, off + b, 1, n, d0, nd)[:, 0], whole[:, b]), b


def test_extremes_of_the_radius(bare):
    key, col = H.extreme_key("radius_0")
    dev = bare.philox_normal(*key)[0, 0]
    assert np.isfinite(dev).all() and np.all(dev[col:col + 2] == 0), dev[col - 4:col + 8]
    key, col = H.extreme_key("radius_max")
    dev = bare.philox_normal(*key)[0, 0].astype(np.float64)
    z, r = H.normal_f64(*key)
    assert r[0, 0, col] == H.R_MAX
    rad = float(np.hypot(dev[col], dev[col + 1]))
    print(f"largest radius on the device: {rad:.7f} (float64: {H.R_MAX:.7f})")
    assert abs(rad - H.R_MAX) < H.BAR * H.R_MAX * 2  # (two components, each within BAR * r)


# ------------------------------------------------------------------------------------------------ b. drawn inside = injected
def _nets(dataset, T, widths="tiny", amp=True):
    F = synth.num_node_features(dataset)
    over_e, over_p = (TINY, TINY_P) if widths == "tiny" else (dict(nf=192, n_layers=2), dict(nf=196, n_layers=2))
    eargs = synth.edm_args(dataset=dataset, diffusion_steps=T, **over_e)
    pargs = synth.pred_args(dataset=dataset, **over_p)
    esd = synth.synth_edm_state_dict(eargs, F, seed=21, amplify_coord=amp)
    psd = synth.synth_predictor_state_dict(pargs, F, K, seed=22, amplify_coord=amp)
    return eargs, esd, pargs, psd


def _batch(dataset, sizes=None):
    sizes = (CATA if dataset == "cata" else HETERO) if sizes is None else sizes
    nm3, em_flat, N = build_masks(sizes, max(sizes), dataset != "cata")
    B = len(sizes)
    D = 3 + synth.num_node_features(dataset)
    if dataset != "cata":
        assert (N * D) % 4 == 2 and N * D > 128  # a partial last quad, and quads past 31
    return nm3.reshape(B, N), em_flat.reshape(B, N, N), B, N, D


def _molecules(nm, D, seed):
    """Given molecules: masked, mean-free coordinates and one ring type per live node."""
    B, N = nm.shape
    rng = np.random.default_rng(seed)
    m = nm[:, :, None]
    x = rng.standard_normal((B, N, 3)).astype(np.float32) * 2.0 * m
    x = (x - x.sum(1, keepdims=True) / np.maximum(m.sum(1, keepdims=True), 1) * m).astype(np.float32)
    oh = (np.eye(D - 3, dtype=np.float32)[rng.integers(0, D - 3, (B, N))] * m).astype(np.float32)
    return x, oh


def _draws(eng, B, N, D, n_draws, sample=O, nb=None):
    """Draws 0 .. n_draws - 1 of (S, sample + b) in the layout of injected noise: [n_draws, B, N, D], element n * D + d."""
    nb = B if nb is None else nb
    return np.ascontiguousarray(eng.philox_normal(S, sample, nb, N * D, 0, n_draws).reshape(n_draws, nb, N, D))


def _same(a, b, what):
    assert len(a) == len(b), what
    n = 0
    for u, v in zip(a, b):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v), (what, float(np.abs(u.astype(np.float64) - v).max()))
            n += 1
    assert n >= 2 and np.isfinite(a[0]).all(), what


CONFIGS = {
    "default_packed": dict(env={}, packed=True),
    "one_molecule_per_workgroup": dict(env=dict(GAUDI_PACK=0)),
    "waves4": dict(env=dict(GAUDI_WAVES=4)),
    "global_node_buffers_4": dict(env=dict(GAUDI_FORCE_GN=1)),
}


@pytest.mark.parametrize("dataset", ["hetro", "cata"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_sample_drawn_equals_injected(config, dataset):
    """gaudi_sample, unguided and guided: noise [T+2, B, N, D], draw k of (S, O + b) at noise[k, b]."""
    c = CONFIGS[config]
    T = 5
    nm, em, B, N, D = _batch(dataset)
    eng = engine(*_nets(dataset, T), **c["env"])
    noise = _draws(eng, B, N, D, T + 2)
    for kw in (dict(std=0.7), dict(target_w=W, scale=SCALE)):
        a = eng.sample(nm, em, seed=S, sample_offset=O, return_z0=True, **kw)
        shape = eng.last_launch_shape()
        b = eng.sample(nm, em, noise=noise, return_z0=True, **kw)
        assert eng.last_launch_shape() == shape
        _same(a, b, (config, dataset, sorted(kw)))
        if c.get("packed"):
            assert shape[0] < B, shape  # the packed path really ran
        if config == "one_molecule_per_workgroup":
            assert shape == (B, N), shape
    if config in ("waves4", "global_node_buffers_4"):
        assert eng.kernel_variant()[1] == 4
    eng.close()


def test_sample_drawn_equals_injected_in_wide_groups():
    """GAUDI_PAIRS=2 on the default widths: two 11-node molecules share a workgroup (the PG kernel)."""
    T = 4
    nm, em, B, N, D = _batch("cata", [11] * 6)
    eng = engine(*_nets("cata", T, widths="default"), GAUDI_PAIRS=2)
    noise = _draws(eng, B, N, D, T + 2)
    for kw in (dict(target_w=W, scale=SCALE), dict(std=0.7)):
        a = eng.sample(nm, em, seed=S, sample_offset=O, return_z0=True, **kw)
        shape = eng.last_launch_shape()
        assert shape[0] < B and shape[1] > N, shape
        b = eng.sample(nm, em, noise=noise, return_z0=True, **kw)
        _same(a, b, sorted(kw))
    launched = eng.kernel_keys_launched()
    print("launched " + " | ".join(launched))
    assert any(" PG=1 " in k for k in launched), launched
    eng.close()


@pytest.mark.parametrize("dataset", ["hetro", "cata"])
def test_grid_chains_drawn_equal_injected(dataset):
    """A coarse grid from the prior (the step down to s reads draw T - s) and from given molecules (draw 0 noises them to
    g[0]: the chain's draw_base path), unguided and guided."""
    T = 6
    nm, em, B, N, D = _batch(dataset)
    eng = engine(*_nets(dataset, T))
    noise = _draws(eng, B, N, D, T + 2)
    x0, oh0 = _molecules(nm, D, 4)
    for kw in ({}, dict(target_w=W, scale=SCALE)):
        a = eng.sample(nm, em, seed=S, sample_offset=O, grid=[6, 3, 1, 0], return_z0=True, **kw)
        b = eng.sample(nm, em, noise=noise, grid=[6, 3, 1, 0], return_z0=True, **kw)
        _same(a, b, ("prior", dataset, sorted(kw)))
        st = dict(grid=[4, 2, 0], start=(x0, oh0), return_z0=True, return_zt=True)
        a = eng.sample(nm, em, seed=S, sample_offset=O, **st, **kw)
        b = eng.sample(nm, em, noise=noise, **st, **kw)
        assert len(a) == 5
        _same(a, b, ("start", dataset, sorted(kw)))
    eng.close()


@pytest.mark.parametrize("dataset", ["hetro", "cata"])
def test_target_callback_and_chain_drivers_drawn_equal_injected(dataset):
    """gaudi_sample_target with a curved spec, gaudi_sample_cb / gaudi_sample_cbz, gaudi_sample_chain."""
    T = 5
    nm, em, B, N, D = _batch(dataset)
    eng = engine(*_nets(dataset, T))
    noise = _draws(eng, B, N, D, T + 2)
    rng = np.random.default_rng(11)
    side = rng.integers(-1, 2, (B, K)).astype(np.int32)
    side[:, :3] = np.array([0, 1, -1], np.int32)
    spec = dict(w=(0.5 * rng.standard_normal((B, K))).astype(np.float32), q=rng.uniform(0.2, 1.5, (B, K)).astype(np.float32),
                c=(0.5 * rng.standard_normal((B, K))).astype(np.float32), side=side, scale=rng.uniform(0.2, 2.0, B).astype(np.float32))
    a = eng.sample_target(nm, em, spec, seed=S, sample_offset=O, return_z0=True, trace=True)
    b = eng.sample_target(nm, em, spec, noise=noise, return_z0=True, trace=True)
    _same(a, b, "sample_target")
    assert np.abs(a[4]).max() > 0  # the trace: the target was evaluated
    a = eng.sample_callback(nm, em, nonlinear_target_grad, seed=S, sample_offset=O, scale=SCALE, return_z0=True)
    b = eng.sample_callback(nm, em, nonlinear_target_grad, noise=noise, scale=SCALE, return_z0=True)
    _same(a, b, "sample_callback")
    tz = direct_z_target_grad(nm)
    a = eng.sample_callback(nm, em, tz, seed=S, sample_offset=O, scale=SCALE, with_z=True, return_z0=True)
    b = eng.sample_callback(nm, em, tz, noise=noise, scale=SCALE, with_z=True, return_z0=True)
    _same(a, b, "sample_callback with_z")
    a = eng.sample_chain(nm, em, 3, seed=S, sample_offset=O, std=0.7)
    b = eng.sample_chain(nm, em, 3, noise=noise, std=0.7)
    assert a.shape == (3, B, N, D) and np.isfinite(a).all() and np.array_equal(a, b)
    eng.close()


@pytest.mark.parametrize("dataset", ["hetro", "cata"])
def test_nll_and_training_entry_points_drawn_equal_injected(dataset):
    """gaudi_edm_nll (draws 0 and 1 as [2, B, N, D]), gaudi_predict_noised, gaudi_predictor_loss_grad and gaudi_edm_loss_grad
    (draw 0 as [B, N, D])."""
    T = 6
    nm, em, B, N, D = _batch(dataset)
    eng = engine(*_nets(dataset, T))
    noise = _draws(eng, B, N, D, 2)
    x, oh = _molecules(nm, D, 5)
    t_int = (np.arange(B) % T + 1).astype(np.int32)
    a = eng.edm_nll(x, oh, t_int, nm, em, seed=S, sample_offset=O, return_terms=True)
    b = eng.edm_nll(x, oh, t_int, nm, em, seed=0, sample_offset=0, noise=noise, return_terms=True)
    _same(a, b, "edm_nll")
    a = eng.predict_noised(x, oh, t_int, nm, em, seed=S, sample_offset=O)
    b = eng.predict_noised(x, oh, t_int, nm, em, noise=noise[0])
    _same(a, b, "predict_noised")
    y = np.random.default_rng(6).standard_normal((B, K)).astype(np.float32)
    la, pa, ga = eng.predictor_loss_grad(x, oh, t_int, nm, em, y, seed=S, sample_offset=O)
    lb, pb, gb = eng.predictor_loss_grad(x, oh, t_int, nm, em, y, noise=noise[0])
    assert la == lb and np.isfinite(la) and np.array_equal(pa, pb) and np.array_equal(pa, a[1])
    assert sum(v is not None for v in ga.values()) > 4
    for k, v in ga.items():
        assert (v is None) == (gb[k] is None) and (v is None or np.array_equal(v, gb[k])), k
    t0 = (np.arange(B) % (T + 1)).astype(np.int32)  # (t = 0 is the loss's other branch)
    for loss_type in ("l2", "vlb"):
        la, na, ga = eng.edm_loss_grad(x, oh, t0, nm, em, seed=S, sample_offset=O, loss_type=loss_type)
        lb, nb, gb = eng.edm_loss_grad(x, oh, t0, nm, em, noise=noise[0], loss_type=loss_type)
        assert np.array_equal(la, lb) and np.array_equal(na, nb) and np.isfinite(la).all(), loss_type
        assert sum(v is not None for v in ga.values()) > 4
        for k, v in ga.items():
            assert (v is None) == (gb[k] is None) and (v is None or np.array_equal(v, gb[k])), (loss_type, k)
    eng.close()


@pytest.mark.parametrize("dataset", ["hetro", "cata"])
def test_fix_noise_drawn_equals_injected(dataset):
    """set_fix_noise(True, key_sample): every molecule receives the stream of global sample key_sample, whatever the call's
    sample_offset -- the injected form is [T + 2, 1, N, D]."""
    T = 4
    key_sample = 2 ** 33 + 5
    nm, em, B, N, D = _batch(dataset)
    eng = engine(*_nets(dataset, T))
    noise = _draws(eng, B, N, D, T + 2, sample=key_sample, nb=1)
    plain = eng.sample(nm, em, seed=S, sample_offset=O, return_z0=True)
    eng.set_fix_noise(True, key_sample)
    for kw in (dict(target_w=W, scale=SCALE), {}):
        a = eng.sample(nm, em, seed=S, sample_offset=O, return_z0=True, **kw)
        b = eng.sample(nm, em, noise=noise, return_z0=True, **kw)
        _same(a, b, ("fix_noise", dataset, sorted(kw)))
        assert np.array_equal(a[3], eng.sample(nm, em, seed=S, sample_offset=77, return_z0=True, **kw)[3])
    assert not np.array_equal(a[3], plain[3])
    # the low word of the key alone is another stream
    eng.set_fix_noise(True, 5)
    assert not np.array_equal(eng.sample(nm, em, seed=S, sample_offset=O, return_z0=True)[3], a[3])
    eng.close()


# ------------------------------------------------------------------------------------------------ c. the end-to-end anchor
@pytest.mark.parametrize("dataset", ["hetro", "cata"])
def test_chain_against_float64_oracle_fed_the_reference_stream(dataset):
    """T = 3 chains drawn on the device at (S, O) against oracle.gaudi_oracle.sample in float64 on normal_f64's draws (cast to
    float32, as injected noise is): the kernel census's bar, 1e-4 per molecule, and equal one-hot output."""
    from oracle import gaudi_oracle as G
    T = 3
    nm, em, B, N, D = _batch(dataset)
    eargs, esd, pargs, psd = _nets(dataset, T)
    eng = engine(eargs, esd, pargs, psd)
    noise = H.normal_f64(S, O, B, N * D, 0, T + 2)[0].astype(np.float32).reshape(T + 2, B, N, D)
    got = {"unguided": eng.sample(nm, em, seed=S, sample_offset=O), "guided": eng.sample(nm, em, seed=S, sample_offset=O, target_w=W, scale=SCALE)}
    eng.close()
    dead = nm == 0
    for kind, (x, h, diag) in got.items():
        kw = dict(pred_sd=psd, pcfg=pargs, target_w=W, scale=SCALE) if kind == "guided" else {}
        xo, ho, _ = G.sample(esd, eargs, nm[:, :, None], em, noise, dtype=np.float64, **kw)
        xo = np.asarray(xo)
        err = np.abs(x - xo).reshape(B, -1).max(1) / np.abs(xo).reshape(B, -1).max(1)
        print(f"{dataset} {kind}: per-molecule error vs the float64 oracle on the reference stream {err.max():.2e}")
        assert err.max() < 1e-4, (kind, err)
        assert np.array_equal(h, np.asarray(ho, h.dtype)), kind
        assert np.all(x[dead] == 0) and np.all(h[dead] == 0) and diag["max_masked_leak"] == 0
