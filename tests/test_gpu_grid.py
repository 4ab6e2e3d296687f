"""Chains on a chosen time grid, from the prior or from given molecules (gaudi_sample_grid, gaudi_step_pair,
gaudi_sample_cb_grid) on the GPU: the unit grid is today's chain bit for bit in every kernel family, strided steps and whole
chains match the reference (g28 fixtures, the tolerance rule of tests/grid_helpers.py), noise is keyed by time index, and a
molecule's result does not depend on sharding or packing on any grid."""
import types

import numpy as np
import pytest

from gaudi_amd import synth
from gaudi_amd._lib import GaudiError
from gaudi_amd.sampling_edm import build_masks, time_grid
from tests.grid_helpers import assert_g28, engine, oracle_step_pair
from tests.helpers import TINY, TINY_P, cfg_of, direct_z_target_grad, edm_from_cfg, nonlinear_target_grad, pred_from_cfg, rel_err

pytestmark = pytest.mark.gpu

W = np.array([0.5, -1.0, 0.25, 0.0, 1.0], np.float32)
GAP = np.array([0.0, -1.0, 0.0, 0.0, 0.0], np.float32)


@pytest.fixture(scope="module")
def O():
    from oracle import gaudi_oracle
    return gaudi_oracle


def _case(dataset, sizes, T, widths="tiny", sin=False, seed=11, amp=True):
    F = synth.num_node_features(dataset)
    over_e, over_p = (TINY, TINY_P) if widths == "tiny" else ({}, {})
    eargs = synth.edm_args(dataset=dataset, diffusion_steps=T, **(dict(sin_embedding=True) if sin else {}), **over_e)
    pargs = synth.pred_args(dataset=dataset, **over_p)
    esd = synth.synth_edm_state_dict(eargs, F, seed=seed, amplify_coord=amp)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=seed + 1, amplify_coord=amp)
    nm3, em_flat, N = build_masks(sizes, max(sizes), dataset != "cata")
    B = len(sizes)
    return eargs, esd, pargs, psd, nm3.reshape(B, N), em_flat.reshape(B, N, N), N, 3 + F


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v)
    assert np.isfinite(a[0]).all()


def _seeds(nm, D, seed):
    """Given molecules: masked, mean-free coordinates and one ring type per live node."""
    B, N = nm.shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, N, 3)).astype(np.float32) * 2.0 * nm[:, :, None]
    x = (x - x.sum(1, keepdims=True) / np.maximum(nm.sum(1), 1)[:, None, None] * nm[:, :, None]).astype(np.float32)
    oh = np.zeros((B, N, D - 3), np.float32)
    np.put_along_axis(oh, rng.integers(0, D - 3, (B, N, 1)), 1.0, axis=2)
    return x, oh * nm[:, :, None]


# ---------------------------------------------------------------------------------------------- unit grid = today's chain
UNIT_CASES = {
    "default": dict(dataset="cata", sizes=[6, 8, 8, 3], T=20),
    "steps_per_launch_7": dict(dataset="cata", sizes=[6, 8, 8, 3], T=20, spl=7),
    "steps_per_launch_25": dict(dataset="cata", sizes=[6, 8, 8, 3], T=30, spl=25),
    "fix_noise": dict(dataset="cata", sizes=[7, 7, 7], T=12, fix=True),
    "packed_hetero": dict(dataset="hetro", sizes=[3, 5, 4, 3, 2, 5, 3, 4], T=12, packed=True),
    "wide_groups": dict(dataset="cata", sizes=[11] * 6, T=8, env=dict(GAUDI_PAIRS=2), wide=True),
    "n40_default_widths": dict(dataset="hetro", sizes=[20, 6], T=4, widths="default"),
    "waves4": dict(dataset="hetro", sizes=[3, 5, 4], T=12, env=dict(GAUDI_WAVES=4)),
    "fp32_edges": dict(dataset="cata", sizes=[6, 8, 8, 3], T=12, env=dict(GAUDI_EDGE_MATH="fp32")),
    "sin_embedding": dict(dataset="hetro", sizes=[3, 5, 4], T=8, sin=True),
}


@pytest.mark.parametrize("name", list(UNIT_CASES))
def test_unit_grid_equals_sample_bit_for_bit(name):
    """grid = T, T-1, ..., 0 through gaudi_sample_grid against gaudi_sample: guided and unguided, Philox and injected noise."""
    c = UNIT_CASES[name]
    T = c["T"]
    eargs, esd, pargs, psd, nm, em, N, D = _case(c["dataset"], c["sizes"], T, c.get("widths", "tiny"), c.get("sin", False))
    B = len(c["sizes"])
    eng = engine(eargs, esd, pargs, psd, **c.get("env", {}))
    if "spl" in c:
        eng.set_steps_per_launch(c["spl"])
    if c.get("fix"):
        eng.set_fix_noise(True, 5)
    noise = np.random.default_rng(3).standard_normal((T + 2, 1 if c.get("fix") else B, N, D)).astype(np.float32)
    grid = time_grid(T, T)
    for kw in (dict(seed=9, sample_offset=4, target_w=W, scale=0.6), dict(seed=9, sample_offset=4, std=0.7),
               dict(noise=noise, target_w=W, scale=0.6), dict(noise=noise)):
        a = eng.sample(nm, em, return_z0=True, **kw)
        shape = eng.last_launch_shape()
        b = eng.sample(nm, em, return_z0=True, grid=grid, **kw)
        assert eng.last_launch_shape() == shape
        _same(b, a)
        if c.get("packed"):
            assert shape[0] < B, shape
        if c.get("wide"):
            assert shape[0] < B and shape[1] > N, shape
    if name == "n40_default_widths":
        assert eng.node_buffers_global()
    if name == "waves4":
        assert eng.kernel_variant() == (4, 4)
    if name == "fp32_edges":
        assert eng.edge_math()[1] == 0
    eng.close()


def test_step_with_default_t_idx_is_step_bit_for_bit():
    eargs, esd, pargs, psd, nm, em, N, D = _case("hetro", [3, 5, 4], 50)
    eng = engine(eargs, esd, pargs, psd)
    rng = np.random.default_rng(1)
    z = rng.standard_normal((3, N, D)).astype(np.float32) * nm[:, :, None]
    eps = rng.standard_normal((3, N, D)).astype(np.float32)
    for s in (0, 17, 49):
        for kw in ({}, dict(target_w=W, scale=0.6)):
            assert np.array_equal(eng.step(s, z, nm, em, eps, t_idx=s + 1, **kw), eng.step(s, z, nm, em, eps, **kw))
    for s, t in ((5, 5), (5, 4), (-1, 3), (3, 51)):
        with pytest.raises(GaudiError, match="s_idx < t_idx"):
            eng.step(s, z, nm, em, eps, t_idx=t)
    eng.close()


# ---------------------------------------------------------------------------------------------- against the reference (g28)
FAMILIES = {"default": {}, "waves4": dict(GAUDI_WAVES=4), "global_node_buffers_8": dict(GAUDI_FORCE_GN8=1),
            "global_node_buffers_4": dict(GAUDI_FORCE_GN=1), "fp32_edges": dict(GAUDI_EDGE_MATH="fp32")}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("name", ["cata", "hetro", "cata_full"])
def test_strided_steps_teacher_forced_vs_reference(golden, name, family):
    """sample_p_zs_given_zt(s, t) and sample_p_zs_given_zt_guidance(s, t) (scale 0.6: clip branch off, 400: on) for strides
    2, 10, 50 at the top, middle and bottom of the schedule and the pair (T, 0)."""
    g = golden("g28_grid_steps")
    cfg = cfg_of(g, name)
    eargs, esd = edm_from_cfg(dict(dataset=cfg["dataset"], over=cfg["eover"], wseed=cfg["eseed"], amp=cfg["amp"]), diffusion_steps=cfg["T"])
    pargs, psd = pred_from_cfg(dict(dataset=cfg["dataset"], over=cfg["pover"], wseed=cfg["pseed"], amp=cfg["amp"]))
    eng = engine(eargs, esd, pargs, psd, **FAMILIES[family])
    z, nm, em = g[name + "_z"], g[name + "_node_mask"], g[name + "_edge_mask"]
    second_branch = []
    for t_i, s_i in g["pairs"]:
        key = f"{name}_t{t_i}_s{s_i}"
        for kind, kw in (("unguided", {}), ("guided_scale0.6", dict(target_w=GAP, scale=0.6)), ("guided_scale400.0", dict(target_w=GAP, scale=400.0))):
            zs = eng.step(int(s_i), z, nm, em, g[key + "_eps"], t_idx=int(t_i), **kw)
            spread = g[f"{key}_zs_{kind}_spread"]
            if float(spread) >= 5e-5:
                second_branch.append((int(t_i), int(s_i)))
            assert_g28(zs, g[f"{key}_zs_{kind}"], spread, f"{family} {key} {kind}")
    assert all(p == (cfg["T"], 0) for p in second_branch), second_branch  # at most the (T, 0) pairs
    eng.close()


@pytest.mark.parametrize("name", ["cata_tiny", "hetro_tiny", "cata_tiny_amp"])
def test_chains_on_even_and_uneven_grids_vs_reference(golden, name):
    """T = 50 chains from the prior on time_grid(50, 10) and time_grid(50, 7), unguided and guided, injected noise read by
    time index out of the usual [T+2,B,N,D] buffer."""
    g = golden("g28_grid_chains")
    cfg = cfg_of(g, name)
    T = cfg["T"]
    base = dict(dataset=cfg["dataset"], amp=cfg["amp"])
    eargs, esd = edm_from_cfg(dict(base, over=TINY, wseed=cfg["eseed"]), diffusion_steps=T)
    pargs, psd = pred_from_cfg(dict(base, over=TINY_P, wseed=cfg["pseed"]))
    eng = engine(eargs, esd, pargs, psd)
    nm, em, noise = g[name + "_node_mask"], g[name + "_edge_mask"], g[name + "_noise"]
    for n_steps in (10, 7):
        grid = time_grid(T, n_steps)
        assert np.array_equal(grid, g[f"{name}_grid{n_steps}"])
        for kind, kw in (("unguided", dict(std=cfg["std_unguided"])), ("guided", dict(std=cfg["std_guided"], target_w=GAP, scale=cfg["scale"]))):
            x, h, diag = eng.sample(nm, em, noise=noise, grid=grid, **kw)
            key = f"{name}_prior{n_steps}_{kind}"
            if not cfg["amp"]:
                assert float(g[key + "_x_spread"]) < 5e-5  # only the amplified-head chains may take the second branch
            assert_g28(x, g[key + "_x"], g[key + "_x_spread"], key)
            assert np.array_equal(h, g[key + "_h"])
            assert diag["max_masked_leak"] == 0 and diag["nan_count"] == 0
    eng.close()


@pytest.mark.parametrize("name", ["cata_tiny", "hetro_tiny", "cata_tiny_amp"])
def test_refinement_from_given_molecules(golden, name):
    """start = (x, onehot): z_{t_start} is predict_noised's z_t bit for bit (same draw 0, same seed), equals the reference's
    sample_edm_t; the refined molecules equal the reference's chain from that z_t; scale = 0 relates to the unguided
    refinement as it does on today's chain."""
    g = golden("g28_grid_chains")
    cfg = cfg_of(g, name)
    T, t0 = cfg["T"], cfg["t_start"]
    base = dict(dataset=cfg["dataset"], amp=cfg["amp"])
    eargs, esd = edm_from_cfg(dict(base, over=TINY, wseed=cfg["eseed"]), diffusion_steps=T)
    pargs, psd = pred_from_cfg(dict(base, over=TINY_P, wseed=cfg["pseed"]))
    eng = engine(eargs, esd, pargs, psd)
    nm, em, noise = g[name + "_node_mask"], g[name + "_edge_mask"], g[name + "_noise"]
    x0, oh0 = g[name + "_x0"], g[name + "_onehot0"]
    zt_pn, _ = eng.predict_noised(x0, oh0, t0, nm, em, noise=noise[0])
    assert_g28(zt_pn, g[name + "_zt20"], g[name + "_zt20_spread"], name + " z_t of predict_noised")
    for n_steps in (20, 5):
        grid = time_grid(T, n_steps, t0)
        assert np.array_equal(grid, g[f"{name}_refine_grid{n_steps}"])
        for kind, kw in (("unguided", {}), ("guided", dict(target_w=GAP, scale=cfg["scale"]))):
            x, h, diag, zt = eng.sample(nm, em, noise=noise, grid=grid, start=(x0, oh0), return_zt=True, **kw)
            assert np.array_equal(zt, zt_pn)
            key = f"{name}_refine{n_steps}_{kind}"
            if not cfg["amp"]:
                assert float(g[key + "_x_spread"]) < 5e-5
            assert_g28(x, g[key + "_x"], g[key + "_x_spread"], key)
            assert np.array_equal(h, g[key + "_h"])
            assert diag["max_masked_leak"] == 0
    # the same with on-device Philox noise: draw 0 of (seed, global sample index) in both calls
    zt_pn, _ = eng.predict_noised(x0, oh0, t0, nm, em, seed=77, sample_offset=5)
    out = eng.sample(nm, em, seed=77, sample_offset=5, grid=time_grid(T, 5, t0), start=(x0, oh0), return_zt=True, return_z0=True)
    assert len(out) == 5 and np.array_equal(out[4], zt_pn)
    # scale = 0: today's guided chain against today's unguided chain first, then the refinement held to the same relation --
    # bit-equal if those are; otherwise both differ only by the guided step's second mean removal of an already mean-free
    # z (a few ulp per step, at most 20 steps here): rel_err < 1e-5
    grid = time_grid(T, 5, t0)
    unit_u = eng.sample(nm, em, noise=noise)[0]
    unit_g = eng.sample(nm, em, noise=noise, target_w=GAP, scale=0.0)[0]
    ref_u = eng.sample(nm, em, noise=noise, grid=grid, start=(x0, oh0))
    ref_g = eng.sample(nm, em, noise=noise, grid=grid, start=(x0, oh0), target_w=GAP, scale=0.0)
    print(f"scale 0 vs unguided: unit chain {rel_err(unit_g, unit_u):.2e}, refinement {rel_err(ref_g[0], ref_u[0]):.2e}")
    if np.array_equal(unit_u, unit_g):
        assert np.array_equal(ref_u[0], ref_g[0])
    else:
        assert rel_err(ref_g[0], ref_u[0]) < 1e-5
    assert np.array_equal(ref_u[1], ref_g[1])
    eng.close()


# ---------------------------------------------------------------------------------------------- noise keying
def _replay(eng, nm, em, noise, grid, z, T, **kw):
    for t_i, s_i in zip(grid[:-1], grid[1:]):
        z = eng.step(int(s_i), z, nm, em, noise[T - s_i], t_idx=int(t_i), **kw)
    return eng.decode(z, nm, em, noise[T + 1]), z


@pytest.mark.parametrize("env", [{}, dict(GAUDI_WAVES=4), dict(GAUDI_FORCE_GN=1)], ids=["default", "waves4", "global_node_buffers_4"])
@pytest.mark.parametrize("guided", [False, True])
def test_noise_is_keyed_by_time_index(O, guided, env):
    """A chain replayed step by step through Engine.step(s, z, ..., noise[T - s], t_idx=t) and Engine.decode(..., noise[T + 1])
    from the same start reproduces the chain's x, h BIT FOR BIT -- measured first on the unit chain (the state kept in LDS
    across the steps of a launch against a round trip through memory per step: exact, it is the same fp32 data), then held
    on the coarse grids, from the prior and from given molecules."""
    T = 24
    eargs, esd, pargs, psd, nm, em, N, D = _case("hetro", [3, 5, 4, 2], T)
    B = nm.shape[0]
    eng = engine(eargs, esd, pargs, psd, **env)  # (global_node_buffers_4: a guided step is two launches, run_chain's other loop)
    noise = np.random.default_rng(8).standard_normal((T + 2, B, N, D)).astype(np.float32)
    kw = dict(target_w=W, scale=0.6) if guided else {}
    # z_T is not an output of a chain: it is rebuilt here from draw 0, quantised to 1/256 so that the masked mean is exact in
    # fp32 in any summation order and the host's z_T equals the kernel's bit for bit
    noise[0] = np.round(noise[0] * 256) / 256
    zT = O._combined_noise(noise[0], nm[:, :, None], 1.0).astype(np.float32)
    for grid in (time_grid(T, T), time_grid(T, 6), time_grid(T, 5), np.array([24, 23, 9, 8, 1, 0], np.int32)):
        x, h, _, z0 = eng.sample(nm, em, noise=noise, grid=grid, return_z0=True, **kw)
        (xr, hr), zr = _replay(eng, nm, em, noise, grid, zT, T, **kw)
        assert np.array_equal(zr, z0), list(grid)
        assert np.array_equal(xr, x) and np.array_equal(hr, h), list(grid)
    x0, oh0 = _seeds(nm, D, 4)
    for grid in (time_grid(T, 10, 10), time_grid(T, 3, 10)):
        x, h, _, z0, zt = eng.sample(nm, em, noise=noise, grid=grid, start=(x0, oh0), return_z0=True, return_zt=True, **kw)
        (xr, hr), zr = _replay(eng, nm, em, noise, grid, zt, T, **kw)
        assert np.array_equal(zr, z0) and np.array_equal(xr, x) and np.array_equal(hr, h), list(grid)
    eng.close()


@pytest.mark.parametrize("seeded", [False, True])
def test_coarse_grid_is_invariant_to_sharding_and_packing(seeded):
    """A molecule gives the same bits alone, in a shard (sample_offset) and in the whole batch, packed and unpacked."""
    T = 20
    sizes = [3, 5, 4, 3, 2, 5, 3, 4, 5]
    eargs, esd, pargs, psd, nm, em, N, D = _case("hetro", sizes, T)
    B = len(sizes)
    packed = engine(eargs, esd, pargs, psd)
    solo = engine(eargs, esd, pargs, psd, GAUDI_PACK=0)
    x0, oh0 = _seeds(nm, D, 6)
    grid = time_grid(T, 4, 12) if seeded else time_grid(T, 6)
    noise = np.random.default_rng(2).standard_normal((T + 2, B, N, D)).astype(np.float32)

    def run(eng, lo, hi, **kw):
        st = dict(start=(x0[lo:hi], oh0[lo:hi])) if seeded else {}
        hint = eng.plan_hint_for(nm, em)
        eng.set_plan_hint(*hint)  # shards plan with the whole batch's figures (dist.sample_sharded)
        try:
            return eng.sample(nm[lo:hi], em[lo:hi], grid=grid, return_z0=True, **st, **kw)
        finally:
            eng.set_plan_hint(0, 0)

    for kw in (dict(target_w=W, scale=0.6), {}):
        whole = run(packed, 0, B, seed=21, sample_offset=100, **kw)
        assert packed.last_launch_shape()[0] < B
        unpacked = run(solo, 0, B, seed=21, sample_offset=100, **kw)
        assert solo.last_launch_shape() == (B, N)
        _same(unpacked, whole)
        for lo, hi in ((0, 4), (4, 9), (6, 7)):
            part = run(packed, lo, hi, seed=21, sample_offset=100 + lo, **kw)
            for u, v in zip(part, whole):
                if isinstance(u, np.ndarray):
                    assert np.array_equal(u, v[lo:hi]), (lo, hi)
        # injected noise: a shard reads its molecules' rows
        whole = run(packed, 0, B, noise=noise, **kw)
        part = run(solo, 2, 6, noise=np.ascontiguousarray(noise[:, 2:6]), **kw)
        for u, v in zip(part, whole):
            if isinstance(u, np.ndarray):
                assert np.array_equal(u, v[2:6])
    packed.close()
    solo.close()


def test_family_split_buckets_on_a_grid_from_given_molecules():
    """GAUDI_FAMILY_SPLIT=1 runs a request as two buckets (resident kernels / global node buffers), gathered and scattered by
    the host: grid, start and the returned z_t follow a molecule through its bucket -- the whole call equals every molecule
    alone (its own global sample index), and z_t equals predict_noised's."""
    T = 8
    rings = [3, 20, 6, 12]
    F = synth.num_node_features("hetro")
    eargs, pargs = synth.edm_args(dataset="hetro", diffusion_steps=T), synth.pred_args(dataset="hetro")
    esd, psd = synth.synth_edm_state_dict(eargs, F, seed=21), synth.synth_predictor_state_dict(pargs, F, 5, seed=22)
    nm3, em_flat, N = build_masks(rings, 20, True)
    B = len(rings)
    nm, em = nm3.reshape(B, N), em_flat.reshape(B, N, N)
    eng = engine(eargs, esd, pargs, psd, GAUDI_FAMILY_SPLIT=1)
    x0, oh0 = _seeds(nm, 3 + F, 2)
    grid = np.array([6, 4, 1, 0], np.int32)
    w = np.array([3, 0, 1, 1, 0], np.float32)
    for kw in (dict(target_w=w, scale=0.6), {}):
        x, h, d, z0, zt = eng.sample(nm, em, seed=5, grid=grid, start=(x0, oh0), return_z0=True, return_zt=True, **kw)
        assert 0 < d["family_split_resident"] < B and np.isfinite(x).all()
        for b in range(B):
            xb, hb, _, z0b, ztb = eng.sample(nm[b:b + 1], em[b:b + 1], seed=5, sample_offset=b, grid=grid, start=(x0[b:b + 1], oh0[b:b + 1]),
                                             return_z0=True, return_zt=True, **kw)
            assert np.array_equal(xb[0], x[b]) and np.array_equal(hb[0], h[b]) and np.array_equal(z0b[0], z0[b]), b
            assert np.array_equal(ztb[0], zt[b]), b
        assert np.array_equal(zt, eng.predict_noised(x0, oh0, 6, nm, em, seed=5)[0])
    eng.close()


# ---------------------------------------------------------------------------------------------- callback chains
@pytest.mark.parametrize("env", [{}, dict(GAUDI_WAVES=4), dict(GAUDI_FORCE_GN=1)])
def test_callback_chains_on_a_coarse_grid_vs_oracle(O, env):
    """A non-affine target (gaudi_sample_cb) and one that depends on z directly (gaudi_sample_cbz) on a coarse grid against
    the numpy composition of oracle.edm_phi / predictor_grad / step_coefficients at rel_err < 1e-4: the whole coarse chain,
    and teacher-forced single steps (T, 0) from the prior and (t, 0) from given molecules; the callback sees t = g[k] / T; an
    affine callback equals the fused chain bit for bit."""
    T = 20
    eargs, esd, pargs, psd, nm, em, N, D = _case("hetro", [3, 5, 4], T, amp=False)
    B = nm.shape[0]
    eng = engine(eargs, esd, pargs, psd, **env)
    gamma = O.gamma_table("polynomial_2", T, 1e-5)
    noise = np.random.default_rng(12).standard_normal((T + 2, B, N, D)).astype(np.float32)
    grid = np.array([20, 17, 10, 9, 2, 0], np.int32)
    zT = O._combined_noise(noise[0], nm[:, :, None], 1.0).astype(np.float32)
    tz = direct_z_target_grad(nm)
    for with_z in (False, True):
        seen, states = [], []

        def cb(*a):
            seen.append(a[-1])
            if with_z:
                states.append(a[0].copy())
                return tz(*a)
            return nonlinear_target_grad(*a)

        x, h, diag, z0 = eng.sample_callback(nm, em, cb, noise=noise, scale=0.6, grid=grid, with_z=with_z, return_z0=True)
        assert seen == [float(np.float32(t) / np.float32(T)) for t in grid[:-1]]
        # the whole coarse chain against the oracle's chain over the same pairs (non-amplified heads: well conditioned)
        z = zT
        for t_i, s_i in zip(grid[:-1], grid[1:]):
            z = oracle_step_pair(O, esd, eargs, gamma, int(s_i), int(t_i), z, nm, em, noise[T - s_i], psd, pargs, scale=0.6,
                                 **(dict(target_z=tz) if with_z else dict(target_w=nonlinear_target_grad)))
        print(f"callback chain (with_z={with_z}) z_0 vs oracle: {rel_err(z0, z):.2e}")
        assert rel_err(z0, z) < 1e-4
        xo, ho = O.decode_z0(esd, eargs, gamma, z0, nm[:, :, None], em, noise[T + 1])
        assert rel_err(x, xo) < 1e-4 and np.array_equal(h, ho)
    # teacher-forced steps: a one-step chain IS one step.  From the prior at T down to 0 ...
    for with_z in (False, True):
        fn = tz if with_z else nonlinear_target_grad
        x, h, diag, z0 = eng.sample_callback(nm, em, fn, noise=noise, scale=0.6, grid=[T, 0], with_z=with_z, return_z0=True)
        want = oracle_step_pair(O, esd, eargs, gamma, 0, T, zT, nm, em, noise[T], psd, pargs, scale=0.6,
                                **(dict(target_z=tz) if with_z else dict(target_w=nonlinear_target_grad)))
        assert rel_err(z0, want) < 1e-4
    # ... and from given molecules at several t, each from the device's own z_t
    x0, oh0 = _seeds(nm, D, 3)
    for t_i in (15, 6, 1):
        for with_z in (False, True):
            fn = tz if with_z else nonlinear_target_grad
            out = eng.sample_callback(nm, em, fn, noise=noise, scale=0.6, grid=[t_i, 0], start=(x0, oh0), with_z=with_z,
                                      return_z0=True, return_zt=True)
            zt = out[4]
            assert np.array_equal(zt, eng.predict_noised(x0, oh0, t_i, nm, em, noise=noise[0])[0])
            want = oracle_step_pair(O, esd, eargs, gamma, 0, t_i, zt, nm, em, noise[T], psd, pargs, scale=0.6,
                                    **(dict(target_z=tz) if with_z else dict(target_w=nonlinear_target_grad)))
            assert rel_err(out[3], want) < 1e-4, (t_i, with_z)
    # an affine callback = the fused chain, bit for bit, on the coarse grid too
    a = eng.sample_callback(nm, em, lambda p, t: np.broadcast_to(W, p.shape), noise=noise, scale=0.6, grid=grid, return_z0=True)
    b = eng.sample(nm, em, noise=noise, target_w=W, scale=0.6, grid=grid, return_z0=True)
    _same(a, b)
    eng.close()


# ---------------------------------------------------------------------------------------------- refusals that need a handle
def test_grid_refusals_through_the_abi():
    T = 20
    eargs, esd, pargs, psd, nm, em, N, D = _case("cata", [4, 6], T)
    eng = engine(eargs, esd, pargs, psd)
    x0, oh0 = _seeds(nm, D, 1)
    for grid, msg in (([20], "at least two"), ([20, 10, 10, 0], "strictly descending"), ([20, 10, 12, 0], "strictly descending"),
                      ([20, 10], "end in 0"), ([21, 0], "exceeds T"), ([10, 5, 0], "from the prior must start at time index T")):
        with pytest.raises(GaudiError, match=msg):
            eng.sample(nm, em, grid=grid)
        with pytest.raises(GaudiError, match=msg):
            eng.sample_callback(nm, em, lambda p, t: p, grid=grid)
    for start in ((x0, None), (None, oh0)):
        with pytest.raises(GaudiError, match="both x0 and onehot0"):
            eng.sample(nm, em, grid=[10, 5, 0], start=start)
    with pytest.raises(GaudiError, match="needs the time grid"):
        eng.sample(nm, em, start=(x0, oh0))
    with pytest.raises(GaudiError, match="return_zt"):
        eng.sample(nm, em, grid=[20, 0], return_zt=True)
    eng.set_fix_noise(True, 0)
    with pytest.raises(GaudiError, match="fix_noise"):
        eng.sample(nm, em, grid=[10, 5, 0], start=(x0, oh0))
    eng.set_fix_noise(False, 0)
    x, h, diag = eng.sample(nm, em, grid=[10, 5, 0], start=(x0, oh0))  # the handle is still usable
    assert np.isfinite(x).all()
    eng.close()


# ---------------------------------------------------------------------------------------------- the reference-shaped layers
def test_model_and_driver_layers_end_to_end():
    """GaudiModel.sample / sample_guidance(grid=), GaudiModel.refine, sampling_edm.sample_pos_edm / sample_guidance(n_steps=),
    generation_guidance.design(n_steps=) and generation_guidance.refine on synthetic weights: shapes, keys, masks, zero mean;
    a closure with a guidance window the grid skips runs fused, one the grid visits runs through the callback."""
    import torch
    from gaudi_amd import generation_guidance, sampling_edm
    from gaudi_amd.models_edm import get_cond_predictor_model, get_model
    T = 40
    eargs = synth.edm_args(dataset="cata", diffusion_steps=T, **TINY)
    pargs = synth.pred_args(dataset="cata", **TINY_P)
    model, _, _ = get_model(eargs, state_dict=synth.synth_edm_state_dict(eargs, 1, seed=3))
    cp = get_cond_predictor_model(pargs, model=model, state_dict=synth.synth_predictor_state_dict(pargs, 1, 5, seed=4))
    model.seed = 5
    args = types.SimpleNamespace(device="cuda", dataset="cata", max_nodes=9, batch_size=6)

    def tf_gap(z, nm, em, t):
        return -cp(z, nm, em, t)[:, 1]

    x, h, nm, em = sampling_edm.sample_pos_edm(args, model, [5, 9, 7], n_steps=8)
    assert x.shape == (3, 9, 3) and h.shape == (3, 9, 1)
    x, h, nm, em = sampling_edm.sample_guidance(args, model, tf_gap, [5, 9, 7], scale=0.6, n_steps=8)
    assert x.shape == (3, 9, 3) and h.shape == (3, 9, 1) and nm.shape == (3, 9, 1)
    sampling_edm._check(x, nm)
    assert "affine_recheck_failed" not in model.last_diag
    # n_steps = T is today's chain bit for bit (same seed and stream position)
    model.sample_offset = 0
    a = sampling_edm.sample_guidance(args, model, tf_gap, [5, 9, 7], scale=0.6)[0]
    model.sample_offset = 0
    b = sampling_edm.sample_guidance(args, model, tf_gap, [5, 9, 7], scale=0.6, n_steps=T)[0]
    assert torch.equal(a, b)

    def windowed(lo, hi):
        def tf(z, nm, em, t):
            tt = float(torch.as_tensor(t).reshape(-1)[0])
            return -cp(z, nm, em, t)[:, 1] * (0.0 if lo < tt < hi else 1.0)
        return tf

    grid = time_grid(T, 8)  # t = 1, 0.875, ..., 0.125
    nm_np, em_np, _ = build_masks([5, 9, 7], 9, False)
    model.sample_guidance(3, windowed(0.51, 0.61), nm_np, em_np, 0.6, grid=grid)  # the grid skips the window: fused
    assert "affine_recheck_failed" not in model.last_diag
    model.sample_guidance(3, windowed(0.70, 0.80), nm_np, em_np, 0.6, grid=grid)  # the grid visits t = 0.75: the general path
    assert model.last_diag.get("affine_recheck_failed") == 1

    # refinement of given molecules (not yet centred: refine removes the masked mean)
    x0, oh0 = _seeds(nm_np.reshape(3, 9), 4, 9)
    x0 = x0 + 0.3 * nm_np
    xr, hr = model.refine(x0, oh0, nm_np, em_np, t_start=12, target_function=tf_gap, scale=0.6, n_steps=4)
    assert xr.shape == (3, 9, 3) and hr["categorical"].shape == (3, 9, 1)
    sampling_edm._check(xr, nm_np)
    xr2, _ = model.refine(x0, {"categorical": oh0, "integer": None}, nm_np, em_np, t_start=12)  # unguided, all 12 steps
    sampling_edm._check(xr2, nm_np)
    with pytest.raises(GaudiError):
        model.refine(x0 + (1 - nm_np), oh0, nm_np, em_np, t_start=12, n_steps=13)

    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5)
    assert out["x"].shape == (6, 7, 3) and {"stability", "target_function_values", "pred", "best", "best_stable"} <= set(out)
    seeds = out
    ref = generation_guidance.refine(args, model, cp, tf_gap, seeds["x"], seeds["one_hot"], seeds["node_mask"], seeds["edge_mask"],
                                     t_start=10, scale=0.6, n_steps=5)
    assert set(out) | {"seed_target_function_values"} == set(ref)
    assert ref["x"].shape == (6, 7, 3) and ref["seed_target_function_values"].shape == (6,)
    assert rel_err(ref["seed_target_function_values"].numpy(), seeds["target_function_values"].numpy()) < 1e-5
    sampling_edm._check(ref["x"], ref["node_mask"])
    model.engine.close()
