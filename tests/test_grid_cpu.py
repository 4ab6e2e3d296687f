"""Chains on a time grid, the parts that need no device: the per-call step table (gaudi_host_grid_coefficients, the function
the chains call), time_grid, the refusals of malformed grids, the affine check on the grid's own t values, and the sharded
call's handling of grid / start."""
import numpy as np
import pytest

from gaudi_amd._lib import GaudiError

SCHEDULES = {"polynomial_2": (2.0, 1e-5), "cosine": (0.0, 2e-5)}  # name -> (noise_power, rtol of test_host_schedule_matches_reference)


def _L():
    from gaudi_amd import _lib, build
    build.build()
    _lib.load_library()
    return _lib


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_grid_coefficients_match_reference_and_oracle(golden, sched):
    """Every pair of g28 against the reference's own scalars and against oracle.step_coefficients, at the bar the unit-stride
    table is held to."""
    from oracle import gaudi_oracle as O
    L = _L()
    power, rtol = SCHEDULES[sched]
    g = golden("g28_grid_steps")
    T = 1000
    gamma = O.gamma_table(sched, T, 1e-5)
    assert len(g[f"coef_{sched}"]) == len(g["pairs"]) >= 10
    for row in g[f"coef_{sched}"]:
        t_i, s_i = int(row[0]), int(row[1])
        coef, land = L.grid_coefficients(T, power, 1e-5, [t_i, s_i] + ([0] if s_i else []))
        assert land[0] == s_i and land[-1] == 0
        np.testing.assert_allclose(coef[0], row[2:6], rtol=rtol, err_msg=str((t_i, s_i)))
        c = O.step_coefficients(gamma, s_i, t_i)
        np.testing.assert_allclose(coef[0, :3], [c["alpha_ts"], c["eps_coef"], c["sigma"]], rtol=rtol, err_msg=str((t_i, s_i)))
        assert coef[0, 3] == np.float32(t_i) / np.float32(T)


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("T", [50, 1000])
def test_unit_grid_is_the_unit_stride_table_bit_for_bit(sched, T):
    L = _L()
    lib = L.load_library()
    power = SCHEDULES[sched][0]
    table, gamma = np.empty((T, 4), np.float32), np.empty(T + 1, np.float32)
    assert lib.gaudi_host_schedule(T, power, 1e-5, L.fptr(gamma), L.fptr(table)) == 0
    coef, land = L.grid_coefficients(T, power, 1e-5, np.arange(T, -1, -1))
    assert np.array_equal(land, np.arange(T - 1, -1, -1))
    assert np.array_equal(coef[::-1].view(np.uint32), table.view(np.uint32))  # step k lands on T-1-k: row T-1-k of the table
    # ... and a coarse grid's rows are functions of their own pair only
    grid = [T, T // 2, 3, 0]
    coarse, _ = L.grid_coefficients(T, power, 1e-5, grid)
    for k in range(3):
        alone, _ = L.grid_coefficients(T, power, 1e-5, [grid[k], grid[k + 1]] + ([0] if grid[k + 1] else []))
        assert np.array_equal(coarse[k].view(np.uint32), alone[0].view(np.uint32))


def test_time_grid():
    from gaudi_amd.sampling_edm import time_grid
    for T in (50, 1000):
        assert np.array_equal(time_grid(T, T), np.arange(T, -1, -1))
        for n in (1, 2, 7, 10, T // 4, T - 1):
            g = time_grid(T, n)
            assert g.dtype == np.int32 and len(g) == n + 1 and g[0] == T and g[-1] == 0
            assert (np.diff(g) < 0).all()
            assert np.abs(g - T * (n - np.arange(n + 1)) / n).max() <= 0.5
    assert list(time_grid(50, 10)) == list(range(50, -1, -5))
    assert list(time_grid(50, 7)) == [50, 43, 36, 29, 21, 14, 7, 0]
    assert list(time_grid(50, 5, 20)) == [20, 16, 12, 8, 4, 0]
    assert list(time_grid(1000, 20, 20)) == list(range(20, -1, -1))
    for bad in (dict(T=50, n_steps=51), dict(T=50, n_steps=0), dict(T=50, n_steps=21, t_start=20), dict(T=50, n_steps=5, t_start=51),
                dict(T=50, n_steps=5, t_start=0)):
        with pytest.raises(GaudiError):
            time_grid(**bad)


@pytest.mark.parametrize("grid", [[5], [], [5, 5, 0], [5, 6, 0], [5, 3], [51, 0], [50, 0, 0], [50, 10, -1, 0]])
def test_malformed_grids_are_refused(grid):
    """GAUDI_E_INVALID through the ABI, from the check the device entry points share (no device needed)."""
    L = _L()
    lib = L.load_library()
    g = np.asarray(grid, np.int32)
    coef = np.zeros((8, 4), np.float32)
    rc = lib.gaudi_host_grid_coefficients(50, 2.0, 1e-5, len(g), g.ctypes.data_as(L.IP), L.fptr(coef), None)
    assert rc == -1
    with pytest.raises(GaudiError):
        L.grid_coefficients(50, 2.0, 1e-5, grid)
    assert lib.gaudi_host_grid_coefficients(50, 2.0, 1e-5, 2, None, L.fptr(coef), None) == -1
    ok = np.asarray([50, 0], np.int32)
    assert lib.gaudi_host_grid_coefficients(50, 2.0, 1e-5, 2, ok.ctypes.data_as(L.IP), None, None) == -1
    assert lib.gaudi_host_grid_coefficients(50, 2.0, 1e-5, 2, ok.ctypes.data_as(L.IP), L.fptr(coef), None) == 0


def test_grid_entry_points_refuse_a_null_handle():
    L = _L()
    lib = L.load_library()
    g = np.asarray([50, 0], np.int32)
    assert lib.gaudi_sample_grid(None, 1, 1, None, None, 0, 0, None, 1.0, None, 1.0, 2, g.ctypes.data_as(L.IP), None, None, None,
                                 None, None, None, None) == -1
    assert lib.gaudi_step_pair(None, 1, 1, 0, 5, None, None, None, None, None, 1.0, None) == -1
    assert lib.gaudi_sample_cb_grid(None, 1, 1, None, None, 0, 0, None, 1.0, L.TARGET_CB(), L.TARGET_CBZ(), None, 1.0, 2,
                                    g.ctypes.data_as(L.IP), None, None, None, None, None, None, None) == -1


def test_affine_check_visits_the_grids_t_values():
    """A closure switched off on a window of t: affine on a grid that skips the window, not affine on one that visits it.
    The existing signature (fn, w, T) keeps visiting 1/T .. 1."""
    import torch
    from gaudi_amd.models_edm import affine_gradient_holds
    from gaudi_amd.sampling_edm import time_grid
    T = 50
    w = np.array([0.0, -1.0, 0.0, 0.0, 0.0], np.float32)

    def window(lo, hi):
        def fn(pred, t):
            return -pred[:, 1] if not lo < t < hi else 0.0 * pred[:, 1]
        return fn

    grid = time_grid(T, 10)  # visits t = 1.0, 0.9, ..., 0.1
    assert affine_gradient_holds(window(0.41, 0.49), w, T, grid)       # between 0.5 and 0.4: skipped by the grid ...
    assert not affine_gradient_holds(window(0.41, 0.49), w, T)         # ... visited by the unit grid (0.42 .. 0.48)
    assert not affine_gradient_holds(window(0.41, 0.49), w, T, time_grid(T, T))
    assert not affine_gradient_holds(window(0.35, 0.45), w, T, grid)   # holds 0.4: visited
    # the landing index 0 is no step's t: a window around t = 0 only is never visited
    assert affine_gradient_holds(window(-1.0, 0.01), w, T, grid)
    assert affine_gradient_holds(window(-1.0, 0.01), w, T)
    # a refinement grid visits t_start / T and below only
    assert affine_gradient_holds(window(0.45, 2.0), w, T, time_grid(T, 5, 20))
    assert not affine_gradient_holds(window(0.3, 2.0), w, T, time_grid(T, 5, 20))
    assert torch.is_tensor(window(0, 0)(torch.zeros(2, 5), 0.5))


def test_sample_sharded_slices_start_by_global_index():
    from gaudi_amd import dist
    B, N, F = 7, 4, 2
    nm = np.ones((B, N), np.float32)
    em = np.ones((B, N, N), np.float32)
    x0 = np.arange(B * N * 3, dtype=np.float32).reshape(B, N, 3)
    oh = np.arange(B * N * F, dtype=np.float32).reshape(B, N, F)
    seen = []

    def fn(nm_s, em_s, off, **kw):
        seen.append((off, kw))
        return kw["start"][0] if "start" in kw else nm_s[:, :, None].repeat(3, 2), nm_s

    parts = [dist.sample_sharded(fn, nm, em, r, 3, grid=[50, 25, 0], start=(x0, oh)) for r in range(3)]
    assert [p[:2] for p in parts] == [(0, 3), (3, 5), (5, 7)]
    for (lo, hi, x, _), (off, kw) in zip(parts, seen):
        assert off == lo and kw["grid"] == [50, 25, 0]
        assert np.array_equal(kw["start"][0], x0[lo:hi]) and np.array_equal(kw["start"][1], oh[lo:hi])
    assert np.array_equal(np.concatenate([p[2] for p in parts]), x0)
    seen.clear()
    dist.sample_sharded(fn, nm, em, 0, 2)  # neither given: the callable is called as before
    assert seen[0][1] == {}
