"""The numpy twin of the device noise stream (gaudi_amd/philox.py) without a device: its integer stage against the published
Philox4x32-10 vectors, its fp32 normals against a float64 Box-Muller of the same integers (tests/noise_helpers.py: normal_f64)
at the keys production uses -- 62-bit seeds, sample indices across 2^32, partial last quads, draws up to 1001 -- and at the two
pinned extremes of the radius, its counter layout, and the moments of 2^20 draws.

Measured over all of noise_helpers.all_keys() (83209 values, numpy's fp32 libm): max |twin - z| / max(1, r) = 4.12e-7,
max |twin - z| = 1.55e-6.  The bar on the scaled figure is twice that, 8.24e-7 (noise_helpers.BAR);
tests/test_gpu_noise.py holds the device to the same bar."""
import numpy as np
import pytest

from gaudi_amd.philox import philox4x32_10, philox_normal
from tests import noise_helpers as H


def test_integer_stage_returns_the_published_vectors():
    for ctr, key, out in H.KAT:
        got = philox4x32_10(*ctr, *key)
        assert tuple(int(w) for w in got) == out, [hex(int(w)) for w in got]
    # ... and vectorised, as philox_normal calls it
    c = [np.array([k[0][i] for k in H.KAT], np.uint32) for i in range(4)]
    k = [np.array([k[1][i] for k in H.KAT], np.uint32) for i in range(2)]
    got = philox4x32_10(*c, *k)
    for i in range(4):
        assert [int(w) for w in got[i]] == [k[2][i] for k in H.KAT]


def test_pinned_extremes_are_what_they_claim():
    for name, top in (("radius_0", 0xFFFFFF), ("radius_max", 0)):
        (seed, sample, draw, quad), want = H.EXTREMES[name]
        got = philox4x32_10(quad, draw, sample & 0xFFFFFFFF, sample >> 32, seed & 0xFFFFFFFF, seed >> 32)
        assert tuple(int(w) for w in got) == want
        assert want[0] >> 8 == top
        key, col = H.extreme_key(name)
        z, r = H.normal_f64(*key)
        assert r[0, 0, col] == r[0, 0, col + 1] == (0.0 if name == "radius_0" else H.R_MAX)
    key, col = H.extreme_key("radius_0")
    twin = philox_normal(*key)[0, 0]
    assert np.all(twin[col:col + 2] == 0) and np.isfinite(twin).all()


def test_twin_normals_against_float64_reference():
    worst_s = worst_p = 0.0
    n = 0
    for key in H.all_keys():
        twin = philox_normal(*key)
        z, r = H.normal_f64(*key)
        assert twin.dtype == np.float32 and twin.shape == z.shape == (key[5], key[2], key[3])
        assert np.isfinite(twin).all()
        s, p = H.scaled_error(twin, z, r)
        print(f"{key}: scaled {s:.3e} plain {p:.3e}")
        worst_s, worst_p, n = max(worst_s, s), max(worst_p, p), n + twin.size
    print(f"twin vs float64 over {n} values: scaled {worst_s:.4e}, plain {worst_p:.4e} (bar {H.BAR:.2e})")
    assert worst_s < H.BAR


def test_counter_layout_of_the_twin():
    """The stream does not depend on batch sharding: a value is keyed by (seed, global sample, draw, element) alone."""
    carry, past, wide = philox_normal(*H.KEY_CARRY), philox_normal(*H.KEY_PAST), philox_normal(*H.KEY_212)
    assert np.array_equal(carry[:, 2:], past)                 # rows 2.. of the batch at 2^32 - 2 = the batch at 2^32
    assert np.array_equal(carry, wide[:, :, :210])            # a partial last quad is the head of the whole one
    assert not np.array_equal(carry[:, 0], carry[:, 1])
    seed, off, B, n, d0, nd = H.KEY_CARRY
    for other in (philox_normal(seed ^ (1 << 40), off, B, n, d0, nd),    # only the high key word
                  philox_normal(seed, off + (1 << 40), B, n, d0, nd),    # only the high sample word
                  philox_normal(seed, off, B, n, d0 + nd, nd)):          # other draws
        assert np.all(other != carry)
    # the wrap through zero: samples 2^64 - 2, 2^64 - 1, 0, 1
    seed, off, B, n, d0, nd = next(k for k in H.KEYS if k[1] == -2)
    wrap = philox_normal(seed, off, B, n, d0, nd)
    assert np.array_equal(wrap[:, 2:], philox_normal(seed, 0, 2, n, d0, nd))
    assert H.scaled_error(wrap[:, :2], *H.normal_f64(seed, 2 ** 64 - 2, 2, n, d0, nd))[0] < H.BAR


def _moments(v):
    v = np.asarray(v, np.float64).reshape(-1)
    m = v.mean()
    c = v - m
    var = (c ** 2).mean()
    return m, var, (c ** 3).mean() / var ** 1.5, (c ** 4).mean() / var ** 2 - 3.0


@pytest.mark.parametrize("which", ["twin", "float64"])
def test_moments_of_a_million_draws(which):
    """Mean, variance, skewness and excess kurtosis of 2^20 draws at a 62-bit seed, each within 5 standard errors of its sampling
    distribution under N(0, 1): 1/sqrt(n), sqrt(2/n), sqrt(6/n), sqrt(24/n).  (The discretisation to 24-bit uniforms moves the
    variance by far less than that.)"""
    key = (H.S62, H.CARRY, 8, 4096, 0, 32)
    v = philox_normal(*key) if which == "twin" else H.normal_f64(*key)[0]
    n = v.size
    assert n == 1 << 20
    m, var, skew, kurt = _moments(v)
    print(f"{which}: mean {m:.3e} var-1 {var - 1:.3e} skew {skew:.3e} kurt {kurt:.3e}; one standard error "
          f"{1 / np.sqrt(n):.2e} {np.sqrt(2 / n):.2e} {np.sqrt(6 / n):.2e} {np.sqrt(24 / n):.2e}")
    assert abs(m) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(skew) < 5 * np.sqrt(6 / n)
    assert abs(kurt) < 5 * np.sqrt(24 / n)
