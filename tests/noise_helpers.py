"""Helpers of the noise-stream tests (test_philox_cpu.py, test_gpu_noise.py): a float64 reference of the device stream
(csrc/device_common.h: philox_normal4), the published Philox4x32-10 known-answer vectors, and the keys both files run.

The reference takes only the INTEGER stage from gaudi_amd.philox (held to KAT by test_philox_cpu.py) and does the uniform
mapping and Box-Muller in float64, so neither numpy's fp32 libm nor the device's enters it."""
import numpy as np

from gaudi_amd.philox import philox4x32_10

MASK64 = (1 << 64) - 1

# Random123's kat_vectors for philox4x32-10: (counter, key, output)
KAT = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)

S62 = 0x2545F4914F6CDD1D  # a 62-bit seed with both words set, as GaudiModel.next_stream draws them (torch.randint(0, 2**62))
S_HI = 1 << 32            # only the high key word
S_LO = 0x9E3779B9         # only the low key word
CARRY = 2 ** 32 - 2       # sample_offset + b crosses 2^32 at b = 2

# (seed, sample_offset, B, n_elem, draw0, n_draws)
KEY_CARRY = (S62, CARRY, 6, 210, 998, 4)      # the carry inside the batch; 210 = 30 * 7 is 2 mod 4; draws up to T + 1 = 1001
KEY_PAST = (S62, 2 ** 32, 4, 210, 998, 4)     # rows 2.. of KEY_CARRY
KEY_212 = (S62, CARRY, 6, 212, 998, 4)        # whole quads: its first 210 columns are KEY_CARRY
KEY_LARGE = (S62, CARRY, 7, 3300, 0, 3)       # 69300 values: the stand-alone kernel's 65536 threads make a second, partial trip
KEYS = (
    (S_HI, 0, 2, 5, 0, 2),
    (S_LO, 3, 3, 3, 0, 2),
    KEY_CARRY,
    KEY_PAST,
    KEY_212,
    (S62, 2 ** 40 + 7, 2, 2, 1000, 2),
    (S62, -2, 4, 5, 0, 3),                    # samples 2^64 - 2, 2^64 - 1, 0, 1: the wrap through zero, as both sides do it today
    (S62, 7, 1, 1, 0, 3),
    (S_HI | 1, 2 ** 32 - 1, 1, 2, 1000, 2),
    KEY_LARGE,
)

# Counters of seed S62 whose word 0 has its top 24 bits all set (u1 = 1, radius 0) / all clear (u1 = 2^-24, radius
# sqrt(48 ln 2) = 5.7681, the largest there is): (seed, sample, draw, quad), the four words.  Found once by a numpy search of
# the 2^26 counters sample = 2^33 + 0..1023, draw 0..1023, quad 0..63 (the first hit of each in that order).
EXTREMES = {
    "radius_0": ((S62, 2 ** 33 + 33, 303, 22), (0xFFFFFF4C, 0xA8ED9EF8, 0x694E9501, 0x3F00AC13)),
    "radius_max": ((S62, 2 ** 33 + 69, 973, 51), (0x00000094, 0xAC6B20F4, 0xF17D3104, 0xF1DFB295)),
}
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))


def words(seed, sample_offset, B, n_elem, draw0, n_draws):
    """-> the four uint32 words [n_draws, B, ceil(n_elem / 4)] of counter (quad, draw, sample lo, sample hi), key (seed lo, hi)."""
    nq = (n_elem + 3) // 4
    samples = [(int(sample_offset) + b) & MASK64 for b in range(B)]
    lo = np.array([s & 0xFFFFFFFF for s in samples], np.uint32)
    hi = np.array([s >> 32 for s in samples], np.uint32)
    dr = (np.arange(n_draws, dtype=np.int64) + draw0).astype(np.uint32)
    q = np.arange(nq, dtype=np.uint32)
    shape = (n_draws, B, nq)
    c0 = np.broadcast_to(q[None, None, :], shape)
    c1 = np.broadcast_to(dr[:, None, None], shape)
    c2 = np.broadcast_to(lo[None, :, None], shape)
    c3 = np.broadcast_to(hi[None, :, None], shape)
    seed = int(seed) & MASK64
    return philox4x32_10(c0, c1, c2, c3, np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))


def normal_f64(seed, sample_offset, B, n_elem, draw0, n_draws):
    """-> (z [n_draws, B, n_elem] float64, r same shape: the radius that multiplied each value)."""
    w = [np.asarray(x, np.uint32) for x in words(seed, sample_offset, B, n_elem, draw0, n_draws)]
    two24 = 16777216.0
    u1 = ((w[0] >> np.uint32(8)).astype(np.float64) + 1.0) / two24
    u2 = (w[1] >> np.uint32(8)).astype(np.float64) / two24
    u3 = ((w[2] >> np.uint32(8)).astype(np.float64) + 1.0) / two24
    u4 = (w[3] >> np.uint32(8)).astype(np.float64) / two24
    ra = np.sqrt(-2.0 * np.log(u1))
    rb = np.sqrt(-2.0 * np.log(u3))
    a, b = 2.0 * np.pi * u2, 2.0 * np.pi * u4
    z = np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], axis=-1)
    r = np.stack([ra, ra, rb, rb], axis=-1)
    shape = (n_draws, B, z.shape[2] * 4)
    return z.reshape(shape)[:, :, :n_elem], r.reshape(shape)[:, :, :n_elem]


def extreme_key(name):
    """-> (key tuple for philox_normal / normal_f64, first column of the pinned quad): one sample, one draw, the elements up
    to one quad past the pinned one."""
    (seed, sample, draw, quad), _ = EXTREMES[name]
    return (seed, sample, 1, 4 * quad + 8, draw, 1), 4 * quad


def all_keys():
    return list(KEYS) + [extreme_key(n)[0] for n in EXTREMES]


def scaled_error(got, z, r):
    """-> (max |got - z| / max(1, r), max |got - z|)."""
    d = np.abs(np.asarray(got, np.float64) - z)
    return float((d / np.maximum(1.0, r)).max()), float(d.max())


# max over all_keys() of the numpy twin's scaled / plain error against normal_f64, measured by test_philox_cpu.py (numpy's fp32
# libm, deterministic); the bar of both files is twice the scaled figure
TWIN_SCALED, TWIN_PLAIN = 4.12e-7, 1.56e-6
BAR = 2.0 * TWIN_SCALED
