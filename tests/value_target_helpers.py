"""Shared by the value-target tests: the seed of the fused target family as a numpy float32 expression."""
import numpy as np


def numpy_seed(w, q, c, side, scale, p):
    """The seed in numpy float32, in the order the issue fixes: (w + (q + q) * a(p - c, side)) * scale."""
    f = np.float32
    w, q, c, p = (np.asarray(v, f) for v in (w, q, c, p))
    side = np.broadcast_to(np.asarray(side), p.shape)
    scale = np.asarray(scale, f).reshape(-1, 1) if np.ndim(scale) else f(scale)
    d = (p - c).astype(f)
    a = np.where(side == 0, d, np.where(side > 0, np.where(d > 0, d, f(0)), np.where(d < 0, d, f(0)))).astype(f)
    return (((w + ((q + q).astype(f) * a).astype(f)).astype(f)) * scale).astype(f)
