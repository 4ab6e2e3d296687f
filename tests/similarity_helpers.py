"""Shared by test_similarity_cpu.py and test_gpu_similarity.py: the circular count fingerprint restated in Python straight from
its definition, the host twins of the two kernels, numpy's evaluation of the similarity order, and the
fixtures' fingerprints computed once."""
import numpy as np

from gaudi_amd import _lib
from tests.bond_order_helpers import C, H, fixture, pack
from tests.canonical_helpers import N_ELEMS, host_canon

OK, GAVE_UP, BAD_INPUT, OVERFLOW, EMPTY = range(5)
M32 = 0xFFFFFFFF
_CACHE = {}


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def restated_counts(elem, bonds, radius, n_bins):
    """The definition, on Python integers: -> the number of features per bin, before saturation (int64 [n_bins])."""
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    heavy = [a for a in range(len(elem)) if elem[a] != H]
    nbrs = {a: [] for a in heavy}
    n_h = {a: 0 for a in heavy}
    n_bonds = {a: 0 for a in heavy}
    for i, j in bonds:
        i, j = int(i), int(j)
        for a, o in ((i, j), (j, i)):
            if elem[a] == H:
                continue
            n_bonds[a] += 1
            if elem[o] == H:
                n_h[a] += 1
            else:
                nbrs[a].append(o)
    ids = {}
    for a in heavy:
        implied = 1 if elem[a] == C and n_bonds[a] == 2 else 0
        label = int(elem[a]) * 8 + n_h[a] + implied
        ids[a] = mix(0x9E3779B9 + label * 16 + len(nbrs[a]))
    features = list(ids.values())
    for r in range(1, radius + 1):
        new = {}
        for a in heavy:
            h = mix(r)
            h = mix(h ^ ids[a])
            for x in sorted(ids[o] for o in nbrs[a]):
                h = mix(h ^ x)
            new[a] = h
        ids = new
        features += list(ids.values())
    return np.bincount(np.array(features, np.int64) & (n_bins - 1), minlength=n_bins)


def restated_fingerprint(elem, bonds, radius, n_bins):
    """-> (row uint8 [n_bins], total): the counts saturated at 255, and the sum of the stored bytes."""
    row = np.minimum(restated_counts(elem, bonds, radius, n_bins), 255).astype(np.uint8)
    return row, int(row.sum())


def host_fp(mols, radius=2, n_bins=1024):
    """Fixture molecules or (elem, bonds) pairs -> the raw outputs of the host twin, in the fixture's element list."""
    return _lib.host_circular_fingerprint(N_ELEMS, H, C, *pack(mols), radius, n_bins)


def device_fp(engine, mols, radius=2, n_bins=1024):
    return engine.circular_fingerprint(N_ELEMS, H, C, *pack(mols), radius, n_bins)


class HostEngine:
    """What gaudi_amd.similarity asks of an engine for fingerprints, on the kernel's host build."""

    def circular_fingerprint(self, n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, radius, n_bins):
        return _lib.host_circular_fingerprint(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, radius, n_bins)


def g32_fingerprints(radius=2, n_bins=1024):
    """The host twin's outputs for the whole of g32, computed once per setting and never written to."""
    key = ("g32", radius, n_bins)
    if key not in _CACHE:
        out = host_fp(fixture()[1], radius, n_bins)
        for a in out.values():
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def g32_keys():
    """canon_key-like identities of g32 from the canonical kernel's host twin: bytes per molecule, None without a numbering."""
    if "keys" not in _CACHE:
        from gaudi_amd.gor2goa import canon_code
        raw = host_canon(fixture()[1])
        _CACHE["keys"] = [canon_code(raw, i) if raw["status"][i] == OK else None for i in range(len(raw["status"]))]
    return _CACHE["keys"]


def numpy_common(q, lib):
    """[B,M] int64: sum of the byte-wise minimum."""
    q, lib = np.asarray(q, np.int64), np.asarray(lib, np.int64)
    return np.stack([np.minimum(row[None, :], lib).sum(-1) for row in q]) if len(q) else np.zeros((0, len(lib)), np.int64)


def numpy_nearest(q, lib, k):
    """The total order evaluated without the C text: exact rational comparison through integer cross-multiplication in Python
    integers, a union of 0 as similarity 0, ties to the smaller index -> (idx, common, union) int32 [B,k], padded -1, 0, 0."""
    from fractions import Fraction
    q, lib = np.asarray(q), np.asarray(lib)
    common = numpy_common(q, lib)
    union = q.astype(np.int64).sum(-1)[:, None] + lib.astype(np.int64).sum(-1)[None, :] - common
    B, M = common.shape
    idx, co, un = np.full((B, k), -1, np.int32), np.zeros((B, k), np.int32), np.zeros((B, k), np.int32)
    for b in range(B):
        sims = [Fraction(int(common[b, m]), int(union[b, m])) if union[b, m] else Fraction(0) for m in range(M)]
        order = sorted(range(M), key=lambda m: (-sims[m], m))[:k]
        idx[b, :len(order)], co[b, :len(order)], un[b, :len(order)] = order, common[b, order], union[b, order]
    return idx, co, un


def numpy_diversity(fp, total):
    """1 - the mean off-diagonal similarity over rows with total > 0; 0.0 with fewer than two such rows."""
    fp = np.asarray(fp)[np.asarray(total) > 0]
    n = len(fp)
    if n < 2:
        return 0.0
    common = numpy_common(fp, fp)
    t = fp.astype(np.int64).sum(-1)
    union = t[:, None] + t[None, :] - common
    sim = common / np.maximum(union, 1)
    return float(1.0 - (sim.sum() - np.trace(sim)) / (n * (n - 1)))


def stars(centre=3, leaf=2, n_leaves=4, copies=38):
    """`copies` disjoint stars: a centre atom bonded to n_leaves leaf atoms.  All leaves are alike, so each radius contributes
    copies * n_leaves equal features; with the defaults (38 N centres with 4 B leaves each, 190 atoms) two of the leaves' four
    ids of radius 0..3 fall into one of 256 bins: 304 features in it -> (elem, bonds)."""
    e, b = [], []
    for _ in range(copies):
        c = len(e)
        e.append(centre)
        for _ in range(n_leaves):
            e.append(leaf)
            b.append((c, len(e) - 1))
    return np.array(e, np.int32), np.array(b, np.int32).reshape(-1, 2)
