"""How ALIKE two built molecules are: circular count fingerprints of the graph of atoms and their min/max (Tanimoto) similarity,
on the GPU (csrc/fp.inc).  ``canon_key`` (gaudi_amd.gor2goa.canonical) says whether two molecules are the
same; this module says how far apart they are -- the nearest training molecule of a designed one, the diversity of a batch, how
far a refinement moved from its seed.  What RDKit users get from Morgan fingerprints and Tanimoto, without RDKit.

The fingerprint is a COUNT vector (uint8 per bin, saturating at 255), not a bit set: a cata-condensed PAH has a few dozen distinct
atom environments and isomers differ in how often each occurs.  The kernels return integers (common = sum of the byte-wise
minimum, union = total_a + total_b - common); the quotient is formed here, in float64, so device, host build and numpy agree
exactly."""
from __future__ import annotations

import numpy as np

from ._lib import FP_BINS, GaudiError, fp_threshold
from .analyze import _engine


def fingerprints(molecules, dataset="cata", radius=2, n_bins=1024, engine=None) -> dict:
    """Fingerprints for a batch in one launch.  ``molecules``: records of rings_to_atoms or ``(atom_types [n], bonds [m,2])``
    pairs, with or without placed hydrogens (the fingerprint is the same).  radius 0..3; n_bins 256, 512 or 1024.
    -> dict(fp uint8 [B,n_bins], total int32 [B] = the row sums, status int32 [B]: 0, or CANON_BAD_INPUT / OVERFLOW / EMPTY with
    a zero row; a record that was not built gives EMPTY)."""
    from .gor2goa import _pack_atoms, atoms_list
    molecules = list(molecules)
    if n_bins not in FP_BINS or not 0 <= int(radius) <= 3:
        raise GaudiError(f"radius must be 0..3 and n_bins one of {FP_BINS}, got {radius}, {n_bins}")
    if not molecules:
        return dict(fp=np.zeros((0, n_bins), np.uint8), total=np.zeros(0, np.int32), status=np.zeros(0, np.int32))
    atoms = atoms_list(dataset)
    elem, na, bonds, nb = _pack_atoms(molecules)
    return _engine(engine).circular_fingerprint(len(atoms), atoms.index("H"), atoms.index("C"), elem, na, bonds, nb, int(radius), int(n_bins))


def _quotient(common, union) -> np.ndarray:
    """common / union in float64, 0.0 where union = 0."""
    common, union = np.asarray(common, np.float64), np.asarray(union, np.float64)
    return np.divide(common, union, out=np.zeros_like(common), where=union > 0)


def _result(raw):
    return raw["idx"].astype(np.int64), _quotient(raw["common"], raw["union"])


class Library:
    """A fingerprint library kept resident on the device (gaudi_fp_library_set): upload once, query often.  An engine holds ONE
    resident library; a second Library on the same engine replaces the first, whose queries then raise."""

    def __init__(self, fp, engine=None):
        fp = np.ascontiguousarray(fp, dtype=np.uint8)
        if fp.ndim != 2 or fp.shape[0] < 1 or fp.shape[1] not in FP_BINS:
            raise GaudiError(f"a library is [M >= 1, n_bins in {FP_BINS}], got shape {fp.shape}")
        self.engine = _engine(engine)
        self.M, self.n_bins = int(fp.shape[0]), int(fp.shape[1])
        self.engine.fp_library_set(fp)
        self.engine._fp_library = self

    def _live(self):
        if getattr(self.engine, "_fp_library", None) is not self:
            raise GaudiError("this Library is no longer resident (closed, or replaced by another Library on the same engine)")

    def nearest(self, query_fp, k=1):
        """The k library rows most similar to every query row, most similar first, ties to the smaller index ->
        (index int64 [B,k], similarity float64 [B,k]); beyond M rows: -1 and 0.0."""
        self._live()
        return _result(self.engine.fp_nearest(query_fp, None, k, M=self.M))

    def close(self):
        if getattr(self.engine, "_fp_library", None) is self:
            self.engine.fp_library_set(None)
            self.engine._fp_library = None


def nearest(query_fp, library_fp, k=1, engine=None):
    """Library(...).nearest in one call, the library uploaded for this call only."""
    return _result(_engine(engine).fp_nearest(query_fp, library_fp, k))


def similarity_matrix(a, b=None, engine=None) -> np.ndarray:
    """float64 [Ba,Bb]: the similarity of every row of a with every row of b (b = a when None)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.uint8)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), np.float64)
    common = _engine(engine).fp_common(a, b).astype(np.int64)
    union = a.sum(-1, dtype=np.int64)[:, None] + b.sum(-1, dtype=np.int64)[None, :] - common
    return _quotient(common, union)


def internal_diversity(fp, total, engine=None) -> float:
    """1 - the mean off-diagonal similarity over the rows with total > 0; 0.0 with fewer than two such rows."""
    fp = np.asarray(fp)[np.asarray(total) > 0]
    n = len(fp)
    if n < 2:
        return 0.0
    sim = similarity_matrix(fp, engine=engine)
    return float(1.0 - (sim.sum() - np.trace(sim)) / (n * (n - 1)))


def _threshold(threshold):
    from fractions import Fraction
    num, den = fp_threshold(threshold)
    return num, den, Fraction(num, den)


def neighbours(fp, threshold, engine=None) -> dict:
    """For every row the live rows (total > 0) at least ``threshold`` similar to it, itself included, ascending, as CSR:
    dict(count int64 [N], offsets int64 [N+1], list int64 [offsets[N]], threshold).  A row that is not live has no neighbours and is
    nobody's.  ``threshold``: a float (it becomes Fraction(threshold).limit_denominator(65536)), a Fraction or a (num, den) pair;
    the returned ``threshold`` is the exact Fraction compared with (csrc/fp_select.inc: no float is compared anywhere)."""
    num, den, thr = _threshold(threshold)
    raw = _engine(engine).fp_neighbours(fp, num, den)
    return dict(count=raw["count"].astype(np.int64), offsets=raw["offsets"].astype(np.int64), list=raw["list"].astype(np.int64),
                threshold=thr)


def cluster(fp, threshold, engine=None) -> dict:
    """Butina clusters at ``threshold`` (as for ``neighbours``): the rows by neighbour count descending, then index; a live row
    not yet assigned becomes the next centroid and claims the unassigned rows of its neighbour list ->
    dict(cluster int64 [N] (-1: not live), centroids int64 [n_clusters], sizes int64 [n_clusters], count int64 [N], n_clusters,
    threshold)."""
    num, den, thr = _threshold(threshold)
    raw = _engine(engine).fp_cluster(fp, num, den)
    n = raw["n_clusters"]
    return dict(cluster=raw["cluster"].astype(np.int64), centroids=raw["centroid"][:n].astype(np.int64),
                sizes=raw["size"][:n].astype(np.int64), count=raw["count"].astype(np.int64), n_clusters=n, threshold=thr)


def pick_diverse(fp, k, threshold=None, seeds=None, first=None, engine=None) -> dict:
    """Up to k MaxMin picks: each the live row least similar to everything chosen before it (ties to the smaller index).
    ``seeds``: rows chosen earlier -- an array [S,n_bins], or a ``Library`` for the engine's resident one; without seeds the
    first pick is row ``first`` (None: the first live row).  With a ``threshold`` picking also stops once every live row is at
    least that similar to something chosen: the picks then cover the batch at that radius ->
    dict(picked int64 [n_picked] in pick order, pick_similarity float64 [n_picked]: to the nearest chosen element when picked,
    owner int64 [N]: the pick (a row index) or seed s (-2 - s) nearest to each row, -1 for a row that is not live,
    owner_similarity float64 [N], n_picked, threshold: the exact Fraction or None)."""
    num, den, thr = (0, 0, None) if threshold is None else _threshold(threshold)
    eng = _engine(engine)
    if isinstance(seeds, Library):
        if first is not None:
            raise ValueError("first is read only without seeds")
        if seeds.engine is not eng:
            raise GaudiError("a Library as seeds is the resident library of ITS engine: pass that engine")
        seeds._live()
        raw = eng.fp_pick_diverse(fp, k, num, den, None, -1, S=seeds.M)
    else:
        if seeds is not None and first is not None:
            raise ValueError("first is read only without seeds")
        raw = eng.fp_pick_diverse(fp, k, num, den, seeds, -1 if first is None else int(first))
    n = raw["n_picked"]
    return dict(picked=raw["picked"][:n].astype(np.int64), pick_similarity=_quotient(raw["pick_common"][:n], raw["pick_union"][:n]),
                owner=raw["owner"].astype(np.int64), owner_similarity=_quotient(raw["owner_common"], raw["owner_union"]),
                n_picked=n, threshold=thr)


def rowwise_similarity(a, b) -> np.ndarray:
    """float64 [B]: row i of a with row i of b, in numpy (no kernel: B pairs)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    common = np.minimum(a, b).sum(-1)
    return _quotient(common, a.sum(-1) + b.sum(-1) - common)
