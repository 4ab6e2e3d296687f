"""Does a built molecule CONTAIN a motif, where, and how often: substructure search over graphs of atoms on the GPU
(csrc/sub.inc).  ``canon_key`` says whether two molecules are the same and gaudi_amd.similarity how alike
they are; this module answers the question between the two -- a thiophene ring, a B-N pair, an unsubstituted naphthalene edge.
What RDKit users get from a SMARTS match without bond primitives, without RDKit.

Graphs on both sides are the one of ``canonical``: the non-hydrogen atoms with their element and H count (listed hydrogens, plus
one for a carbon with exactly two bonds), and the bonds between them, unlabelled.  A pattern is a CONNECTED graph of 1..32 such
atoms.  An embedding maps pattern atoms to distinct molecule atoms of the same element so that every pattern bond lies on a
molecule bond (the molecule may have more bonds among them: a monomorphism).  ``hydrogens="exact"`` also asks for equal H
counts, ``closed=True`` for equal numbers of non-hydrogen neighbours (nothing else attached)."""
from __future__ import annotations

import numpy as np

from ._lib import SUB_CLOSED, SUB_GAVE_UP, SUB_H_EXACT, SUB_MAX_PATTERNS, GaudiError
from .analyze import _engine

STATUS_NAMES = {0: "searched", 1: "gave up (a root needed more than 8192 candidate tests): count is a lower bound, 0 is undecided",
                2: "molecule: a bond index outside the atom list, a repeated bond or an element outside the table",
                3: "molecule: more than 384 atoms, 192 heavy atoms or 384 bonds, or an atom with more than 8 bonds",
                4: "molecule: no atoms (not built)",
                5: "pattern refused: empty, not connected, more than 32 heavy atoms, or a bad bond"}


def pattern(symbols_or_types, bonds, dataset="cata"):
    """A pattern from element symbols ("C", "S", ...; "H" for a listed hydrogen) or atom types, and bonds [m,2] ->
    (atom_types int32 [n], bonds int32 [m,2])."""
    from .gor2goa import atoms_list
    names = atoms_list(dataset)
    types = []
    for s in symbols_or_types:
        if isinstance(s, str):
            if s not in names:
                raise GaudiError(f"pattern: element {s!r} is not in the {dataset} atom list {names}")
            types.append(names.index(s))
        else:
            types.append(int(s))
    return np.array(types, np.int32), np.asarray(bonds, np.int32).reshape(-1, 2)


def ring_pattern(symbols, dataset="cata"):
    """A ring of the given atoms in order: ring_pattern("CCCCS") is thiophene's five-ring, ring_pattern("CCCCCC") benzene's."""
    n = len(symbols)
    if n < 3:
        raise GaudiError("ring_pattern: a ring has at least three atoms")
    return pattern(list(symbols), [(k, (k + 1) % n) for k in range(n)], dataset)


def read_smiles(text, dataset="cata"):
    """A pattern from a SMILES string of the dialect gaudi_amd.gor2goa.smiles writes (gor2goa.read_smiles) -> (atom_types, bonds).
    Its hydrogens -- implied and bracketed -- become listed hydrogens, which matter with ``hydrogens="exact"`` only; its bond
    orders and charges are dropped."""
    from .gor2goa import read_smiles as parse
    types, bonds, _, _ = parse(text, dataset)
    return types.astype(np.int32), bonds.astype(np.int32)


def _as_pair(p):
    if isinstance(p, dict):  # a record of rings_to_atoms
        if p.get("status", 0) != 0:
            return np.zeros(0, np.int32), np.zeros((0, 2), np.int32)
        return p["atom_types"], p["bonds"]
    return p[0], p[1]


def search(molecules, patterns, dataset="cata", hydrogens="ignore", closed=False, engine=None) -> dict:
    """Every molecule against every pattern, 64 patterns to a launch.  ``molecules``: records of rings_to_atoms or
    ``(atom_types [n], bonds [m,2])`` pairs, with or without placed hydrogens.  ``patterns``: pairs from pattern / ring_pattern /
    read_smiles, or records.  A pattern's bond orders and charges are no part of the search: a pattern given with them (a record,
    a parsed SMILES) has them dropped.  hydrogens: "ignore", or "exact" for equal H counts; closed: equal heavy degrees.
    -> dict with
      count [B,P] int32      embeddings found;          status [B,P] int32 (STATUS_NAMES);      steps [B,P] int32 candidate tests
      hit [B,P] bool         count > 0 (True under GAVE_UP only with an embedding in hand)
      undecided [B,P] bool   status == GAVE_UP and count == 0
      first                  list of B lists of P arrays [n_atoms of the pattern]: the smallest embedding as molecule atom indices
                             in the pattern's atom order, -1 at pattern hydrogens and everywhere without a hit
      covered [B,P,A] uint8  1 where some embedding found uses the molecule's atom (A: the widest molecule)
      symmetry [P] int64     the pattern matched against itself under the same flags: the order of its automorphism group (0 for
                             a refused pattern)
      n_unique [B,P] int64   count // symmetry: the distinct subgraphs of the molecule that are images of the pattern; exact when
                             status is OK"""
    from .gor2goa import _pack_atoms, atoms_list
    if hydrogens not in ("ignore", "exact"):
        raise GaudiError(f'hydrogens must be "ignore" or "exact", got {hydrogens!r}')
    molecules, patterns = list(molecules), [_as_pair(p) for p in patterns]
    B, P = len(molecules), len(patterns)
    flags = (SUB_H_EXACT if hydrogens == "exact" else 0) | (SUB_CLOSED if closed else 0)
    atoms = atoms_list(dataset)
    ne, he, ce = len(atoms), atoms.index("H"), atoms.index("C")
    eng = _engine(engine)
    A = 1
    out = dict(count=np.zeros((B, P), np.int32), status=np.zeros((B, P), np.int32), steps=np.zeros((B, P), np.int32),
               first=[[None] * P for _ in range(B)], symmetry=np.zeros(P, np.int64))
    covered = []
    if P:
        pe, pna, pb, pnb = _pack_atoms(patterns)
        mols = _pack_atoms(molecules) if B else None
        A = mols[0].shape[1] if B else 1
        for lo in range(0, P, SUB_MAX_PATTERNS):
            hi = min(lo + SUB_MAX_PATTERNS, P)
            chunk = (np.ascontiguousarray(pe[lo:hi]), np.ascontiguousarray(pna[lo:hi]), np.ascontiguousarray(pb[lo:hi]),
                     np.ascontiguousarray(pnb[lo:hi]), np.full(hi - lo, flags, np.int32))
            own = eng.substructure_search(ne, he, ce, *chunk[:4], *chunk)
            out["symmetry"][lo:hi] = np.diagonal(own["count"])
            if not B:
                continue
            raw = eng.substructure_search(ne, he, ce, *mols, *chunk)
            for name in ("count", "status", "steps"):
                out[name][:, lo:hi] = raw[name]
            covered.append(raw["covered"])
            for b in range(B):
                for p in range(lo, hi):
                    out["first"][b][p] = raw["first"][b, p - lo, :pna[p]].astype(np.int64)
    out["covered"] = np.concatenate(covered, 1) if covered else np.zeros((B, P, A), np.uint8)
    out["hit"] = out["count"] > 0
    out["undecided"] = (out["status"] == SUB_GAVE_UP) & (out["count"] == 0)
    out["n_unique"] = out["count"].astype(np.int64) // np.maximum(out["symmetry"], 1)[None, :]
    return out


def contains(molecules, pattern, dataset="cata", hydrogens="ignore", closed=False, engine=None) -> np.ndarray:
    """bool [B]: search(...)["hit"] for one pattern."""
    return search(molecules, [pattern], dataset, hydrogens, closed, engine)["hit"][:, 0]
