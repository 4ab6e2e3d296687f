"""Kekule structure counts, Pauling bond orders, sextets, Fries and Clar numbers of built molecules on the GPU (csrc/kekule.inc,
DESIGN.md section 8o): the classical descriptors of a polycyclic aromatic system, from the set of ALL its Kekule structures.

The graph, the sigma degree and the valence table are those of ``gor2goa.bond_orders``.  Every atom takes its first, neutral
option; ``sel`` is the set of atoms that add a bond; a Kekule structure is a perfect matching of the bonds between sel atoms.
Exact integer combinatorics with no parameter.  Not here: counts beyond the budget of 2^20 search nodes (no factorisation over
components, no determinant method), charged resonance forms, lone-pair sextets of five-rings, resonance energies in eV."""
from __future__ import annotations

import numpy as np

from ._lib import KEKULE_EMPTY, KEKULE_OK
from .analyze import _engine

STATUS_NAMES = {0: "counted", 1: "no Kekule structure: an odd number of atoms that add a bond, or no perfect matching among them",
                2: "an atom whose only option is charged", 3: "not connected", 4: "an atom without an option",
                5: "a bond index outside the atom list, a repeated bond or an element outside the table",
                6: "more than 384 atoms, 192 heavy atoms, 384 bonds, 128 atoms that add a bond, 192 bonds among them or 32 hexagons",
                7: "no atoms (not built)", 8: "undecided: the search tree has more than 2^20 nodes"}


def _raw(molecules, dataset, engine):
    from .gor2goa import _pack_atoms, c_valence_tables
    elem, na, bonds, nb = _pack_atoms(molecules)
    return _engine(engine).kekule(c_valence_tables(dataset), elem, na, bonds, nb), na, nb


def records(raw, n_bonds, in_sel) -> list:
    """The raw arrays of gaudi_kekule / gaudi_host_kekule (_lib.KEKULE_ARRAYS) and ``sel_bonds`` as resonance returns them."""
    out = []
    none = np.zeros(0, np.int64)
    for i in range(len(n_bonds)):
        m, r, ok = int(n_bonds[i]), int(raw["n_hex"][i]), int(raw["status"][i]) == KEKULE_OK
        K = int(raw["k"][i])
        dc, sc = raw["double_count"][i, :m].astype(np.int64), raw["sextet_count"][i, :r].astype(np.int64)
        out.append(dict(status=int(raw["status"][i]), kekule_count=K, double_count=dc,
                        pauling_bond_order=dc / float(K) if ok else np.full(m, np.nan),
                        localized_double=np.flatnonzero(in_sel[i, :m] & (dc == K)) if ok else none,
                        localized_single=np.flatnonzero(in_sel[i, :m] & (dc == 0)) if ok else none,
                        hexagons=raw["hex_atoms"][i, :r].astype(np.int64), sextet_count=sc,
                        sextet_fraction=sc / float(K) if ok else np.full(r, np.nan), fries=int(raw["fries"][i]),
                        clar=int(raw["clar"][i]), n_nodes=int(raw["n_nodes"][i])))
    return out


def resonance(molecules, dataset="cata", engine=None) -> list:
    """One launch for the whole list.  ``molecules``: records of rings_to_atoms or ``(atom_types [n], bonds [m,2])`` pairs, with
    or without placed hydrogens.  Returns one dict per molecule:
      status              0 = counted (STATUS_NAMES); for every other status the values below are zero / empty / NaN
      kekule_count        K, a Python int
      double_count        [m] structures in which the bond is double (0 for a bond that does not join two sel atoms)
      pauling_bond_order  [m] float64 double_count / K: the pi bond order, 1.0 = a double bond in every structure
      localized_double    indices of the bonds between sel atoms with order exactly 1;  localized_single: with order exactly 0
      hexagons            [r,6] atom indices, ordered by sorted atom tuple, each from its smallest atom towards the smaller of
                          that atom's two ring neighbours
      sextet_count        [r] structures in which the hexagon has three double bonds;  sextet_fraction: that over K
      fries, clar         the most sextets / the most pairwise atom-disjoint sextets of one structure (the Clar number)
      n_nodes             nodes of the search tree"""
    molecules = list(molecules)
    if not molecules:
        return []
    from .gor2goa import _pack_atoms, c_valence_tables
    elem, na, bonds, nb = _pack_atoms(molecules)
    t = c_valence_tables(dataset)
    return records(_engine(engine).kekule(t, elem, na, bonds, nb), nb, sel_bonds(t, elem, na, bonds, nb))


def sel_bonds(tables, elem, n_atoms, bonds, n_bonds) -> np.ndarray:
    """bool [B,M]: the listed bonds that join two atoms whose first option adds a bond (the bonds of G[sel]), from the table."""
    B, M = bonds.shape[0], bonds.shape[1]
    out = np.zeros((B, M), bool)
    add = np.array([[tables.option[e][d][0][0] if tables.n_options[e][d] else 0 for d in range(5)] for e in range(8)], np.int64)
    for i in range(B):
        n, m = int(n_atoms[i]), int(n_bonds[i])
        b = bonds[i, :m]
        if m == 0 or b.min() < 0 or b.max() >= n or elem[i, :n].min() < 0 or elem[i, :n].max() >= tables.n_elems:
            continue
        deg = np.bincount(b.reshape(-1), minlength=n)
        deg = deg + ((elem[i, :n] == tables.c_elem) & (deg == 2))
        sel = np.where(deg <= 4, add[elem[i, :n], np.minimum(deg, 4)], 0).astype(bool)
        out[i, :m] = sel[b[:, 0]] & sel[b[:, 1]]
    return out


def kekule_count(molecules, dataset="cata", engine=None) -> np.ndarray:
    """int64 [B]: the number of Kekule structures, 0 where the status is not 0."""
    molecules = list(molecules)
    if not molecules:
        return np.zeros(0, np.int64)
    return _raw(molecules, dataset, engine)[0]["k"].astype(np.int64)


def clar_number(molecules, dataset="cata", engine=None) -> np.ndarray:
    """int64 [B]: the Clar number, 0 where the status is not 0 (and for a counted molecule without a hexagon)."""
    molecules = list(molecules)
    if not molecules:
        return np.zeros(0, np.int64)
    return _raw(molecules, dataset, engine)[0]["clar"].astype(np.int64)


def summary_fields(molecules, dataset="cata", engine=None) -> dict:
    """What design / design_sweep / refine(..., aromaticity=True) add: ``kekule_count`` and ``clar``, int64 [B], from one launch."""
    molecules = list(molecules)
    if not molecules:
        return dict(kekule_count=np.zeros(0, np.int64), clar=np.zeros(0, np.int64))
    raw = _raw(molecules, dataset, engine)[0]
    return dict(kekule_count=raw["k"].astype(np.int64), clar=raw["clar"].astype(np.int64))


def record_fields(molecules, dataset="cata", engine=None) -> list:
    """What rings_to_atoms(..., aromaticity=True) adds to every record."""
    molecules = list(molecules)
    if not molecules:
        return []
    raw, _, nb = _raw(molecules, dataset, engine)
    out = []
    for i in range(len(molecules)):
        ok = raw["status"][i] == KEKULE_OK
        dc = raw["double_count"][i, :nb[i]]
        out.append(dict(kekule_count=int(raw["k"][i]), clar=int(raw["clar"][i]), fries=int(raw["fries"][i]),
                        max_pauling_order=float(dc.max()) / float(raw["k"][i]) if ok and len(dc) else float("nan"),
                        resonance_status=int(raw["status"][i])))
    return out


__all__ = ["STATUS_NAMES", "KEKULE_EMPTY", "KEKULE_OK", "resonance", "kekule_count", "clar_number", "record_fields", "summary_fields", "records",
           "sel_bonds"]
