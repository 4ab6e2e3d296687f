"""Kekule structure counts, Pauling bond orders, sextets, Fries and Clar numbers of built molecules on the GPU (csrc/kekule.inc,
DESIGN.md section 8o): the classical descriptors of a polycyclic aromatic system, from the set of ALL its Kekule structures.

The graph, the sigma degree and the valence table are those of ``gor2goa.bond_orders``.  Every atom takes its first, neutral
option; ``sel`` is the set of atoms that add a bond; a Kekule structure is a perfect matching of the bonds between sel atoms.
Exact integer combinatorics with no parameter.  Not here: counts beyond the budget of 2^20 search nodes (no factorisation over
components, no determinant method), charged resonance forms, lone-pair sextets of five-rings, resonance energies in eV.

``ring_currents`` is the magnetic criterion next to that structural one (csrc/ring_current.inc): the
Hueckel-London pi current a perpendicular field induces in every bond and every ring of 4 to 6 pi centres, in units of benzene's --
positive (diatropic) in aromatic rings, negative (paratropic) in antiaromatic ones, four-rings and five-rings with a lone-pair
heteroatom included.  The pi centres and the table are ``gaudi_amd.huckel``'s, the geometry is the record's ``atoms3d``.  Not
here: coupled (PPP) currents, open shells, current-density maps, NICS, non-planar corrections."""
from __future__ import annotations

import numpy as np

from ._lib import KEKULE_EMPTY, KEKULE_OK, RING_CURRENT_RINGS_UNDEFINED
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


RING_CURRENT_STATUS_NAMES = {0: "solved", 1: "not converged: 30 Jacobi sweeps left an off-diagonal element above 2^-24",
                             2: "a bond index outside the atom list, a repeated bond, an element outside the table, or a charge the pi "
                                "system cannot carry",
                             3: "more than 128 pi centres, 384 atoms, 192 heavy atoms or 384 bonds, or an atom with more than 8 bonds",
                             4: "no atoms (not built)", 5: "no atom is a pi centre", 6: "the parameter table cannot be used",
                             7: "open shell: an odd number of pi electrons",
                             8: "bad geometry: a non-finite coordinate on a pi centre, or two pi centres closer than 0.5 Angstrom",
                             9: "small gap: HOMO and LUMO closer than 1e-3 |beta| (or no occupied / no empty level): the paramagnetic "
                                "term diverges"}


def _ring_raw(molecules, dataset, charge, parameters, engine):
    """One gaudi_ring_currents call for the list."""
    from .huckel import _charges, c_huckel_tables
    from .ppp import _pack
    elem, na, bonds, nb, xyz = _pack(molecules)
    raw = _engine(engine).ring_currents(c_huckel_tables(dataset, parameters), elem, na, bonds, nb, xyz, _charges(charge, len(na)))
    return raw, na, nb


def _ring_extremes(raw):
    """(max, min) ring current per molecule, float64 [B]: NaN where nothing was solved or the rings are undefined, 0 for a solved
    molecule without a ring."""
    r = raw["n_rings"]
    cur = raw["ring_current"].astype(np.float64)
    live = np.arange(cur.shape[1])[None, :] < r[:, None]
    solved = (raw["status"] == 0) & ((raw["flags"] & RING_CURRENT_RINGS_UNDEFINED) == 0)
    hi = np.where(live, cur, -np.inf).max(1, initial=-np.inf)
    lo = np.where(live, cur, np.inf).min(1, initial=np.inf)
    return np.where(solved, np.where(r > 0, hi, 0.0), np.nan), np.where(solved, np.where(r > 0, lo, 0.0), np.nan)


def ring_currents(molecules, dataset="cata", charge=0, parameters=None, engine=None) -> list:
    """One launch per capacity tier (32 / 64 / 128 pi centres) for the whole list.  ``molecules``: records of rings_to_atoms (their
    ``atoms3d`` is the geometry) or ``(atom_types [n], bonds [m,2], xyz [n,3])`` triples in Angstrom, as ``ppp.orbitals`` takes them;
    ``charge`` and ``parameters`` as ``huckel.orbitals`` takes them (the electron count must be even).  Returns one dict per molecule:
      status             0 = solved (RING_CURRENT_STATUS_NAMES; ``status_name`` is its text); otherwise the values below are zero / empty / NaN
      bond_current       [m] float32: the current of listed bond (i, j) in the direction i -> j, in units of benzene's; zero on bonds
                         not between pi centres
      rings              [r, up to 6] atom indices (a list of int64 arrays): the chordless cycles of 4 to 6 pi centres, ordered by sorted
                         atom tuple, each from its smallest atom counter-clockwise seen from the tip of ``normal``
      ring_current       [r] float32: positive = diatropic (aromatic), negative = paratropic;  ring_area: [r] Angstrom^2
      ring_current_max, ring_current_min: their extremes (0.0 without a ring, NaN where the rings are undefined)
      rings_undefined    the flag: the chordless cycles are no basis of the cycle space (or more than 32, or one without an area);
                         the bond currents stay valid
      normal             [3] the unit normal of the best plane through the pi centres;  rms_out_of_plane: their rms distance from it
      gap                x_HOMO - x_LUMO in |beta|;  residual: max |C I - b|, how well ring currents reproduce the bond currents
      n_pi, n_electrons, sweeps, flags"""
    molecules = list(molecules)
    if not molecules:
        return []
    raw, na, nb = _ring_raw(molecules, dataset, charge, parameters, engine)
    hi, lo = _ring_extremes(raw)
    out = []
    for i in range(len(na)):
        r = int(raw["n_rings"][i])
        rec = {k: int(raw[k][i]) for k in ("status", "n_pi", "n_electrons", "sweeps", "flags")}
        rec.update({k: float(raw[k][i]) for k in ("rms_out_of_plane", "gap", "residual")})
        rec.update(status_name=RING_CURRENT_STATUS_NAMES.get(rec["status"], str(rec["status"])),
                   bond_current=raw["bond_current"][i, :nb[i]].copy(),
                   rings=[raw["ring_atoms"][i, k, :raw["ring_size"][i, k]].astype(np.int64) for k in range(r)],
                   ring_current=raw["ring_current"][i, :r].copy(), ring_area=raw["ring_area"][i, :r].copy(),
                   ring_current_max=float(hi[i]), ring_current_min=float(lo[i]),
                   rings_undefined=bool(rec["flags"] & RING_CURRENT_RINGS_UNDEFINED), normal=raw["normal"][i].copy())
        out.append(rec)
    return out


def ring_current_extremes(molecules, dataset="cata", charge=0, parameters=None, engine=None) -> dict:
    """The array form, one call -> {"ring_current_max", "ring_current_min": float64 [B] (NaN where nothing was solved or the rings
    are undefined, 0.0 for a solved molecule without a ring), "status": int64 [B]}.  What design / design_sweep / refine(...,
    ring_currents=True) add."""
    molecules = list(molecules)
    if not molecules:
        return dict(ring_current_max=np.zeros(0), ring_current_min=np.zeros(0), status=np.zeros(0, np.int64))
    raw = _ring_raw(molecules, dataset, charge, parameters, engine)[0]
    hi, lo = _ring_extremes(raw)
    return dict(ring_current_max=hi, ring_current_min=lo, status=raw["status"].astype(np.int64))


def ring_current_fields(molecules, dataset="cata", engine=None) -> list:
    """What rings_to_atoms(..., ring_currents=True) adds to every record."""
    ext = ring_current_extremes(molecules, dataset, engine=engine)
    return [dict(ring_current_max=float(hi), ring_current_min=float(lo), ring_current_status=int(st))
            for hi, lo, st in zip(ext["ring_current_max"], ext["ring_current_min"], ext["status"])]


__all__ = ["RING_CURRENT_STATUS_NAMES", "ring_currents", "ring_current_extremes", "ring_current_fields", "STATUS_NAMES", "KEKULE_EMPTY", "KEKULE_OK", "resonance", "kekule_count", "clar_number", "record_fields", "summary_fields", "records",
           "sel_bonds"]
