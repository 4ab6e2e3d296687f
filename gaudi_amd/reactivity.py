"""Hueckel localization energies of built molecules on the GPU (csrc/reactivity.inc): WHERE a conjugated
molecule reacts and how easily, with no learned parameter -- the question a chemist asks of a low-gap polycycle before spending
xTB / DFT time on it.  The localization energy is the pi energy lost when the attacked centres are taken out of conjugation, in
|beta| (the smaller, the more reactive the position):

  atom localization (Wheland)   substitution and radical attack at one centre; three kinds by the pi electrons that stay on the
                                attacked centre: 0 nucleophilic, 1 radical, 2 electrophilic
  para localization (Brown)     Diels-Alder / endoperoxide addition across a six-ring: anthracene 9,10 3.31, pentacene 3.18,
                                phenanthrene 3.77, benzene 4.00
  ortho localization            addition to a bond: phenanthrene's 9,10 bond 3.06
  free valence                  sqrt(3) less the pi bond orders at a centre (the carbon scale)

The pi centres, the table, ``charge`` and ``parameters`` are ``gaudi_amd.huckel``'s; no coordinates are needed.  One molecule
costs n_pi + 3 * six-rings + pi bonds diagonalisations beside its own.  Not here: PPP-level localization, transition states,
steric effects, regioselectivity beyond these indices."""
from __future__ import annotations

import numpy as np

from ._lib import REACTIVITY_RINGS_TRUNCATED, REACTIVITY_SWEEP_CAP
from .analyze import _engine

STATUS_NAMES = {0: "solved", 1: "not converged: 30 Jacobi sweeps of the parent left an off-diagonal element above 2^-24",
                2: "a bond index outside the atom list, a repeated bond, an element outside the table, or a charge the pi system "
                   "cannot carry",
                3: "more than 128 pi centres, 384 atoms, 192 heavy atoms or 384 bonds, or an atom with more than 8 bonds",
                4: "no atoms (not built)", 5: "no atom is a pi centre", 6: "the parameter table cannot be read"}
KINDS = ("nucleophilic", "radical", "electrophilic")  # q = 0, 1, 2 pi electrons stay on the attacked centre
RADICAL = 1


def _raw(molecules, dataset, charge, parameters, bonds, engine):
    """One gaudi_reactivity call for the list -> (raw arrays, elem, n_atoms, bond list, n_bonds)."""
    from .gor2goa import _pack_atoms
    from .huckel import _charges, c_huckel_tables
    elem, na, bl, nb = _pack_atoms(molecules)
    raw = _engine(engine).reactivity(c_huckel_tables(dataset, parameters), elem, na, bl, nb, _charges(charge, len(na)), with_bonds=bonds)
    return raw, elem, na, bl, nb


def _has_hydrogen(dataset, elem, na, bl, nb) -> np.ndarray:
    """bool [B,A]: the atoms that carry a hydrogen as the graph counts them -- a listed one, or the one a carbon with exactly two
    bonds implies."""
    from .gor2goa import atoms_list
    atoms = atoms_list(dataset)
    h, c = atoms.index("H"), atoms.index("C")
    out = np.zeros(elem.shape, bool)
    for i in range(len(na)):
        n, m = int(na[i]), int(nb[i])
        b = bl[i, :m]
        if m and (b.min() < 0 or b.max() >= n):
            continue
        deg = np.bincount(b.reshape(-1), minlength=n)[:n] if m else np.zeros(n, np.int64)
        is_h = elem[i, :n] == h
        listed = np.zeros(n, np.int64)
        if m:
            np.add.at(listed, b[:, 0], is_h[b[:, 1]])
            np.add.at(listed, b[:, 1], is_h[b[:, 0]])
        out[i, :n] = ~is_h & ((listed > 0) | ((elem[i, :n] == c) & (deg == 2)))
    return out


def _nanmin(values):
    """(the smallest value that is a number, its flat index) or (NaN, -1)."""
    v = np.asarray(values, np.float64).reshape(-1)
    if not len(v) or np.isnan(v).all():
        return float("nan"), -1
    k = int(np.nanargmin(v))
    return float(v[k]), k


def _minima(raw, i, with_h, n_atoms, n_bonds):
    """The three minima of molecule i and where they occur."""
    r = int(raw["n_rings"][i])
    at = np.where(with_h[i, :n_atoms], raw["atom_localization"][i, RADICAL, :n_atoms], np.nan)
    a_min, a_at = _nanmin(at)
    p_min, p_at = _nanmin(raw["para_localization"][i, :r])
    o_min, o_at = _nanmin(raw["ortho_localization"][i, :n_bonds])
    return dict(min_atom_localization=a_min, min_atom_localization_atom=a_at,
                min_para_localization=p_min, min_para_localization_ring=p_at // 3 if p_at >= 0 else -1,
                min_para_localization_pair=p_at % 3 if p_at >= 0 else -1,
                min_ortho_localization=o_min, min_ortho_localization_bond=o_at)


def localization(molecules, dataset="cata", charge=0, parameters=None, bonds=True, engine=None) -> list:
    """One launch per capacity tier (32 / 64 / 128 pi centres) for the whole list.  ``molecules``: records of rings_to_atoms or
    ``(atom_types [n], bonds [m,2])`` pairs, with or without placed hydrogens; ``charge`` and ``parameters`` as ``huckel.orbitals``
    takes them.  ``bonds=False`` leaves the ortho localization energies out (one solve per pi bond less).  Returns one dict per
    molecule, every array trimmed to the molecule's size, NaN where an entry does not apply (a hydrogen, an atom that is no pi
    centre, a four- or five-ring, a bond to an atom that is no pi centre, a kind whose electron count the residual system cannot
    carry):
      status               0 = solved (STATUS_NAMES; ``status_name`` is its text); otherwise the arrays are zero and the minima NaN
      atom_localization    {"nucleophilic", "radical", "electrophilic"} -> [n] float32, |beta|
      free_valence         [n] float32
      rings                [r, up to 6] atom indices (a list of int64 arrays): the chordless cycles of 4 to 6 pi centres ordered by
                           sorted atom tuple, each in cycle order from its smallest atom
      para_localization    [r,3] float32: ring k's positions (c[p], c[p+3]), p = 0..2; NaN rows for four- and five-rings
      ortho_localization   [m] float32 per listed bond
      e_pi                 the parent's pi energy in |beta| (``huckel.orbitals``' e_pi)
      min_atom_localization  over the pi centres that carry a hydrogen, radical kind, with ``min_atom_localization_atom``
      min_para_localization  with ``min_para_localization_ring`` (index into rings) and ``min_para_localization_pair``
      min_ortho_localization with ``min_ortho_localization_bond``; a minimum over nothing is NaN and its index -1
      rings_truncated, sweep_cap   the flags: more than 32 rings (para values for the kept ones only); a residual solve used 30
                           sweeps (its entry is NaN)
      n_pi, n_electrons, n_jobs (diagonalisations beside the parent's), sweeps (all of them), flags"""
    molecules = list(molecules)
    if not molecules:
        return []
    raw, elem, na, bl, nb = _raw(molecules, dataset, charge, parameters, bonds, engine)
    with_h = _has_hydrogen(dataset, elem, na, bl, nb)
    out = []
    for i in range(len(na)):
        n, m, r = int(na[i]), int(nb[i]), int(raw["n_rings"][i])
        rec = {k: int(raw[k][i]) for k in ("status", "n_pi", "n_electrons", "n_jobs", "sweeps", "flags")}
        rings = raw["rings"][i, :r]
        rec.update(status_name=STATUS_NAMES.get(rec["status"], str(rec["status"])), e_pi=float(raw["e_pi"][i]),
                   atom_localization={name: raw["atom_localization"][i, q, :n].copy() for q, name in enumerate(KINDS)},
                   free_valence=raw["free_valence"][i, :n].copy(), rings=[row[row >= 0].astype(np.int64) for row in rings],
                   para_localization=raw["para_localization"][i, :r].copy(), ortho_localization=raw["ortho_localization"][i, :m].copy(),
                   rings_truncated=bool(rec["flags"] & REACTIVITY_RINGS_TRUNCATED), sweep_cap=bool(rec["flags"] & REACTIVITY_SWEEP_CAP))
        if rec["status"] == 0:
            rec.update(_minima(raw, i, with_h, n, m))
        else:
            rec.update(min_atom_localization=float("nan"), min_atom_localization_atom=-1, min_para_localization=float("nan"),
                       min_para_localization_ring=-1, min_para_localization_pair=-1, min_ortho_localization=float("nan"),
                       min_ortho_localization_bond=-1)
        out.append(rec)
    return out


def most_reactive(molecules, dataset="cata", charge=0, parameters=None, bonds=True, engine=None) -> dict:
    """The array form, one call -> {"min_atom_localization", "min_para_localization", "min_ortho_localization": float64 [B] (NaN
    where the status is not 0 or nothing of the kind exists; the ortho values also with ``bonds=False``), "status": int64 [B]}."""
    molecules = list(molecules)
    keys = ("min_atom_localization", "min_para_localization", "min_ortho_localization")
    if not molecules:
        return dict({k: np.zeros(0) for k in keys}, status=np.zeros(0, np.int64))
    raw, elem, na, bl, nb = _raw(molecules, dataset, charge, parameters, bonds, engine)
    with_h = _has_hydrogen(dataset, elem, na, bl, nb)
    out = {k: np.full(len(na), np.nan) for k in keys}
    for i in range(len(na)):
        if raw["status"][i] == 0:
            mins = _minima(raw, i, with_h, int(na[i]), int(nb[i]))
            for k in keys:
                out[k][i] = mins[k]
    out["status"] = raw["status"].astype(np.int64)
    return out


def record_fields(molecules, dataset="cata", engine=None) -> list:
    """What rings_to_atoms(..., reactivity=True) adds to every record (no ortho solves)."""
    molecules = list(molecules)
    if not molecules:
        return []
    ext = most_reactive(molecules, dataset, bonds=False, engine=engine)
    return [dict(min_atom_localization=float(a), min_para_localization=float(p), reactivity_status=int(st))
            for a, p, st in zip(ext["min_atom_localization"], ext["min_para_localization"], ext["status"])]


__all__ = ["STATUS_NAMES", "KINDS", "localization", "most_reactive", "record_fields"]
