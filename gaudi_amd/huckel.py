"""Hueckel molecular-orbital levels, the HOMO-LUMO gap, pi charges and pi bond orders of built molecules on the GPU
(csrc/huckel.inc): a second opinion on the property guidance steers towards, with no learned parameter.

The graph is the one of ``canonical``: the non-hydrogen atoms with their element, H count (listed hydrogens, plus one for a
carbon with exactly two bonds) and heavy degree.  coordination = heavy degree + H count; ``data/huckel_tables.json`` maps
(element, coordination) to a site class with a Coulomb term ``h``, an electron count ``n_e`` and a bond factor ``k``, or to
"not a pi centre" (left out and counted in ``n_excluded``).  In units of |beta| with alpha = 0: M_rr = h_r, M_rs = k_r k_s
for bonded centres.  An orbital's energy is alpha + x beta with beta < 0, so the larger x the lower the level; ``gap`` is
x_HOMO - x_LUMO >= 0 in |beta|.  The table is data: ``parameters=`` replaces any of it.  Nothing here is in eV: ``calibrate``
fits the line that turns |beta| into a user's own reference values."""
from __future__ import annotations

import copy
import json
import os

import numpy as np

from ._lib import HUCKEL_DEGENERATE, HUCKEL_MAX_CLASSES, HUCKEL_OPEN_SHELL, GaudiError, HuckelTables
from .analyze import _engine

STATUS_NAMES = {0: "solved", 1: "not converged: 30 Jacobi sweeps left an off-diagonal element above 2^-24",
                2: "a bond index outside the atom list, a repeated bond, an element outside the table, or a charge the pi system "
                   "cannot carry",
                3: "more than 128 pi centres, 384 atoms, 192 heavy atoms or 384 bonds, or an atom with more than 8 bonds",
                4: "no atoms (not built)", 5: "no atom is a pi centre", 6: "the parameter table cannot be read"}
_DEFAULT = None


def default_parameters() -> dict:
    """data/huckel_tables.json: {"classes": {name: {h, n_e, k}}, "sites": {element: {coordination: class}}, "k_pair": {"a|b": k}}."""
    global _DEFAULT
    if _DEFAULT is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "huckel_tables.json")) as f:
            _DEFAULT = json.load(f)
    return _DEFAULT


def tables(dataset="cata", parameters=None) -> dict:
    """The table one call uses, as a plain dict: the default, with ``parameters`` laid over it -- ``classes`` entries are merged
    field by field (a new name adds a class), ``sites`` per element and coordination (None: not a pi centre), ``k_pair`` per
    "classA|classB" key (None: back to the product).  Only the elements of ``dataset`` are kept."""
    from .gor2goa import atoms_list
    T = copy.deepcopy({k: default_parameters()[k] for k in ("classes", "sites", "k_pair")})
    P = parameters or {}
    unknown = set(P) - {"classes", "sites", "k_pair"}
    if unknown:
        raise GaudiError(f"huckel parameters: unknown section(s) {sorted(unknown)}")
    for name, fields in P.get("classes", {}).items():
        T["classes"].setdefault(name, {"h": 0.0, "n_e": 1, "k": 1.0}).update(fields)
    for sym, by_coord in P.get("sites", {}).items():
        T["sites"].setdefault(sym, {}).update({str(c): v for c, v in by_coord.items()})
    T["k_pair"].update(P.get("k_pair", {}))
    atoms = atoms_list(dataset)
    T["sites"] = {sym: {c: v for c, v in by.items() if v is not None} for sym, by in T["sites"].items() if sym in atoms}
    T["k_pair"] = {k: v for k, v in T["k_pair"].items() if v is not None}
    T["atoms"] = list(atoms)
    return T


def c_huckel_tables(dataset="cata", parameters=None) -> HuckelTables:
    """gaudi_huckel_tables for one dataset: ``tables(dataset, parameters)`` in the order of ATOMS_LIST[dataset]."""
    T = tables(dataset, parameters)
    names = list(T["classes"])
    if len(names) > HUCKEL_MAX_CLASSES:
        raise GaudiError(f"huckel parameters: {len(names)} classes, at most {HUCKEL_MAX_CLASSES}")
    t = HuckelTables()
    atoms = T["atoms"]
    t.n_elems, t.h_elem, t.c_elem, t.n_classes = len(atoms), atoms.index("H"), atoms.index("C"), len(names)
    for e in range(8):
        for c in range(5):
            t.site_class[e][c] = -1
    for sym, by_coord in T["sites"].items():
        for coord, name in by_coord.items():
            if not 0 <= int(coord) <= 4:
                raise GaudiError(f"huckel parameters: coordination {coord} of {sym} outside 0..4")
            if name not in names:
                raise GaudiError(f"huckel parameters: site {sym}/{coord} names the unknown class {name!r}")
            t.site_class[atoms.index(sym)][int(coord)] = names.index(name)
    for i, name in enumerate(names):
        c = T["classes"][name]
        t.h[i], t.n_e[i], t.k[i] = float(c["h"]), int(c["n_e"]), float(c["k"])
    for i in range(16):
        for j in range(16):
            t.k_pair[i][j] = float("nan")
    for key, value in T["k_pair"].items():
        a, _, b = key.partition("|")
        if a not in names or b not in names:
            raise GaudiError(f"huckel parameters: k_pair {key!r} names an unknown class")
        t.k_pair[names.index(a)][names.index(b)] = t.k_pair[names.index(b)][names.index(a)] = float(value)
    return t


def _charges(charge, B):
    c = np.asarray(charge, np.int32)
    if c.ndim == 0:
        return None if int(c) == 0 else np.full(B, int(c), np.int32)
    if c.shape != (B,):
        raise GaudiError(f"charge must be one integer or one per molecule ({B}), got shape {c.shape}")
    return np.ascontiguousarray(c)


def _raw(molecules, dataset, charge, parameters, engine):
    from .gor2goa import _pack_atoms
    elem, na, bonds, nb = _pack_atoms(molecules)
    raw = _engine(engine).huckel(c_huckel_tables(dataset, parameters), elem, na, bonds, nb, _charges(charge, len(na)))
    return raw, na, nb


def orbitals(molecules, dataset="cata", charge=0, parameters=None, engine=None) -> list:
    """One launch per capacity tier (32 / 64 / 128 pi centres) for the whole list.  ``molecules``: records of rings_to_atoms or
    ``(atom_types [n], bonds [m,2])`` pairs, with or without placed hydrogens.  ``charge``: one integer or one per molecule
    (n_electrons = sum of n_e - charge).  Returns one dict per molecule:
      status         0 = solved (STATUS_NAMES); for every other status but 1 the values below are zero / empty
      n_pi, n_electrons, n_excluded, sweeps
      levels         [n_pi] float32, x by ascending energy (descending x);  occupation: [n_pi] 0, 1 or 2
      homo, lumo, gap, e_pi   in |beta|; gap = homo - lumo
      open_shell     an odd electron count: homo = lumo = the singly occupied level, gap 0
      degenerate     the frontier levels are closer than 1e-3: charges and bond orders are returned but not unique
      flags          the two above as bits
      pi_charge      [n] float32, zero on hydrogens and excluded atoms;  pi_bond_order: [m] float32, zero on bonds not between
                     pi centres;  site_class: [n] index into ``tables(...)["classes"]``, -1 = none"""
    molecules = list(molecules)
    if not molecules:
        return []
    raw, na, nb = _raw(molecules, dataset, charge, parameters, engine)
    out = []
    for i in range(len(na)):
        n = int(raw["n_pi"][i])
        flags = int(raw["flags"][i])
        rec = {k: int(raw[k][i]) for k in ("status", "n_pi", "n_electrons", "n_excluded", "sweeps", "flags")}
        rec.update({k: float(raw[k][i]) for k in ("homo", "lumo", "gap", "e_pi")})
        rec.update(levels=raw["levels"][i, :n].copy(), occupation=raw["occupation"][i, :n].copy(),
                   open_shell=bool(flags & HUCKEL_OPEN_SHELL), degenerate=bool(flags & HUCKEL_DEGENERATE),
                   pi_charge=raw["pi_charge"][i, :na[i]].copy(), pi_bond_order=raw["pi_bond_order"][i, :nb[i]].copy(),
                   site_class=raw["site_class"][i, :na[i]].copy())
        out.append(rec)
    return out


def gap(molecules, dataset="cata", charge=0, parameters=None, engine=None) -> np.ndarray:
    """float64 [B]: the HOMO-LUMO gap in |beta|, NaN where the status is not 0."""
    molecules = list(molecules)
    if not molecules:
        return np.zeros(0)
    raw, _, _ = _raw(molecules, dataset, charge, parameters, engine)
    return np.where(raw["status"] == 0, raw["gap"].astype(np.float64), np.nan)


def record_fields(molecules, dataset="cata", engine=None) -> list:
    """What rings_to_atoms(..., huckel=True) adds to every record."""
    molecules = list(molecules)
    if not molecules:
        return []
    raw, _, _ = _raw(molecules, dataset, 0, None, engine)
    return [dict(huckel_gap=float(raw["gap"][i]), huckel_homo=float(raw["homo"][i]), huckel_lumo=float(raw["lumo"][i]),
                 huckel_flags=int(raw["flags"][i]), huckel_status=int(raw["status"][i])) for i in range(len(molecules))]


def calibrate(x, reference):
    """The least-squares line reference ~ a + b * x on the host -> (a, b): what turns |beta| units into the units of a user's own
    reference values (DFT gaps in eV, say).  No constants are shipped: none have been measured here."""
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(reference, np.float64).reshape(-1)
    if x.shape != y.shape or len(x) < 2 or not (np.isfinite(x).all() and np.isfinite(y).all()) or np.ptp(x) == 0.0:
        raise GaudiError("calibrate needs two or more finite (x, reference) pairs with distinct x")
    b, a = np.polyfit(x, y, 1)
    return float(a), float(b)
