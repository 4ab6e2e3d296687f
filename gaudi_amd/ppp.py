"""Pariser-Parr-Pople self-consistent pi levels, the HOMO-LUMO gap, Koopmans IP and EA, pi charges and pi bond orders of built
molecules on the GPU, in eV (csrc/ppp.inc): what ``gaudi_amd.huckel`` leaves out -- geometry and electron
repulsion -- on the same pi centres.

The sites are huckel's: the graph of ``canonical``, coordination = heavy degree + H count, and ``sites`` maps (element,
coordination) to a class or to "not a pi centre".  ``data/ppp_tables.json`` gives every class a valence-state ionisation energy
``I``, a one-centre repulsion ``gamma`` (both eV), a core charge ``z`` (the electrons it contributes) and a bond factor ``k``;
beta_rs = beta0 * k_r * k_s for bonded centres (or the ``beta_pair`` value), gamma_rs from the distance by the Mataga-Nishimoto or
the Ohno formula, and a closed-shell SCF with damping (include/gaudi_hip.h spells the model out).  The table is data and its
values are recalled, not verified: ``parameters=`` replaces any of it, and no accuracy in eV is claimed --
``gaudi_amd.huckel.calibrate`` fits the line to a user's own reference values.

``excited_states`` / ``optical`` / ``spectrum`` go one step further (csrc/ppp_cis.inc): configuration
interaction over single excitations on that ground state, in an active window of at most 8 occupied and 8 empty levels -- the
lowest singlet and triplet excitation energies, the singlet-triplet gap, oscillator strengths and the lowest bright singlet.

``states`` / ``ionization`` / ``triplet`` take open shells (csrc/ppp_open.inc): Dewar's half-electron method --
one restricted SCF with occupations 2 / 1 / 0 and a closed-form energy correction -- for radical ions, neutral radicals and
triplets; delta-SCF ionisation potentials and electron affinities (orbital relaxation included) next to the Koopmans values, and
the spin density of the unpaired electrons.

``scf="diis"`` on ``orbitals`` / ``frontier`` / ``gap`` / ``states`` / ``ionization`` / ``triplet`` runs the same model with Pulay's
DIIS (csrc/ppp_scf.inc, gaudi_ppp_scf): the Fock matrix is extrapolated from a ring of ``diis_size`` earlier
ones from iteration ``diis_start`` on -- the same fixed points in about half the iterations, and nearly every row the damped
iteration leaves NOT_CONVERGED solved.  The default, ``scf="damped"``, is what it was; ``excited_states`` and the CIS hand-over take
the damped ground state only."""
from __future__ import annotations

import copy
import json
import os

import numpy as np

from ._lib import (HUCKEL_MAX_CLASSES, PPP_CIS_FLAGS, PPP_CIS_JACOBI_CAP, PPP_CIS_TRIPLET_UNSTABLE, PPP_CIS_TRUNCATED, PPP_CIS_WINDOW_EDGE,
                   PPP_DEGENERATE, PPP_DIIS_MAX, PPP_JACOBI_CAP, PPP_MATAGA_NISHIMOTO, PPP_OHNO, PPP_OPEN_SHELL, PPP_OPEN_TIE, PPP_SCF_CAP, GaudiError,
                   PPPTables)
from .analyze import _engine
from .huckel import _charges

STATUS_NAMES = {0: "solved", 1: "not converged: 64 SCF iterations left delta_p above 2^-16, or a diagonalisation used 30 Jacobi sweeps "
                   "(flags says which)",
                2: "a bond index outside the atom list, a repeated bond, an element outside the table, or a charge the pi system "
                   "cannot carry",
                3: "more than 128 pi centres, 384 atoms, 192 heavy atoms or 384 bonds, or an atom with more than 8 bonds",
                4: "no atoms (not built)", 5: "no atom is a pi centre", 6: "the parameter table, the damping or the repulsion formula "
                   "cannot be used",
                7: "open shell: an odd number of pi electrons", 8: "bad geometry: a non-finite coordinate on a pi centre, or two pi "
                   "centres closer than 0.5 Angstrom"}
REPULSIONS = {"mataga-nishimoto": PPP_MATAGA_NISHIMOTO, "ohno": PPP_OHNO}
_SECTIONS = ("classes", "sites", "beta_pair", "beta0")
_DEFAULT = None


def default_parameters() -> dict:
    """data/ppp_tables.json: {"beta0": eV, "classes": {name: {I, gamma, z, k}}, "sites": {element: {coordination: class}},
    "beta_pair": {"a|b": eV}}."""
    global _DEFAULT
    if _DEFAULT is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "ppp_tables.json")) as f:
            _DEFAULT = json.load(f)
    return _DEFAULT


def tables(dataset="cata", parameters=None) -> dict:
    """The table one call uses, as a plain dict: the default, with ``parameters`` laid over it -- ``beta0`` replaced, ``classes``
    entries merged field by field (a new name adds a class), ``sites`` per element and coordination (None: not a pi centre),
    ``beta_pair`` per "classA|classB" key (None: back to the product).  Only the elements of ``dataset`` are kept."""
    from .gor2goa import atoms_list
    T = copy.deepcopy({k: default_parameters()[k] for k in _SECTIONS})
    P = parameters or {}
    unknown = set(P) - set(_SECTIONS)
    if unknown:
        raise GaudiError(f"ppp parameters: unknown section(s) {sorted(unknown)}")
    if "beta0" in P:
        T["beta0"] = float(P["beta0"])
    for name, fields in P.get("classes", {}).items():
        T["classes"].setdefault(name, {"I": 11.16, "gamma": 11.13, "z": 1, "k": 1.0}).update(fields)
    for sym, by_coord in P.get("sites", {}).items():
        T["sites"].setdefault(sym, {}).update({str(c): v for c, v in by_coord.items()})
    T["beta_pair"].update(P.get("beta_pair", {}))
    atoms = atoms_list(dataset)
    T["sites"] = {sym: {c: v for c, v in by.items() if v is not None} for sym, by in T["sites"].items() if sym in atoms}
    T["beta_pair"] = {k: v for k, v in T["beta_pair"].items() if v is not None}
    T["atoms"] = list(atoms)
    return T


def c_ppp_tables(dataset="cata", parameters=None) -> PPPTables:
    """gaudi_ppp_tables for one dataset: ``tables(dataset, parameters)`` in the order of ATOMS_LIST[dataset]."""
    T = tables(dataset, parameters)
    names = list(T["classes"])
    if len(names) > HUCKEL_MAX_CLASSES:
        raise GaudiError(f"ppp parameters: {len(names)} classes, at most {HUCKEL_MAX_CLASSES}")
    t = PPPTables()
    atoms = T["atoms"]
    t.n_elems, t.h_elem, t.c_elem, t.n_classes, t.beta0 = len(atoms), atoms.index("H"), atoms.index("C"), len(names), float(T["beta0"])
    for e in range(8):
        for c in range(5):
            t.site_class[e][c] = -1
    for sym, by_coord in T["sites"].items():
        for coord, name in by_coord.items():
            if not 0 <= int(coord) <= 4:
                raise GaudiError(f"ppp parameters: coordination {coord} of {sym} outside 0..4")
            if name not in names:
                raise GaudiError(f"ppp parameters: site {sym}/{coord} names the unknown class {name!r}")
            t.site_class[atoms.index(sym)][int(coord)] = names.index(name)
    for i, name in enumerate(names):
        c = T["classes"][name]
        t.I[i], t.gamma[i], t.z[i], t.k[i] = float(c["I"]), float(c["gamma"]), int(c["z"]), float(c["k"])
    for i in range(16):
        for j in range(16):
            t.beta_pair[i][j] = float("nan")
    for key, value in T["beta_pair"].items():
        a, _, b = key.partition("|")
        if a not in names or b not in names:
            raise GaudiError(f"ppp parameters: beta_pair {key!r} names an unknown class")
        t.beta_pair[names.index(a)][names.index(b)] = t.beta_pair[names.index(b)][names.index(a)] = float(value)
    return t


def _repulsion(repulsion) -> int:
    if repulsion not in REPULSIONS:
        raise GaudiError(f"repulsion must be one of {sorted(REPULSIONS)}, got {repulsion!r}")
    return REPULSIONS[repulsion]


def _pack(molecules):
    """Records (their atoms3d) or (atom_types, bonds, xyz) triples -> elem, n_atoms, bonds, n_bonds, xyz [B,A,3] float32."""
    from .gor2goa import _np, _pack_atoms
    graphs, coords = [], []
    for i, mol in enumerate(molecules):
        if isinstance(mol, dict):
            if mol["status"] != 0:
                graphs.append(mol)
                coords.append(np.zeros((0, 3), np.float32))
                continue
            xyz = mol.get("atoms3d")
            graphs.append(mol)
        else:
            xyz = mol[2] if len(mol) > 2 else None
            graphs.append((mol[0], mol[1]))
        if xyz is None:
            raise GaudiError(f"molecule {i} has no coordinates: ppp needs atoms3d of a record or an (atom_types, bonds, xyz) triple")
        coords.append(np.asarray(_np(xyz), np.float32).reshape(-1, 3))
    elem, na, bonds, nb = _pack_atoms(graphs)
    xyz = np.zeros(elem.shape + (3,), np.float32)
    for i, c in enumerate(coords):
        if len(c) != na[i]:
            raise GaudiError(f"molecule {i}: {len(c)} coordinates for {na[i]} atoms")
        xyz[i, :len(c)] = c
    return elem, na, bonds, nb, xyz


SCF = ("damped", "diis")


def _scf(scf, diis_size, diis_start) -> bool:
    """Whether the DIIS entry point serves the call."""
    scf = "damped" if scf is None else scf
    if scf not in SCF:
        raise GaudiError(f"scf must be one of {list(SCF)}, got {scf!r}")
    if scf == "diis" and not (2 <= int(diis_size) <= PPP_DIIS_MAX and int(diis_start) >= 2):
        raise GaudiError(f"diis_size must be 2..{PPP_DIIS_MAX} and diis_start at least 2, got {diis_size} and {diis_start}")
    return scf == "diis"


def _raw(molecules, dataset, charge, parameters, repulsion, damping, engine, window=None, scf="damped", diis_size=6, diis_start=3):
    """One gaudi_ppp call, or with a window one gaudi_ppp_cis call, for the list; with scf="diis" (no window) one gaudi_ppp_scf call
    of multiplicity 1, the rows of an odd electron count set to OPEN_SHELL as gaudi_ppp has them."""
    if _scf(scf, diis_size, diis_start):
        raw, na, nb = _raw_open(molecules, dataset, charge, 1, parameters, repulsion, damping, engine, scf, diis_size, diis_start)
        odd = np.flatnonzero(raw["status"] == 2)
        if len(odd):  # BAD_INPUT at multiplicity 1 and anything else at the lowest multiplicity: the parity was the reason
            q = _charges(charge, len(na))
            again, _, _ = _raw_open([molecules[i] for i in odd], dataset, 0 if q is None else q[odd], 0, parameters, repulsion, damping,
                                    engine, scf, diis_size, diis_start)
            raw["status"][odd[again["status"] != 2]] = PPP_OPEN_SHELL
        return raw, na, nb
    elem, na, bonds, nb, xyz = _pack(molecules)
    args = (c_ppp_tables(dataset, parameters), elem, na, bonds, nb, xyz, _charges(charge, len(na)), _repulsion(repulsion), float(damping))
    raw = _engine(engine).ppp(*args) if window is None else _engine(engine).ppp_cis(*args, int(window))
    return raw, na, nb


def _orbital_record(raw, i, na, nb) -> dict:
    n = int(raw["n_pi"][i])
    flags = int(raw["flags"][i])
    rec = {k: int(raw[k][i]) for k in ("status", "n_pi", "n_electrons", "n_excluded", "iterations", "sweeps", "flags")}
    rec.update({k: float(raw[k][i]) for k in ("homo", "lumo", "gap", "e_electronic", "e_core", "delta_p")})
    rec.update(ip=-rec["homo"], ea=-rec["lumo"], e_total=rec["e_electronic"] + rec["e_core"],
               levels=raw["levels"][i, :n].copy(), occupation=raw["occupation"][i, :n].copy(),
               open_shell=rec["status"] == PPP_OPEN_SHELL, degenerate=bool(flags & PPP_DEGENERATE),
               pi_charge=raw["pi_charge"][i, :na[i]].copy(), pi_bond_order=raw["pi_bond_order"][i, :nb[i]].copy(),
               site_class=raw["site_class"][i, :na[i]].copy())
    if "diis_error" in raw:
        rec.update(diis_error=float(raw["diis_error"][i]), n_extrapolated=int(raw["n_extrapolated"][i]))
    return rec


def orbitals(molecules, dataset="cata", charge=0, parameters=None, repulsion="mataga-nishimoto", damping=0.25, engine=None, scf="damped", diis_size=6, diis_start=3) -> list:
    """One launch per capacity tier (32 / 64 / 128 pi centres) for the whole list.  ``molecules``: records of rings_to_atoms (their
    ``atoms3d`` is the geometry) or ``(atom_types [n], bonds [m,2], xyz [n,3])`` triples in Angstrom, with or without placed
    hydrogens; a molecule without coordinates raises.  ``charge``: one integer or one per molecule (n_electrons = sum of z - charge,
    which must be even).  ``repulsion``: "mataga-nishimoto" or "ohno".  ``damping``: the share of the old density kept per
    iteration, in [0, 1).  Returns one dict per molecule:
      status         0 = solved (STATUS_NAMES); for every other status but 1 the values below are zero / empty
      n_pi, n_electrons, n_excluded, iterations (SCF), sweeps (Jacobi, all iterations), delta_p (the last max |P_new - P|)
      levels         [n_pi] float32, eV, ascending;  occupation: [n_pi] 0 or 2
      homo, lumo, gap = lumo - homo, ip = -homo, ea = -lumo (Koopmans), e_electronic, e_core, e_total = their sum: eV
      open_shell     status 7: an odd electron count, nothing solved (``states`` solves these)
      degenerate     the frontier levels are closer than 1e-3 eV: charges and bond orders are returned but not unique
      flags          degenerate (2); why the status is 1: the iteration cap (4), a Jacobi solve at its cap (8)
      pi_charge      [n] float32 = z - P_rr, zero on hydrogens and excluded atoms;  pi_bond_order: [m] float32, zero on bonds not
                     between pi centres;  site_class: [n] index into ``tables(...)["classes"]``, -1 = none
    ``scf``: "damped" (gaudi_ppp) or "diis" (gaudi_ppp_scf at multiplicity 1, DESIGN.md section 8t: the same model and fixed points,
    not the same bits), with a history of ``diis_size`` Fock matrices (2..8) from iteration ``diis_start`` (at least 2) on.  With
    "diis" a record also has ``diis_error`` (the last iteration's max |F P - P F| in eV) and ``n_extrapolated`` (the iterations whose
    Fock matrix was a combination)."""
    molecules = list(molecules)
    if not molecules:
        return []
    raw, na, nb = _raw(molecules, dataset, charge, parameters, repulsion, damping, engine, None, scf, diis_size, diis_start)
    return [_orbital_record(raw, i, na, nb) for i in range(len(na))]


def _raw_open(molecules, dataset, charge, multiplicity, parameters, repulsion, damping, engine, scf="damped", diis_size=6, diis_start=3):
    """One gaudi_ppp_open call, or with scf="diis" one gaudi_ppp_scf call, for the list: a row is (molecule, charge, multiplicity)."""
    diis = _scf(scf, diis_size, diis_start)
    elem, na, bonds, nb, xyz = _pack(molecules)
    mult = _charges(multiplicity, len(na))
    args = (c_ppp_tables(dataset, parameters), elem, na, bonds, nb, xyz, _charges(charge, len(na)), mult, _repulsion(repulsion))
    if diis:
        return _engine(engine).ppp_scf(*args, int(diis_size), int(diis_start), float(damping)), na, nb
    return _engine(engine).ppp_open(*args, float(damping)), na, nb


def states(molecules, dataset="cata", charge=0, multiplicity=0, parameters=None, repulsion="mataga-nishimoto", damping=0.25,
           engine=None, scf="damped", diis_size=6, diis_start=3) -> list:
    """``orbitals`` for open and closed shells alike, by the half-electron method (gaudi_ppp_open): one
    launch per capacity tier for the whole list.  A row is (molecule, charge, multiplicity); ``charge`` and ``multiplicity`` are
    one integer or one per molecule.  ``multiplicity``: 1, 2 or 3; 0 is the lowest the electron count allows (1 for an even count,
    2 for an odd one); a multiplicity the electron count cannot have is status 2.  Returns one dict per row with every key of
    ``orbitals`` (``occupation`` holds 2 / 1 / 0; ``homo`` is the highest occupied level, the singly occupied one where there is
    one, ``lumo`` the first empty one; ``open_shell`` is never set) and
      e_state        float (float64): the energy of the state in eV, electronic and core, the half-electron correction included --
                     differences of these are ionisation potentials, electron affinities and triplet energies
      he_correction  float (float64): -J_mm / 4 for a doublet, -(J_mm + J_nn) / 4 - K_mn / 2 for a triplet, 0 for a singlet
      spin_density   [n] float32: the sum over the singly occupied orbitals of v_r^2 per atom (it sums to n_open)
      n_open, somo   the number of singly occupied levels and their ranks in ``levels`` (a list of n_open integers)
      multiplicity   n_open + 1
      open_tie       a level within 1e-3 eV of the singly occupied set on either side, in some iteration or in the result: which
                     orbital of a degenerate pair holds the unpaired electron was arbitrary (the benzene cation), and charges, bond
                     orders and spin densities depend on it
    ``scf``, ``diis_size``, ``diis_start``: as ``orbitals`` takes them (gaudi_ppp_scf); with "diis" a record also has ``diis_error``
    and ``n_extrapolated``."""
    molecules = list(molecules)
    if not molecules:
        return []
    raw, na, nb = _raw_open(molecules, dataset, charge, multiplicity, parameters, repulsion, damping, engine, scf, diis_size, diis_start)
    out = []
    for i in range(len(na)):
        rec = _orbital_record(raw, i, na, nb)
        k = int(raw["n_open"][i])
        rec.update(e_state=float(raw["e_state"][i]), he_correction=float(raw["he_correction"][i]),
                   spin_density=raw["spin_density"][i, :na[i]].copy(), n_open=k, somo=[int(v) for v in raw["somo"][i, :k]],
                   multiplicity=k + 1 if rec["status"] in (0, 1) else 0, open_tie=bool(rec["flags"] & PPP_OPEN_TIE))
        out.append(rec)
    return out


def _ionization(raw, B) -> dict:
    """ip, ea, ... from the raw arrays of a 3B-row call: neutral, cation, anion."""
    ok = (raw["status"] == 0).reshape(3, B)
    e = raw["e_state"].reshape(3, B)
    tie = ((raw["flags"] & PPP_OPEN_TIE) != 0).reshape(3, B)
    ip = np.where(ok[0] & ok[1], e[1] - e[0], np.nan)
    ea = np.where(ok[0] & ok[2], e[0] - e[2], np.nan)
    out = dict(ip=ip, ea=ea, fundamental_gap=ip - ea, ip_koopmans=np.where(ok[0], -raw["homo"][:B].astype(np.float64), np.nan),
               ea_koopmans=np.where(ok[0], -raw["lumo"][:B].astype(np.float64), np.nan), open_tie=tie.any(0),
               status=raw["status"].reshape(3, B).copy())
    if "diis_error" in raw:
        out.update(diis_error=raw["diis_error"].reshape(3, B).copy(), n_extrapolated=raw["n_extrapolated"].reshape(3, B).copy())
    return out


def ionization(molecules, dataset="cata", charge=0, parameters=None, repulsion="mataga-nishimoto", damping=0.25, engine=None, scf="damped", diis_size=6, diis_start=3) -> dict:
    """Delta-SCF ionisation potential and electron affinity at the fixed geometry, in ONE call of 3B rows: every molecule at
    ``charge`` (its "neutral" form), with one electron less and with one more, each at its lowest multiplicity -- so a neutral
    radical works too.  Returns float64 [B] arrays in eV: ``ip`` = e_state(cation) - e_state(neutral), ``ea`` = e_state(neutral) -
    e_state(anion), ``fundamental_gap`` = ip - ea, and the Koopmans values of the neutral form ``ip_koopmans`` = -homo,
    ``ea_koopmans`` = -lumo (for a radical both are read off the half-electron levels); NaN where a state needed is not solved.
    ``open_tie`` bool [B]: one of the three states chose its singly occupied orbital within a degenerate pair (the energies are
    still those of one valid choice).  ``status`` int32 [3, B]: the rows' statuses, neutral / cation / anion.  ``scf``,
    ``diis_size``, ``diis_start``: as ``orbitals`` takes them; with "diis" also ``diis_error`` float32 and ``n_extrapolated`` int32
    [3, B]."""
    molecules = list(molecules)
    B = len(molecules)
    diis = _scf(scf, diis_size, diis_start)
    if not B:
        out = dict({k: np.zeros(0) for k in ("ip", "ea", "fundamental_gap", "ip_koopmans", "ea_koopmans")}, open_tie=np.zeros(0, bool),
                   status=np.zeros((3, 0), np.int32))
        if diis:
            out.update(diis_error=np.zeros((3, 0), np.float32), n_extrapolated=np.zeros((3, 0), np.int32))
        return out
    q = _charges(charge, B)
    q = np.zeros(B, np.int32) if q is None else q
    raw, _, _ = _raw_open(molecules * 3, dataset, np.concatenate([q, q + 1, q - 1]).astype(np.int32), 0, parameters, repulsion, damping,
                          engine, scf, diis_size, diis_start)
    return _ionization(raw, B)


def triplet(molecules, dataset="cata", charge=0, parameters=None, repulsion="mataga-nishimoto", damping=0.25, engine=None, scf="damped", diis_size=6, diis_start=3) -> dict:
    """The delta-SCF triplet energy of even-electron molecules in ONE call of 2B rows (singlet, triplet): ``t1`` float64 [B] =
    e_state(triplet) - e_state(singlet) in eV, next to ``optical``'s CIS ``t1``; NaN where either state is not solved (an odd
    electron count among them).  ``open_tie`` bool [B] as ``ionization`` gives it; ``status`` int32 [2, B].  ``scf``, ``diis_size``,
    ``diis_start``: as ``orbitals`` takes them; with "diis" also ``diis_error`` float32 and ``n_extrapolated`` int32 [2, B]."""
    molecules = list(molecules)
    B = len(molecules)
    diis = _scf(scf, diis_size, diis_start)
    if not B:
        out = dict(t1=np.zeros(0), open_tie=np.zeros(0, bool), status=np.zeros((2, 0), np.int32))
        if diis:
            out.update(diis_error=np.zeros((2, 0), np.float32), n_extrapolated=np.zeros((2, 0), np.int32))
        return out
    q = _charges(charge, B)
    q = np.zeros(B, np.int32) if q is None else q
    raw, _, _ = _raw_open(molecules * 2, dataset, np.concatenate([q, q]).astype(np.int32),
                          np.concatenate([np.ones(B, np.int32), np.full(B, 3, np.int32)]), parameters, repulsion, damping, engine,
                          scf, diis_size, diis_start)
    ok = (raw["status"] == 0).reshape(2, B)
    e = raw["e_state"].reshape(2, B)
    out = dict(t1=np.where(ok[0] & ok[1], e[1] - e[0], np.nan), open_tie=((raw["flags"] & PPP_OPEN_TIE) != 0).reshape(2, B).any(0),
               status=raw["status"].reshape(2, B).copy())
    if diis:
        out.update(diis_error=raw["diis_error"].reshape(2, B).copy(), n_extrapolated=raw["n_extrapolated"].reshape(2, B).copy())
    return out


def dscf_fields(molecules, dataset="cata", engine=None, scf="damped") -> dict:
    """What the keyword ppp_dscf=True adds: {"ppp_ip_dscf", "ppp_ea_dscf"} float64 [B] (``ionization``'s ip and ea, NaN where not
    solved) and "ppp_dscf_status" int [B], the largest of the three states' statuses (0: all solved)."""
    ion = ionization(molecules, dataset, engine=engine, scf=scf)
    return dict(ppp_ip_dscf=ion["ip"], ppp_ea_dscf=ion["ea"], ppp_dscf_status=ion["status"].max(0) if ion["status"].size else np.zeros(0, np.int32))


def gap(molecules, dataset="cata", charge=0, parameters=None, repulsion="mataga-nishimoto", damping=0.25, engine=None, scf="damped", diis_size=6, diis_start=3) -> np.ndarray:
    """float64 [B]: the HOMO-LUMO gap in eV, NaN where the status is not 0.  ``scf``, ``diis_size``, ``diis_start``: as ``orbitals``
    takes them."""
    return frontier(molecules, dataset, charge, parameters, repulsion, damping, engine, scf, diis_size, diis_start)["gap"]


def frontier(molecules, dataset="cata", charge=0, parameters=None, repulsion="mataga-nishimoto", damping=0.25, engine=None, scf="damped", diis_size=6, diis_start=3) -> dict:
    """One call -> {"gap", "ip", "ea"}: float64 [B] in eV (ip = -homo, ea = -lumo), NaN where the status is not 0.  ``scf``,
    ``diis_size``, ``diis_start``: as ``orbitals`` takes them; with "diis" also ``diis_error`` float32 and ``n_extrapolated`` int32 [B]."""
    molecules = list(molecules)
    diis = _scf(scf, diis_size, diis_start)
    if not molecules:
        out = dict(gap=np.zeros(0), ip=np.zeros(0), ea=np.zeros(0))
        if diis:
            out.update(diis_error=np.zeros(0, np.float32), n_extrapolated=np.zeros(0, np.int32))
        return out
    raw, _, _ = _raw(molecules, dataset, charge, parameters, repulsion, damping, engine, None, scf, diis_size, diis_start)
    ok = raw["status"] == 0
    out = dict(gap=np.where(ok, raw["gap"].astype(np.float64), np.nan), ip=np.where(ok, -raw["homo"].astype(np.float64), np.nan),
               ea=np.where(ok, -raw["lumo"].astype(np.float64), np.nan))
    if diis:
        out.update(diis_error=raw["diis_error"].copy(), n_extrapolated=raw["n_extrapolated"].copy())
    return out


def _frontier(raw) -> dict:
    ok = _scf_status(raw) == 0
    return dict(gap=np.where(ok, raw["gap"].astype(np.float64), np.nan), ip=np.where(ok, -raw["homo"].astype(np.float64), np.nan),
                ea=np.where(ok, -raw["lumo"].astype(np.float64), np.nan))


def _scf_status(raw) -> np.ndarray:
    """The status gaudi_ppp alone gives: NOT_CONVERGED that only a CIS solve caused is OK."""
    cis_only = (raw["status"] == 1) & ((raw["flags"] & (PPP_SCF_CAP | PPP_JACOBI_CAP)) == 0)
    return np.where(cis_only, 0, raw["status"])


def _optical(raw, f_min) -> dict:
    """s1, t1, s1_f, bright, bright_f, st_gap as float64 [B] from the raw arrays of a gaudi_ppp_cis call."""
    B = len(raw["status"])
    have = (raw["status"] == 0) & (raw["n_states"] > 0)
    pick = lambda a: np.where(have, a.astype(np.float64), np.nan)
    live = np.arange(raw["osc"].shape[1])[None, :] < raw["n_states"][:, None]
    lit = live & (raw["osc"] >= np.float32(f_min)) & have[:, None]
    first = np.where(lit.any(1), lit.argmax(1), 0)
    rows = np.arange(B)
    s1, t1 = pick(raw["singlet"][:, 0]), pick(raw["triplet"][:, 0])
    return dict(s1=s1, t1=t1, s1_f=pick(raw["osc"][:, 0]), bright=np.where(lit.any(1), raw["singlet"][rows, first].astype(np.float64), np.nan),
                bright_f=np.where(lit.any(1), raw["osc"][rows, first].astype(np.float64), np.nan), st_gap=s1 - t1)


def excited_states(molecules, dataset="cata", charge=0, parameters=None, repulsion="mataga-nishimoto", damping=0.25, window=8,
                   engine=None) -> list:
    """``orbitals`` and the CIS stage in one gaudi_ppp_cis call (the SCF launches, then one launch for every molecule).  ``window``:
    the number of highest occupied and of lowest empty levels that take part, 1..8 (anything else: status 6 for every molecule).
    Returns one dict per molecule with every key of ``orbitals`` (``flags`` carries the CIS bits too) and
      n_states       n_active_occ * n_active_virt <= 64; 0 for a molecule without an electron or without an empty level
      singlet, triplet   [n_states] float32, excitation energies in eV, ascending
      osc, dipole    [n_states] oscillator strength and [n_states, 3] transition dipole (e Angstrom) of every singlet
      lead, lead_weight   [n_states, 2] (occupied rank, empty rank) of a singlet's largest configuration and its weight X^2
      s1, t1, s1_f, st_gap = s1 - t1   float, NaN without a state
      cis_sweeps, n_active_occ, n_active_virt
      cis_not_converged  a CIS diagonalisation used all its sweeps (status 1)
      truncated      the window is smaller than the single-excitation space
      window_edge    a level just outside the window within 1e-3 eV of the window's edge: the results depend on how a degenerate
                     pair was oriented
      triplet_unstable   t1 <= 0: the closed-shell ground state is not the lowest state (information, not an error)
    A molecule whose status is not 0 has no states."""
    molecules = list(molecules)
    if not molecules:
        return []
    raw, na, nb = _raw(molecules, dataset, charge, parameters, repulsion, damping, engine, window)
    opt = _optical(raw, 0.0)
    out = []
    for i in range(len(na)):
        rec = _orbital_record(raw, i, na, nb)
        k, flags = int(raw["n_states"][i]), rec["flags"]
        rec.update({name: raw[name][i, :k].copy() for name in ("singlet", "triplet", "osc", "dipole", "lead", "lead_weight")})
        rec.update({name: int(raw[name][i]) for name in ("n_states", "n_active_occ", "n_active_virt", "cis_sweeps")})
        rec.update({name: float(opt[name][i]) for name in ("s1", "t1", "s1_f", "st_gap")})
        rec.update(cis_not_converged=bool(flags & PPP_CIS_JACOBI_CAP), truncated=bool(flags & PPP_CIS_TRUNCATED),
                   window_edge=bool(flags & PPP_CIS_WINDOW_EDGE), triplet_unstable=bool(flags & PPP_CIS_TRIPLET_UNSTABLE))
        out.append(rec)
    return out


def optical(molecules, dataset="cata", charge=0, parameters=None, repulsion="mataga-nishimoto", damping=0.25, window=8, engine=None,
            f_min=0.01) -> dict:
    """One gaudi_ppp_cis call -> {"s1", "t1", "s1_f", "bright", "bright_f", "st_gap"}: float64 [B], energies in eV.  ``bright`` is
    the lowest singlet with an oscillator strength of at least ``f_min`` (the optical gap) and ``bright_f`` its strength; NaN where
    the status is not 0, there is no state, or no singlet is that bright."""
    molecules = list(molecules)
    if not molecules:
        return {k: np.zeros(0) for k in ("s1", "t1", "s1_f", "bright", "bright_f", "st_gap")}
    raw, _, _ = _raw(molecules, dataset, charge, parameters, repulsion, damping, engine, window)
    return _optical(raw, f_min)


def spectrum(states, grid_ev, width=0.3) -> np.ndarray:
    """The absorption line shape of one ``excited_states`` record (or a list of them: their sum) on ``grid_ev``: every singlet a
    normalised Gaussian of standard deviation ``width`` eV weighted by its oscillator strength.  Plain numpy on the host."""
    grid = np.asarray(grid_ev, np.float64)
    out = np.zeros(grid.shape, np.float64)
    for rec in [states] if isinstance(states, dict) else list(states):
        e, f = np.asarray(rec["singlet"], np.float64), np.asarray(rec["osc"], np.float64)
        if len(e):
            out += (f * np.exp(-0.5 * ((grid[..., None] - e) / width) ** 2)).sum(-1) / (width * np.sqrt(2.0 * np.pi))
    return out


def summary_fields(molecules, dataset="cata", engine=None, ppp=False, ppp_cis=True, scf="damped") -> dict:
    """What design(..., ppp_cis=True) adds: {"ppp_s1", "ppp_t1", "ppp_bright"} float64 [B]; with ``ppp`` also ``frontier``'s
    ppp_gap / ppp_ip / ppp_ea from the same call -- or with scf="diis" from a gaudi_ppp_scf call of their own (the CIS stage takes
    the damped ground state only)."""
    molecules = list(molecules)
    raw = None
    diis = _scf(scf, 6, 3) and ppp
    if molecules and (ppp_cis or not diis):
        raw, _, _ = _raw(molecules, dataset, 0, None, "mataga-nishimoto", 0.25, engine, 8 if ppp_cis else None)
    out = {}
    if ppp:
        if diis:
            front = {k: v for k, v in frontier(molecules, dataset, engine=engine, scf=scf).items() if k in ("gap", "ip", "ea")}
        else:
            front = _frontier(raw) if molecules else dict(gap=np.zeros(0), ip=np.zeros(0), ea=np.zeros(0))
        out.update({"ppp_" + k: v for k, v in front.items()})
    if ppp_cis:
        opt = _optical(raw, 0.01) if molecules else {k: np.zeros(0) for k in ("s1", "t1", "bright")}
        out.update({"ppp_" + k: opt[k] for k in ("s1", "t1", "bright")})
    return out


def record_fields(molecules, dataset="cata", engine=None, ppp=True, ppp_cis=False, scf="damped") -> list:
    """What rings_to_atoms(..., ppp=True) adds to every record -- ppp_gap, ppp_homo, ppp_lumo, ppp_flags, ppp_status -- and / or
    what ppp_cis=True adds -- ppp_s1, ppp_t1, ppp_s1_f, ppp_bright (eV; NaN without a solved state) and ppp_cis_flags; asked for
    together, one gaudi_ppp_cis call serves both.  scf="diis": the first five come from a gaudi_ppp_scf call (the CIS stage takes
    the damped ground state only, in a call of its own)."""
    molecules = list(molecules)
    if not molecules:
        return []
    diis = _scf(scf, 6, 3) and ppp
    raw = None
    if ppp_cis or not diis:
        raw, _, _ = _raw(molecules, dataset, 0, None, "mataga-nishimoto", 0.25, engine, 8 if ppp_cis else None)
    out = [{} for _ in molecules]
    if ppp:
        ground = _raw(molecules, dataset, 0, None, "mataga-nishimoto", 0.25, engine, None, scf)[0] if diis else raw
        status = _scf_status(ground)
        for i, rec in enumerate(out):
            rec.update(ppp_gap=float(ground["gap"][i]), ppp_homo=float(ground["homo"][i]), ppp_lumo=float(ground["lumo"][i]),
                       ppp_flags=int(ground["flags"][i]) & ~PPP_CIS_FLAGS, ppp_status=int(status[i]))
    if ppp_cis:
        opt = _optical(raw, 0.01)
        for i, rec in enumerate(out):
            rec.update(ppp_s1=float(opt["s1"][i]), ppp_t1=float(opt["t1"][i]), ppp_s1_f=float(opt["s1_f"][i]),
                       ppp_bright=float(opt["bright"][i]), ppp_cis_flags=int(raw["flags"][i]) & PPP_CIS_FLAGS)
    return out
