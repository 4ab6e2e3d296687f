"""Host mirror of data/gor2goa.py: a graph of rings -> a graph of atoms, on top of gaudi_rings_to_atoms.

``gor2goa(x, rings_types, dataset, tol)`` has the reference's signature and return for one molecule; ``rings_to_atoms`` is the
batched form: every molecule of a call is converted in ONE kernel launch (one wavefront per molecule), with optional hydrogen
placement and an optional 64-bit fingerprint of the heavy-atom graph.  ``write_xyz`` / ``write_molfile`` are host code.  The
constants (ring templates, RINGS_DICT, ATOMS_LIST, ...) ship as data in ``gaudi_amd/data/ring_tables.json`` under "goa".

``bond_orders`` (and ``rings_to_atoms(..., bond_orders=True)``) is the valence check the reference gets from xyz2mol.AC2BO inside
rdkit_valid (gor2goa.py:298-324): bond orders 1 / 2 and formal charges from elements and connectivity alone, on the device
(gaudi_bond_orders, one wavefront per molecule); the rule is stated in DESIGN.md section 8h.  "Built" means gor2goa did not raise;
"valid" means built and ``kekule_status == 0``.

``canonical`` (and ``rings_to_atoms(..., canonical=True)``) numbers the heavy atoms canonically on the device
(gaudi_canonical_order, one wavefront per molecule): ``canon_key`` is equal for two molecules if and only
if their graphs of atoms are isomorphic, which is what the reference uses the InChI string for when it counts molecules.
``canonical_molecule`` rebuilds the molecule in that numbering, and ``smiles`` / ``write_smiles`` write it as Kekule SMILES.

What is NOT here: RDKit itself -- its sanitiser after AC2BO, ResonanceMolSupplier's single-structure condition (AC2mol) and InChI
strings (gor2goa.py:264-324).  The fingerprint is a hash: equal fingerprints do not prove that two molecules are isomorphic; equal
``canon_key`` values do.  There is no CPU implementation behind these functions: without the HIP library they raise GaudiError."""
from __future__ import annotations

import re

import numpy as np

from ._lib import (ATOMS_FINGERPRINT, ATOMS_MAX_ATOMS, ATOMS_MAX_BONDS, ATOMS_PLACE_H, BONDS_EMPTY, CANON_GAVE_UP, CANON_OK,
                   AtomTables, GaudiError, ValenceTables)
from .analyze import _engine, _key, _np, _pack, c_tables, ring_tables

STATUS_NAMES = {0: "built", 1: "a ring without a fused neighbour in a multi-ring molecule",
                2: "the orientation type or a type outside the table among the rings", 3: "no rings",
                4: "more atoms, bonds or fused pairs than the kernel holds"}
KEKULE_STATUS_NAMES = {0: "a structure with at most 4 charged atoms", 1: "no structure with up to 6 charged atoms",
                       2: "no structure within 4 charged atoms, but one with 5 or 6",
                       3: "the bond graph is not connected", 4: "an atom whose bonds exceed every allowed valence",
                       5: "a bond index outside the atom list, a repeated bond or an element outside the table",
                       6: "more than 384 atoms, 192 heavy atoms or 384 bonds", 7: "no atoms (not built)",
                       8: "undecided: the subset search gave up (more than 25 atoms with two options; may depend on the numbering)"}
CANON_STATUS_NAMES = {0: "canonical", 1: "gave up (more than 4096 search-tree nodes or 16 levels): a valid numbering, not canonical",
                      2: "a bond index outside the atom list, a repeated bond or an element outside the table",
                      3: "more than 384 atoms, 192 heavy atoms or 384 bonds, or an atom with more than 8 bonds", 4: "no atoms (not built)"}


def atoms_list(dataset: str):
    """ATOMS_LIST[dataset] (data/aromatic_dataloader.py:26-30)."""
    return ring_tables()["goa"]["atoms"][_key(dataset)]


def c_atom_tables(dataset: str) -> AtomTables:
    """gaudi_atom_tables for one dataset."""
    ds = _key(dataset)
    T = ring_tables()
    G = T["goa"]
    rings, atoms = T["rings"][ds], G["atoms"][ds]
    t = AtomTables()
    t.n_types = len(rings)
    for i, sym in enumerate(rings):
        if sym not in G["ring_atoms"]:  # the orientation type "."
            continue
        elems, templ = G["ring_atoms"][sym], G["templates"][G["ring_template"][sym]]
        if len(elems) != len(templ):
            raise GaudiError(f"ring {sym}: {len(elems)} elements but a template of {len(templ)} points")
        if any(e not in atoms for e in elems):
            continue  # a ring of another dataset's elements never appears in this one
        t.ring_size[i] = len(elems)
        for k, (e, p) in enumerate(zip(elems, templ)):
            t.ring_elem[i][k] = atoms.index(e)
            t.templ[i][k][0], t.templ[i][k][1] = p
        t.no_orientation[i] = int(sym in G["no_orientation"])
        t.extra_angle[i] = float(G["extra_angle"].get(sym, 0.0))
        parents = G["template_h"].get(sym, [])
        t.n_template_h[i] = len(parents)
        for q, a in enumerate(parents):
            t.template_h_parent[i][q] = a
    t.h_elem, t.c_elem = atoms.index("H"), atoms.index("C")
    t.h_bond = float(G["h_bond"])
    return t


def c_valence_tables(dataset: str) -> ValenceTables:
    """gaudi_valence_tables for one dataset: the "valence" section of ring_tables.json in the order of ATOMS_LIST[dataset]."""
    atoms = atoms_list(dataset)
    V = ring_tables()["valence"]
    t = ValenceTables()
    t.n_elems = len(atoms)
    for e, sym in enumerate(atoms):
        for d, opts in enumerate(V["options"][sym]):
            t.n_options[e][d] = len(opts)
            for k, (added, charge) in enumerate(opts):
                t.option[e][d][k][0], t.option[e][d][k][1] = added, charge
    t.h_elem, t.c_elem = atoms.index("H"), atoms.index("C")
    return t


def _pack_atoms(molecules):
    """Records or (atom_types, bonds) pairs -> elem [B,A], n_atoms [B], bonds [B,M,2], n_bonds [B] (int32, zero padded)."""
    mols = []
    for mol in molecules:
        if isinstance(mol, dict):
            built = mol["status"] == 0
            mol = (mol["atom_types"], mol["bonds"]) if built else ((), ())
        mols.append((np.asarray(_np(mol[0]), np.int32).reshape(-1), np.asarray(_np(mol[1]), np.int32).reshape(-1, 2)))
    B = len(mols)
    A, M = max(1, max(len(t) for t, _ in mols)), max(1, max(len(b) for _, b in mols))
    elem, bonds = np.zeros((B, A), np.int32), np.zeros((B, M, 2), np.int32)
    na, nb = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for i, (t, b) in enumerate(mols):
        elem[i, :len(t)], bonds[i, :len(b)], na[i], nb[i] = t, b, len(t), len(b)
    return elem, na, bonds, nb


def bond_orders(molecules, dataset="cata", engine=None):
    """Bond orders and formal charges for a batch in one launch.  ``molecules``: a list of records from rings_to_atoms or of
    ``(atom_types [n], bonds [m,2])`` pairs, with or without placed hydrogens (a carbon with two bonds counts the H the reference
    would add).  Returns one dict per molecule:
      kekule_status  0 = a structure was found (KEKULE_STATUS_NAMES); otherwise the arrays below are zero
      orders         [m] 1 or 2 per bond;  charges: [n] formal charge per atom;  n_charged: atoms with a nonzero charge -- the
                     fewest any structure of the molecule has (0: a neutral Kekule structure)
    A record whose ``status != 0`` (not built) yields kekule_status 7 (EMPTY).  kekule_status 8 (GAVE_UP) is no verdict: the
    bounded subset search ran out (possible only with more than 25 atoms that have two options), a structure may exist, and
    another atom numbering may find it -- every other status and n_charged do not depend on the numbering."""
    molecules = list(molecules)
    if not molecules:
        return []
    elem, na, bonds, nb = _pack_atoms(molecules)
    B = len(na)
    raw = _engine(engine).bond_orders(c_valence_tables(dataset), elem, na, bonds, nb)
    return [dict(kekule_status=int(raw["status"][i]), orders=raw["order"][i, :nb[i]].astype(np.int64),
                 charges=raw["charge"][i, :na[i]].astype(np.int64), n_charged=int(raw["n_charged"][i])) for i in range(B)]


_bond_orders = bond_orders  # (rings_to_atoms has a parameter of that name)


def _is_packed(molecules) -> bool:
    """(x [B,N,3], ring_type [B,N], n_nodes [B]) rather than a list of (positions, ring_type) pairs: three entries that are
    arrays (not pairs themselves) of 3, 2 and 1 dimensions."""
    if not isinstance(molecules, (tuple, list)) or len(molecules) != 3 or any(isinstance(m, (tuple, list)) for m in molecules):
        return False
    return [np.ndim(_np(m)) for m in molecules] == [3, 2, 1]


def rings_to_atoms(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None, bond_orders=False,
                   canonical=False, huckel=False, ppp=False, ppp_cis=False, aromaticity=False, ring_currents=False, reactivity=False,
                   ppp_dscf=False, ppp_scf="damped"):
    """gor2goa for a batch in one launch.  ``molecules``: a list of ``(positions [n,3], ring_type [n] or one-hot [n,R])`` pairs as
    analyze_validity_for_molecules takes them, or packed arrays ``(x [B,N,3], ring_type [B,N], n_nodes [B])`` with every
    molecule's valid nodes first.  For datasets other than "cata" the second half of a molecule's nodes are its orientation nodes.

    Returns one record (dict) per molecule:
      status       0 = built; otherwise the reference raises for this input (STATUS_NAMES) and the arrays below are empty
      atoms        [n,2] float64, the aligned frame: what the reference returns
      atoms3d      [n,3] float64, the same points lifted back into the input frame
      atom_types   [n] indices into ATOMS_LIST[dataset];  bonds: [m,2], each pair i <= j, the list sorted
      fingerprint  int (0 unless asked for): equal for isomorphic heavy-atom graphs; equal keys do NOT prove isomorphism
    place_hydrogens: template H's leave the origin and every carbon with two heavy neighbours gets an H (appended after all other
    atoms in ascending parent index), 1.09 A out on the bisector in the molecular plane -- a complete structure.
    bond_orders: a second launch (gaudi_bond_orders) adds kekule_status, orders, charges and n_charged to every record.
    canonical: a launch of gaudi_canonical_order adds canon_status, canon_rank, canon_key and canon_nodes (see ``canonical``);
    with bond_orders one further gaudi_bond_orders launch, on canonical_molecule's arrays, adds canon_kekule_status,
    canon_orders, canon_charges and canon_n_charged: the structure of the molecule in its canonical numbering, the same for
    every numbering of the input (empty / EMPTY for a molecule without a numbering).  The other keys are left as they are.
    huckel: a call of gaudi_huckel (gaudi_amd.huckel) adds huckel_gap, huckel_homo, huckel_lumo (|beta|),
    huckel_flags and huckel_status (gaudi_amd.huckel.STATUS_NAMES; 4 for a molecule that was not built) to every record.
    ppp: a call of gaudi_ppp (gaudi_amd.ppp) on the records' atoms3d adds ppp_gap, ppp_homo, ppp_lumo (eV),
    ppp_flags and ppp_status (gaudi_amd.ppp.STATUS_NAMES; 4 for a molecule that was not built) to every record.
    ppp_cis: a call of gaudi_ppp_cis (gaudi_amd.ppp.excited_states; window 8) adds ppp_s1, ppp_t1 (the lowest
    singlet and triplet excitation energies, eV), ppp_s1_f (the oscillator strength of S1), ppp_bright (the lowest singlet with
    f >= 0.01) -- NaN where nothing was solved -- and ppp_cis_flags (the GAUDI_PPP_CIS_* bits).  With ppp as well, the one call
    serves both.
    aromaticity: a launch of gaudi_kekule (gaudi_amd.aromaticity) adds kekule_count (the number of Kekule
    structures), clar, fries, max_pauling_order (the largest double_count / kekule_count of a bond; NaN where nothing was counted)
    and resonance_status (gaudi_amd.aromaticity.STATUS_NAMES; 7 for a molecule that was not built) to every record.
    ring_currents: a call of gaudi_ring_currents (gaudi_amd.aromaticity.ring_currents) on the records' atoms3d
    adds ring_current_max, ring_current_min (the extreme Hueckel-London ring currents in units of benzene's; NaN where nothing was
    solved, 0.0 without a ring) and ring_current_status (gaudi_amd.aromaticity.RING_CURRENT_STATUS_NAMES; 4 for a molecule that was
    not built) to every record.  With ring_currents=False nothing changes and no launch is made.
    reactivity: a call of gaudi_reactivity (gaudi_amd.reactivity; no ortho solves) adds
    min_atom_localization (the smallest radical localization energy over the pi centres that carry a hydrogen), min_para_localization
    (the smallest para-localization energy over the six-rings), both in |beta| and NaN where nothing was solved or nothing of the
    kind exists, and reactivity_status (gaudi_amd.reactivity.STATUS_NAMES; 4 for a molecule that was not built) to every record.
    With reactivity=False nothing changes and no launch is made.
    ppp_dscf: a call of gaudi_ppp_open (gaudi_amd.ppp.ionization; three rows per molecule: neutral, cation,
    anion) on the records' atoms3d adds ppp_ip_dscf and ppp_ea_dscf (the delta-SCF ionisation potential and electron affinity in eV,
    NaN where a state was not solved) and ppp_dscf_status (the largest status of the three states, gaudi_amd.ppp.STATUS_NAMES; 4 for
    a molecule that was not built) to every record.  With ppp_dscf=False nothing changes and no launch is made.
    ppp_scf: "damped" (the default: what it was) or "diis" -- the calls that ppp=True and ppp_dscf=True make go to gaudi_ppp_scf
    (Pulay's DIIS) instead; the keys they add are the same.  It launches nothing by itself."""
    if _is_packed(molecules):
        X = np.ascontiguousarray(_np(molecules[0]), dtype=np.float32)
        B, N = X.shape[0], X.shape[1]
        T = np.ascontiguousarray(_np(molecules[1]), dtype=np.int32).reshape(B, N)
        nn = np.ascontiguousarray(_np(molecules[2]), dtype=np.int32).reshape(B)
        if B == 0:
            return []
    else:
        molecules = list(molecules)
        if not molecules:
            return []
        X, T, nn = _pack(molecules)
    eng = _engine(engine)
    orient = dataset != "cata"
    max_rings = int((nn // 2 if orient else nn).max())
    max_atoms = int(min(ATOMS_MAX_ATOMS, max(1, max_rings) * (12 if place_hydrogens else 8)))
    max_bonds = int(min(ATOMS_MAX_BONDS, max_atoms))
    flags = (ATOMS_PLACE_H if place_hydrogens else 0) | (ATOMS_FINGERPRINT if fingerprint else 0)
    raw = eng.rings_to_atoms(c_tables(dataset, tol), c_atom_tables(dataset), X, T, nn, flags, max_atoms, max_bonds)
    out = []
    for b in range(X.shape[0]):
        na, nb = int(raw["n_atoms"][b]), int(raw["n_bonds"][b])
        out.append(dict(status=int(raw["status"][b]), atoms=raw["xy"][b, :na].copy(), atoms3d=raw["xyz"][b, :na].copy(),
                        atom_types=raw["atom_type"][b, :na].astype(np.int64), bonds=raw["bonds"][b, :nb].astype(np.int64),
                        fingerprint=int(raw["fingerprint"][b])))
    if bond_orders:
        for rec, extra in zip(out, _bond_orders(out, dataset, engine=eng)):
            rec.update(extra)
    if canonical:
        extras, codes = _canonical_raw(out, dataset, eng)
        for rec, extra in zip(out, extras):
            rec.update(extra)
        if bond_orders:
            mols = [_molecule_from_code(c, dataset) if c is not None else ((), ()) for c in codes]
            for rec, extra in zip(out, _bond_orders(mols, dataset, engine=eng)):
                rec.update({"canon_" + k: v for k, v in extra.items()})
    if huckel:
        from .huckel import record_fields
        for rec, extra in zip(out, record_fields(out, dataset, engine=eng)):
            rec.update(extra)
    if ppp or ppp_cis:
        from .ppp import record_fields as ppp_fields
        for rec, extra in zip(out, ppp_fields(out, dataset, engine=eng, scf=ppp_scf, **({"ppp": bool(ppp), "ppp_cis": True} if ppp_cis else {}))):
            rec.update(extra)
    if aromaticity:
        from .aromaticity import record_fields as resonance_fields
        for rec, extra in zip(out, resonance_fields(out, dataset, engine=eng)):
            rec.update(extra)
    if ring_currents:
        from .aromaticity import ring_current_fields
        for rec, extra in zip(out, ring_current_fields(out, dataset, engine=eng)):
            rec.update(extra)
    if reactivity:
        from .reactivity import record_fields as reactivity_fields
        for rec, extra in zip(out, reactivity_fields(out, dataset, engine=eng)):
            rec.update(extra)
    if ppp_dscf:
        from .ppp import dscf_fields
        extra = dscf_fields(out, dataset, engine=eng, scf=ppp_scf)
        for i, rec in enumerate(out):
            rec.update(ppp_ip_dscf=float(extra["ppp_ip_dscf"][i]), ppp_ea_dscf=float(extra["ppp_ea_dscf"][i]),
                       ppp_dscf_status=int(extra["ppp_dscf_status"][i]))
    return out


def gor2goa(x, rings_types, dataset="cata", tol=0.1, engine=None):
    """data/gor2goa.py:133-261 for one molecule -> (atoms [n,2] float64, atoms_types [n] int64, bonds: list of (i, j) tuples,
    i <= j, sorted -- the reference returns them in set order).  Raises GaudiError where the reference raises."""
    rec = rings_to_atoms([(x, rings_types)], dataset, tol, engine=engine)[0]
    if rec["status"]:
        raise GaudiError(f"gor2goa: {STATUS_NAMES.get(rec['status'], rec['status'])} (the reference raises here)")
    atoms, types, bonds = rec["atoms"], rec["atom_types"], [tuple(int(v) for v in p) for p in rec["bonds"]]
    try:
        import torch
        return torch.from_numpy(atoms), torch.from_numpy(types), bonds
    except ImportError:
        return atoms, types, bonds


def _symbols(atom_types, dataset):
    names = atoms_list(dataset)
    return [names[int(t)] for t in atom_types]


def _open(path_or_file):
    return (path_or_file, False) if hasattr(path_or_file, "write") else (open(path_or_file, "w"), True)


def write_xyz(path_or_file, atoms3d, atom_types, dataset="cata", comment=""):
    """XYZ file of one molecule: atoms3d [n,3] (2-D coordinates get z = 0), atom_types as indices into ATOMS_LIST[dataset]."""
    xyz = np.asarray(_np(atoms3d), np.float64)
    if xyz.ndim != 2 or xyz.shape[1] not in (2, 3) or len(xyz) != len(atom_types):
        raise GaudiError(f"write_xyz: {xyz.shape} coordinates for {len(atom_types)} atoms")
    if xyz.shape[1] == 2:
        xyz = np.concatenate([xyz, np.zeros((len(xyz), 1))], 1)
    f, close = _open(path_or_file)
    try:
        f.write(f"{len(xyz)}\n{str(comment).splitlines()[0] if comment else ''}\n")
        for sym, p in zip(_symbols(atom_types, dataset), xyz):
            f.write(f"{sym:<2s} {p[0]:14.8f} {p[1]:14.8f} {p[2]:14.8f}\n")
    finally:
        if close:
            f.close()


def write_molfile(path_or_file, atoms3d, atom_types, bonds, dataset="cata", comment="", orders=None, charges=None):
    """V2000 molfile of one molecule: bond type 4 (aromatic) between heavy atoms, 1 (single) to hydrogen -- the bond orders
    build_molecule_aromatic gives them (data/gor2goa.py:282-286).  With ``orders`` (one per bond, from bond_orders) the bond types
    are those, 1 / 2: a Kekule structure; ``charges`` (one per atom) become ``M  CHG`` lines, 8 entries each."""
    xyz = np.asarray(_np(atoms3d), np.float64)
    if xyz.ndim != 2 or xyz.shape[1] not in (2, 3) or len(xyz) != len(atom_types):
        raise GaudiError(f"write_molfile: {xyz.shape} coordinates for {len(atom_types)} atoms")
    if xyz.shape[1] == 2:
        xyz = np.concatenate([xyz, np.zeros((len(xyz), 1))], 1)
    bonds = np.asarray(_np(bonds), np.int64).reshape(-1, 2)
    if len(xyz) > 999 or len(bonds) > 999:
        raise GaudiError("write_molfile: a V2000 counts line holds at most 999 atoms and bonds")
    if len(bonds) and (bonds.min() < 0 or bonds.max() >= len(xyz)):
        raise GaudiError("write_molfile: bond index outside the atom list")
    sym = _symbols(atom_types, dataset)
    if orders is not None:
        orders = np.asarray(_np(orders), np.int64).reshape(-1)
        if len(orders) != len(bonds) or (len(orders) and (orders.min() < 1 or orders.max() > 3)):
            raise GaudiError(f"write_molfile: {len(orders)} bond orders in 1..3 wanted for {len(bonds)} bonds")
    charged = []
    if charges is not None:
        charges = np.asarray(_np(charges), np.int64).reshape(-1)
        if len(charges) != len(xyz):
            raise GaudiError(f"write_molfile: {len(charges)} charges for {len(xyz)} atoms")
        charged = [(a + 1, int(q)) for a, q in enumerate(charges) if q]
    f, close = _open(path_or_file)
    try:
        f.write(f"{str(comment).splitlines()[0] if comment else ''}\n  gaudi_amd\n\n")
        f.write(f"{len(xyz):3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000\n")
        for s, p in zip(sym, xyz):
            f.write(f"{p[0]:10.4f}{p[1]:10.4f}{p[2]:10.4f} {s:<3s} 0  0  0  0  0  0  0  0  0  0  0  0\n")
        for k, (i, j) in enumerate(bonds):
            order = int(orders[k]) if orders is not None else 1 if "H" in (sym[i], sym[j]) else 4
            f.write(f"{i + 1:3d}{j + 1:3d}{order:3d}  0\n")
        for k in range(0, len(charged), 8):
            row = charged[k:k + 8]
            f.write(f"M  CHG{len(row):3d}" + "".join(f"{a:4d}{q:4d}" for a, q in row) + "\n")
        f.write("M  END\n")
    finally:
        if close:
            f.close()


def canon_code(raw, i) -> bytes:
    """The code of molecule i of a raw gaudi_canonical_order result: n_heavy (int32), the labels in rank order (uint8 each,
    element * 8 + H count), the heavy-atom bonds as sorted (lo, hi) rank pairs (uint16 each), little-endian."""
    H, E = int(raw["n_heavy"][i]), int(raw["n_hbonds"][i])
    return np.array([H], "<i4").tobytes() + raw["label"][i, :H].tobytes() + raw["cbonds"][i, :E].astype("<u2").tobytes()


def _canonical_raw(molecules, dataset, engine):
    """-> (per-molecule dicts of canonical(), codes): the code of every molecule that has a numbering (OK or GAVE_UP), else None."""
    atoms = atoms_list(dataset)
    elem, na, bonds, nb = _pack_atoms(molecules)
    raw = _engine(engine).canonical_order(len(atoms), atoms.index("H"), atoms.index("C"), elem, na, bonds, nb)
    out, codes = [], []
    for i in range(len(na)):
        st = int(raw["status"][i])
        code = canon_code(raw, i) if st in (CANON_OK, CANON_GAVE_UP) else None
        codes.append(code)
        out.append(dict(canon_status=st, canon_rank=raw["rank"][i, :na[i]].astype(np.int64), canon_key=code if st == CANON_OK else None,
                        canon_nodes=int(raw["nodes"][i])))
    return out, codes


def canonical(molecules, dataset="cata", engine=None):
    """Canonical numbering of the heavy atoms for a batch in one launch.  ``molecules``: as bond_orders takes them.  Returns one
    dict per molecule:
      canon_status  0 = canonical (CANON_STATUS_NAMES); 1 = gave up: canon_rank is a valid numbering, but may differ under
                    renumbering (more than 4096 search-tree nodes: several identical disconnected pieces); above 1 the input was
                    refused and canon_rank is zero
      canon_rank    [n] the canonical index of every heavy atom, -1 for hydrogens
      canon_key     bytes (canon_code: n_heavy, the (element, H count) labels in rank order, the heavy-atom bonds as sorted rank
                    pairs), or None unless canon_status == 0.  Equal keys <=> isomorphic graphs of atoms, hydrogens placed or not
      canon_nodes   search-tree nodes spent"""
    molecules = list(molecules)
    return _canonical_raw(molecules, dataset, engine)[0] if molecules else []


def _molecule_from_code(code: bytes, dataset):
    atoms = atoms_list(dataset)
    H = int(np.frombuffer(code[:4], "<i4")[0])
    label = np.frombuffer(code[4:4 + H], np.uint8).astype(np.int64)
    heavy = np.frombuffer(code[4 + H:], "<u2").astype(np.int64).reshape(-1, 2)
    n_h = label & 7
    parents = np.repeat(np.arange(H, dtype=np.int64), n_h)
    types = np.concatenate([label >> 3, np.full(len(parents), atoms.index("H"), np.int64)])
    bonds = np.concatenate([heavy, np.stack([parents, H + np.arange(len(parents), dtype=np.int64)], 1)]).reshape(-1, 2)
    return types, bonds[np.lexsort((bonds[:, 1], bonds[:, 0]))]


def canonical_molecule(record_or_pair, dataset="cata", engine=None):
    """The molecule in its canonical numbering -> (atom_types [n], bonds [m,2]): the heavy atoms in rank order, then every
    hydrogen -- the listed ones and the one a carbon with two bonds implies -- in ascending parent rank; bonds as i <= j pairs,
    the list sorted.  Isomorphic inputs give identical arrays, so bond_orders on them is a function of the molecule and not of
    its numbering (unless either stage gave up).  A record that carries ``canon_key`` is decoded on the host; anything else takes
    one gaudi_canonical_order launch.  Raises GaudiError for a molecule without a numbering."""
    if isinstance(record_or_pair, dict) and record_or_pair.get("canon_key") is not None:
        return _molecule_from_code(record_or_pair["canon_key"], dataset)
    out, codes = _canonical_raw([record_or_pair], dataset, engine)
    if codes[0] is None:
        raise GaudiError(f"canonical_molecule: {CANON_STATUS_NAMES.get(out[0]['canon_status'], out[0]['canon_status'])}")
    return _molecule_from_code(codes[0], dataset)


_SMILES_VALENCES = {"B": (3,), "C": (4,), "N": (3, 5), "O": (2,), "S": (2, 4, 6)}


def _smiles_atom(sym, n_h, charge, order_sum):
    """Bare inside the organic subset when neutral and the H count is the implied one, else a bracket atom."""
    if charge == 0 and sym in _SMILES_VALENCES:
        fit = [v for v in _SMILES_VALENCES[sym] if v >= order_sum]
        if n_h == (fit[0] - order_sum if fit else 0):
            return sym
    q = "" if charge == 0 else ("+" if charge > 0 else "-") + (str(abs(charge)) if abs(charge) > 1 else "")
    return "[" + sym + ("" if n_h == 0 else "H" if n_h == 1 else f"H{n_h}") + q + "]"


def smiles(record, dataset="cata"):
    """Kekule SMILES of a record from rings_to_atoms(..., canonical=True, bond_orders=True), or None unless
    ``canon_status == 0 and canon_kekule_status == 0``.  Host formatting, as write_molfile.  The string is a function of the
    molecule: components joined by ".", each started at its lowest canonical rank; depth first, neighbours in ascending rank, all
    but the last child in parentheses; the other bonds are ring closures with the lowest number free when the earlier atom is
    written (a number closed at an atom is free again from the next atom on; 10..99 as %nn); "=" before the child atom or the
    closing digit, single bonds never written; upper-case symbols; an atom is bare (B C N O S) when it is neutral and its H count
    is the one the organic subset implies for the sum of its written bond orders, else bracketed."""
    if record.get("canon_status") != CANON_OK or record.get("canon_kekule_status") != 0 or record.get("canon_key") is None:
        return None
    names = atoms_list(dataset)
    types, bonds = _molecule_from_code(record["canon_key"], dataset)
    orders, charges = np.asarray(record["canon_orders"], np.int64), np.asarray(record["canon_charges"], np.int64)
    h_type = names.index("H")
    H = int((types != h_type).sum())
    if charges[H:].any():
        raise GaudiError("smiles: a charged hydrogen")
    adj = [dict() for _ in range(H)]
    n_h = np.zeros(H, np.int64)
    for (i, j), o in zip(bonds, orders):
        if j >= H:
            n_h[i] += 1
        else:
            adj[i][int(j)] = int(o)
            adj[j][int(i)] = int(o)
    order, children, closes, opens = {}, [[] for _ in range(H)], [[] for _ in range(H)], [[] for _ in range(H)]
    roots = []
    for root in range(H):
        if root in order:
            continue
        roots.append(root)
        order[root] = len(order)
        stack = [(root, -1, iter(sorted(adj[root])))]
        while stack:
            a, parent, it = stack[-1]
            for nb in it:
                if nb == parent:
                    continue
                if nb not in order:
                    order[nb] = len(order)
                    children[a].append(nb)
                    stack.append((nb, a, iter(sorted(adj[nb]))))
                    break
                if order[nb] < order[a]:
                    closes[a].append(nb)
                    opens[nb].append(a)
            else:
                stack.pop()
    used, number = set(), {}

    def digit(k):
        return str(k) if k < 10 else f"%{k}"

    def emit(a, parent):
        out = ["=" if parent >= 0 and adj[a][parent] == 2 else "",
               _smiles_atom(names[int(types[a])], int(n_h[a]), int(charges[a]), sum(adj[a].values()))]
        for d in opens[a]:
            k = next(k for k in range(1, 101) if k not in used)
            if k > 99:
                raise GaudiError("smiles: more than 99 ring closures open at once")
            used.add(k)
            number[(a, d)] = k
        for nb in closes[a]:
            out.append(("=" if adj[a][nb] == 2 else "") + digit(number[(nb, a)]))
        out += [digit(number[(a, d)]) for d in opens[a]]
        for nb in closes[a]:
            used.discard(number.pop((nb, a)))
        for i, c in enumerate(children[a]):
            text = emit(c, a)
            out.append(text if i == len(children[a]) - 1 else "(" + text + ")")
        return "".join(out)

    import sys
    limit = sys.getrecursionlimit()
    if limit < 3 * H + 100:
        sys.setrecursionlimit(3 * H + 100)
    try:
        return ".".join(emit(r, -1) for r in roots)
    finally:
        sys.setrecursionlimit(limit)


def write_smiles(path_or_file, records, dataset="cata"):
    """One line per record: its SMILES, or an empty line where smiles() gives None.  -> the number of strings written."""
    f, close = _open(path_or_file)
    n = 0
    try:
        for rec in records:
            text = smiles(rec, dataset)
            n += text is not None
            f.write((text or "") + "\n")
    finally:
        if close:
            f.close()
    return n


_READ_BRACKET = re.compile(r"\[([A-Z][a-z]?)(H\d*)?([+-]\d*)?\]")


def read_smiles(text, dataset="cata"):
    """The inverse of smiles() for the dialect that function writes -> (atom_types [n], bonds [m,2], orders [m], charges [n]): the
    heavy atoms in the order they are written, then their hydrogens -- those a bare B C N O S implies for the sum of its bond
    orders and those a bracket atom names -- in ascending parent order, every one an atom of its own with a single bond.
    Understood: upper-case bare B C N O S, bracket atoms [Sym], [SymH], [SymHn] with an optional charge (+, -, +n, -n), "=",
    branches, ring closures 1..9 and %nn, "." between components.  Lower-case aromatic atoms, stereo marks (@ / \\), isotopes, "#",
    "-", ":" and anything else raise GaudiError naming the position."""
    names = atoms_list(dataset)

    def bad(i, what):
        raise GaudiError(f"read_smiles: {what} at position {i} of {text!r}")

    syms, given_h, charges, heavy_bonds, bare = [], [], [], [], []
    prev, pending, stack, ring = -1, 1, [], {}

    def atom(i, sym, n_h, charge):
        nonlocal prev, pending
        if sym not in names or sym == "H":
            bad(i, f"element {sym!r} outside the {dataset} atom list")
        syms.append(sym)
        given_h.append(n_h)
        charges.append(charge)
        a = len(syms) - 1
        if prev >= 0:
            heavy_bonds.append((prev, a, pending))
        elif pending != 1:
            bad(i, "a bond symbol with no atom before it")
        prev, pending = a, 1

    def closure(i, k):
        nonlocal pending
        if prev < 0:
            bad(i, "a ring closure with no atom before it")
        if k in ring:
            j = ring.pop(k)
            if j == prev or any({a, b} == {j, prev} for a, b, _ in heavy_bonds):
                bad(i, "a ring closure that repeats a bond or joins an atom to itself")
            heavy_bonds.append((j, prev, pending))
        else:
            if pending != 1:
                bad(i, "'=' before an opening ring digit (the dialect writes it before the closing one)")
            ring[k] = prev
        pending = 1

    i = 0
    while i < len(text):
        ch = text[i]
        if ch == ".":
            if stack or pending != 1:
                bad(i, "'.' inside a branch or after a bond symbol")
            prev = -1
        elif ch == "(":
            if prev < 0:
                bad(i, "a branch with no atom before it")
            stack.append(prev)
        elif ch == ")":
            if not stack or pending != 1:
                bad(i, "an unmatched ')'")
            prev = stack.pop()
        elif ch == "=":
            if pending != 1 or prev < 0:
                bad(i, "a misplaced '='")
            pending = 2
        elif ch.isdigit():
            if ch == "0":
                bad(i, "ring closure 0")
            closure(i, int(ch))
        elif ch == "%":
            if not text[i + 1:i + 3].isdigit() or len(text[i + 1:i + 3]) != 2 or int(text[i + 1:i + 3]) < 10:
                bad(i, "'%' without two digits")
            closure(i, int(text[i + 1:i + 3]))
            i += 2
        elif ch == "[":
            m = _READ_BRACKET.match(text, i)
            if not m:
                bad(i, "a bracket atom outside [Sym], [SymHn], [SymHn+q]")
            n_h = 0 if not m.group(2) else int(m.group(2)[1:] or 1)
            q = 0 if not m.group(3) else int(m.group(3)[1:] or 1) * (1 if m.group(3)[0] == "+" else -1)
            atom(i, m.group(1), n_h, q)
            i = m.end() - 1
        elif ch in _SMILES_VALENCES:
            atom(i, ch, None, 0)
            bare.append(prev)
        elif ch.islower():
            bad(i, f"lower-case (aromatic) atom {ch!r}")
        elif ch in "@/\\":
            bad(i, f"stereo mark {ch!r}")
        else:
            bad(i, f"unsupported character {ch!r}")
        i += 1
    if ring:
        bad(len(text), f"ring closure {sorted(ring)[0]} never closed")
    if stack or pending != 1:
        bad(len(text), "an open branch or a trailing bond symbol")
    total = [0] * len(syms)
    for a, b, o in heavy_bonds:
        total[a] += o
        total[b] += o
    for a in bare:
        fit = [v for v in _SMILES_VALENCES[syms[a]] if v >= total[a]]
        given_h[a] = fit[0] - total[a] if fit else 0
    H = len(syms)
    types = [names.index(s) for s in syms]
    bonds, orders = [(a, b) for a, b, _ in heavy_bonds], [o for _, _, o in heavy_bonds]
    for a in range(H):
        for _ in range(given_h[a]):
            bonds.append((a, len(types)))
            orders.append(1)
            types.append(names.index("H"))
            charges.append(0)
    return (np.array(types, np.int64), np.array(bonds, np.int64).reshape(-1, 2), np.array(orders, np.int64),
            np.array(charges, np.int64))
