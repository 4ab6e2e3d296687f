"""Host mirror of data/gor2goa.py: a graph of rings -> a graph of atoms, on top of gaudi_rings_to_atoms.

``gor2goa(x, rings_types, dataset, tol)`` has the reference's signature and return for one molecule; ``rings_to_atoms`` is the
batched form: every molecule of a call is converted in ONE kernel launch (one wavefront per molecule), with optional hydrogen
placement and an optional 64-bit fingerprint of the heavy-atom graph.  ``write_xyz`` / ``write_molfile`` are host code.  The
constants (ring templates, RINGS_DICT, ATOMS_LIST, ...) ship as data in ``gaudi_amd/data/ring_tables.json`` under "goa".

What is NOT here: the RDKit half of the reference (build_molecule_aromatic, rdkit_valid, InChI: gor2goa.py:264-324).  "Built"
means gor2goa did not raise -- not that RDKit would sanitise the molecule; the fingerprint stands in for the InChI string when
molecules are counted, and equal fingerprints do not prove that two molecules are isomorphic.  There is no CPU implementation
behind these functions: without the HIP library they raise GaudiError."""
from __future__ import annotations

import numpy as np

from ._lib import ATOMS_FINGERPRINT, ATOMS_MAX_ATOMS, ATOMS_MAX_BONDS, ATOMS_PLACE_H, AtomTables, GaudiError
from .analyze import _engine, _key, _np, _pack, c_tables, ring_tables

STATUS_NAMES = {0: "built", 1: "a ring without a fused neighbour in a multi-ring molecule",
                2: "the orientation type or a type outside the table among the rings", 3: "no rings",
                4: "more atoms, bonds or fused pairs than the kernel holds"}


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


def _is_packed(molecules) -> bool:
    """(x [B,N,3], ring_type [B,N], n_nodes [B]) rather than a list of (positions, ring_type) pairs: three entries that are
    arrays (not pairs themselves) of 3, 2 and 1 dimensions."""
    if not isinstance(molecules, (tuple, list)) or len(molecules) != 3 or any(isinstance(m, (tuple, list)) for m in molecules):
        return False
    return [np.ndim(_np(m)) for m in molecules] == [3, 2, 1]


def rings_to_atoms(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None):
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
    atoms in ascending parent index), 1.09 A out on the bisector in the molecular plane -- a complete structure."""
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


def write_molfile(path_or_file, atoms3d, atom_types, bonds, dataset="cata", comment=""):
    """V2000 molfile of one molecule: bond type 4 (aromatic) between heavy atoms, 1 (single) to hydrogen -- the bond orders
    build_molecule_aromatic gives them (data/gor2goa.py:282-286)."""
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
    f, close = _open(path_or_file)
    try:
        f.write(f"{str(comment).splitlines()[0] if comment else ''}\n  gaudi_amd\n\n")
        f.write(f"{len(xyz):3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000\n")
        for s, p in zip(sym, xyz):
            f.write(f"{p[0]:10.4f}{p[1]:10.4f}{p[2]:10.4f} {s:<3s} 0  0  0  0  0  0  0  0  0  0  0  0\n")
        for i, j in bonds:
            order = 1 if "H" in (sym[i], sym[j]) else 4
            f.write(f"{i + 1:3d}{j + 1:3d}{order:3d}  0\n")
        f.write("M  END\n")
    finally:
        if close:
            f.close()
