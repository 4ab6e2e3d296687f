"""A graph of atoms -> a graph of rings, on top of gaudi_atoms_to_rings: the inverse of gaudi_amd.gor2goa.

What the reference does per molecule in Python and caches to disk (data/aromatic_dataloader.py:131-152: load_xyz,
get_connectivity_matrix with skip_hydrogen=True, networkx.minimum_cycle_basis, get_rings, get_rings_adj) is one kernel launch for
a whole batch here, one wavefront per molecule.  ``atoms_to_rings`` is the batched form, ``goa2gor`` has the return of
``AromaticDataset.get_rings`` for one molecule, ``read_xyz`` inverts ``gor2goa.write_xyz``.  Covalent radii, RINGS_DICT and the
lists ship as data in ``gaudi_amd/data/ring_tables.json`` under "goa".

The rings are the chordless cycles of 4 to 6 heavy atoms, accepted only when they number E - V + C and are independent over
GF(2): then they ARE the minimum cycle basis, whatever order networkx would have used.  Where that fails (sterically clashing
structures, a ring of 7 or more) the status is NOT_A_BASIS and the molecule has no rings; the reference's answer there depends on
networkx's tie-breaking or raises.  There is no CPU implementation behind these functions: without the HIP library they raise
GaudiError."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import GaudiError, PerceptionTables
from .analyze import _engine, _key, _np, ring_tables
from .gor2goa import atoms_list

STATUS_NAMES = {_lib.RINGS_OK: "OK", _lib.RINGS_NO_RINGS: "NO_RINGS", _lib.RINGS_BAD_TYPE: "BAD_TYPE",
                _lib.RINGS_NOT_A_BASIS: "NOT_A_BASIS", _lib.RINGS_OVERFLOW: "OVERFLOW"}

_SYMBOLS = ("H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc "
            "Ru Rh Pd Ag Cd In Sn Sb Te I Xe").split()


def c_perception_tables(dataset: str) -> PerceptionTables:
    """gaudi_perception_tables for one dataset."""
    ds = _key(dataset)
    T = ring_tables()
    G = T["goa"]
    rings, atoms = T["rings"][ds], atoms_list(dataset)
    t = PerceptionTables()
    t.n_elems = len(atoms)
    for i, e in enumerate(atoms):
        t.cov_radius[i] = float(G["cov_radii"][e])
    t.h_elem, t.c_elem = atoms.index("H"), atoms.index("C")
    t.b_elem = atoms.index("B") if "B" in atoms else -1
    t.n_types = len(rings)
    for i, sym in enumerate(rings):
        elems = G["ring_atoms"].get(sym)  # None: the orientation type "."
        if elems is None or any(e not in atoms for e in elems):
            continue
        t.ring_size[i] = len(elems)
        for k, e in enumerate(elems):
            t.ring_elem[i][k] = atoms.index(e)
        t.no_orientation[i] = int(sym in G["no_orientation"])
    t.db_type = rings.index("Db") if "Db" in rings else -1
    t.dhdb_type = rings.index("DhDb") if "DhDb" in rings else -1
    return t


def read_xyz(path_or_file):
    """XYZ file -> (symbols: list of str, xyz [n,3] float64), as data/mol.py:202-229 (load_xyz) reads it: two header lines are
    skipped, an atomic number stands for its symbol, symbols are capitalised.  Inverts gor2goa.write_xyz."""
    f, close = (path_or_file, False) if hasattr(path_or_file, "read") else (open(path_or_file, "r"), True)
    try:
        lines = f.read().splitlines()
    finally:
        if close:
            f.close()
    symbols, xyz = [], []
    for line in lines[2:]:
        if not line.strip():
            continue
        parts = line.split()
        if len(parts) != 4:
            raise GaudiError(f"read_xyz: expected `symbol x y z`, got {line!r}")
        sym = parts[0]
        if not sym.isalpha():
            z = int(sym)
            if not 1 <= z <= len(_SYMBOLS):
                raise GaudiError(f"read_xyz: atomic number {z} outside 1..{len(_SYMBOLS)}")
            sym = _SYMBOLS[z - 1]
        symbols.append(sym.capitalize())
        xyz.append([float(v) for v in parts[1:]])
    return symbols, np.asarray(xyz, np.float64).reshape(-1, 3)


def _pack_atoms(molecules, dataset):
    """list of (symbols or type indices, xyz) -> xyz [B,A,3] float64, elem [B,A] int32, n_atoms [B] int32."""
    names = atoms_list(dataset)
    els, xs = [], []
    for m, (sym, xyz) in enumerate(molecules):
        x = np.asarray(_np(xyz), np.float64).reshape(-1, 3)
        if len(sym) and isinstance(sym[0], str):
            bad = [s for s in sym if s not in names]
            if bad:
                raise GaudiError(f"molecule {m}: element {bad[0]!r} is not in ATOMS_LIST[{dataset!r}] = {names}")
            e = np.array([names.index(s) for s in sym], np.int32)
        else:
            e = np.asarray(_np(sym)).astype(np.int32).reshape(-1)
            if len(e) and (e.min() < 0 or e.max() >= len(names)):
                raise GaudiError(f"molecule {m}: element index outside ATOMS_LIST[{dataset!r}] (0..{len(names) - 1})")
        if len(e) != len(x):
            raise GaudiError(f"molecule {m}: {len(e)} elements for {len(x)} positions")
        els.append(e)
        xs.append(x)
    B, A = len(xs), max(1, max(len(x) for x in xs))
    X = np.zeros((B, A, 3), np.float64)
    E = np.zeros((B, A), np.int32)
    n = np.zeros(B, np.int32)
    for b, (e, x) in enumerate(zip(els, xs)):
        X[b, :len(x)], E[b, :len(e)], n[b] = x, e, len(x)
    return X, E, n


def atoms_to_rings(molecules, dataset="cata", use_hydrogens=False, covalency_factor=1.3, engine=None):
    """Ring perception for a batch in one launch.  ``molecules``: a list of ``(symbols or indices into ATOMS_LIST[dataset], xyz
    [n,3])`` pairs.  Hydrogens take no part (the dataset path, skip_hydrogen=True); with ``use_hydrogens`` a CCBCCB ring whose
    boron carries an H is DhDb instead of Db.  An element outside ATOMS_LIST[dataset] raises GaudiError.

    Returns one record (dict) per molecule:
      status         0 = OK, otherwise STATUS_NAMES and the arrays below are empty
      x              [n,3] float32 ring centres (the float64 centres cast, as the reference's torch.tensor(..., float32))
      centres        [n,3] float64
      ring_type      [n] indices into RINGS_LIST[dataset];  node_features: [n,R] float32 one-hot
      adj            [n,n] float32, 1 where two rings share an atom
      ring_atoms     [n,6] atom indices ascending, padded with -1; rings ascending by their atom tuple
      orientation    list of [k,3] float64 arrays: the candidates an orientation node is drawn from"""
    molecules = list(molecules)
    if not molecules:
        return []
    X, E, n = _pack_atoms(molecules, dataset)
    flags = _lib.RINGS_USE_H if use_hydrogens else 0
    raw = _engine(engine).atoms_to_rings(c_perception_tables(dataset), X, E, n, flags, float(covalency_factor))
    R = len(ring_tables()["rings"][_key(dataset)])
    out = []
    for b in range(len(molecules)):
        k = int(raw["n_rings"][b])
        ty = raw["ring_type"][b, :k].astype(np.int64)
        oh = np.zeros((k, R), np.float32)
        oh[np.arange(k), ty] = 1.0
        cen = raw["centre"][b, :k].copy()
        out.append(dict(status=int(raw["status"][b]), x=cen.astype(np.float32), centres=cen, ring_type=ty, node_features=oh,
                        adj=raw["adj"][b, :k, :k].astype(np.float32), ring_atoms=raw["ring_atoms"][b, :k].astype(np.int64),
                        orientation=[raw["orient"][b, r, :int(raw["n_orient"][b, r])].copy() for r in range(k)]))
    return out


def goa2gor(symbols, xyz, dataset="cata", engine=None):
    """One molecule -> (x [n,3] float32, adj [n,n], node_features [n,R], orientation: list of lists of [x, y, z]), what
    AromaticDataset.get_rings returns (data/aromatic_dataloader.py:131-152).  Raises GaudiError carrying the status name where
    the status is not OK."""
    rec = atoms_to_rings([(symbols, xyz)], dataset, engine=engine)[0]
    if rec["status"]:
        raise GaudiError(f"goa2gor: {STATUS_NAMES.get(rec['status'], rec['status'])}")
    orientation = [[[float(v) for v in p] for p in o] for o in rec["orientation"]]
    try:
        import torch
        return torch.from_numpy(rec["x"]), torch.from_numpy(rec["adj"]), torch.from_numpy(rec["node_features"]), orientation
    except ImportError:
        return rec["x"], rec["adj"], rec["node_features"], orientation
