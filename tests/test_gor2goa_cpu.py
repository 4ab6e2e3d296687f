"""Graph of rings -> graph of atoms, the parts that need no GPU: the g30 fixture's own consistency, the declared symbol, the file
writers, the shipped constants and the counting in analyze_atoms_for_molecules."""
import io
import json
import os
import re

import numpy as np

from tests.gor2goa_helpers import n_rings, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_g30_is_consistent(golden):
    mols = unpack(golden("g30_gor2goa"))
    assert 150 <= len(mols) <= 180
    assert sum(m["threw"] for m in mols) >= 3 and any(n_rings(m) == 32 for m in mols)
    assert any(m["dataset"] == "hetro" and len(m["x"]) % 2 == 1 and not m["threw"] for m in mols)  # the reference builds odd counts
    n_stable = 0
    for m in mols:
        if m["threw"]:
            assert len(m["ref_types"]) == 0 and m["iso_class"] == -1 and m["twin_iso_class"] == -1
            continue
        b = m["ref_bonds"]
        assert len(m["ref_atoms"]) == len(m["ref_types"]) and b.min() >= 0 and b.max() < len(m["ref_types"])
        assert np.all(b[:, 0] <= b[:, 1])  # each pair sorted ...
        keys = b[:, 0] * 1000 + b[:, 1]
        assert np.all(np.diff(keys) > 0)  # ... the list sorted and without duplicates
        assert m["iso_class"] == m["twin_iso_class"] >= 0  # rings permuted, rotated, reflected: the same molecule
        assert sorted(m["twin_types"][: n_rings(m)]) == sorted(m["types"][: n_rings(m)])
        if m["dataset"] == "cata" and m["stable"]:
            n_stable += 1
            assert len(m["ref_types"]) == 4 * n_rings(m) + 2 and np.all(m["ref_types"] == 1)  # C(4n+2) before hydrogens
    assert n_stable >= 40
    classes = {m["iso_class"] for m in mols if not m["threw"]}
    assert classes == set(range(len(classes))) and len(classes) >= 60


def test_entry_point_is_declared_and_bound():
    from gaudi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    assert re.search(r"\bint gaudi_rings_to_atoms\(", hdr) and "gaudi_rings_to_atoms" in _lib.EXPORTS
    assert len(_lib.EXPORTS["gaudi_rings_to_atoms"][1]) == 19
    assert f"#define GAUDI_ATOMS_MAX_ATOMS {_lib.ATOMS_MAX_ATOMS}" in hdr and f"#define GAUDI_ATOMS_MAX_BONDS {_lib.ATOMS_MAX_BONDS}" in hdr
    assert _lib.ATOMS_MAX_ATOMS >= 32 * 12  # 32 DhDb rings: 6 ring atoms, 2 template H, 4 placed H each


def test_ring_tables_carry_the_templates():
    from gaudi_amd.gor2goa import atoms_list, c_atom_tables
    T = json.load(open(os.path.join(ROOT, "gaudi_amd", "data", "ring_tables.json")))
    G = T["goa"]
    hexagon = np.array(G["templates"]["hexagon"])
    assert hexagon.shape == (6, 2) and np.allclose(np.linalg.norm(hexagon, axis=1), 1.3846, atol=2e-6)
    ang = np.rad2deg(np.arctan2(hexagon[:, 1], hexagon[:, 0]))
    assert np.allclose((ang + 60.0 * (np.arange(6) + 1) + 180) % 360 - 180, 0, atol=1e-3)  # vertex k at -60 (k + 1) degrees
    assert np.array(G["templates"]["pentagon"]).shape == (5, 2) and np.array(G["templates"]["square"]).shape == (4, 2)
    assert G["ring_atoms"]["Bn"] == list("CCCCCC") and G["ring_atoms"]["Pl"] == list("CCCCN") and G["ring_atoms"]["Cbd"] == list("CCCC")
    assert sorted(G["no_orientation"]) == ["Bn", "Cbd"]
    assert atoms_list("cata") == ["H", "C"] and atoms_list("hetro") == ["H", "C", "B", "N", "O", "S"]
    for sym, elems in G["ring_atoms"].items():
        assert len(G["templates"][G["ring_template"][sym]]) == len(elems)
    t = c_atom_tables("hetro")
    rings = T["rings"]["hetro"]
    assert t.n_types == len(rings) and t.ring_size[rings.index(".")] == 0 and t.ring_size[rings.index("Cbd")] == 4
    i = rings.index("DhDb")
    assert t.n_template_h[i] == 2 and list(t.template_h_parent[i]) == [2, 5] and t.ring_elem[i][2] == 2  # B
    assert abs(t.extra_angle[rings.index("Bn")] - np.pi / 6) < 1e-15 and abs(t.extra_angle[rings.index("Cbd")] - np.pi / 4) < 1e-15
    c = c_atom_tables("cata")
    assert c.n_types == 1 and c.ring_size[0] == 6 and c.no_orientation[0] == 1 and (c.h_elem, c.c_elem) == (0, 1)


def _naphthalene():
    """Hand-made: ten carbons (two fused hexagons), eight hydrogens."""
    r = 1.3846
    hexa = np.array([[r * np.cos(np.deg2rad(30 + 60 * k)), r * np.sin(np.deg2rad(30 + 60 * k))] for k in range(6)])
    dx = 2 * r * np.cos(np.deg2rad(30))
    c = {tuple(np.round(p, 6)) for p in hexa} | {tuple(np.round(p + [dx, 0], 6)) for p in hexa}
    heavy = np.array(sorted(c))
    assert len(heavy) == 10
    d = np.sqrt(((heavy[:, None] - heavy[None]) ** 2).sum(-1))
    cc = [(i, j) for i in range(10) for j in range(i + 1, 10) if d[i, j] < 1.5]
    assert len(cc) == 11
    xyz, types, bonds = [list(p) + [0.0] for p in heavy], [1] * 10, list(cc)
    centre = heavy.mean(0)
    for i in range(10):
        if sum(i in b for b in cc) == 2:
            out = heavy[i] - centre
            out = heavy[i] + 1.09 * out / np.linalg.norm(out)
            bonds.append((i, len(xyz)))
            xyz.append([out[0], out[1], 0.0])
            types.append(0)
    return np.array(xyz), np.array(types), np.array(bonds)


def test_writers_round_trip():
    from gaudi_amd.gor2goa import write_molfile, write_xyz
    xyz, types, bonds = _naphthalene()
    assert len(xyz) == 18 and len(bonds) == 19
    f = io.StringIO()
    write_xyz(f, xyz, types, "cata", comment="naphthalene")
    lines = f.getvalue().splitlines()
    assert int(lines[0]) == 18 and lines[1] == "naphthalene" and len(lines) == 20
    assert [ln.split()[0] for ln in lines[2:]] == ["C"] * 10 + ["H"] * 8
    back = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[2:]])
    assert np.allclose(back, xyz, atol=1e-8)
    f = io.StringIO()
    write_molfile(f, xyz, types, bonds, "cata", comment="naphthalene")
    lines = f.getvalue().split("\n")
    assert lines[0] == "naphthalene" and lines[3].endswith("V2000")
    assert int(lines[3][0:3]) == 18 and int(lines[3][3:6]) == 19
    atom_block, bond_block = lines[4:22], lines[22:41]
    assert [ln[31:34].strip() for ln in atom_block] == ["C"] * 10 + ["H"] * 8
    assert np.allclose([[float(ln[0:10]), float(ln[10:20]), float(ln[20:30])] for ln in atom_block], xyz, atol=1e-4)
    got = [(int(ln[0:3]) - 1, int(ln[3:6]) - 1, int(ln[6:9])) for ln in bond_block]
    assert [(i, j) for i, j, _ in got] == [tuple(b) for b in bonds.tolist()]
    assert [o for _, _, o in got] == [4] * 11 + [1] * 8  # aromatic between ring atoms, single to H
    assert lines[41] == "M  END"
    # 2-D coordinates are accepted (z = 0), and a path works as well as a file object
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_xyz(os.path.join(d, "a.xyz"), xyz[:, :2], types, "cata")
        assert open(os.path.join(d, "a.xyz")).read().splitlines()[0] == "18"


def test_analyze_atoms_arithmetic(monkeypatch):
    """mol_built / mol_unique / mol_novel from a stubbed batched call: no device involved."""
    import gaudi_amd.gor2goa as G
    from gaudi_amd import analyze
    keys = [11, 22, 11, 0, 33, 22, 11]
    status = [0, 0, 0, 2, 0, 0, 0]
    calls = []

    def fake(molecules, dataset="cata", tol=0.1, place_hydrogens=False, fingerprint=False, engine=None):
        calls.append((len(molecules), dataset, tol, fingerprint))
        return [dict(status=s, fingerprint=k) for s, k in zip(status, keys)]

    monkeypatch.setattr(G, "rings_to_atoms", fake)
    mols = [(np.zeros((1, 3), np.float32), np.zeros(1, np.int64)) for _ in keys]
    d, built = analyze.analyze_atoms_for_molecules(mols, tol=0.2, dataset="cata")
    assert calls == [(7, "cata", 0.2, True)]
    assert d["mol_built"] == 6 / 7 and d["mol_unique"] == 3 / 6 and "mol_novel" not in d
    assert d["molecule_built_bool"] == [True, True, True, False, True, True, True] and d["fingerprints"] == keys
    assert len(built) == 6
    d, _ = analyze.analyze_atoms_for_molecules(mols, dataset="cata", train_fingerprints=[22, 99])
    assert d["mol_novel"] == 4 / 6  # 11, 11, 33, 11 are not in the training set
    status[:] = [1] * 7
    d, built = analyze.analyze_atoms_for_molecules(mols, dataset="cata", train_fingerprints=[])
    assert d["mol_built"] == 0 and d["mol_unique"] == 0 and d["mol_novel"] == 0 and built == []


def _inertia(x):
    """Sum over the nodes of |r|^2 1 - r r^T, the terms in the precision of x: what align_to_xy_plane diagonalises."""
    out = np.zeros((3, 3))
    for r in x:
        out += np.array([[r[1] ** 2 + r[2] ** 2, -r[0] * r[1], -r[0] * r[2]],
                         [-r[0] * r[1], r[0] ** 2 + r[2] ** 2, -r[1] * r[2]],
                         [-r[0] * r[2], -r[1] * r[2], r[0] ** 2 + r[1] ** 2]])
    return out


def test_eigh3_has_the_signs_of_numpy_eigh(golden):
    """The kernel's 3 x 3 eigensolver (LAPACK's dsyevd path restated, atoms.inc), compiled for the host as gaudi_host_eigh3,
    against np.linalg.eigh: the same eigenvectors WITH the same signs -- the atom order of gor2goa depends on them.  Matrices:
    the inertia tensors of g30's molecules and of their twins, of random planar and non-planar point sets, random symmetric
    matrices, and the shapes the tridiagonalisation treats apart (a31 = 0, diagonal).  Matrices whose eigenvalues are closer than
    1e-6 of the largest are left out: their eigenvectors are not determined to the precision compared here.
    g30's bond lists come from numpy 2.2.6 on OpenBLAS 0.3.29 (graph of atoms)."""
    import ctypes as C
    from gaudi_amd import _lib
    lib = _lib.load_library()
    rng = np.random.default_rng(31)
    mats = []
    for m in unpack(golden("g30_gor2goa")):
        mats += [_inertia(m["x"]), _inertia(m["twin_x"])]
    for k in range(1500):
        n = int(rng.integers(2, 40))
        p = rng.standard_normal((n, 3)) * rng.uniform(0.5, 6.0, 3)
        if k % 2:
            p[:, 2] *= 0.005  # nearly planar, as molecules are
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        mats.append(_inertia((p @ q + rng.standard_normal(3) * (k % 3)).astype(np.float32)))
    for k in range(1500):
        a = rng.standard_normal((3, 3)) * 10.0 ** rng.uniform(-3, 3)
        mats.append(a + a.T)
    for k in range(100):
        a = rng.standard_normal((3, 3))
        a = a + a.T
        a[2, 0] = a[0, 2] = 0.0
        mats.append(a)
        mats.append(np.diag(rng.standard_normal(3)))
    A = np.ascontiguousarray(np.array(mats, np.float64))
    E = np.zeros_like(A)
    assert lib.gaudi_host_eigh3(len(A), A.ctypes.data_as(_lib.DP), E.ctypes.data_as(_lib.DP)) == 0
    n = 0
    for a, e in zip(A, E):
        w, v = np.linalg.eigh(a)
        if not np.diff(w).min() > 1e-6 * np.abs(w).max():  # (the zero matrix of a node at the origin included)
            continue
        gap = np.diff(w).min() / np.abs(w).max()
        n += 1
        assert np.all((e * v).sum(0) > 0.999999), (a, e, v)  # column k . column k: +1, never -1
        # both solvers are backward stable to a few eps |A| and an eigenvector moves by that over the gap; 64 = a few dozen roundings
        assert np.abs(e - v).max() <= 64 * np.finfo(np.float64).eps / gap, (a, e, v)
    assert n >= 3000


def test_packed_form_is_told_from_a_list_of_three_molecules():
    from gaudi_amd.gor2goa import _is_packed, rings_to_atoms
    mol = (np.zeros((2, 3), np.float32), np.zeros(2, np.int64))
    assert not _is_packed([mol, mol, mol]) and not _is_packed((mol, mol, mol)) and not _is_packed([mol, mol])
    big = (np.zeros((4, 3), np.float32), np.zeros(4, np.int64))
    assert not _is_packed((mol, big, mol))  # ragged: np.asarray of it would raise
    assert _is_packed((np.zeros((5, 2, 3), np.float32), np.zeros((5, 2), np.int32), np.full(5, 2, np.int32)))
    assert rings_to_atoms([]) == [] and rings_to_atoms((np.zeros((0, 2, 3), np.float32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32))) == []
