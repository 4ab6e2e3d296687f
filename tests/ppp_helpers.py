"""Shared by test_ppp_cpu.py and test_gpu_ppp.py: a float64 oracle restated in numpy from DESIGN.md section 8m (site classes, the
PPP Fock matrix, the damped closed-shell SCF; numpy.linalg.eigh; it reads the table file itself and shares no code with the
kernel), the molecules the tests are made of with a geometry builder, the host build as an engine stand-in, and results computed
once.

MEASURED (the host build, which the device equals bit for bit, against the fixed-point oracle; g30's 155 converged molecules plus
the twelve of the tier-edge set, default settings): the largest error of a level / homo / lumo / gap / e_electronic per centre
is MEASURED_EV, of a charge / bond order (gap >= 0.1 eV) MEASURED_P.  The tolerances are four times that
(a small sample, and a stopping rule that leaves an error of order delta_p * gamma which varies from molecule to molecule); the
issue's condition is TOL_EV <= 2e-3 and TOL_P <= 2e-4."""
import json
import os

import numpy as np

from gaudi_amd import _lib
from tests.bond_order_helpers import C, H
from tests.substructure_helpers import graph_of

OK, NOT_CONVERGED, BAD_INPUT, OVERFLOW, EMPTY, NO_PI, BAD_TABLE, OPEN_SHELL, BAD_GEOMETRY = range(9)
DEGENERATE, SCF_CAP, JACOBI_CAP = 2, 4, 8
ATOMS = ("H", "C", "B", "N", "O", "S")  # ATOMS_LIST["hetro"]; ATOMS_LIST["cata"] is its prefix
B_, N_, O_, S_ = 2, 3, 4, 5
DATASET = "hetro"
MEASURED_EV, MEASURED_P = 7.25e-5, 2.88e-5  # eV; electrons: g30 + the tier-edge set, the default (Mataga-Nishimoto) formula
TOL_EV, TOL_P = 4 * MEASURED_EV, 4 * MEASURED_P  # 2.9e-4 eV, 1.152e-4 (the Ohno formula measures 1.41e-4 eV and 9.31e-5: inside too)
CAP, STOP = 64, 2.0 ** -16
SIDE = 1.40
EDGE_SIZES = (2, 3, 31, 32, 33, 62, 63, 64, 65, 126, 127, 128)
TABLE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gaudi_amd", "data", "ppp_tables.json")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def table():
    if "table" not in _CACHE:
        with open(TABLE_FILE) as f:
            _CACHE["table"] = json.load(f)
    return _CACHE["table"]


def c_tables(parameters=None):
    from gaudi_amd.ppp import c_ppp_tables
    return c_ppp_tables(DATASET, parameters)


def oracle(mol, charge=0, repulsion="mataga-nishimoto", damping=0.25):
    """Section 8m by the book in float64 on the float32-rounded coordinates -> dict.  The iteration is run to delta_p <= 1e-10
    (at most 2 000 times): ``levels`` ... ``pi_bond_order`` are the fixed point's (``fixed`` says whether it was reached).  The same
    trajectory read under the kernel's rule (2^-16, 64 iterations) gives ``status``, ``iterations`` and ``decisive``: converged in
    at most 56 iterations, or still at delta_p >= 1e-4 at iteration 64."""
    elem, bonds, xyz = mol
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    xyz = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    n, T = len(elem), table()
    names = list(T["classes"])
    out = dict(status=OK, n_pi=0, n_electrons=0, n_excluded=0, iterations=0, decisive=True, fixed=False)
    if n == 0:
        return dict(out, status=EMPTY)
    if n > 384 or len(bonds) > 384:
        return dict(out, status=OVERFLOW)
    pairs = [tuple(sorted((int(i), int(j)))) for i, j in bonds]
    if ((elem < 0) | (elem >= len(ATOMS))).any() or any(i < 0 or j >= n or i == j for i, j in pairs) or len(set(pairs)) != len(pairs):
        return dict(out, status=BAD_INPUT)
    heavy, attr, nbrs = graph_of(elem, bonds)
    deg = np.bincount(bonds.reshape(-1), minlength=n) if len(bonds) else np.zeros(n, np.int64)
    if len(heavy) > 192 or deg.max() > 8:
        return dict(out, status=OVERFLOW)
    cls = {}
    for a in heavy:
        e, n_h, hd = attr[a]
        name = T["sites"].get(ATOMS[e], {}).get(str(n_h + hd))
        if name is not None:
            cls[a] = names.index(name)
    pi = sorted(cls)
    if not pi:
        return dict(out, status=NO_PI)
    if len(pi) > 128:
        return dict(out, status=OVERFLOW)
    par = [T["classes"][names[cls[a]]] for a in pi]
    z = np.array([float(p["z"]) for p in par])
    n_el = int(z.sum()) - charge
    if n_el < 0 or n_el > 2 * len(pi):
        return dict(out, status=BAD_INPUT)
    if n_el & 1:
        return dict(out, status=OPEN_SHELL)
    X = xyz[pi]
    R = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1))
    if not np.isfinite(X).all() or (R + 10.0 * np.eye(len(pi)) < 0.5).any():
        return dict(out, status=BAD_GEOMETRY)
    m = len(pi)
    at = {a: r for r, a in enumerate(pi)}
    g1 = np.array([float(p["gamma"]) for p in par])
    ion = np.array([float(p["I"]) for p in par])
    a_rs = 2 * 14.397 / (g1[:, None] + g1[None])
    G = 14.397 / np.sqrt(R ** 2 + a_rs ** 2) if repulsion == "ohno" else 14.397 / (R + a_rs)
    G[np.arange(m), np.arange(m)] = g1
    beta = np.zeros((m, m))
    for a in pi:
        for o in nbrs[a]:
            if o in at:
                key = [k for k in (f"{names[cls[a]]}|{names[cls[o]]}", f"{names[cls[o]]}|{names[cls[a]]}") if k in T["beta_pair"]]
                beta[at[a], at[o]] = T["beta_pair"][key[0]] if key else T["beta0"] * par[at[a]]["k"] * par[at[o]]["k"]
    G0 = G - np.diag(g1)
    Hc = beta + np.diag(-ion - G0 @ z)
    n_occ = n_el // 2

    def fock(P):
        d = np.diag(P)
        return Hc + np.diag(0.5 * d * g1 + G0 @ d) - 0.5 * P * G0

    P = np.diag(z)
    history = []
    for _ in range(2000):
        w, V = np.linalg.eigh(fock(P))
        Pn = 2.0 * V[:, :n_occ] @ V[:, :n_occ].T
        history.append(float(np.abs(Pn - P).max()))
        P = (1.0 - damping) * Pn + damping * P
        if history[-1] <= 1e-10:
            break
    first = next((k + 1 for k, d in enumerate(history) if d <= STOP), None)
    converged = first is not None and first <= CAP
    decisive = (converged and first <= CAP - 8) or (not converged and len(history) >= CAP and history[CAP - 1] >= 1e-4)
    F = fock(Pn)
    w, V = np.linalg.eigh(F)
    Pn = 2.0 * V[:, :n_occ] @ V[:, :n_occ].T
    ih, il = n_occ - 1, n_occ
    ih = il if ih < 0 else ih
    il = ih if il >= m else il
    q, p = np.zeros(n), np.zeros(len(bonds))
    site = np.full(n, -1, np.int64)
    for a in pi:
        site[a] = cls[a]
        q[a] = z[at[a]] - Pn[at[a], at[a]]
    for k, (i, j) in enumerate(bonds):
        if int(i) in at and int(j) in at:
            p[k] = Pn[at[int(i)], at[int(j)]]
    return dict(out, status=OK if converged else NOT_CONVERGED, iterations=first if converged else CAP, decisive=decisive,
                fixed=history[-1] <= 1e-10, history=history, n_pi=m, n_electrons=n_el, n_excluded=len(heavy) - m, site_class=site,
                levels=w, occupation=np.array([2] * n_occ + [0] * (m - n_occ)), homo=w[ih], lumo=w[il], gap=w[il] - w[ih],
                e_electronic=0.5 * float((Pn * (Hc + F)).sum()), e_core=float(np.triu(np.outer(z, z) * G0, 1).sum()), pi_charge=q,
                pi_bond_order=p)


# ---- molecules: (elem [n], bonds [m,2], xyz [n,3]) triples

def _finish(elem, bonds, xyz):
    return np.array(elem, np.int32), np.array(bonds, np.int32).reshape(-1, 2), np.array(xyz, np.float64).reshape(-1, 3)


def _add_h(elem, bonds, xyz, parent, count):
    """``count`` hydrogens listed on ``parent``, 1.09 A out, away from the mean of its neighbours and fanned in the plane."""
    nb = [j if i == parent else i for i, j in bonds if parent in (i, j)]
    out = np.asarray(xyz[parent]) - np.mean([xyz[k] for k in nb], axis=0)
    ang = np.arctan2(out[1], out[0])
    for k in range(count):
        t = ang + (0.0 if count == 1 else np.deg2rad(60.0) * (2 * k - 1))
        bonds.append((parent, len(elem)))
        elem.append(H)
        xyz.append([xyz[parent][0] + 1.09 * np.cos(t), xyz[parent][1] + 1.09 * np.sin(t), 0.0])


def chain_molecule(n):
    """A zig-zag chain of n carbons (ethylene, allyl, ...), two hydrogens listed at either end."""
    elem, bonds, xyz = [C] * n, [(a, a + 1) for a in range(n - 1)], []
    for a in range(n):
        xyz.append([a * SIDE * np.cos(np.deg2rad(30.0)), (a & 1) * SIDE * np.sin(np.deg2rad(30.0)), 0.0])
    _add_h(elem, bonds, xyz, 0, 2)
    _add_h(elem, bonds, xyz, n - 1, 2)
    return _finish(elem, bonds, xyz)


def phenacene(rings, chain=0):
    """Zig-zag fused regular hexagons of side 1.40 A (centre steps alternating 0 and 60 degrees), 4 * rings + 2 carbons, with a
    zig-zag chain of ``chain`` carbons on the lower-left vertex of the first ring (two hydrogens listed on the chain's end)."""
    step = SIDE * np.sqrt(3.0)
    centre, index, xyz, bonds = np.zeros(2), {}, [], set()
    for k in range(rings):
        ring = []
        for j in range(6):
            t = np.deg2rad(30.0 + 60.0 * j)
            p = centre + SIDE * np.array([np.cos(t), np.sin(t)])
            key = (int(round(p[0] * 100)), int(round(p[1] * 100)))
            if key not in index:
                index[key] = len(xyz)
                xyz.append([p[0], p[1], 0.0])
            ring.append(index[key])
        bonds |= {tuple(sorted((ring[j], ring[(j + 1) % 6]))) for j in range(6)}
        t = np.deg2rad(60.0 * (k & 1))
        centre = centre + step * np.array([np.cos(t), np.sin(t)])
    elem, bonds = [C] * len(xyz), sorted(bonds)
    t0 = np.deg2rad(210.0)
    at = index[(int(round(SIDE * np.cos(t0) * 100)), int(round(SIDE * np.sin(t0) * 100)))]
    for k in range(chain):
        t = np.deg2rad(210.0 if k % 2 == 0 else 150.0)
        bonds.append((at, len(elem)))
        xyz.append([xyz[at][0] + SIDE * np.cos(t), xyz[at][1] + SIDE * np.sin(t), 0.0])
        elem.append(C)
        at = len(elem) - 1
    if chain:
        _add_h(elem, bonds, xyz, at, 2)
    return _finish(elem, bonds, xyz)


def edge_molecule(n_pi):
    """The tier-edge molecule with n_pi centres and the charge that closes its shell."""
    if n_pi < 6:
        return chain_molecule(n_pi), n_pi & 1
    rings = (n_pi - 2) // 4
    return phenacene(rings, n_pi - (4 * rings + 2)), n_pi & 1


def edge_set():
    if "edge" not in _CACHE:
        _CACHE["edge"] = [edge_molecule(n) for n in EDGE_SIZES]
    return [m for m, _ in _CACHE["edge"]], np.array([c for _, c in _CACHE["edge"]], np.int32)


def cycle(elems, h_on=()):
    """A regular polygon of side 1.40 A with the given elements; ``h_on``: ring atoms that list one hydrogen."""
    n = len(elems)
    rad = SIDE / (2.0 * np.sin(np.pi / n))
    xyz = [[rad * np.cos(2 * np.pi * k / n), rad * np.sin(2 * np.pi * k / n), 0.0] for k in range(n)]
    elem, bonds = list(elems), [(k, (k + 1) % n) for k in range(n)]
    for a in h_on:
        _add_h(elem, bonds, xyz, a, 1)
    return _finish(elem, bonds, xyz)


def benzene():
    return cycle([C] * 6)


def naphthalene():
    return phenacene(2)


def pyridine():
    return cycle([N_] + [C] * 5)


def hand_made():
    """name -> (molecule, charge): all closed shell."""
    return {"ethylene": (chain_molecule(2), 0), "allyl cation": (chain_molecule(3), 1), "benzene": (benzene(), 0),
            "naphthalene": (naphthalene(), 0), "pyridine": (pyridine(), 0), "pyrrole": (cycle([N_] + [C] * 4, h_on=(0,)), 0),
            "furan": (cycle([O_] + [C] * 4), 0), "thiophene": (cycle([S_] + [C] * 4), 0), "borabenzene": (cycle([B_] + [C] * 5), 0)}


def g30_molecules():
    """The molecules of golden g30 the reference built: its atoms (in the plane, z = 0), types and bonds."""
    if "g30" not in _CACHE:
        from tests.gor2goa_helpers import unpack
        mols = []
        for m in unpack(np.load(os.path.join(GOLDEN, "g30_gor2goa.npz"))):
            if m["threw"] or len(m["ref_types"]) == 0:
                continue
            xy = np.asarray(m["ref_atoms"], np.float64)
            mols.append((m["ref_types"].astype(np.int32), m["ref_bonds"].astype(np.int32), np.concatenate([xy, np.zeros((len(xy), 1))], 1)))
        _CACHE["g30"] = mols
    return _CACHE["g30"]


def g30_oracle():
    if "g30_oracle" not in _CACHE:
        _CACHE["g30_oracle"] = [oracle(m) for m in g30_molecules()]
    return _CACHE["g30_oracle"]


def edge_oracle_one(k):
    """The oracle's result for tier-edge molecule k, computed once."""
    if ("edge_oracle", k) not in _CACHE:
        mols, charge = edge_set()
        _CACHE["edge_oracle", k] = oracle(mols[k], int(charge[k]))
    return _CACHE["edge_oracle", k]


def pack(mols, A=None, M=None):
    """Triples -> elem [B,A], n_atoms [B], bonds [B,M,2], n_bonds [B], xyz [B,A,3] float32 (zero padded; A, M at least what is given)."""
    B = len(mols)
    A = max([1, A or 1] + [len(m[0]) for m in mols])
    M = max([1, M or 1] + [len(np.asarray(m[1]).reshape(-1, 2)) for m in mols])
    elem, bonds, xyz = np.zeros((B, A), np.int32), np.zeros((B, M, 2), np.int32), np.zeros((B, A, 3), np.float32)
    na, nb = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for i, (e, b, x) in enumerate(mols):
        b = np.asarray(b, np.int32).reshape(-1, 2)
        elem[i, :len(e)], bonds[i, :len(b)], na[i], nb[i] = e, b, len(e), len(b)
        xyz[i, :len(e)] = np.asarray(x, np.float32).reshape(-1, 3)
    return elem, na, bonds, nb, xyz


def _charge(charge, B):
    return None if charge is None else np.ascontiguousarray(np.broadcast_to(np.asarray(charge, np.int32), (B,)))


def host(mols, charge=None, repulsion=0, damping=0.25, parameters=None, A=None, M=None):
    """Triples -> the raw outputs of the host build."""
    return _lib.host_ppp(c_tables(parameters), *pack(mols, A, M), _charge(charge, len(mols)), repulsion, damping)


def device(engine, mols, charge=None, repulsion=0, damping=0.25, parameters=None, A=None, M=None):
    return engine.ppp(c_tables(parameters), *pack(mols, A, M), _charge(charge, len(mols)), repulsion, damping)


class HostEngine:
    """What gaudi_amd.ppp asks of an engine, on the kernel's host build."""

    def ppp(self, *args):
        return _lib.host_ppp(*args)


def g30_host():
    """The host build's outputs for the whole of g30, computed once, never written to."""
    if "host" not in _CACHE:
        out = host(g30_molecules())
        for a in out.values():
            a.setflags(write=False)
        _CACHE["host"] = out
    return _CACHE["host"]


def edge_host_one(k):
    """The host build's outputs for tier-edge molecule k alone (a 128-centre molecule takes it two seconds), computed once, never
    written to."""
    if ("edge_host", k) not in _CACHE:
        mols, charge = edge_set()
        out = host([mols[k]], charge[k:k + 1])
        for a in out.values():
            a.setflags(write=False)
        _CACHE["edge_host", k] = out
    return _CACHE["edge_host", k]


def errors(out, i, want, mol):
    """(the largest error in eV over levels, homo, lumo, gap, e_electronic / n_pi; the largest over charges and bond orders) of row i
    of raw outputs against an oracle result."""
    n, na, nb = want["n_pi"], len(mol[0]), len(np.asarray(mol[1]).reshape(-1, 2))
    ev = max(np.abs(out["levels"][i, :n].astype(np.float64) - want["levels"]).max(), abs(out["homo"][i] - want["homo"]),
             abs(out["lumo"][i] - want["lumo"]), abs(out["gap"][i] - want["gap"]),
             abs(out["e_electronic"][i] - want["e_electronic"]) / n)
    p = max(np.abs(out["pi_charge"][i, :na] - want["pi_charge"]).max(), np.abs(out["pi_bond_order"][i, :nb] - want["pi_bond_order"]).max())
    return float(ev), float(p)


def assert_same_bits(got, want, rows=None):
    """Every output array equal in dtype, shape and bytes (floats compared as their bits)."""
    for name in _lib.PPP_ARRAYS:
        g, w = got[name], want[name] if rows is None else want[name][rows]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), name


def row(out, i, n_atoms, n_bonds):
    """Molecule i's outputs trimmed to its own sizes: what must not depend on the batch it ran in."""
    r = {k: out[k][i].copy() for k in _lib.PPP_ARRAYS}
    r["pi_charge"], r["site_class"], r["pi_bond_order"] = r["pi_charge"][:n_atoms], r["site_class"][:n_atoms], r["pi_bond_order"][:n_bonds]
    return r


def assert_rows_equal(a, b):
    for k in _lib.PPP_ARRAYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
