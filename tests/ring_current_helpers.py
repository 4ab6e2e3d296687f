"""Shared by test_ring_current_cpu.py and test_gpu_ring_current.py: a float64 oracle of DESIGN.md section 8p that shares nothing with
the kernel -- a finite-field calculation (H(f) = E o exp(i f s), complex numpy.linalg.eigh at f = 1e-5, J_rs = 2 Im(H_rs P_sr) / f,
no perturbation formula), rings by brute-force path walking over Python sets, numpy.linalg.lstsq for the ring currents and its own
plane from numpy.linalg.eigh; it reads the table file itself.  Also the molecules the tests are made of (regular polyhexes of side
1.40 A), the host build as an engine stand-in, and results computed once."""
import numpy as np

from gaudi_amd import _lib
from tests import huckel_helpers as hh
from tests import ppp_helpers as pp
from tests.substructure_helpers import graph_of

OK, NOT_CONVERGED, BAD_INPUT, OVERFLOW, EMPTY, NO_PI, BAD_TABLE, OPEN_SHELL, BAD_GEOMETRY, SMALL_GAP = range(10)
RINGS_UNDEFINED = 1
ATOMS, DATASET = hh.ATOMS, hh.DATASET
C = pp.C
SIDE = 1.40
FIELD = 1e-5
SMALL = 1e-3
MIN_AREA = 1e-3
MAX_RINGS = 32
C0 = 2.0 * (1.5 * np.sqrt(3.0) * SIDE ** 2) / 9.0  # the bond current of benzene: a regular hexagon of 1.40 A with k = 1
TOL = 1e-4  # times max(1, |oracle value|): the issue sets it
FLOATS = ("bond_current", "ring_current", "ring_area", "normal", "rms_out_of_plane", "gap", "residual")
_CACHE = {}


def c_tables(parameters=None):
    return hh.c_tables(parameters)


def plane(X):
    """(centroid, unit normal, rms distance from the plane) of points X [n,3]: the eigenvector of the smallest eigenvalue of the
    scatter matrix, its component of largest magnitude positive (the lower index wins a tie)."""
    c = X.mean(0)
    w, V = np.linalg.eigh((X - c).T @ (X - c))
    n = V[:, 0]
    k = int(np.argmax(np.abs(n) >= np.abs(n).max()))
    n = n if n[k] > 0 else -n
    return c, n, float(np.sqrt(max(w[0], 0.0) / len(X)))


def chordless_cycles(nbrs, sizes=(4, 5, 6)):
    """Every chordless cycle of the given sizes in the graph {vertex: set of neighbours}: a list of vertex tuples in cyclic order,
    each cycle once, from its smallest vertex, sorted by sorted vertex tuple."""
    found = {}

    def walk(path):
        last = path[-1]
        for nxt in sorted(nbrs[last]):
            if nxt == path[0] and len(path) in sizes:
                S = set(path)
                if all(len(nbrs[v] & S) == 2 for v in path):
                    found.setdefault(tuple(sorted(path)), tuple(path))
            if nxt > path[0] and nxt not in path and len(path) < max(sizes):
                walk(path + [nxt])

    for v in sorted(nbrs):
        walk([v])
    return [found[k] for k in sorted(found)]


def oracle(mol, charge=0, field=FIELD):
    """Section 8p by the book in float64 on the float32-rounded coordinates -> dict (zeros where the status is not OK)."""
    elem, bonds, xyz = mol
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    xyz = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    n, T = len(elem), hh.table()
    names = list(T["classes"])
    out = dict(status=OK, flags=0, n_pi=0, n_electrons=0, gap=0.0, bond_current=np.zeros(len(bonds)), n_rings=0, rings=[],
               ring_current=np.zeros(0), ring_area=np.zeros(0), normal=np.zeros(3), rms_out_of_plane=0.0, residual=0.0)
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
    n_el = sum(p["n_e"] for p in par) - charge
    if n_el < 0 or n_el > 2 * len(pi):
        return dict(out, status=BAD_INPUT)
    if n_el & 1:
        return dict(out, status=OPEN_SHELL)
    m, at = len(pi), {a: r for r, a in enumerate(pi)}
    E = -np.diag([float(p["h"]) for p in par])
    pig = {r: set() for r in range(m)}
    for a in pi:
        for o in nbrs[a]:
            if o in at:
                key = [k for k in (f"{names[cls[a]]}|{names[cls[o]]}", f"{names[cls[o]]}|{names[cls[a]]}") if k in T.get("k_pair", {})]
                E[at[a], at[o]] = -(T["k_pair"][key[0]] if key else par[at[a]]["k"] * par[at[o]]["k"])
                pig[at[a]].add(at[o])
    n_edges = sum(len(v) for v in pig.values()) // 2
    seen, comps = set(), 0
    for r in range(m):
        if r not in seen:
            comps += 1
            todo = [r]
            while todo:
                v = todo.pop()
                if v not in seen:
                    seen.add(v)
                    todo.extend(pig[v] - seen)
    cyclo = n_edges - m + comps
    n_occ = n_el // 2
    eps = np.linalg.eigvalsh(E)
    gap = float(eps[n_occ] - eps[n_occ - 1]) if 0 < n_occ < m else 0.0
    out.update(n_pi=m, n_electrons=n_el, gap=gap)
    if not 0 < n_occ < m or gap < SMALL:
        return dict(out, status=SMALL_GAP, n_pi=0, n_electrons=0, gap=0.0)
    if cyclo == 0:
        return out
    X = xyz[pi]
    R = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1))
    if not np.isfinite(X).all() or (R + 10.0 * np.eye(len(pi)) < 0.5).any():
        return dict(out, status=BAD_GEOMETRY, n_pi=0, n_electrons=0, gap=0.0)
    c, nrm, rms = plane(X)
    D = X - c
    s = 0.5 * np.einsum("k,rsk->rs", nrm, np.cross(D[:, None, :], D[None, :, :]))
    Hf = E * np.exp(1j * field * s)
    w, V = np.linalg.eigh(Hf)
    P = 2.0 * V[:, :n_occ] @ V[:, :n_occ].conj().T
    J = 2.0 * np.imag(Hf * P.T) / field
    cur = np.zeros(len(bonds))
    for k, (i, j) in enumerate(bonds):
        if int(i) in at and int(j) in at:
            cur[k] = -J[at[int(i)], at[int(j)]] / C0
    out.update(bond_current=cur, normal=nrm, rms_out_of_plane=rms)
    rings = []
    for cyc in chordless_cycles(pig):
        area = sum(s[cyc[j], cyc[(j + 1) % len(cyc)]] for j in range(len(cyc)))
        if area < 0:
            cyc, area = (cyc[0],) + tuple(reversed(cyc[1:])), -area
        rings.append((cyc, area))
    undefined = len(rings) != cyclo or len(rings) > MAX_RINGS or any(a <= MIN_AREA for _, a in rings)
    if not undefined:
        listed = [(k, at[int(i)], at[int(j)]) for k, (i, j) in enumerate(bonds) if int(i) in at and int(j) in at]
        Cm = np.zeros((len(listed), len(rings)))
        for q, (cyc, _) in enumerate(rings):
            for j in range(len(cyc)):
                x, y = cyc[j], cyc[(j + 1) % len(cyc)]
                for e, (_, r, t) in enumerate(listed):
                    Cm[e, q] += (r, t) == (x, y)
                    Cm[e, q] -= (r, t) == (y, x)
        b = np.array([cur[k] for k, _, _ in listed])
        I, _, rank, _ = np.linalg.lstsq(Cm, b, rcond=None)
        undefined = rank < len(rings)
    if undefined:
        return dict(out, flags=RINGS_UNDEFINED)
    return dict(out, n_rings=len(rings), rings=[tuple(pi[v] for v in cyc) for cyc, _ in rings], ring_current=I,
                ring_area=np.array([a for _, a in rings]), residual=float(np.abs(Cm @ I - b).max()))


# ---- molecules: (elem [n], bonds [m,2], xyz [n,3]) triples

def polyhex(cells):
    """Fused regular hexagons of side 1.40 A, all carbon, no listed hydrogen: ``cells`` are the hexagons' lattice coordinates (q, r),
    their centres at q * (1, 0) + r * (cos 60, sin 60) times 1.40 * sqrt(3).  -> (molecule, the centres [len(cells),3])."""
    step = SIDE * np.sqrt(3.0)
    index, xyz, bonds, centres = {}, [], set(), []
    for q, r in cells:
        centre = step * (q * np.array([1.0, 0.0]) + r * np.array([0.5, np.sqrt(0.75)]))
        centres.append([centre[0], centre[1], 0.0])
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
    return (np.array([C] * len(xyz), np.int32), np.array(sorted(bonds), np.int32).reshape(-1, 2), np.array(xyz, np.float64)), np.array(centres)


# name -> (cells, the ring current of every cell): the textbook Hueckel-London values the issue lists
KNOWN = {
    "benzene": ([(0, 0)], [1.0]),
    "naphthalene": ([(0, 0), (1, 0)], [1.0926, 1.0926]),
    "anthracene": ([(0, 0), (1, 0), (2, 0)], [1.0844, 1.2794, 1.0844]),
    "tetracene": ([(0, 0), (1, 0), (2, 0), (3, 0)], [1.0680, 1.3054, 1.3054, 1.0680]),
    "phenanthrene": ([(0, 0), (1, 0), (1, 1)], [1.1366, 0.9748, 1.1366]),
    "pyrene": ([(0, 0), (1, 0), (0, 1), (1, 1)], [1.3267, 0.9634, 0.9634, 1.3267]),
    "triphenylene": ([(0, 0), (1, 0), (-1, 1), (0, -1)], [0.7483, 1.1093, 1.1093, 1.1093]),
    "coronene": ([(0, 0), (1, 0), (0, 1), (-1, 1), (-1, 0), (0, -1), (1, -1)], [1.0376] + [1.4593] * 6),
}


def known(name):
    return polyhex(KNOWN[name][0])[0]


def by_cell(name, rec, mol):
    """The ring currents of a result (a dict with ``rings`` / ``ring_current``) in the order of KNOWN[name]'s cells."""
    _, centres = polyhex(KNOWN[name][0])
    xyz = np.asarray(mol[2])
    got = []
    for c in centres:
        hit = [k for k, ring in enumerate(rec["rings"]) if np.abs(xyz[list(ring)].mean(0) - c).max() < 1e-3]
        assert len(hit) == 1
        got.append(float(rec["ring_current"][hit[0]]))
    return got


def acene(rings):
    return polyhex([(k, 0) for k in range(rings)])[0]


def cyclobutadiene():
    return pp.cycle([C] * 4)


def biphenyl():
    """Two regular hexagons joined by a 1.48 A bond along x."""
    (e, b, x), _ = polyhex([(0, 0)])
    x = x @ np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # a vertex on the x axis
    right = int(np.argmax(x[:, 0]))
    x2 = x.copy()
    x2[:, 0] = -x2[:, 0] + 2 * x[right, 0] + 1.48
    left2 = 6 + int(np.argmin(x2[:, 0]))
    return (np.concatenate([e, e]), np.concatenate([b, b + 6, [[right, left2]]]).astype(np.int32), np.concatenate([x, x2])), len(b) * 2


def bent(mol, angle_deg=20.0):
    """The molecule folded about the y axis through its centroid: the atoms right of it are lifted out of the plane."""
    e, b, x = mol
    x = np.array(x, np.float64)
    mid = x[:, 0].mean()
    t = np.deg2rad(angle_deg)
    r = x[:, 0] > mid
    d = x[r, 0] - mid
    x[r, 0], x[r, 2] = mid + d * np.cos(t), d * np.sin(t)
    return e, b, x


def rotated(mol, seed):
    """The molecule under a random proper rotation and a translation."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.linalg.det(Q))
    e, b, x = mol
    return e, b, np.asarray(x, np.float64) @ Q.T + rng.uniform(-3.0, 3.0, 3), Q


def relabelled(mol, seed):
    """The atoms in a random order and the bond list shuffled, its pairs swapped at random -> (molecule, perm: old atom -> new,
    order: new bond k was old bond order[k], swapped [m] bool)."""
    rng = np.random.default_rng(seed)
    e, b, x = mol
    b = np.asarray(b).reshape(-1, 2)
    perm = rng.permutation(len(e))
    inv = np.argsort(perm)
    order = rng.permutation(len(b))
    swapped = rng.random(len(b)) < 0.5
    nb = perm[b[order]]
    nb[swapped] = nb[swapped][:, ::-1]
    return (np.asarray(e)[inv].astype(np.int32), nb.astype(np.int32), np.asarray(x)[inv]), perm, order, swapped


def _charge(charge, B):
    return None if charge is None else np.ascontiguousarray(np.broadcast_to(np.asarray(charge, np.int32), (B,)))


def host(mols, charge=None, parameters=None, A=None, M=None):
    """Triples -> the raw outputs of the host build."""
    return _lib.host_ring_currents(c_tables(parameters), *pp.pack(mols, A, M), _charge(charge, len(mols)))


def device(engine, mols, charge=None, parameters=None, A=None, M=None):
    return engine.ring_currents(c_tables(parameters), *pp.pack(mols, A, M), _charge(charge, len(mols)))


class HostEngine:
    """What gaudi_amd.aromaticity.ring_currents asks of an engine, on the kernel's host build."""

    def ring_currents(self, *args):
        return _lib.host_ring_currents(*args)


def record(out, i, mol):
    """Row i of raw outputs as the oracle returns a molecule."""
    r, m = int(out["n_rings"][i]), len(np.asarray(mol[1]).reshape(-1, 2))
    return dict(status=int(out["status"][i]), flags=int(out["flags"][i]), n_pi=int(out["n_pi"][i]), n_electrons=int(out["n_electrons"][i]),
                gap=float(out["gap"][i]), bond_current=out["bond_current"][i, :m].astype(np.float64), n_rings=r,
                rings=[tuple(int(a) for a in out["ring_atoms"][i, k, :out["ring_size"][i, k]]) for k in range(r)],
                ring_current=out["ring_current"][i, :r].astype(np.float64), ring_area=out["ring_area"][i, :r].astype(np.float64),
                normal=out["normal"][i].astype(np.float64), rms_out_of_plane=float(out["rms_out_of_plane"][i]),
                residual=float(out["residual"][i]), sweeps=int(out["sweeps"][i]))


def worst(got, want):
    """The largest |got - want| / max(1, |want|) over every float of two results of one molecule (their integers asserted equal)."""
    for k in ("status", "flags", "n_pi", "n_electrons", "n_rings"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert [tuple(r) for r in got["rings"]] == [tuple(r) for r in want["rings"]]
    err = 0.0
    for k in FLOATS:
        g, w = np.atleast_1d(np.asarray(got[k], np.float64)), np.atleast_1d(np.asarray(want[k], np.float64))
        assert g.shape == w.shape, k
        if len(g):
            err = max(err, float((np.abs(g - w) / np.maximum(1.0, np.abs(w))).max()))
    return err


def g30_molecules():
    return pp.g30_molecules()


def g30_oracle():
    if "g30_oracle" not in _CACHE:
        _CACHE["g30_oracle"] = [oracle(m) for m in g30_molecules()]
    return _CACHE["g30_oracle"]


def g30_host():
    """The host build's outputs for the whole of g30, computed once, never written to."""
    if "g30_host" not in _CACHE:
        out = host(g30_molecules())
        for a in out.values():
            a.setflags(write=False)
        _CACHE["g30_host"] = out
    return _CACHE["g30_host"]


def assert_same_bits(got, want, rows=None):
    """Every output array equal in dtype, shape and bytes (floats compared as their bits)."""
    for name in _lib.RING_CURRENT_ARRAYS:
        g, w = got[name], want[name] if rows is None else want[name][rows]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), name
