"""Shared by test_ppp_scf_cpu.py and test_gpu_ppp_scf.py: a float64 restatement in numpy of the PPP SCF with Pulay's DIIS of DESIGN.md
section 8t (the model of sections 8m / 8s, numpy.linalg.eigh with an occupation vector 2 / 1 / 0, commutator DIIS with a ring of
``diis_size`` entries from iteration ``diis_start`` on, a hand-written Gaussian elimination; it reads the table file itself and shares
no code with the kernel), the host build as an engine stand-in, and results computed once.

MEASURED (the host build, which the device equals bit for bit, against this oracle, over every settled row of ``compared_sets``: g30
under the four state kinds and ``small_rows()``; default settings).  The largest error of
  a level / homo / lumo / gap / e_state per centre                  MEASURED_EV
  he_correction                                                     MEASURED_HE
  a charge / bond order / spin density                              MEASURED_P
  a difference ip / ea / t1 of two e_state values                   MEASURED_DIFF
The tolerances are four times that (the convention of sections 8m and 8s); the hard conditions are TOL_EV, TOL_HE, TOL_DIFF <= 2e-3
eV and TOL_P <= 2e-4; four times the density figure would pass the hard condition, so the hard condition itself is the tolerance.
These are below section 8s's figures (3.32e-4, 2.42e-4, 1.68e-4, 2.34e-4): without damping the iteration stops closer to its
fixed point.

DIIS_ERROR is the kernel's kPppDiisError, 2^-10 eV.  The largest ``diis_error`` the host build shows on the compared rows under it
is MEASURED_DIIS_ERROR = 2.88e-4 eV: a margin of 3.4, not of 4.  "The smallest power of two at least four times the largest
measured value" has no answer here, because the bound decides where a row stops and so what is measured: under 2^-9 the largest
value is 1.45e-3 eV (the 15-centre radical of ``small_rows()`` then stops at iteration 6, 4.4e-4 from the fixed point's densities --
beyond the hard condition of 2e-4), and under 2^-7 it is larger again.  A commutator e leaves a density error of about e over
the smallest occupied-to-empty level difference (2 to 7 eV on these molecules), so 2^-10 eV keeps a row that the rule accepts within
the 2e-4 asked of the densities, while no compared row is held back by it for the fp32 commutator's rounding alone (every one of
them passes it within the cap)."""
import os

import numpy as np

from gaudi_amd import _lib
from tests.ppp_helpers import (ATOMS, BAD_GEOMETRY, BAD_INPUT, CAP, EMPTY, GOLDEN, NO_PI, NOT_CONVERGED, OK, OVERFLOW, STOP, _charge, c_tables,
                               pack, table)
from tests.ppp_open_helpers import KINDS, _mult, edge_molecule, g30_rows, small_rows
from tests.substructure_helpers import graph_of

MEASURED_EV, MEASURED_HE, MEASURED_P, MEASURED_DIFF = 5.98e-5, 7.30e-5, 9.08e-5, 9.55e-5  # eV, eV, electrons, eV
MEASURED_DIIS_ERROR = 2.88e-4  # eV
DIIS_ERROR = 2.0 ** -10  # eV: kPppDiisError
TOL_EV, TOL_HE, TOL_P, TOL_DIFF = 4 * MEASURED_EV, 4 * MEASURED_HE, min(4 * MEASURED_P, 2e-4), 4 * MEASURED_DIFF
assert max(TOL_EV, TOL_HE, TOL_DIFF) <= 2e-3 and TOL_P <= 2e-4
assert 3 * MEASURED_DIIS_ERROR <= DIIS_ERROR
PIVOT = 2.0 ** -40
LONG_JOBS = os.path.join(GOLDEN, "ppp_scf_long_jobs.npz")
_CACHE = {}


def _combine(Bm):
    """The DIIS coefficients of a scaled B matrix [m, m]: the bordered system [[B, 1], [1^T, 0]] (c, lambda) = (0, 1) by Gaussian
    elimination with partial pivoting (the first largest element of a column).  None: a pivot below 2^-40."""
    m = len(Bm)
    N = m + 1
    M = np.zeros((N, N + 1))
    M[:m, :m], M[:m, m], M[m, :m], M[m, N] = Bm, 1.0, 1.0, 1.0
    for p in range(N):
        pr, big = p, abs(M[p, p])
        for i in range(p + 1, N):
            if abs(M[i, p]) > big:
                pr, big = i, abs(M[i, p])
        if not big >= PIVOT:
            return None
        if pr != p:
            M[[p, pr]] = M[[pr, p]]
        for i in range(p + 1, N):
            f = M[i, p] / M[p, p]
            for j in range(p + 1, N + 1):
                M[i, j] = M[i, j] - f * M[p, j]
    x = np.zeros(N)
    for i in range(N - 1, -1, -1):
        acc = M[i, N]
        for j in range(i + 1, N):
            acc = acc - M[i, j] * x[j]
        x[i] = acc / M[i, i]
    return x[:m]


def _model(mol, charge, multiplicity, repulsion):
    """The model of sections 8m / 8s -> a refusal status, or what the iteration needs."""
    elem, bonds, xyz = mol
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    xyz = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    n, T = len(elem), table()
    names = list(T["classes"])
    if n == 0:
        return EMPTY
    if n > 384 or len(bonds) > 384:
        return OVERFLOW
    pairs = [tuple(sorted((int(i), int(j)))) for i, j in bonds]
    if ((elem < 0) | (elem >= len(ATOMS))).any() or any(i < 0 or j >= n or i == j for i, j in pairs) or len(set(pairs)) != len(pairs):
        return BAD_INPUT
    heavy, attr, nbrs = graph_of(elem, bonds)
    deg = np.bincount(bonds.reshape(-1), minlength=n) if len(bonds) else np.zeros(n, np.int64)
    if len(heavy) > 192 or deg.max() > 8:
        return OVERFLOW
    cls = {}
    for a in heavy:
        e, n_h, hd = attr[a]
        name = T["sites"].get(ATOMS[e], {}).get(str(n_h + hd))
        if name is not None:
            cls[a] = names.index(name)
    pi = sorted(cls)
    if not pi:
        return NO_PI
    if len(pi) > 128:
        return OVERFLOW
    m = len(pi)
    par = [T["classes"][names[cls[a]]] for a in pi]
    z = np.array([float(p["z"]) for p in par])
    n_el = int(z.sum()) - charge
    if n_el < 0 or n_el > 2 * m or not 0 <= multiplicity <= 3:
        return BAD_INPUT
    n_open = (multiplicity or 1 + (n_el & 1)) - 1
    if n_el < n_open or (n_el - n_open) & 1 or (n_el - n_open) // 2 + n_open > m:
        return BAD_INPUT
    X = xyz[pi]
    R = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1))
    if not np.isfinite(X).all() or (R + 10.0 * np.eye(m) < 0.5).any():
        return BAD_GEOMETRY
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
    return dict(n=n, m=m, bonds=bonds, pi=pi, at=at, cls=cls, z=z, n_el=n_el, n_open=n_open, n_c=(n_el - n_open) // 2, g1=g1, G=G, G0=G0,
                Hc=beta + np.diag(-ion - G0 @ z), n_heavy=len(heavy))


def _iterate(Q, diis_size, diis_start, damping, round32, limit):
    """The iteration of section 8t, ``limit`` times at the most or until delta_p <= 1e-10 and the commutator <= 1e-8 -> (the last
    eigenvectors' density, per iteration: delta_p, diis_error, the boundary gap, whether F was a combination)."""
    m, n_c, n_open, g1, G0, Hc = Q["m"], Q["n_c"], Q["n_open"], Q["g1"], Q["G0"], Q["Hc"]
    occ = np.array([2.0] * n_c + [1.0] * n_open + [0.0] * (m - n_c - n_open))
    top = n_c + n_open
    r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if round32 else (lambda a: a)

    def fock(P):
        d = np.diag(P)
        return Hc + np.diag(0.5 * d * g1 + G0 @ d) - 0.5 * P * G0

    def boundary(w):
        gaps = [np.inf]
        if n_open and n_c >= 1:
            gaps.append(w[n_c] - w[n_c - 1])
        if n_open and top < m:
            gaps.append(w[top] - w[top - 1])
        return float(min(gaps))

    P = np.diag(Q["z"])
    Fs, Es, Bm = [], [], np.zeros((0, 0))
    trace = []
    Pn = P
    for k in range(1, limit + 1):
        F = r32(fock(P))
        use, err, mixed = F, 0.0, False
        if k >= diis_start:
            G_ = F @ P
            e = r32(G_ - G_.T)
            err = float(np.abs(e).max())
            if len(Fs) == diis_size:
                Fs, Es, Bm = Fs[1:], Es[1:], Bm[1:, 1:]
            Fs.append(F)
            Es.append(e)
            new = np.array([float((ei * e).sum()) for ei in Es])
            Bm = np.block([[Bm, new[:-1, None]], [new[None, :-1], new[-1:, None]]])
            first = 0
            while len(Fs) - first >= 2:
                sub = Bm[first:, first:]
                c = _combine(sub / np.diag(sub).max()) if np.diag(sub).max() > 0.0 else None
                if c is not None:
                    c32 = c.astype(np.float32).astype(np.float64)
                    use, mixed = r32(sum(ci * Fi for ci, Fi in zip(c32, Fs[first:]))), True
                    break
                first += 1
            Fs, Es, Bm = Fs[first:], Es[first:], Bm[first:, first:]
        w, V = np.linalg.eigh(use)
        Pn = r32((V * occ) @ V.T)
        delta = float(np.abs(Pn - P).max())
        trace.append((delta, err, boundary(w), mixed))
        P = Pn if k >= diis_start else r32((1.0 - damping) * Pn + damping * P)
        if delta <= 1e-10 and err <= 1e-8:
            break
    return Pn, trace


def _kernel_rule(trace):
    first = next((k + 1 for k, t in enumerate(trace[:CAP]) if t[0] <= STOP and t[1] <= DIIS_ERROR), None)
    return first


def oracle(mol, charge=0, multiplicity=0, repulsion="mataga-nishimoto", damping=0.25, diis_size=6, diis_start=3):
    """Section 8t by the book in float64 on the float32-rounded coordinates -> dict.  The iteration is run to delta_p <= 1e-10 and a
    commutator <= 1e-8 (at most 200 times): the values are that point's (``fixed`` says whether it was reached).  The same trajectory
    read under the kernel's rule (delta_p <= 2^-16 and diis_error <= DIIS_ERROR, 64 iterations) gives ``status``, ``iterations``,
    ``n_extrapolated`` and ``decisive`` as tests/ppp_helpers.py defines it.  ``settled``: the answer does not hang on rounding -- the
    boundary tie is at least 1e-2 eV over the iterations run, the oracle converged in at most 56 iterations, a second run with F, e
    and P rounded to float32 in every iteration reaches the same e_state within 1e-3 eV, and where the fixed-point oracle of
    tests/ppp_open_helpers.py reached its fixed point its e_state agrees within 1e-3 eV."""
    out = dict(status=OK, n_pi=0, n_electrons=0, n_excluded=0, iterations=0, decisive=True, settled=True, fixed=False, tie=np.inf, n_open=0,
               n_extrapolated=0)
    Q = _model(mol, charge, multiplicity, repulsion)
    if not isinstance(Q, dict):
        return dict(out, status=Q)
    res = _result(Q, *_iterate(Q, diis_size, diis_start, damping, False, 200))
    if res["status"] == OK and res["tie"] >= 1e-2 and res["iterations"] <= CAP - 8:
        again = _result(Q, *_iterate(Q, diis_size, diis_start, damping, True, 200))
        settled = again["status"] == OK and abs(again["e_state"] - res["e_state"]) <= 1e-3
        if settled:
            from tests.ppp_open_helpers import oracle as fixed_point
            other = fixed_point(mol, charge, multiplicity, repulsion, damping)
            settled = not other["fixed"] or abs(other["e_state"] - res["e_state"]) <= 1e-3
    else:
        settled = False
    return dict(out, **res, settled=settled)


def _result(Q, Pn, trace):
    m, n_c, n_open, g1, G, G0, Hc, z, at, pi, bonds, n = (Q[k] for k in ("m", "n_c", "n_open", "g1", "G", "G0", "Hc", "z", "at", "pi", "bonds", "n"))
    top = n_c + n_open
    occ = np.array([2.0] * n_c + [1.0] * n_open + [0.0] * (m - top))
    first = _kernel_rule(trace)
    converged = first is not None
    decisive = (converged and first <= CAP - 8) or (not converged and len(trace) >= CAP and trace[CAP - 1][0] >= 1e-4)
    run = first if converged else min(CAP, len(trace))
    d = np.diag(Pn)
    F = Hc + np.diag(0.5 * d * g1 + G0 @ d) - 0.5 * Pn * G0
    w, V = np.linalg.eigh(F)
    Pn = (V * occ) @ V.T
    e_he = 0.5 * float((Pn * (Hc + F)).sum())
    open_cols = [V[:, k] for k in range(n_c, top)]
    J = [float((v ** 2) @ G @ (v ** 2)) for v in open_cols]
    corr = 0.0
    if n_open == 1:
        corr = -J[0] / 4
    elif n_open == 2:
        mn = open_cols[0] * open_cols[1]
        corr = -(J[0] + J[1]) / 4 - float(mn @ G @ mn) / 2
    e_core = float(np.triu(np.outer(z, z) * G0, 1).sum())
    ih, il = top - 1, top
    ih = il if ih < 0 else ih
    il = ih if il >= m else il
    gaps = [np.inf]
    if n_open and n_c >= 1:
        gaps.append(w[n_c] - w[n_c - 1])
    if n_open and top < m:
        gaps.append(w[top] - w[top - 1])
    q, p, spin = np.zeros(n), np.zeros(len(bonds)), np.zeros(n)
    site = np.full(n, -1, np.int64)
    for a in pi:
        site[a] = Q["cls"][a]
        q[a] = z[at[a]] - Pn[at[a], at[a]]
        spin[a] = sum(v[at[a]] ** 2 for v in open_cols)
    for k, (i, j) in enumerate(bonds):
        if int(i) in at and int(j) in at:
            p[k] = Pn[at[int(i)], at[int(j)]]
    last = trace[-1]
    return dict(status=OK if converged else NOT_CONVERGED, iterations=run, decisive=decisive, fixed=last[0] <= 1e-10 and last[1] <= 1e-8,
                history=[t[0] for t in trace], errors=[t[1] for t in trace], n_extrapolated=sum(t[3] for t in trace[:run]),
                tie=min(min(t[2] for t in trace[:run]), float(min(gaps))), n_pi=m, n_electrons=Q["n_el"], n_excluded=Q["n_heavy"] - m,
                n_open=n_open, somo=[n_c + k if k < n_open else -1 for k in range(2)], site_class=site, levels=w,
                occupation=occ.astype(np.int64), homo=w[ih], lumo=w[il], gap=w[il] - w[ih], e_he=e_he, he_correction=corr, e_core=e_core,
                e_state=e_he + corr + e_core, pi_charge=q, pi_bond_order=p, spin_density=spin)


def comparable(ref):
    """A row whose values the host build is held to: settled, and run to the oracle's fixed point."""
    return ref["status"] == OK and ref["settled"] and ref["fixed"]


# ---- rows, the host build, results computed once

def long_rows():
    """The rows that take the host build seconds each: the 126-, 127- and 128-centre tier-edge molecules with one electron removed.
    Their host results are recorded in tests/golden/ppp_scf_long_jobs.npz; the CPU suite holds the record to the live host build and
    the GPU suite holds the device to the record."""
    rows = [edge_molecule(n) for n in (126, 127, 128)]
    return [m for m, _ in rows], np.array([q + 1 for _, q in rows], np.int32), np.zeros(3, np.int32), ["edge 126", "edge 127", "edge 128"]


def long_host():
    if "long" not in _CACHE:
        z = np.load(LONG_JOBS)
        _CACHE["long"] = {k: z[k] for k in _lib.PPP_SCF_ARRAYS}
    return _CACHE["long"]


def write_long_host():
    np.savez_compressed(LONG_JOBS, **hosts("long", long_rows()))


def compared_sets():
    return {"g30": g30_rows(), "small": small_rows()}


def oracles(key, rows, **settings):
    """The oracle's results for a row set, computed once per settings."""
    tag = ("oracle", key, tuple(sorted(settings.items())))
    if tag not in _CACHE:
        mols, charge, mult, _ = rows
        _CACHE[tag] = [oracle(m, int(q), int(s), **settings) for m, q, s in zip(mols, charge, mult)]
    return _CACHE[tag]


def host(mols, charge=None, multiplicity=None, repulsion=0, damping=0.25, diis_size=6, diis_start=3, parameters=None, A=None, M=None):
    """Triples -> the raw outputs of the host build."""
    return _lib.host_ppp_scf(c_tables(parameters), *pack(mols, A, M), _charge(charge, len(mols)), _mult(multiplicity, len(mols)),
                             repulsion, diis_size, diis_start, damping)


def device(engine, mols, charge=None, multiplicity=None, repulsion=0, damping=0.25, diis_size=6, diis_start=3, parameters=None, A=None,
           M=None):
    return engine.ppp_scf(c_tables(parameters), *pack(mols, A, M), _charge(charge, len(mols)), _mult(multiplicity, len(mols)),
                          repulsion, diis_size, diis_start, damping)


class HostEngine:
    """What gaudi_amd.ppp asks of an engine, on the kernels' host builds."""

    def ppp(self, *args):
        return _lib.host_ppp(*args)

    def ppp_open(self, *args):
        return _lib.host_ppp_open(*args)

    def ppp_scf(self, *args):
        return _lib.host_ppp_scf(*args)


def hosts(key, rows, **settings):
    """The host build's outputs for a row set in one call, computed once per settings, never written to."""
    tag = ("host", key, tuple(sorted(settings.items())))
    if tag not in _CACHE:
        mols, charge, mult, _ = rows
        out = host(mols, charge, mult, **settings)
        for a in out.values():
            a.setflags(write=False)
        _CACHE[tag] = out
    return _CACHE[tag]


def assert_same_bits(got, want, rows=None, names=None):
    """Every output array equal in dtype, shape and bytes (floats and doubles compared as their bits)."""
    for name in names or _lib.PPP_SCF_ARRAYS:
        g, w = got[name], want[name] if rows is None else want[name][rows]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), name
