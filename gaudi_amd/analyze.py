"""Host mirror of analyze/analyze.py (graph-of-rings stability) on top of gaudi_check_stability.

Same call shapes as the reference -- ``check_stability(positions, ring_type, tol, dataset)`` for one molecule,
``analyze_validity_for_molecules(molecule_list, tol, dataset)`` for a list of ``(positions, ring_type)`` pairs,
``positions2adj(x, ring_type, tol, dataset)`` for a batch -- but all molecules of a call are checked in ONE kernel launch
(one wavefront per molecule).  The geometry tables (ring-ring distance windows, 3-ring angle windows, dihedral
thresholds: utils/helpers.py:11-157) ship as data in ``gaudi_amd/data/ring_tables.json``.  There is no CPU
implementation behind these functions: without the HIP library they raise GaudiError."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from ._lib import GaudiError, RingTables, StabilityAux, f32, fptr

FLAG_NAMES = ("orientation_nodes", "dist_stable", "connected", "angels3", "angels4")
_TABLES = None


def ring_tables() -> dict:
    global _TABLES
    if _TABLES is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "ring_tables.json")) as f:
            _TABLES = json.load(f)
    return _TABLES


def rings_list(dataset: str):
    """RINGS_LIST[dataset] (data/aromatic_dataloader.py:31-35)."""
    return ring_tables()["rings"][_key(dataset)]


def _key(dataset: str) -> str:
    if dataset == "peri":  # same rings and distances as cata (utils/helpers.py:151-155); angle tables are cata's
        return "cata"
    if dataset not in ("cata", "hetro"):
        raise GaudiError(f"no geometry tables for dataset {dataset!r}")
    return dataset


def c_tables(dataset: str, tol: float = 0.1) -> RingTables:
    """gaudi_ring_tables for one dataset."""
    ds = _key(dataset)
    T = ring_tables()
    R = len(T["rings"][ds])
    t = RingTables()
    t.n_types = R
    t.orientation = int(dataset != "cata")  # analyze/analyze.py:66
    t.check_dihedrals = int(dataset != "hetro")  # analyze/analyze.py:40
    t.tol = float(tol)
    t.min_dist = float(T["min_dist"][ds])
    for i in range(R):
        for j in range(R):
            t.dist_lo[i][j] = T["dist_lo"][ds][i][j]
            t.dist_hi[i][j] = T["dist_hi"][ds][i][j]
        wins = T["a3"][ds][i]
        t.a3_count[i] = len(wins)
        for q, (lo, hi) in enumerate(wins):
            t.a3_lo[i][q], t.a3_hi[i][q] = lo, hi
    t.a4_0, t.a4_180 = T["a4"][ds]["0"], T["a4"][ds]["180"]
    return t


def _np(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _engine(engine):
    if engine is not None:
        return engine
    from .engine import Engine
    return Engine.default()


def check_stability_batch(x, ring_type, n_nodes, tol=0.1, dataset="cata", engine=None, want_adj=False, want_aux=False):
    """x [B,N,3], ring_type [B,N] (int) and n_nodes [B] with each molecule's valid nodes first
    -> flags [B,5] bool (FLAG_NAMES order) (+ dist, adj [B,N,N]) (+ aux record array)."""
    eng = _engine(engine)
    x = f32(x)
    B, N = x.shape[0], x.shape[1]
    ty = np.ascontiguousarray(_np(ring_type), dtype=np.int32).reshape(B, N)
    nn = np.ascontiguousarray(_np(n_nodes), dtype=np.int32).reshape(B)
    flags = np.zeros((B, 5), np.uint8)
    dist = np.zeros((B, N, N), np.float32) if want_adj else None
    adj = np.zeros((B, N, N), np.float32) if want_adj else None
    aux = (StabilityAux * B)() if want_aux else None
    t = c_tables(dataset, tol)
    rc = eng.lib.gaudi_check_stability(eng.h, C.byref(t), B, N, fptr(x), ty.ctypes.data_as(C.POINTER(C.c_int32)),
                                       nn.ctypes.data_as(C.POINTER(C.c_int32)),
                                       flags.ctypes.data_as(C.POINTER(C.c_uint8)), fptr(dist), fptr(adj), aux)
    eng._check(rc, "gaudi_check_stability")
    out = [flags.astype(bool)]
    if want_adj:
        out += [dist, adj]
    if want_aux:
        out.append(np.array([tuple(getattr(a, f) for f, _ in StabilityAux._fields_) for a in aux],
                            dtype=[(f, np.int32 if "n_" in f else np.float32) for f, _ in StabilityAux._fields_]))
    return out[0] if len(out) == 1 else tuple(out)


def _pack(molecule_list):
    B = len(molecule_list)
    if B == 0:
        raise GaudiError("empty molecule list")
    xs = [_np(x).astype(np.float32).reshape(-1, 3) for x, _ in molecule_list]
    ts = []
    for _, t in molecule_list:
        t = _np(t)
        ts.append((t.argmax(1) if t.ndim == 2 else t).astype(np.int32))  # analyze/analyze.py:62-63
    N = max(1, max(len(x) for x in xs))
    X = np.zeros((B, N, 3), np.float32)
    T = np.zeros((B, N), np.int32)
    nn = np.zeros(B, np.int32)
    for b, (x, t) in enumerate(zip(xs, ts)):
        if len(x) != len(t):
            raise GaudiError(f"molecule {b}: {len(x)} positions but {len(t)} ring types")
        X[b, : len(x)], T[b, : len(x)], nn[b] = x, t, len(x)
    return X, T, nn


def check_stability(positions, ring_type, tol=0.1, dataset="cata", engine=None) -> dict:
    """analyze/analyze.py:50-100 for one molecule -> {orientation_nodes, dist_stable, connected, angels3, angels4}."""
    X, T, nn = _pack([(positions, ring_type)])
    flags = check_stability_batch(X, T, nn, tol, dataset, engine)
    return {k: bool(v) for k, v in zip(FLAG_NAMES, flags[0])}


def analyze_validity_for_molecules(molecule_list, tol=0.1, dataset="cata", engine=None):
    """analyze/analyze.py:139-177 -> (validity_dict, molecule_stable_list); one launch for the whole list."""
    X, T, nn = _pack(molecule_list)
    flags = check_stability_batch(X, T, nn, tol, dataset, engine)
    stable = flags.all(1)
    n = float(len(molecule_list))
    d = {"mol_stable": int(stable.sum()) / n}
    for i, k in enumerate(FLAG_NAMES):
        d[k] = int(flags[:, i].sum()) / n
    d["molecule_stable_bool"] = [bool(s) for s in stable]
    return d, [m for m, s in zip(molecule_list, stable) if s]


def positions2adj(x, ring_type, tol=0.1, dataset="cata", engine=None):
    """utils/helpers.py:167-190: x [B,n,3], ring_type [B,n] or one-hot [B,n,R] -> (dist, adj) [B,n,n].  Every node is
    treated as a ring (the reference function knows nothing about orientation nodes)."""
    x = f32(_np(x))
    t = _np(ring_type)
    if t.ndim == 3:
        t = t.argmax(2)
    B, N = x.shape[0], x.shape[1]
    tb = c_tables(dataset, tol)
    tb.orientation = 0
    eng = _engine(engine)
    flags = np.zeros((B, 5), np.uint8)
    dist = np.zeros((B, N, N), np.float32)
    adj = np.zeros((B, N, N), np.float32)
    ty = np.ascontiguousarray(t, dtype=np.int32)
    nn = np.full(B, N, np.int32)
    rc = eng.lib.gaudi_check_stability(eng.h, C.byref(tb), B, N, fptr(x), ty.ctypes.data_as(C.POINTER(C.c_int32)),
                                       nn.ctypes.data_as(C.POINTER(C.c_int32)),
                                       flags.ctypes.data_as(C.POINTER(C.c_uint8)), fptr(dist), fptr(adj), None)
    eng._check(rc, "gaudi_check_stability")
    return dist, adj


def analyze_atoms_for_molecules(molecule_list, tol=0.1, dataset="cata", train_fingerprints=None, engine=None, valence_check=False,
                                exact=False, train_keys=None, similarity=False, train_library=None, patterns=None,
                                pattern_options=None, huckel=False, ppp=False, ppp_cis=False, aromaticity=False,
                                ring_currents=False, cluster_threshold=None, reactivity=False, ppp_dscf=False, ppp_scf=None):
    """The call shape of analyze_rdkit_validity_for_molecules (analyze/analyze.py:180-231) on top of gaudi_rings_to_atoms: every
    molecule is converted to its graph of atoms (gaudi_amd.gor2goa.rings_to_atoms, one launch for the whole list) and counted.

    What differs from the reference, plainly: there is no RDKit here.  ``mol_built`` is the fraction for which gor2goa did not
    raise, and molecules are told apart by the 64-bit fingerprint of their heavy-atom graph, not by InChI: equal keys do not
    prove that two molecules are the same (``exact=True`` below replaces the fingerprint by an exact key).  The reference's ``mol_valid`` has a counterpart only with ``valence_check=True``.

    -> (dict, built_list): ``mol_built``; ``mol_unique`` = distinct keys / built molecules (0.0 when none was built);
    ``molecule_built_bool``; ``fingerprints`` (one int per molecule, 0 where not built); ``mol_novel`` = built molecules whose
    key is not in ``train_fingerprints`` / built molecules, only when ``train_fingerprints`` is given.

    valence_check: a second launch (gaudi_bond_orders) assigns bond orders and formal charges from connectivity, the step the
    reference takes through xyz2mol.AC2BO inside rdkit_valid (DESIGN.md section 8h has the rule; RDKit's sanitiser, the
    single-resonance-structure condition and InChI strings are still not there).  The dict gains ``mol_valid`` = molecules that are built
    and have a structure / all molecules, ``molecule_valid_bool``, ``mol_unique_valid`` = distinct keys / valid molecules,
    ``mol_novel_valid`` (with ``train_fingerprints``), and the second return value becomes the VALID molecules.

    exact: a further launch (gaudi_canonical_order) numbers every built molecule canonically, and molecules
    are told apart by ``canon_key`` -- equal keys <=> isomorphic graphs of atoms, what the reference's InChI comparison decides.
    A built molecule without a key (the bounded search gave up) falls back to ``("fp", fingerprint)``.  ``mol_unique*`` count
    these keys, ``mol_novel*`` compare them with ``train_keys`` (a collection of ``bytes``; ``train_fingerprints`` is not used),
    and the dict gains ``canon_keys`` (one per molecule, None where not built), ``mol_undecided`` = built molecules without a
    key / built molecules and, with ``valence_check``, ``smiles`` (one string or None per molecule).

    similarity: one more launch (gaudi_circular_fingerprint) gives every built molecule its circular count
    fingerprint, and the dict gains ``diversity`` = 1 - the mean pairwise similarity of the built molecules (0.0 with fewer than
    two).  With ``train_library`` (a gaudi_amd.similarity.Library of fingerprints of radius 2, resident on the engine used here)
    also ``nearest_train_similarity`` and ``nearest_train_index``, one per molecule: how close the nearest training molecule is
    and which it is, 0.0 and -1 where the molecule was not built.  Membership (``train_keys``) says novel or not; this says how
    novel.  With ``cluster_threshold`` (a float, a Fraction or a (num, den) pair, as gaudi_amd.similarity.cluster takes it;
    DESIGN.md section 8q) the built molecules are clustered by Butina's method at that similarity and the dict gains
    ``n_clusters`` and ``largest_cluster_fraction`` = the size of the largest cluster / built molecules (0.0 when none was
    built): one mean cannot tell a batch spread evenly from three skeletons plus noise, a cluster count can.  With
    ``cluster_threshold=None`` nothing changes and no launch is made.

    patterns: a list of patterns for gaudi_amd.substructure.search (one more launch per 64 patterns, and
    one for their symmetry), with ``pattern_options`` = its keywords ``hydrogens`` / ``closed``.  The dict gains ``pattern_hits``
    bool [n,P] (rows of unbuilt molecules False) and ``pattern_fraction`` [P] = built molecules that contain the pattern / built
    molecules (0.0 when none was built).  With ``patterns=None`` nothing changes and no launch is made.

    huckel: one more call (gaudi_amd.huckel) solves the Hueckel problem of every built molecule.  The dict
    gains ``huckel_gap``, an array over the BUILT molecules in list order with their HOMO-LUMO gap in |beta| (NaN where the status
    is not OK), and ``huckel_open_shell_fraction`` = built molecules with an odd pi electron count / built molecules (0.0 when
    none was built).  With ``huckel=False`` nothing changes and no launch is made.

    ppp: one more call (gaudi_amd.ppp) runs the PPP SCF of every built molecule on its built geometry.  The
    dict gains ``ppp_gap``, an array over the BUILT molecules in list order with their HOMO-LUMO gap in eV (NaN where the status
    is not OK), and ``ppp_not_converged_fraction`` = built molecules whose SCF did not converge / built molecules (0.0 when none
    was built).  With ``ppp=False`` nothing changes and no launch is made.

    ppp_cis: the CIS stage on that ground state (gaudi_amd.ppp.excited_states; with ``ppp`` the same call).
    The dict gains ``ppp_s1``, ``ppp_t1`` and ``ppp_bright``, arrays over the BUILT molecules in list order with the lowest singlet,
    the lowest triplet and the lowest singlet with f >= 0.01 in eV (NaN where nothing was solved), and
    ``ppp_triplet_unstable_fraction`` = built molecules whose lowest triplet lies at or below the closed-shell ground state / built
    molecules (0.0 when none was built).  With ``ppp_cis=False`` nothing changes and no launch is made.

    aromaticity: one more launch (gaudi_amd.aromaticity) enumerates the Kekule structures of every built
    molecule.  The dict gains ``mol_kekule_count`` and ``mol_clar``, int64 arrays over the BUILT molecules in list order (0 where
    the status is not OK), and ``mean_log_kekule_per_center`` = the mean of ln(K) / (number of atoms that are not hydrogen) over
    the built molecules with status OK (0.0 when there are none).  With ``aromaticity=False`` nothing changes and no launch is
    made.

    ring_currents: one more call (gaudi_amd.aromaticity.ring_currents) gives every built molecule its
    Hueckel-London ring currents on its built geometry.  The dict gains ``mol_ring_current_max``, a float64 array over the BUILT
    molecules in list order with the largest ring current in units of benzene's (NaN where nothing was solved), and
    ``paratropic_fraction`` = solved molecules with a ring current below 0 / solved molecules (0.0 when none was solved).  With
    ``ring_currents=False`` nothing changes and no launch is made.

    reactivity: one more call (gaudi_amd.reactivity) gives every built molecule its Hueckel localization
    energies.  The dict gains ``mol_min_para_localization`` and ``mol_min_atom_localization``, float64 arrays over the BUILT
    molecules in list order, in |beta| (NaN where nothing was solved or the molecule has no six-ring / no centre with a hydrogen).
    With ``reactivity=False`` nothing changes and no launch is made.

    ppp_dscf: one more call (gaudi_amd.ppp.ionization) solves every built molecule as neutral, cation and
    anion by the half-electron method.  The dict gains ``mol_ppp_ip_dscf`` and ``mol_ppp_ea_dscf``, float64 arrays over the BUILT
    molecules in list order with the delta-SCF ionisation potential and electron affinity in eV (NaN where a state was not solved).
    With ``ppp_dscf=False`` nothing changes and no launch is made.

    ppp_scf: "diis" sends the calls of ``ppp=True`` and ``ppp_dscf=True`` to gaudi_ppp_scf (Pulay's DIIS); the
    keys are the same.  Absent (None) or "damped": what it was.  It launches nothing by itself."""
    from .gor2goa import rings_to_atoms
    if train_library is not None and not similarity:
        raise ValueError("train_library needs similarity=True")
    if cluster_threshold is not None and not similarity:
        raise ValueError("cluster_threshold needs similarity=True")
    # (the keyword only when asked for: a rings_to_atoms stand-in with the earlier signature, as tests/test_gor2goa_cpu.py passes, keeps working)
    extra = {"bond_orders": True} if valence_check else {}
    if exact:
        extra["canonical"] = True
    if huckel:
        extra["huckel"] = True
    if ppp:
        extra["ppp"] = True
    if ppp_cis:
        extra["ppp_cis"] = True
    if aromaticity:
        extra["aromaticity"] = True
    if ring_currents:
        extra["ring_currents"] = True
    if reactivity:
        extra["reactivity"] = True
    if ppp_dscf:
        extra["ppp_dscf"] = True
    if ppp_scf is not None:
        extra["ppp_scf"] = ppp_scf
    recs = rings_to_atoms(molecule_list, dataset, tol, fingerprint=True, engine=engine, **extra)
    if not recs:
        raise GaudiError("empty molecule list")  # as analyze_validity_for_molecules: no fractions of nothing
    built = [r["status"] == 0 for r in recs]
    keys = [r["fingerprint"] if ok else 0 for r, ok in zip(recs, built)]
    fingerprints = keys
    if exact:
        keys = [None if not ok else r["canon_key"] if r["canon_key"] is not None else ("fp", r["fingerprint"])
                for r, ok in zip(recs, built)]
    built_keys = [k for k, ok in zip(keys, built) if ok]
    n_built = len(built_keys)
    d = {"mol_built": n_built / float(len(recs)),
         "mol_unique": len(set(built_keys)) / float(n_built) if n_built else 0.0,
         "molecule_built_bool": built, "fingerprints": fingerprints}
    train = None if train_fingerprints is None else {int(k) for k in train_fingerprints}
    if exact:
        train = None if train_keys is None else {bytes(k) for k in train_keys}
        d["canon_keys"] = keys
        d["mol_undecided"] = sum(isinstance(k, tuple) for k in built_keys) / float(n_built) if n_built else 0.0
        if valence_check:
            from .gor2goa import smiles
            d["smiles"] = [smiles(r, dataset) if ok else None for r, ok in zip(recs, built)]
    if train is not None:
        d["mol_novel"] = sum(k not in train for k in built_keys) / float(n_built) if n_built else 0.0
    keep = built
    if valence_check:
        keep = [ok and r["kekule_status"] == 0 for r, ok in zip(recs, built)]
        valid_keys = [k for k, ok in zip(keys, keep) if ok]
        n_valid = len(valid_keys)
        d["mol_valid"] = n_valid / float(len(recs))
        d["molecule_valid_bool"] = keep
        d["mol_unique_valid"] = len(set(valid_keys)) / float(n_valid) if n_valid else 0.0
        if train is not None:
            d["mol_novel_valid"] = sum(k not in train for k in valid_keys) / float(n_valid) if n_valid else 0.0
    if similarity:
        d.update(_similarity(recs, built, dataset, _engine(engine), train_library, cluster_threshold))
    if patterns is not None:
        from .substructure import search
        hits = search(recs, patterns, dataset, engine=_engine(engine), **(pattern_options or {}))["hit"]
        hits = hits & np.asarray(built, bool)[:, None]
        d["pattern_hits"] = hits
        d["pattern_fraction"] = hits.sum(0) / float(n_built) if n_built else np.zeros(hits.shape[1])
    if huckel:
        from ._lib import HUCKEL_OPEN_SHELL
        rows = [r for r, ok in zip(recs, built) if ok]
        d["huckel_gap"] = np.array([r["huckel_gap"] if r["huckel_status"] == 0 else np.nan for r in rows], np.float64)
        d["huckel_open_shell_fraction"] = (sum(r["huckel_status"] == 0 and bool(r["huckel_flags"] & HUCKEL_OPEN_SHELL) for r in rows)
                                           / float(n_built) if n_built else 0.0)
    if ppp:
        rows = [r for r, ok in zip(recs, built) if ok]
        d["ppp_gap"] = np.array([r["ppp_gap"] if r["ppp_status"] == 0 else np.nan for r in rows], np.float64)
        d["ppp_not_converged_fraction"] = sum(r["ppp_status"] == 1 for r in rows) / float(n_built) if n_built else 0.0
    if ppp_cis:
        from ._lib import PPP_CIS_TRIPLET_UNSTABLE
        rows = [r for r, ok in zip(recs, built) if ok]
        for k in ("ppp_s1", "ppp_t1", "ppp_bright"):
            d[k] = np.array([r[k] for r in rows], np.float64)
        d["ppp_triplet_unstable_fraction"] = (sum(bool(r["ppp_cis_flags"] & PPP_CIS_TRIPLET_UNSTABLE) for r in rows) / float(n_built)
                                              if n_built else 0.0)
    if aromaticity:
        from .gor2goa import atoms_list
        h = atoms_list(dataset).index("H")
        rows = [r for r, ok in zip(recs, built) if ok]
        d["mol_kekule_count"] = np.array([r["kekule_count"] for r in rows], np.int64)
        d["mol_clar"] = np.array([r["clar"] for r in rows], np.int64)
        logs = [np.log(float(r["kekule_count"])) / float((np.asarray(r["atom_types"]) != h).sum()) for r in rows if r["resonance_status"] == 0]
        d["mean_log_kekule_per_center"] = float(np.mean(logs)) if logs else 0.0
    if ring_currents:
        rows = [r for r, ok in zip(recs, built) if ok]
        d["mol_ring_current_max"] = np.array([r["ring_current_max"] for r in rows], np.float64)
        solved = [r["ring_current_min"] for r in rows if r["ring_current_status"] == 0 and not np.isnan(r["ring_current_min"])]
        d["paratropic_fraction"] = sum(v < 0.0 for v in solved) / float(len(solved)) if solved else 0.0
    if reactivity:
        rows = [r for r, ok in zip(recs, built) if ok]
        d["mol_min_para_localization"] = np.array([r["min_para_localization"] for r in rows], np.float64)
        d["mol_min_atom_localization"] = np.array([r["min_atom_localization"] for r in rows], np.float64)
    if ppp_dscf:
        rows = [r for r, ok in zip(recs, built) if ok]
        d["mol_ppp_ip_dscf"] = np.array([r["ppp_ip_dscf"] for r in rows], np.float64)
        d["mol_ppp_ea_dscf"] = np.array([r["ppp_ea_dscf"] for r in rows], np.float64)
    return d, [m for m, ok in zip(molecule_list, keep) if ok]


def _similarity(recs, built, dataset, engine, train_library=None, cluster_threshold=None, diverse=None) -> dict:
    """``diversity`` of the built records and, with a library, their nearest training molecules (analyze_atoms_for_molecules);
    with a threshold their Butina clusters, with ``diverse`` = k up to k MaxMin picks among them."""
    from .similarity import cluster, fingerprints, internal_diversity, pick_diverse
    n_bins = 1024 if train_library is None else train_library.n_bins
    fp = fingerprints(recs, dataset, n_bins=n_bins, engine=engine)
    out = {"diversity": internal_diversity(fp["fp"], fp["total"], engine=engine)}
    if train_library is not None:
        if train_library.engine is not engine:
            raise GaudiError("train_library is resident on another engine than the one this call runs on")
        idx, sim = train_library.nearest(fp["fp"], 1)
        ok = np.array(built, dtype=bool)
        out["nearest_train_similarity"] = np.where(ok, sim[:, 0], 0.0)
        out["nearest_train_index"] = np.where(ok, idx[:, 0], -1)
    if cluster_threshold is not None or diverse is not None:
        rows = np.where(np.asarray(built, bool)[:, None], fp["fp"], 0).astype(np.uint8)  # (not built: a zero row, never clustered or picked)
        if cluster_threshold is not None:
            cl = cluster(rows, cluster_threshold, engine=engine)
            n_live = int((cl["cluster"] >= 0).sum())
            out["n_clusters"] = cl["n_clusters"]
            out["largest_cluster_fraction"] = float(cl["sizes"].max()) / n_live if cl["n_clusters"] else 0.0
        if diverse is not None:
            out["diverse_indices"] = pick_diverse(rows, int(diverse), engine=engine)["picked"]
    return out
