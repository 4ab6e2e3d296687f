#!/usr/bin/env python3
"""Molecules per second of gaudi_amd.goa2gor.atoms_to_rings (graph of atoms -> graph of rings, one launch per call) at B = 4096
structures produced by rings_to_atoms(place_hydrogens=True): cata-condensed molecules of 11 rings and grown hetero molecules of
10 rings.  Two figures per dataset: the whole call as a user sees it (packing, copies, the per-molecule records) and the kernel
alone (HIP events around the launch).  One warm-up call, then --calls timed calls.  The numbers go into DESIGN.md beside the rate
of the reference's get_rings path that tools/make_golden.py g31 prints; there is no threshold.

    python tools/rings_rate.py [--batch 4096] [--calls 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)

from atoms_rate import cata_molecule  # noqa: E402


def hetero_molecule(rng, n, names):
    """A cata-shaped tree of n rings on the triangular lattice with six-ring hetero types: a ring's hetero atom sits on a corner
    that belongs to no fused edge (its orientation node points at that corner), and a ring without such a corner is Bn."""
    dirs = [(1, 0), (0, 1), (-1, 1), (-1, 0), (0, -1), (1, -1)]  # lattice directions at 0, 60, ... degrees
    occ = [(0, 0)]
    while len(occ) < n:
        a, d = occ[rng.integers(len(occ))], dirs[rng.integers(6)]
        c = (a[0] + d[0], a[1] + d[1])
        if c in occ or sum(((c[0] + e[0], c[1] + e[1]) in occ) for e in dirs) > 1:
            continue
        occ.append(c)
    spacing = 2.45
    xy = np.array([[c[0] + 0.5 * c[1], c[1] * np.sqrt(3) / 2] for c in occ]) * spacing
    hetero = [names.index(s) for s in ("Pd", "Bz")]
    ty, xo = [], []
    for c, p in zip(occ, xy):
        taken = set()  # corners at 30 + 60 k degrees; the fused edge towards direction k has corners k - 1 and k
        for k, e in enumerate(dirs):
            if (c[0] + e[0], c[1] + e[1]) in occ:
                taken |= {(k - 1) % 6, k}
        free = [k for k in range(6) if k not in taken]
        if free:
            ang = np.pi / 6 + np.pi / 3 * free[rng.integers(len(free))]
            ty.append(hetero[rng.integers(len(hetero))])
        else:
            ang = 0.0
            ty.append(names.index("Bn"))
        xo.append(p + 1.4 * np.array([np.cos(ang), np.sin(ang)]))
    x = np.concatenate([xy, np.array(xo)])
    x = np.concatenate([x, np.zeros((2 * n, 1))], 1)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return ((x - x[:n].mean(0)) @ q).astype(np.float32), np.concatenate([np.array(ty, np.int64), np.full(n, len(names) - 1, np.int64)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from gaudi_amd.analyze import rings_list
    from gaudi_amd.engine import Engine
    from gaudi_amd.goa2gor import atoms_to_rings
    from gaudi_amd.gor2goa import rings_to_atoms
    rng = np.random.default_rng(0)
    eng = Engine(0)
    B = a.batch
    for ds, n in (("cata", 11), ("hetro", 10)):
        if ds == "cata":
            pool = [(cata_molecule(rng, n), np.zeros(n, np.int64)) for _ in range(min(B, 256))]
        else:
            pool = [hetero_molecule(rng, n, rings_list(ds)) for _ in range(min(B, 256))]
        built = [r for r in rings_to_atoms(pool, ds, 0.1, place_hydrogens=True, engine=eng) if r["status"] == 0]
        # the pool: structures that were built and whose rings are perceived (a rate of refusals would say nothing)
        first = atoms_to_rings([(r["atom_types"], r["atoms3d"]) for r in built], ds, use_hydrogens=True, engine=eng) if built else []
        built = [r for r, f in zip(built, first) if f["status"] == 0]
        if not built:
            print(json.dumps(dict(metric="rings_molecules_per_s", dataset=ds, error="no pool molecule was built")))
            continue
        mols = [(built[b % len(built)]["atom_types"], built[b % len(built)]["atoms3d"]) for b in range(B)]
        recs = atoms_to_rings(mols, ds, use_hydrogens=True, engine=eng)  # warm-up (workspaces)
        ok = sum(r["status"] == 0 for r in recs)
        eng.profile_reset(True)
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            atoms_to_rings(mols, ds, use_hydrogens=True, engine=eng)
            times.append(time.perf_counter() - t0)
        launches, ms = eng.rings_profile_get()
        eng.profile_reset(False)
        med = float(np.median(times))
        print(json.dumps(dict(metric="rings_molecules_per_s", dataset=ds, batch=B, rings=n, calls=a.calls, ok=ok, pool=len(built),
                              atoms_mean=round(float(np.mean([len(m[0]) for m in mols])), 1),
                              rings_mean=round(float(np.mean([len(r["x"]) for r in recs])), 2),
                              call_median_s=round(med, 5), call_molecules_per_s=round(B / med, 1), launches=launches,
                              kernel_ms_per_launch=round(ms / max(launches, 1), 4),
                              kernel_molecules_per_s=round(B * launches / (ms / 1e3), 1) if ms > 0 else None)))
    eng.close()


if __name__ == "__main__":
    main()
