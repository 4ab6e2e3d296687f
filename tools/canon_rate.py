#!/usr/bin/env python3
"""Molecules per second of gaudi_amd.gor2goa.canonical (canonical numbering of the heavy atoms, one launch per call) at
B = 8192 cata-condensed molecules of 11 rings with their hydrogens placed (46 C + 28 H each), built by rings_to_atoms first, and
on one batch of the highest-symmetry inputs: coronene and circumcoronene (hexagonal patches of 7 and 19 rings, twelve
automorphisms each, 19 search-tree nodes), every copy under a numbering of its own.  Two figures per batch: the whole call as a
user sees it (packing, copies to and from the device, the per-molecule records) and the kernel alone (HIP events around the
launch), each the median of --calls calls after one warm-up call.  The numbers go into DESIGN.md; there is no threshold.

    python tools/canon_rate.py [--batch 8192] [--calls 5]
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


def hex_patch(shells, rng):
    """The atoms of a hexagonal patch of 1 + 3 * shells * (shells + 1) rings, hydrogens on the rim, numbered at random
    -> (atom_types, bonds) in ATOMS_LIST["cata"] (H = 0, C = 1)."""
    a, b = np.array([np.sqrt(3.0), 0.0]), np.array([np.sqrt(3.0) / 2, 1.5])
    centres = [i * a + j * b for i in range(-shells, shells + 1) for j in range(-shells, shells + 1) if abs(i + j) <= shells]
    pts = {}
    for c in centres:
        for k in range(6):
            p = c + np.array([np.cos(np.pi / 6 + k * np.pi / 3), np.sin(np.pi / 6 + k * np.pi / 3)])
            pts[(int(round(p[0] * 100)), int(round(p[1] * 100)))] = p
    xy = np.array(list(pts.values()))
    d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1))
    bonds = [(i, j) for i in range(len(xy)) for j in range(i) if abs(d[i, j] - 1.0) < 0.01]
    deg = np.bincount(np.array(bonds).reshape(-1), minlength=len(xy))
    types = [1] * len(xy)
    for c in np.nonzero(deg == 2)[0]:
        types.append(0)
        bonds.append((int(c), len(types) - 1))
    perm = rng.permutation(len(types))
    t = np.zeros(len(types), np.int64)
    t[perm] = types
    return t, perm[np.array(bonds)]


def measure(eng, mols, calls):
    from gaudi_amd.gor2goa import canonical
    out = canonical(mols, "cata", engine=eng)  # warm-up (workspaces)
    wall, kernel = [], []
    for _ in range(calls):
        eng.profile_reset(True)
        t0 = time.perf_counter()
        canonical(mols, "cata", engine=eng)
        wall.append(time.perf_counter() - t0)
        launches, ms = eng.canon_profile_get()
        assert launches == 1
        kernel.append(ms)
    w, k = float(np.median(wall)), float(np.median(kernel))
    nodes = [o["canon_nodes"] for o in out]
    return dict(batch=len(mols), calls=calls, canonical=sum(o["canon_status"] == 0 for o in out),
                distinct_keys=len({o["canon_key"] for o in out}), nodes_median=float(np.median(nodes)), nodes_max=int(max(nodes)),
                call_median_s=round(w, 5), call_molecules_per_s=round(len(mols) / w, 1), kernel_median_ms=round(k, 4),
                kernel_molecules_per_s=round(len(mols) / (k / 1e3), 1) if k > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from gaudi_amd.engine import Engine
    from gaudi_amd.gor2goa import rings_to_atoms
    rng = np.random.default_rng(0)
    B, n = a.batch, 11
    pool = [cata_molecule(rng, n) for _ in range(min(B, 512))]
    X = np.stack([pool[b % len(pool)] for b in range(B)])
    eng = Engine(0)
    recs = rings_to_atoms((X, np.zeros((B, n), np.int32), np.full(B, n, np.int32)), "cata", 0.1, place_hydrogens=True, engine=eng)
    print(json.dumps(dict(metric="canon_molecules_per_s", input="cata, 11 rings, hydrogens placed",
                          built=sum(r["status"] == 0 for r in recs), **measure(eng, recs, a.calls))))
    sym = [hex_patch(1 + b % 2, rng) for b in range(B)]
    print(json.dumps(dict(metric="canon_molecules_per_s", input="coronene / circumcoronene", **measure(eng, sym, a.calls))))
    eng.close()


if __name__ == "__main__":
    main()
