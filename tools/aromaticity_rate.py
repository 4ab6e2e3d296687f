#!/usr/bin/env python3
"""Rates of gaudi_kekule (csrc/kekule.inc): molecules per second for the built g30 molecules (the molecules of the g32 fixture
that come from g30 and are counted, drawn with a fixed seed: the mix a run produces) and for a batch of ONE 46-carbon 11-ring
cata molecule (a zig-zag row of eleven rings, 233 structures), each next to the gaudi_bond_orders launch of the same batch for
scale.  Per figure: the kernel alone from the profile counters (HIP events; one launch per call), both kernels in one session,
and the whole call as a user of Engine.kekule sees it (packed arrays in, nine arrays out), each the median of --calls calls
after one warm-up call; and the search nodes per second the kernel walked.  The largest n_nodes of g30 and of all of g32 is
printed too.  The numbers go into DESIGN.md section 8o; there is no threshold and no figure of an earlier revision to compare
with.  No hardware counter pass is made here: the line "not_measured" says what this run leaves open.

    python tools/aromaticity_rate.py [--calls 5] [--molecules 4096]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)


def zigzag(rings):
    """A row of fused six-rings with a kink at every ring (cata; F(rings + 2) Kekule structures, the most a chain of that length
    has): 4 * rings + 2 carbons, the hydrogens implied.  Every new ring is fused on the edge next to the last fusion."""
    ring, n = list(range(6)), 6
    bonds = [(k, (k + 1) % 6) for k in range(6)]
    for _ in range(1, rings):
        a, b = ring[2], ring[3]
        chain = [a, n, n + 1, n + 2, n + 3, b]
        bonds += [(chain[k], chain[k + 1]) for k in range(5)]
        ring = [b, a, n, n + 1, n + 2, n + 3]
        n += 4
    return np.full(n, 1, np.int32), np.array(bonds, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--molecules", type=int, default=4096)
    a = ap.parse_args()
    from gaudi_amd._lib import host_kekule
    from gaudi_amd.engine import Engine
    from gaudi_amd.gor2goa import c_valence_tables
    from tests.bond_order_helpers import fixture, pack
    tab = c_valence_tables("hetro")
    fx = fixture()[1]
    ref = host_kekule(tab, *pack(fx))
    good = [m for m in fx if ref["status"][m["index"]] == 0 and m["g30"] >= 0]
    print(json.dumps(dict(metric="kekule_largest_tree", g30_counted=len(good), g30_max_n_nodes=int(max(ref["n_nodes"][m["index"]] for m in good)),
                          g30_max_k=int(max(ref["k"][m["index"]] for m in good)), g32_max_n_nodes=int(ref["n_nodes"].max()),
                          g32_max_k=int(ref["k"].max()))), flush=True)
    rng = np.random.default_rng(0)
    eng = Engine(0)
    B = a.molecules
    for name, mols in (("g30_built", [(good[k]["elem"], good[k]["bonds"]) for k in rng.integers(0, len(good), B)]), ("cata46", [zigzag(11)] * B)):
        packed = pack(mols)
        out = eng.kekule(tab, *packed)  # warm-up (workspaces)
        eng.bond_orders(tab, *packed)
        assert np.array_equal(out["k"][:64], host_kekule(tab, *pack(mols[:64]))["k"])
        wall, kernel, bonds_kernel = [], [], []
        for _ in range(a.calls):
            eng.profile_reset(True)
            t0 = time.perf_counter()
            eng.kekule(tab, *packed)
            wall.append(time.perf_counter() - t0)
            eng.bond_orders(tab, *packed)
            launches, ms = eng.kekule_profile_get()
            assert launches == 1
            kernel.append(ms)
            bonds_kernel.append(eng.bonds_profile_get()[1])
        eng.profile_reset(False)
        w, k, kb = float(np.median(wall)), float(np.median(kernel)), float(np.median(bonds_kernel))
        nodes = int(out["n_nodes"].sum())
        print(json.dumps(dict(metric="kekule_molecules_per_s", workload=name, molecules=B, statuses=np.bincount(out["status"], minlength=9).tolist(),
                              mean_k=round(float(out["k"].mean()), 1), max_k=int(out["k"].max()), mean_n_nodes=round(nodes / B, 1),
                              max_n_nodes=int(out["n_nodes"].max()), mean_hexagons=round(float(out["n_hex"].mean()), 2),
                              kernel_median_ms=round(k, 4), kernel_molecules_per_s=round(B / (k / 1e3), 1) if k > 0 else None,
                              kernel_nodes_per_s=round(nodes / (k / 1e3), 1) if k > 0 else None,
                              bond_orders_kernel_median_ms=round(kb, 4), bond_orders_molecules_per_s=round(B / (kb / 1e3), 1) if kb > 0 else None,
                              call_median_s=round(w, 5), call_molecules_per_s=round(B / w, 1),
                              output_bytes=int(sum(v.nbytes for v in out.values())))), flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, atomic contention, occupancy achieved): no counter pass in this run",
                                        "batches other than the one given", "molecules near the budget"])))
    eng.close()


if __name__ == "__main__":
    main()
