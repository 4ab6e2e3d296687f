#!/usr/bin/env python3
"""Rates of gaudi_ppp_cis (csrc/ppp.inc + csrc/ppp_cis.inc) on tools/ppp_rate.py's two workloads: 4 096 copies of a 46-centre cata
molecule (the 64-centre tier) and 4 096 molecules drawn from the g30 fixture with a fixed seed.  Per workload, in the same run:
gaudi_ppp alone (kernels from its profile log, and the whole call), then gaudi_ppp_cis at window 8 -- its SCF kernels from the same
log, its CIS kernel from the CIS log, the CIS share of the kernel time, and the whole call (twenty-eight arrays out) -- each the
median of --calls calls after one warm-up call; and the mean number of states and of CIS Jacobi sweeps per molecule.  The numbers go
into DESIGN.md section 8n; there is no threshold.  No hardware counter pass is made here: the line "not_measured" says what this
run leaves open.

    python tools/ppp_cis_rate.py [--calls 5] [--molecules 4096]
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


def acene(rings, side=1.40):
    """A row of fused regular six-rings (cata): 4 * rings + 2 carbons in the plane, the hydrogens implied."""
    step = side * np.sqrt(3.0)
    index, xyz, bonds = {}, [], set()
    for k in range(rings):
        ring = []
        for j in range(6):
            t = np.deg2rad(30.0 + 60.0 * j)
            p = (k * step + side * np.cos(t), side * np.sin(t))
            key = (int(round(p[0] * 100)), int(round(p[1] * 100)))
            if key not in index:
                index[key] = len(xyz)
                xyz.append([p[0], p[1], 0.0])
            ring.append(index[key])
        bonds |= {tuple(sorted((ring[j], ring[(j + 1) % 6]))) for j in range(6)}
    return np.full(len(xyz), 1, np.int32), np.array(sorted(bonds), np.int32), np.array(xyz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--molecules", type=int, default=4096)
    a = ap.parse_args()
    from gaudi_amd._lib import host_ppp
    from gaudi_amd.engine import Engine
    from gaudi_amd.ppp import c_ppp_tables
    from tests.ppp_helpers import g30_molecules, pack
    tab = c_ppp_tables("hetro")
    fx = g30_molecules()
    status = host_ppp(tab, *pack(fx))["status"]
    good = [m for m, st in zip(fx, status) if st in (0, 1)]
    rng = np.random.default_rng(0)
    eng = Engine(0)
    B = a.molecules
    for name, mols in (("acene46", [acene(11)] * B), ("g30_mix", [good[k] for k in rng.integers(0, len(good), B)])):
        packed = pack(mols)
        fig = {}
        for what, run in (("ppp", lambda: eng.ppp(tab, *packed)), ("ppp_cis", lambda: eng.ppp_cis(tab, *packed, None, 0, 0.25, 8))):
            out = run()  # warm-up (workspaces, the LDS attribute)
            wall, scf, cis, launches = [], [], [], (0, 0)
            for _ in range(a.calls):
                eng.profile_reset(True)
                t0 = time.perf_counter()
                run()
                wall.append(time.perf_counter() - t0)
                (n_scf, ms_scf), (n_cis, ms_cis) = eng.ppp_profile_get(), eng.ppp_cis_profile_get()
                launches = (n_scf, n_cis)
                scf.append(ms_scf)
                cis.append(ms_cis)
            eng.profile_reset(False)
            fig[what] = (out, float(np.median(wall)), float(np.median(scf)), float(np.median(cis)), launches)
        out, w, k_scf, k_cis, launches = fig["ppp_cis"]
        _, w0, k0, _, launches0 = fig["ppp"]
        rate = lambda ms: round(B / (ms / 1e3), 1) if ms > 0 else None  # noqa: E731
        print(json.dumps(dict(metric="ppp_cis_molecules_per_s", workload=name, molecules=B, scf_launches_per_call=launches[0],
                              cis_launches_per_call=launches[1], ppp_alone_launches_per_call=launches0[0],
                              mean_pi_centres=round(float(out["n_pi"].mean()), 1), max_pi_centres=int(out["n_pi"].max()),
                              mean_states=round(float(out["n_states"].mean()), 1), mean_cis_sweeps=round(float(out["cis_sweeps"].mean()), 2),
                              mean_scf_sweeps=round(float(out["sweeps"].mean()), 2),
                              statuses=np.bincount(out["status"], minlength=9).tolist(),
                              triplet_unstable=int(((out["flags"] & 128) != 0).sum()),
                              ppp_alone_kernel_median_ms=round(k0, 4), ppp_alone_kernel_molecules_per_s=rate(k0),
                              ppp_alone_call_molecules_per_s=round(B / w0, 1),
                              scf_kernel_median_ms=round(k_scf, 4), cis_kernel_median_ms=round(k_cis, 4),
                              cis_share_of_kernels=round(k_cis / (k_scf + k_cis), 4) if k_scf + k_cis > 0 else None,
                              kernel_molecules_per_s=rate(k_scf + k_cis), cis_kernel_molecules_per_s=rate(k_cis),
                              call_median_s=round(w, 5), call_molecules_per_s=round(B / w, 1),
                              output_bytes=int(sum(v.nbytes for v in out.values())))), flush=True)
    print(json.dumps(dict(not_measured=["hardware counters (LDS bank conflicts, VALU utilisation, occupancy achieved): no counter pass in this run",
                                        "the 128-centre tier alone", "batches other than the one given", "windows other than 8", "the Ohno formula's rate"])))
    eng.close()


if __name__ == "__main__":
    main()
