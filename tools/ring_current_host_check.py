#!/usr/bin/env python3
"""AddressSanitizer + UndefinedBehaviorSanitizer over the HOST build of csrc/ring_current.inc (gaudi_host_ring_currents), in a
stand-alone program (tools/ring_current_host_check.cpp) -- not inside python and not on a device.  Dumps the default Hueckel table
and a batch with its charges, coordinates and expected statuses to a flat file -- golden g30, the tier-edge set (31 / 32 / 33,
63 / 64 / 65, 127 / 128 centres) and one molecule for every status and flag -- compiles gaudi_hip.hip with the sanitizers on the
host compilation only, links it with the kernel objects of the ordinary build (python -m gaudi_amd.build first) and the program,
and runs it.  The program runs the batch, every molecule of it alone in exactly-sized buffers, and random graphs of its own.  A
finding aborts the run; a clean run prints status counts.

    python tools/ring_current_host_check.py [--keep]
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch():
    """(molecules, charges, expected statuses; -1 = whatever the kernel says)."""
    from tests import ppp_helpers as pp
    from tests import ring_current_helpers as rc
    mols = list(rc.g30_molecules())
    charge, want = [0] * len(mols), [-1] * len(mols)
    edge, edge_charge = pp.edge_set()
    mols += list(edge)
    charge += [int(c) for c in edge_charge]
    want += [rc.OK] * len(edge)
    benz = rc.known("benzene")
    nan = (benz[0], benz[1], benz[2].copy())
    nan[2][4, 2] = np.nan
    methane = (np.array([1, 0, 0, 0, 0], np.int32), np.array([(0, k) for k in range(1, 5)], np.int32), np.zeros((5, 3)))
    for mol, c, st in ((benz, 0, rc.OK), (rc.known("coronene"), 0, rc.OK), (benz, 1, rc.OPEN_SHELL), (benz, 9, rc.BAD_INPUT),
                       (rc.cyclobutadiene(), 0, rc.SMALL_GAP), (nan, 0, rc.BAD_GEOMETRY), (rc.acene(33), 0, rc.OVERFLOW),
                       (methane, 0, rc.NO_PI), ((np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 3))), 0, rc.EMPTY),
                       (pp.cycle([1] * 10), 0, rc.OK), (rc.biphenyl()[0], 0, rc.OK), (rc.bent(rc.known("anthracene")), 0, rc.OK)):
        mols.append(mol)
        charge.append(c)
        want.append(st)
    return mols, np.array(charge, np.int32), np.array(want, np.int32)


def main():
    from gaudi_amd.build import CSRC, FLAGS, OBJ
    from gaudi_amd.huckel import c_huckel_tables
    from tests import ppp_helpers as pp
    from tests.ring_current_helpers import DATASET
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o"))) if os.path.basename(o) != "gaudi_hip.o"]
    if not objs:
        sys.exit("no kernel objects: run `python -m gaudi_amd.build` first")
    work = tempfile.mkdtemp(prefix="ring_current_host_check_")
    mols, charge, want = batch()
    elem, na, bonds, nb, xyz = pp.pack(mols)
    with open(os.path.join(work, "batch.bin"), "wb") as f:
        f.write(bytes(c_huckel_tables(DATASET)))
        f.write(np.array([elem.shape[0], elem.shape[1], bonds.shape[1]], np.int32).tobytes())
        for a in (elem, na, bonds, nb, charge, want, xyz):
            f.write(a.tobytes())
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    host_obj = os.path.join(work, "gaudi_hip_san.o")
    flags = [x for x in FLAGS if x != "-O3"] + ["-O1", "-g", "-w"] + [y for x in san for y in ("-Xarch_host", x)]
    subprocess.run([hipcc] + flags + ["-c", "gaudi_hip.hip", "-o", host_obj], cwd=CSRC, check=True)
    exe = os.path.join(work, "ring_current_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-g"] + san + ["-I", os.path.join(ROOT, "include"), "-x", "c++",
                    os.path.join(ROOT, "tools", "ring_current_host_check.cpp"), "-x", "none", host_obj] + objs + ["-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    rc = subprocess.run([exe, os.path.join(work, "batch.bin")], env=env).returncode
    print(f"ring_current_host_check: exit status {rc} ({'clean' if rc == 0 else 'FINDING or failure'}); files in {work}")
    if "--keep" not in sys.argv and rc == 0:
        import shutil
        shutil.rmtree(work)
    sys.exit(rc)


if __name__ == "__main__":
    main()
