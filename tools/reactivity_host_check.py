#!/usr/bin/env python3
"""AddressSanitizer + UndefinedBehaviorSanitizer over the HOST build of csrc/reactivity.inc (gaudi_host_reactivity), in a
stand-alone program (tools/reactivity_host_check.cpp) -- not inside python and not on a device.  Dumps the default Hueckel table
and a batch with its charges and expected statuses to a flat file -- every eighth molecule of golden g32 under charges -1 / 0 / +1
in turn, the textbook hydrocarbons, the five-rings with a heteroatom, a ladder with more than 32 rings and one molecule for every
status -- compiles gaudi_hip.hip with the sanitizers on the host compilation only, links it with the kernel objects of the
ordinary build (python -m gaudi_amd.build first) and the program, and runs it.  The program runs the batch, every molecule of it
alone in exactly-sized buffers under another number of slices, chains at every tier edge, random graphs of its own and tables that
must be refused.  A finding aborts the run; a clean run prints status counts.

    python tools/reactivity_host_check.py [--keep]
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
    from tests import huckel_helpers as hh
    from tests import reactivity_helpers as rx
    from tests.bond_order_helpers import fixture
    mols = [(m["elem"], m["bonds"]) for m in fixture()[1][::8]]
    charge, want = [(-1, 0, 1)[k % 3] for k in range(len(mols))], [-1] * len(mols)
    benz = rx.known("benzene")
    methane = hh.with_h(np.array([1], np.int32), np.zeros((0, 2), np.int32), [4])
    named = [(rx.known(k), 0, rx.OK) for k in ("naphthalene", "anthracene", "phenanthrene", "pyrene")]
    named += [(m, 0, rx.OK) for m in rx.hetero_rings()]
    named += [(rx.ladder(70), 0, rx.OK), (benz, 0, rx.OK), (benz, 6, rx.OK), (benz, -6, rx.OK), (benz, 9, rx.BAD_INPUT),
              (rx.acene(33), 0, rx.OVERFLOW), (methane, 0, rx.NO_PI), ((np.zeros(0, np.int32), np.zeros((0, 2), np.int32)), 0, rx.EMPTY)]
    for mol, c, st in named:
        mols.append(mol)
        charge.append(c)
        want.append(st)
    return mols, np.array(charge, np.int32), np.array(want, np.int32)


def main():
    from gaudi_amd.build import CSRC, FLAGS, OBJ
    from gaudi_amd.huckel import c_huckel_tables
    from tests.bond_order_helpers import pack
    from tests.reactivity_helpers import DATASET
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o"))) if os.path.basename(o) != "gaudi_hip.o"]
    if not objs:
        sys.exit("no kernel objects: run `python -m gaudi_amd.build` first")
    work = tempfile.mkdtemp(prefix="reactivity_host_check_")
    mols, charge, want = batch()
    elem, na, bonds, nb = pack(mols)
    with open(os.path.join(work, "batch.bin"), "wb") as f:
        f.write(bytes(c_huckel_tables(DATASET)))
        f.write(np.array([elem.shape[0], elem.shape[1], bonds.shape[1]], np.int32).tobytes())
        for a in (elem, na, bonds, nb, charge, want):
            f.write(a.tobytes())
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    host_obj = os.path.join(work, "gaudi_hip_san.o")
    flags = [x for x in FLAGS if x != "-O3"] + ["-O1", "-g", "-w"] + [y for x in san for y in ("-Xarch_host", x)]
    subprocess.run([hipcc] + flags + ["-c", "gaudi_hip.hip", "-o", host_obj], cwd=CSRC, check=True)
    exe = os.path.join(work, "reactivity_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-g"] + san + ["-I", os.path.join(ROOT, "include"), "-x", "c++",
                    os.path.join(ROOT, "tools", "reactivity_host_check.cpp"), "-x", "none", host_obj] + objs + ["-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    rc = subprocess.run([exe, os.path.join(work, "batch.bin")], env=env).returncode
    print(f"reactivity_host_check: exit status {rc} ({'clean' if rc == 0 else 'FINDING or failure'}); files in {work}")
    if "--keep" not in sys.argv and rc == 0:
        import shutil
        shutil.rmtree(work)
    sys.exit(rc)


if __name__ == "__main__":
    main()
