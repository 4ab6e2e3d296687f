#!/usr/bin/env python3
"""AddressSanitizer + UndefinedBehaviorSanitizer over the HOST build of the PPP SCF with DIIS (gaudi_host_ppp_scf: csrc/ppp_scf.inc, ppp_molecule<P, true, true> of csrc/ppp.inc), in a stand-alone program
(tools/ppp_scf_host_check.cpp) -- not inside python and not on a device.  Dumps the default table and the g30 fixture's molecules
(packed arrays and coordinates) to a flat file, compiles gaudi_hip.hip with the sanitizers on the host compilation only, links it
with the kernel objects of the ordinary build (python -m gaudi_amd.build first) and the program, and runs it.  A finding aborts
the run; a clean run prints status counts.

    python tools/ppp_scf_host_check.py [--keep]
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from gaudi_amd.build import CSRC, FLAGS, OBJ
    from gaudi_amd.ppp import c_ppp_tables
    from tests.ppp_helpers import DATASET, g30_molecules, pack
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o"))) if os.path.basename(o) != "gaudi_hip.o"]
    if not objs:
        sys.exit("no kernel objects: run `python -m gaudi_amd.build` first")
    work = tempfile.mkdtemp(prefix="ppp_scf_host_check_")
    elem, na, bonds, nb, xyz = pack(g30_molecules())
    with open(os.path.join(work, "g30.bin"), "wb") as f:
        f.write(bytes(c_ppp_tables(DATASET)))
        f.write(np.array([elem.shape[0], elem.shape[1], bonds.shape[1]], np.int32).tobytes())
        for a in (elem, na, bonds, nb, xyz):
            f.write(a.tobytes())
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    host_obj = os.path.join(work, "gaudi_hip_san.o")
    flags = [x for x in FLAGS if x != "-O3"] + ["-O1", "-g", "-w"] + [y for x in san for y in ("-Xarch_host", x)]
    subprocess.run([hipcc] + flags + ["-c", "gaudi_hip.hip", "-o", host_obj], cwd=CSRC, check=True)
    exe = os.path.join(work, "ppp_scf_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-g"] + san + ["-I", os.path.join(ROOT, "include"), "-x", "c++",
                    os.path.join(ROOT, "tools", "ppp_scf_host_check.cpp"), "-x", "none", host_obj] + objs + ["-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    rc = subprocess.run([exe, os.path.join(work, "g30.bin")], env=env).returncode
    print(f"ppp_scf_host_check: exit status {rc} ({'clean' if rc == 0 else 'FINDING or failure'}); files in {work}")
    if "--keep" not in sys.argv and rc == 0:
        import shutil
        shutil.rmtree(work)
    sys.exit(rc)


if __name__ == "__main__":
    main()
