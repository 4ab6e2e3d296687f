"""csrc/lds_fold.h on the host: the batched ordered folds give the bits of the plain one-row-per-iteration loops for every run
length 0 .. 16, both batch sizes, consecutive and indexed rows (tools/lds_batch_host_check.cpp).  A stand-alone program, built
plain and with AddressSanitizer + UndefinedBehaviorSanitizer and run on its own: nothing is loaded into python, nothing runs on a
device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "lds_batch_host_check.cpp")
INC = os.path.join(ROOT, "gaudi_amd", "csrc")


def _compiler():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if os.path.exists(hipcc):
        return [hipcc, "-x", "c++"]  # (host only: the program has no device code)
    gxx = shutil.which("g++")
    if gxx:
        return [gxx]
    pytest.fail("neither hipcc nor g++ found")


@pytest.mark.parametrize("flags", [["-O3"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_batched_folds_give_the_plain_loops_bits(flags, tmp_path):
    exe = str(tmp_path / "lds_batch_host_check")
    cc = _compiler()
    build = subprocess.run(cc + ["-std=c++17", "-ffp-contract=off"] + flags + ["-I", INC, SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "run lengths 0..16, 0 mismatches" in run.stdout
