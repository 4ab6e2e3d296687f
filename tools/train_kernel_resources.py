#!/usr/bin/env python3
"""Registers, LDS and private segment of the training kernels, from the compiler's resource-usage remarks: cross-compiles
gaudi_amd/csrc/kernt_pred_train.hip and kernt_edm_train.hip of a source tree for gfx950 (no GPU needed) and prints one line per
kernel.  With a second tree, both and the difference:

    python tools/train_kernel_resources.py [--against /path/to/another/checkout]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaudi_amd.build import FLAGS  # noqa: E402

UNITS = ("kernt_pred_train", "kernt_edm_train")
KEYS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("LDS Size [bytes/block]", "LDS"),
        ("ScratchSize [bytes/lane]", "private"))


def resources(root):
    """-> {kernel: {column: int}} of the two training translation units under `root`."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(root, "gaudi_amd", "csrc")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tu in UNITS:
            r = subprocess.run([hipcc] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", tu + ".hip", "-o",
                                                  os.path.join(tmp, tu + ".o")], cwd=csrc, capture_output=True, text=True, check=True)
            cur = None
            for line in r.stderr.splitlines():
                m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
                if not m:
                    continue
                if m.group(1) == "Function Name":
                    cur = out.setdefault(re.sub(r"^_ZN\d+gaudi_e?train\d+(\w+_kernel).*", r"\1", m.group(2)), {})
                elif cur is not None:
                    for key, col in KEYS:
                        if m.group(1) == key:
                            cur[col] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="another checkout of this repository to compare with (printed first)")
    a = ap.parse_args()
    cols = [c for _, c in KEYS]
    here = resources(ROOT)
    if not a.against:
        print(f"{'kernel':22s} " + " ".join(f"{c:>8s}" for c in cols))
        for k, v in here.items():
            print(f"{k:22s} " + " ".join(f"{v[c]:8d}" for c in cols))
        return
    there = resources(a.against)
    print(f"{'kernel':22s} " + " ".join(f"{c:>14s}" for c in cols) + "   (other -> this tree)")
    gained = []
    for k, v in here.items():
        o = there.get(k)
        print(f"{k:22s} " + " ".join(f"{(str(o[c]) if o else '-') + ' -> ' + str(v[c]):>14s}" for c in cols))
        if o and o["private"] == 0 and v["private"] > 0:
            gained.append(k)
    if gained:
        raise SystemExit(f"gained a private segment: {gained}")


if __name__ == "__main__":
    main()
