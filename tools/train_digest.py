#!/usr/bin/env python3
"""sha256 of what the two training passes return (gaudi_edm_loss_grad, gaudi_predictor_loss_grad), one line per case: the
bit-for-bit record a change to the training code that must not change a number (csrc/train_host.inc, train_device.h and the files
that use them) is checked with.  Run it on the library before the change and on the library after it (GAUDI_LIB names the
library, gaudi_amd/_lib.py) and compare the two listings: they must be identical.

    GAUDI_LIB=/path/to/libgaudi_hip.so python tools/train_digest.py

The cases are those of tests/train_shapes.py (its models and inputs; the predictor's targets as its reference() draws them).  A
case that carries a scratch knob runs once more under it, in chunks of 2: the knob value comes from the scratch per molecule of
the library that runs -- its gaudi_host_train_floats_per_mol, or, for a library from before that export, the formula of that
time.  Then one EDM call with noise=None (the Philox draw) and one forward-only EDM call.  A digest covers the loss, net / pred,
every gradient tensor in name order (dtype, shape, bytes) and the set of tensors without a gradient.

Each network's cases run in a child process of their own under a time limit; after a failure nothing more is started.
"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = ("edm", "pred")
LIMIT = 420  # seconds per child: a few seconds of start-up, well under a second per call, the float64 oracle for the targets


def digest(loss, out, grads) -> str:
    import numpy as np
    h = hashlib.sha256()
    for a in (np.asarray(loss, np.float32).reshape(-1), out):
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype}{a.shape};".encode())
        h.update(a.tobytes())
    for name in sorted(grads):
        if grads[name] is None:
            continue
        a = np.ascontiguousarray(grads[name])
        h.update(f"{name}:{a.dtype}{a.shape};".encode())
        h.update(a.tobytes())
    h.update(("none=" + ",".join(sorted(n for n, v in grads.items() if v is None))).encode())
    return h.hexdigest()


def floats_per_mol(lib, case) -> int:
    """The scratch per molecule of the library that runs."""
    from tests import train_shapes as TS
    net, N, H, L, S, F, K, A = TS.shape_of(case)
    if hasattr(lib, "gaudi_host_train_floats_per_mol"):
        out = C.c_int64(0)
        if lib.gaudi_host_train_floats_per_mol(net, N, H, L, S, F, K, A, C.byref(out)) != 0:
            raise SystemExit(f"{case.name}: gaudi_host_train_floats_per_mol refused {(net, N, H, L, S, F, K, A)}")
        return out.value
    return TS.pt_floats_per_mol_two_buffers(N, H, L, F + 1, K) if net == 0 else TS.et_floats_per_mol(N, H, L, S, F, A)


def run_group(net: str):
    import numpy as np
    import torch
    from gaudi_amd import _lib
    from gaudi_amd.engine import Engine
    from tests import train_shapes as TS

    lib = _lib.load_library()

    def call(eng, case, y, **kw):
        i = TS.inputs(case)
        kw.setdefault("noise", i["noise"])
        if case.net == "edm":
            return eng.edm_loss_grad(i["x"], i["h"], i["t_int"], i["node_mask"], i["edge_mask"], loss_type=case.loss_type,
                                     weight=None if case.weight is None else np.array(case.weight, np.float32), **kw)
        return eng.predictor_loss_grad(i["x"], i["h"], i["t_int"], i["node_mask"], i["edge_mask"], y, **kw)

    def show(name, got):
        print(f"{name} {digest(*got)}", flush=True)

    for case in TS.CASES:
        if case.net != net:
            continue
        eargs, esd, pargs, psd = TS.models(case)
        y = TS.targets(case, TS.run_oracle(case, torch.float64)[1]) if net == "pred" else None  # (reference(name).y)
        eng = Engine(0)
        try:
            eng.load_edm(eargs, esd)
            if net == "pred":
                eng.load_predictor(pargs, psd)
            show(case.name, call(eng, case, y))
            if case.env:
                per = floats_per_mol(lib, case)
                kb = (2 * per * 4 + 1023) // 1024
                if not (kb * 1024 // 4 // per == 2 and len(case.live) > 2):
                    raise SystemExit(f"{case.name}: {kb} KiB does not give chunks of 2")
                os.environ[case.env] = str(kb)  # (read on every call)
                try:
                    show(f"{case.name}/chunks_of_2", call(eng, case, y))
                finally:
                    del os.environ[case.env]
            if case.name == "edm_n17":
                show(f"{case.name}/philox", call(eng, case, y, noise=None, seed=11, sample_offset=3))
                show(f"{case.name}/forward_only", call(eng, case, y, grad=False))
        finally:
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=GROUPS, help="run one network's cases in THIS process (what the parent starts per group)")
    a = ap.parse_args()
    if a.group:
        run_group(a.group)
        return
    for group in GROUPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", group], timeout=LIMIT)
        if r.returncode != 0:  # a fault or a refusal: start nothing more on the device
            raise SystemExit(f"group {group} ended with status {r.returncode}")


if __name__ == "__main__":
    main()
