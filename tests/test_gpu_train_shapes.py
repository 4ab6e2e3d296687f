"""The two training passes (gaudi_edm_loss_grad with kernt_edm_train.hip, gaudi_predictor_loss_grad with kernt_pred_train.hip)
against oracle/train_oracle.py -- float64 autograd, evaluated here -- at the shapes of tests/train_shapes.py: the row tails of
mm_rows and pt_outer_kernel, E = N * N around the thread count and up to the limit of 128 nodes, molecules without a live edge,
the widths 250 / 256 / 20, depth, every switch, the schedule's ends, every element at the default widths, and a batch cut into
several scratch chunks.  tests/test_train_oracle_cpu.py pins the oracle to the reference's own numbers and holds every case to
the conditions that make this comparison meaningful.

Per case: the loss against the oracle's float32 evaluation at 1e-5 (the bar of the fixture tests, which compare with the
reference's float32 loss: kl_prior cancels to its last bits and is only reproducible as the same sequence of float32
operations); net / pred and EVERY gradient tensor element-wise (rel_err) against the float64 oracle at max(1e-4, twice the
oracle's own float32 spread) -- above 1e-4 for sin_embedding only; the set of tensors without a gradient path."""
import time

import numpy as np
import pytest

from tests import train_shapes as TS
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
LOSS_TOL = 1e-5
ZERO_WITHOUT_EDGES = ("edge_mlp.", "att_mlp.", "coord_mlp.")


def _engine(case):
    from gaudi_amd.engine import Engine
    eargs, esd, pargs, psd = TS.models(case)
    eng = Engine(0)
    eng.load_edm(eargs, esd)
    if case.net == "pred":
        eng.load_predictor(pargs, psd)
    return eng


def _call(eng, case, ref):
    i = TS.inputs(case)
    if case.net == "edm":
        return eng.edm_loss_grad(i["x"], i["h"], i["t_int"], i["node_mask"], i["edge_mask"], noise=i["noise"],
                                 loss_type=case.loss_type, weight=None if case.weight is None else np.array(case.weight, np.float32))
    return eng.predictor_loss_grad(i["x"], i["h"], i["t_int"], i["node_mask"], i["edge_mask"], ref.y, noise=i["noise"])


def compare(case, ref, got, what=""):
    """-> (record, failures): the worst error per quantity, and one message per case, tensor and quantity out of bounds."""
    loss, out, grads = got
    bar = TS.bar(ref)
    fails = []
    l32 = np.asarray(ref.loss32, np.float64).reshape(-1)
    lerr = float(np.max(np.abs(np.asarray(loss, np.float64).reshape(-1) - l32) / np.abs(l32)))
    if not lerr <= LOSS_TOL:
        fails.append(f"{case.name}{what}: loss {np.asarray(loss).reshape(-1)} vs {l32}: {lerr:.3g} > {LOSS_TOL}")
    oerr = rel_err(out, ref.out)
    if not oerr < bar:
        fails.append(f"{case.name}{what}: {'net' if case.net == 'edm' else 'pred'}: {oerr:.3g} >= {bar:.3g}")
    none_got = {n for n, v in grads.items() if v is None}
    none_ref = {n for n, v in ref.grads.items() if v is None}
    if none_got != none_ref or set(grads) != set(ref.grads):
        fails.append(f"{case.name}{what}: tensors without a gradient {sorted(none_got)} vs {sorted(none_ref)}")
    worst, worst_name = 0.0, "-"
    for n, v in ref.grads.items():
        if v is None or grads.get(n) is None:
            continue
        err = rel_err(grads[n], v)
        if not np.all(np.isfinite(grads[n])):
            err = float("inf")
        if err > worst:
            worst, worst_name = err, n
        if not err < bar:
            fails.append(f"{case.name}{what}: grad {n}: {err:.3g} >= {bar:.3g}")
        if case.no_edges and any(s in n for s in ZERO_WITHOUT_EDGES) and np.any(grads[n]):
            fails.append(f"{case.name}{what}: grad {n}: not exact zeros without a live edge (max {np.abs(grads[n]).max():.3g})")
    rec = dict(name=case.name + what, loss=lerr, loss64=rel_err(loss, ref.loss), out=oerr, grad=worst, tensor=worst_name, bar=bar)
    return rec, fails


def run_case(name, setenv=None, delenv=None):
    """One case on the device -> (record, failures).  setenv / delenv: how the chunk cases set their knob (monkeypatch's in a test)."""
    case = TS.BY_NAME[name]
    ref = TS.reference(name)
    eng = _engine(case)
    try:
        t0 = time.perf_counter()
        got = _call(eng, case, ref)
        secs = time.perf_counter() - t0
        rec, fails = compare(case, ref, got)
        if case.env:
            B = len(case.live)
            kb = TS.knob_kb(case, 2)
            Bc = TS.chunk_of(case, kb)
            if not (B > Bc == 2 and B % Bc == 1):  # two full chunks and a short last one
                fails.append(f"{name}: the knob gives chunks of {Bc} for B = {B}")
            setenv(case.env, str(kb))
            try:
                t0 = time.perf_counter()
                chunked = _call(eng, case, ref)
                secs += time.perf_counter() - t0
            finally:
                delenv(case.env)
            rec_c, fails_c = compare(case, ref, chunked, " (chunks of 2)")
            fails += fails_c
            for k in ("loss", "out", "grad"):
                if rec_c[k] > rec[k]:
                    rec[k] = rec_c[k]
                    if k == "grad":
                        rec["tensor"] = rec_c["tensor"]
            if not (np.array_equal(chunked[0], got[0]) and np.array_equal(chunked[1], got[1])):
                fails.append(f"{name}: loss / {'net' if case.net == 'edm' else 'pred'} of the chunked call differ in bits from one chunk's")
            for n, v in got[2].items():
                if v is None:
                    continue
                err = rel_err(chunked[2][n], v)  # the summation order depends on the chunk size: not the same bits
                if not err < 1e-4:
                    fails.append(f"{name}: grad {n}: chunked vs one chunk {err:.3g} >= 1e-4")
        rec["seconds"] = secs
    finally:
        eng.close()
    return rec, fails


def line(rec):
    return (f"{rec['name']:28s} loss {rec['loss']:.2e} (vs float64 {rec['loss64']:.2e})  out {rec['out']:.2e}  grad {rec['grad']:.2e} "
            f"{rec['tensor']}  bar {rec['bar']:.1e}  {rec['seconds']:.2f} s")


@pytest.mark.parametrize("name", list(TS.BY_NAME))
def test_kernels_vs_oracle(name, monkeypatch):
    rec, fails = run_case(name, monkeypatch.setenv, monkeypatch.delenv)
    print(line(rec))
    assert not fails, "\n".join(fails)
    case = TS.BY_NAME[name]
    if not (case.net == "edm" and case.edm.get("sin_embedding")):
        assert rec["bar"] == 1e-4
