"""Every case of the kernel census (tests/kernel_census.py) on the GPU: one engine per case under the case's switches, synthetic
weights with amplified coordinate heads, the case's calls on three molecules of mixed size -- then the kernel-table keys the engine
launched must EQUAL the set the case claims (a call the planner routes elsewhere fails here even where the other kernel is right),
and every output is held against the numpy oracle in float64 at the suite's bars for these calls: 1e-4 per molecule for a reverse
step (tests/test_gpu_diet.py), tests/test_gpu_parity.py's TOL for phi and the predictor's gradient, exact zeros on masked nodes.
The keys launched and the measured error of every call are printed before anything is asserted.

Measured on an MI355X, all 65 cases (profiles/kernel_census_mi355x.txt): the keys launched equal the claimed set everywhere; phi 1.9e-7 .. 4.4e-6 (sin_embedding: 5.7e-6 ..
4.1e-5), the predictor 1.0e-7 .. 1.8e-6, its gradient 1.1e-7 .. 3.5e-6, every step 6.6e-8 .. 1.8e-7, the sampled chain 5.3e-7.

phi of a sin_embedding denoiser is what this file found: with the embedding's argument in fp32 (the squared distance, its root times
up to 429) seven of the eleven sin_embedding cases missed 1e-4 -- se2_48_48 1.6e-3, se2_32_32 1.5e-3, se2_64_64 4.5e-4, gn4_se_32_48
3.6e-4, se_32_48 2.4e-4, gn4_se_192_208 2.4e-4, se2_256_256 2.0e-4 -- as far off as the oracle evaluated in float32 is from its own
float64 evaluation (printed as phi_fp32_oracle, not asserted).  The sampler now forms that argument in double from the fp32
coordinates (edm_device.h: sin_features(double)); everything else stays fp32.
"""
import torch  # noqa: F401  (first: the HIP runtime the library links against is torch's)
import numpy as np
import pytest

from gaudi_amd import synth
from tests import kernel_census as KC
from tests.helpers import rel_err
from tests.test_gpu_diet import SCALE, W_TARGET, _per_molecule
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

T_STEPS = 1000
S_IDX = T_STEPS // 2
T_CHAIN = 3  # diffusion steps of the one sampling case


def _masks(c):
    from oracle import gaudi_oracle as O
    B = len(c.sizes)
    if c.dataset == "hetro":
        assert c.mask == 0
        nm, em = O.build_masks(c.sizes, max(c.sizes), True)
        N = 2 * max(c.sizes)
        return np.asarray(nm, np.float32).reshape(B, N), np.asarray(em, np.float32).reshape(B, N, N)
    N = max(c.sizes)
    if c.mask == 0:
        nm, em = O.build_masks(c.sizes, N, False)
        return np.asarray(nm, np.float32).reshape(B, N), np.asarray(em, np.float32).reshape(B, N, N)
    nm, em = np.zeros((B, N), np.float32), np.zeros((B, N, N), np.float32)
    for b, n in enumerate(c.sizes):  # every live node tied to its c.mask neighbours on either side of a cycle
        nm[b, :n] = 1
        for i in range(n):
            for d in range(1, c.mask + 1):
                j = (i + d) % n
                if j != i:
                    em[b, i, j] = em[b, j, i] = 1
    return nm, em


def _engine(c, eargs, esd, pargs, psd, monkeypatch):
    from gaudi_amd.engine import Engine
    for k, v in c.env.items():  # (read once, when the handle is created)
        monkeypatch.setenv(k, str(v))
    eng = Engine(0)
    for k in c.env:
        monkeypatch.delenv(k)
    eng.load_edm(eargs, esd)
    eng.load_predictor(pargs, psd)
    return eng


def _compare(c, got, a):
    """-> ([(figure, measured, bar)], {what must be exactly zero: whether it is}) of the case's outputs against the float64 oracle."""
    from oracle import gaudi_oracle as O
    F64 = np.float64
    nm, em, z, eps, t = a["nm"], a["em"], a["z"], a["eps"], a["t"]
    esd, eargs, psd, pargs = a["esd"], a["eargs"], a["psd"], a["pargs"]
    dead = nm == 0
    gamma = O.gamma_table("polynomial_2", T_STEPS, 1e-5)
    figures, zeros, want_guided = [], {}, None
    for call in c.calls:
        if call == "phi":
            want = O.edm_phi(esd, eargs, z, t, nm, em, dtype=F64)
            figures.append((call, rel_err(got[call], want), TOL))
            if eargs.get("sin_embedding"):  # (printed, not asserted: what an fp32 embedding argument costs this network -- see the docstring)
                figures.append(("phi_fp32_oracle", rel_err(O.edm_phi(esd, eargs, z, t, nm, em), want), None))
            zeros[call] = bool(np.all(got[call][dead] == 0))
        elif call == "pgrad":
            pred_w, grad_w = O.predictor_grad(psd, pargs, z, nm, em, t, a["dpred"], dtype=F64)
            figures += [("pred", rel_err(got[call][0], pred_w), TOL), ("pgrad", rel_err(got[call][1], grad_w), TOL)]
            zeros[call] = bool(np.all(got[call][1][dead] == 0))
        elif call == "unguided":
            want = O.step_unguided(esd, eargs, gamma, S_IDX, z, nm[:, :, None], em, eps, dtype=F64)
            figures.append((call, float(_per_molecule(got[call], want).max()), 1e-4))
            zeros[call] = bool(np.all(got[call][dead] == 0))
        elif call in ("guided", "target"):
            if want_guided is None:
                want_guided = O.step_guided(esd, eargs, psd, pargs, gamma, S_IDX, z, nm[:, :, None], em, eps, W_TARGET, SCALE, dtype=F64)
            figures.append((call, float(_per_molecule(got[call], want_guided).max()), 1e-4))
            zeros[call] = bool(np.all(got[call][dead] == 0))
        elif call == "sample":
            x, h, diag = got[call]
            xo, ho, _ = O.sample(esd, eargs, nm[:, :, None], em, a["noise"], pred_sd=psd, pcfg=pargs, target_w=W_TARGET, scale=SCALE, dtype=F64)
            figures.append((call, float(_per_molecule(x, np.asarray(xo)).max()), 1e-4))
            zeros[call] = bool(np.all(x[dead] == 0) and np.all(h[dead] == 0) and diag["max_masked_leak"] == 0)
            zeros["sample: one-hot equal"] = bool(np.array_equal(h, np.asarray(ho, h.dtype)))
    return figures, zeros


@pytest.mark.parametrize("c", KC.CASES, ids=[c.name for c in KC.CASES])
def test_case_launches_its_kernels_and_matches_the_float64_oracle(c, monkeypatch):
    from oracle import gaudi_oracle as O
    F = synth.num_node_features(c.dataset)
    chain = "sample" in c.calls
    eargs = synth.edm_args(diffusion_steps=T_CHAIN if chain else T_STEPS, **c.edm)
    pargs = synth.pred_args(**c.pred)
    esd = synth.synth_edm_state_dict(eargs, F, seed=21, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=22, amplify_coord=True)
    nm, em = _masks(c)
    B, N = nm.shape
    rng = np.random.default_rng(31)
    z = O._combined_noise(rng.standard_normal((B, N, 3 + F)).astype(np.float32), nm[:, :, None])
    eps = rng.standard_normal((B, N, 3 + F)).astype(np.float32)
    t = np.array([0.3, 0.55, 0.8], np.float32)
    dpred = np.broadcast_to(W_TARGET * np.float32(SCALE), (B, 5)).copy()
    noise = rng.standard_normal((T_CHAIN + 2, B, N, 3 + F)).astype(np.float32)

    eng = _engine(c, eargs, esd, pargs, psd, monkeypatch)
    got = {}
    for call in c.calls:  # (every launch first: a fault must not hide behind a finished comparison)
        if call == "phi":
            got[call] = eng.phi(z, t, nm, em)
        elif call == "pgrad":
            got[call] = eng.predictor_grad(z, t, nm, em, dpred)
        elif call == "guided":
            got[call] = eng.step(S_IDX, z, nm, em, eps, target_w=W_TARGET, scale=SCALE)
        elif call == "unguided":
            got[call] = eng.step(S_IDX, z, nm, em, eps)
        elif call == "target":  # zero curvature, shared arrays: the affine target, which must equal the guided step
            got[call] = eng.step_target(S_IDX, z, nm, em, eps, dict(w=W_TARGET, scale=SCALE))
        elif call == "sample":
            got[call] = eng.sample(nm, em, noise=noise, target_w=W_TARGET, scale=SCALE)
        else:
            raise AssertionError(call)
    launched = eng.kernel_keys_launched()
    eng.close()
    print(f"\n{c.name}: launched " + " | ".join(launched))

    # the keys launched and the measured figures first, every one of them; then the key set, the zeros and the bars
    figures, zeros = _compare(c, got, dict(esd=esd, eargs=eargs, psd=psd, pargs=pargs, nm=nm, em=em, z=z, eps=eps, t=t, dpred=dpred,
                                           noise=noise))
    print(f"{c.name}: max error vs float64 oracle " + " ".join(f"{k}={v:.2e}" for k, v, _ in figures))
    assert set(launched) == set(c.keys), (sorted(set(launched) - c.keys), sorted(c.keys - set(launched)))
    assert all(zeros.values()), zeros
    for k, v, bar in figures:
        assert bar is None or v < bar, (c.name, k, v, bar)
