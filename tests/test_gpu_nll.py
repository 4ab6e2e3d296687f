"""The EDM's eval-mode NLL on the GPU (gaudi_edm_nll: both network passes and the per-molecule sums in one launch of the
EDM-only kernels): against the reference (golden g25) on every kernel family, at scale against a numpy composition around the
already validated gaudi_phi, per molecule independent of its batch, and through GaudiModel / train_edm."""
import os

import numpy as np
import pytest

from gaudi_amd import synth
from tests.nll_helpers import CASES, TERMS, case, check_close, nll_terms

pytestmark = pytest.mark.gpu

FAMILIES = {"default": {}, "waves4": {"GAUDI_WAVES": 4}, "force_gn": {"GAUDI_FORCE_GN": 1}, "fp32_edges": {"GAUDI_EDGE_MATH": "fp32"}}


def _engine(eargs, esd, **env):
    from gaudi_amd.engine import Engine
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        eng = Engine(0)  # the knobs are read once, by gaudi_create
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    eng.load_edm(eargs, esd)
    return eng


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("name", CASES)
def test_edm_nll_vs_reference(golden, name, family):
    g = golden("g25_nll")
    args, sd, inp = case(g, name)
    eng = _engine(args, sd, **FAMILIES[family])
    try:
        nll, terms = eng.edm_nll(inp["x"], inp["h"], inp["t_int"], inp["node_mask"], inp["edge_mask"], seed=0, sample_offset=0,
                                 noise=inp["noise"], return_terms=True)
    finally:
        eng.close()
    ref = g[name + "_terms"]
    for k, what in enumerate(TERMS):
        check_close(terms[:, k], ref[:, k], f"{name} [{family}] {what}")
    check_close(nll, g[name + "_nll"], f"{name} [{family}] nll")


def _cata_batch(B, seed):
    from gaudi_amd.sampling_edm import build_masks
    rng = np.random.default_rng(seed)
    nm3, em, N = build_masks(np.full(B, 11), 11, False)
    return nm3.reshape(B, N), em.reshape(B, N, N), 1


def _hetero_batch(B, seed):
    from gaudi_amd.sampling_edm import build_masks
    rng = np.random.default_rng(seed)
    nm3, em, N = build_masks(rng.integers(3, 11, B), 10, True)
    return nm3.reshape(B, N), em.reshape(B, N, N), synth.num_node_features("hetro")


def _data(nm, F, seed):
    rng = np.random.default_rng(seed)
    B, N = nm.shape
    m = nm[:, :, None]
    x = rng.standard_normal((B, N, 3)).astype(np.float32) * 2.0 * m
    x = (x - x.sum(1, keepdims=True) / np.maximum(m.sum(1, keepdims=True), 1) * m).astype(np.float32)
    h = (np.eye(F, dtype=np.float32)[rng.integers(0, F, (B, N))] * m).astype(np.float32)
    return x, h


@pytest.mark.parametrize("shape", ["cata_256", "hetero_1024"])
def test_edm_nll_at_scale_vs_phi_composition(shape):
    """Philox noise: the fused launch against numpy around two gaudi_phi calls at host-built z_t / z_0 of the same draws."""
    from oracle import gaudi_oracle as O
    ds, B = ("cata", 256) if shape == "cata_256" else ("hetro", 1024)
    nm, em, F = (_cata_batch if ds == "cata" else _hetero_batch)(B, 5)
    args = synth.edm_args(dataset=ds)
    sd = synth.synth_edm_state_dict(args, F, seed=0)
    x, h = _data(nm, F, 6)
    T = int(args["diffusion_steps"])
    t_int = np.random.default_rng(7).integers(1, T + 1, B).astype(np.int32)
    t_int[0], t_int[-1] = 1, T
    eng = _engine(args, sd)
    try:
        seed, off = 1234567, 99
        nll, terms = eng.edm_nll(x, h, t_int, nm, em, seed=seed, sample_offset=off, return_terms=True)
        N, D = nm.shape[1], 3 + F
        raw = eng.philox_normal(seed, off, B, N * D, 0, 2).reshape(2, B, N, D)
        gamma = eng.gamma()
        ref, ref_terms = nll_terms(args, gamma, x, h, nm, t_int, raw[0], raw[1], lambda z, t: eng.phi(z, t, nm, em))
    finally:
        eng.close()
    for k, what in enumerate(TERMS):
        if what != "kl_prior":  # (float64 here: the fp32 cancellation of the device's host code is pinned by test_nll_cpu)
            check_close(terms[:, k], ref_terms[:, k], f"{shape} {what}")
    check_close(terms[:, 0], ref_terms[:, 0], f"{shape} kl_prior", tol=1e-4)
    # the total: 1e-4 of itself, or -- where the terms cancel (neg_log_constants and delta_log_px are -100 .. -150 on an 11-ring
    # molecule, its NLL a few units) -- 1e-5 of the largest term, a few fp32 roundings of the terms the two sides add up
    scale = np.maximum(np.abs(ref), 0.1 * np.abs(ref_terms).max(1))
    bad = np.abs(nll - ref) > 1e-4 * np.maximum(1.0, scale)
    assert not bad.any(), (np.argwhere(bad)[:5].tolist(), nll[bad][:5], ref[bad][:5])


def test_molecule_nll_does_not_depend_on_its_batch():
    """Same key (seed, sample_offset + index) -> the same bits alone and inside a mixed batch."""
    B = 48
    nm, em, F = _hetero_batch(B, 11)
    args = synth.edm_args(dataset="hetro")
    sd = synth.synth_edm_state_dict(args, F, seed=0)
    x, h = _data(nm, F, 12)
    t_int = np.random.default_rng(13).integers(1, int(args["diffusion_steps"]) + 1, B).astype(np.int32)
    eng = _engine(args, sd)
    try:
        full = eng.edm_nll(x, h, t_int, nm, em, seed=77, sample_offset=1000)
        for i in (0, 17, B - 1):
            one = eng.edm_nll(x[i:i + 1], h[i:i + 1], t_int[i:i + 1], nm[i:i + 1], em[i:i + 1], seed=77, sample_offset=1000 + i)
            assert one.view(np.uint32)[0] == full.view(np.uint32)[i], (i, one[0], full[i])
            half = eng.edm_nll(x[i // 2:], h[i // 2:], t_int[i // 2:], nm[i // 2:], em[i // 2:], seed=77,
                               sample_offset=1000 + i // 2)
            assert half.view(np.uint32)[i - i // 2] == full.view(np.uint32)[i]
    finally:
        eng.close()


def test_edm_nll_refuses_t_outside_1_to_T(golden):
    from gaudi_amd._lib import GaudiError
    g = golden("g25_nll")
    args, sd, inp = case(g, "cata_tiny")
    eng = _engine(args, sd)
    try:
        with pytest.raises(GaudiError, match="1..T"):
            eng.edm_nll(inp["x"], inp["h"], np.zeros_like(inp["t_int"]), inp["node_mask"], inp["edge_mask"], seed=0, sample_offset=0)
    finally:
        eng.close()


def test_model_forward_and_val_epoch(golden):
    """GaudiModel(x, h, node_mask, edge_mask): t from torch.randint as the reference draws it, noise from next_stream; injected
    [2,B,N,3+F] draws reproduce the reference's NLL; train_edm.val_epoch averages compute_loss over a loader."""
    import torch
    from gaudi_amd import train_edm
    from gaudi_amd.models_edm import GaudiModel
    g = golden("g25_nll")
    args, sd, inp = case(g, "hetro_tiny")
    eng = _engine(args, sd)
    try:
        model = GaudiModel.from_engine(eng, args)
        B, N = inp["x"].shape[:2]
        x, nm = torch.from_numpy(inp["x"]), torch.from_numpy(inp["node_mask"].reshape(B, N, 1))
        hd = {"categorical": torch.from_numpy(inp["h"]), "integer": torch.zeros(0)}
        em = torch.from_numpy(inp["edge_mask"].reshape(B, N * N))
        torch.manual_seed(3)
        got = model(x, hd, nm, em)
        assert isinstance(got, torch.Tensor) and got.shape == (B,)
        torch.manual_seed(3)
        t = torch.randint(1, model.T + 1, size=(B, 1)).numpy().reshape(B).astype(np.int32)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        want = eng.edm_nll(inp["x"], inp["h"], t, inp["node_mask"], inp["edge_mask"], seed=seed, sample_offset=0)
        assert np.array_equal(got.numpy(), want)
        # injected draws + the fixture's t: the reference's own NLL
        model.injected_noise, model.seed = inp["noise"], 0  # (an explicit seed: next_stream draws nothing from torch)
        real = torch.randint
        torch.randint = lambda lo, hi, size, **kw: torch.from_numpy(inp["t_int"].reshape(B, 1)).long()
        try:
            inj = model(x, hd, nm, em)
        finally:
            torch.randint = real
            model.injected_noise, model.seed = None, None
        check_close(inj.numpy(), g["hetro_tiny_nll"], "model(...) with injected draws")
        loader = [(x, torch.from_numpy(inp["node_mask"]), torch.from_numpy(inp["edge_mask"]), hd["categorical"], None)] * 2
        v = train_edm.val_epoch("val", 0, model, None, None, loader, None)
        assert np.isfinite(v) and v > 0
    finally:
        eng.close()
