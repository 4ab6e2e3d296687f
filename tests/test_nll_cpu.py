"""The EDM's eval-mode NLL without a GPU: the network-free terms of the C++ host code (the exact function gaudi_edm_nll uses)
and a numpy composition of the whole NLL around the oracle's phi, both against the reference (golden g25); the refusals of
the host mirror."""
import ctypes as C

import numpy as np
import pytest

from gaudi_amd import synth
from oracle import gaudi_oracle as O
from tests.nll_helpers import CASES, case, check_close, nll_terms, noise_power


def _lib():
    from gaudi_amd import _lib, build
    build.build()
    return _lib.load_library(), _lib


def _host_terms(args, inp):
    lib, L = _lib()
    x, h, nm = (np.ascontiguousarray(inp[k], np.float32) for k in ("x", "h", "node_mask"))
    B, N, F = h.shape
    ti = np.ascontiguousarray(inp["t_int"], np.int32)
    out = np.empty((B, 4), np.float32)
    nv = args["normalize_factors"]
    rc = lib.gaudi_host_nll_terms(int(args["diffusion_steps"]), noise_power(args), float(args["diffusion_noise_precision"]),
                                  float(nv[0]), float(nv[1]), B, N, F, L.fptr(x), L.fptr(h), L.fptr(nm),
                                  ti.ctypes.data_as(L.IP), L.fptr(out))
    return rc, out


@pytest.mark.parametrize("name", CASES)
def test_host_nll_terms_match_reference(golden, name):
    g = golden("g25_nll")
    args, _, inp = case(g, name)
    rc, out = _host_terms(args, inp)
    assert rc == 0
    ref = g[name + "_terms"]
    np.testing.assert_allclose(out[:, 1], ref[:, 2], rtol=1e-6, atol=0, err_msg="neg_log_constants")
    np.testing.assert_allclose(out[:, 2], ref[:, 4], rtol=1e-6, atol=0, err_msg="delta_log_px")
    # SNR weight exp(gamma_t - gamma_s) - 1: the C++ gamma table equals the reference's to 2e-7 relative (test_abi_cpu), one ulp
    # of gamma near T -- where consecutive gammas differ by a few tenths -- moves the weight by (1 + weight) ulp(gamma)
    snr = g[name + "_snr_weight"].astype(np.float64)
    gamma = np.empty(int(args["diffusion_steps"]) + 1, np.float32)
    assert _lib()[0].gaudi_host_schedule(len(gamma) - 1, noise_power(args), float(args["diffusion_noise_precision"]),
                                         _lib()[1].fptr(gamma), None) == 0
    ti = inp["t_int"].astype(np.int64)
    slack = (1 + snr) * (np.spacing(np.abs(gamma[ti])) + np.spacing(np.abs(gamma[ti - 1])))
    assert np.all(np.abs(out[:, 3] - snr) <= np.maximum(1e-6 * np.abs(snr), slack)), (out[:, 3], snr)
    # kl_prior is a difference of nearly equal fp32 numbers (0.5 (n - 1) 3 sigma_T^2 against 0.5 (n - 1) 3): the same float
    # operations give it to the last bits; the floor is one ulp of the cancelling terms, which a different summation order may move
    floor = np.spacing(np.float32(1.5) * np.maximum(inp["node_mask"].sum(1), 1)).astype(np.float64)
    assert np.all(np.abs(out[:, 0] - ref[:, 0]) <= np.maximum(1e-6 * np.abs(ref[:, 0]), floor)), (out[:, 0], ref[:, 0])


@pytest.mark.parametrize("name", CASES)
def test_numpy_nll_around_the_oracle_phi_reproduces_reference(golden, name):
    g = golden("g25_nll")
    args, sd, inp = case(g, name)
    gamma = O.gamma_table(args["diffusion_noise_schedule"], int(args["diffusion_steps"]), args["diffusion_noise_precision"])
    B, N = inp["x"].shape[:2]
    nm3 = inp["node_mask"].reshape(B, N, 1)

    def phi(z, t):
        return O.edm_phi(sd, args, z, t, nm3, inp["edge_mask"])

    nll, terms = nll_terms(args, gamma, inp["x"], inp["h"], inp["node_mask"], inp["t_int"], inp["noise"][0], inp["noise"][1], phi)
    check_close(nll, g[name + "_nll"], f"{name} nll")
    for k in (1, 2, 3, 4, 5):
        check_close(terms[:, k], g[name + "_terms"][:, k], f"{name} term {k}")


def test_soft_case_exercises_the_categorical_term(golden):
    g = golden("g25_nll")
    assert np.abs(g["hetro_soft_log_ph"]).max() > 1e-3


def test_host_nll_terms_refuse_t_outside_1_to_T(golden):
    g = golden("g25_nll")
    args, _, inp = case(g, "cata_tiny")
    for bad in (0, int(args["diffusion_steps"]) + 1):
        inp2 = dict(inp, t_int=np.full_like(inp["t_int"], bad))
        rc, _ = _host_terms(args, inp2)
        assert rc != 0


def _model_without_device():
    """A GaudiModel whose checks run before any device call (no GPU here)."""
    from gaudi_amd.models_edm import GaudiModel
    m = GaudiModel.__new__(GaudiModel)
    m.args = synth.edm_args(dataset="cata", diffusion_steps=50)
    m.engine, m.T, m.in_node_nf, m.n_dims = None, 50, 1, 3
    m.norm_values, m.norm_biases = [3.0, 4.0, 10.0], (None, 0.0, 0.0)
    m.seed, m.sample_offset, m.injected_noise, m.last_diag = None, 0, None, None
    return m


def _inputs(B=2, N=5):
    import torch
    nm = np.ones((B, N, 1), np.float32)
    nm[1, 3:] = 0
    x = np.random.default_rng(0).standard_normal((B, N, 3)).astype(np.float32) * nm
    x = x - x.sum(1, keepdims=True) / nm.sum(1, keepdims=True) * nm
    h = np.ones((B, N, 1), np.float32) * nm
    em = (nm * nm.transpose(0, 2, 1) * (1 - np.eye(N, dtype=np.float32))).reshape(B, N * N)
    return torch.from_numpy(x), {"categorical": torch.from_numpy(h), "integer": torch.zeros(0)}, torch.from_numpy(nm), torch.from_numpy(em)


def test_forward_refuses_context_train_and_off_centre_positions():
    from gaudi_amd._lib import GaudiError
    m = _model_without_device()
    x, h, nm, em = _inputs()
    with pytest.raises(GaudiError, match="context"):
        m(x, h, nm, em, context=x[:, :, :1])
    with pytest.raises(GaudiError, match="training"):
        m.train()
    assert m.train(False) is m
    with pytest.raises(GaudiError, match="Mean is not zero"):
        m(x + 1.0 * nm, h, nm, em)
    with pytest.raises(GaudiError, match="not masked"):
        m(x, {"categorical": h["categorical"] + 1.0, "integer": h["integer"]}, nm, em)
    with pytest.raises(GaudiError, match="integer"):
        m(x, {"categorical": h["categorical"], "integer": h["categorical"]}, nm, em)


def test_train_edm_compute_loss_refuses_unmasked_positions():
    from gaudi_amd import train_edm
    from gaudi_amd._lib import GaudiError
    m = _model_without_device()
    x, h, nm, em = _inputs()
    with pytest.raises(GaudiError, match="not masked"):
        train_edm.compute_loss(m, x + 1.0, h["categorical"], nm, em)
