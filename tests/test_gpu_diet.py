"""The guided sampler's hot phases with fewer non-arithmetic instructions: the addressing that changed, at the shapes where it can
go wrong.  The ring units of an edge-GEMM trip are dealt to the waves in consecutive runs (one LDS base per trip, the rest through
the load's immediate offset), the node GEMMs' weight loads carry the wave's tile in their vector offset and the second piece in the
immediate, and the segmented scans of the edge -> node sums are one DPP multiply-add per step.  None of it changes the arithmetic:
every case is one teacher-forced guided step at s = T/2 plus one unguided step against the C++ restatement (oracle/gaudi_cpu.cpp;
the numpy oracle on a host without the port's ISA) at 1e-4 per molecule, batches of 3 with mixed molecule sizes."""
import numpy as np
import pytest

from gaudi_amd import synth
from tests.helpers import TINY, TINY_P

pytestmark = pytest.mark.gpu

T_STEPS = 1000
S_IDX = T_STEPS // 2
W_TARGET = np.array([0.5, -1.0, 0.25, 0.0, 1.0], np.float32)
SCALE = 0.6

# name -> (EDM overrides, predictor overrides, live nodes per molecule)
CASES = {
    # 12 and 13 output tiles, the K tail of nf = 196, 24 and 26 ring units per trip on 8 waves
    "default_n11": ({}, {}, [11, 7, 9]),
    # most waves have no row to split
    "default_n3": ({}, {}, [3, 2, 3]),
    # two column tiles, the instantiation that recomputes its lane addresses per call
    "default_n17": ({}, {}, [17, 12, 15]),
    # ... and the half ring where the host picks it: 14 units per trip
    "default_n22": ({}, {}, [22, 20, 21]),
    # fewer K chunks than the node GEMMs' prefetch depth allows for, one trip group per chunk
    "w128_n11": (dict(nf=128), dict(nf=128), [11, 5, 8]),
    "tiny_n11": (TINY, TINY_P, [11, 5, 8]),
}


def _setup(name):
    from oracle import gaudi_oracle as O
    over_e, over_p, sizes = CASES[name]
    F = synth.num_node_features("cata")
    eargs = synth.edm_args(dataset="cata", diffusion_steps=T_STEPS, **over_e)
    pargs = synth.pred_args(dataset="cata", **over_p)
    esd = synth.synth_edm_state_dict(eargs, F, seed=21, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=22, amplify_coord=True)
    N = max(sizes)
    nm, em = O.build_masks(sizes, N, False)
    B = len(sizes)
    nm = np.asarray(nm, np.float32).reshape(B, N)
    em = np.asarray(em, np.float32).reshape(B, N, N)
    rng = np.random.default_rng(31)
    z = O._combined_noise(rng.standard_normal((B, N, 3 + F)).astype(np.float32), nm[:, :, None])
    eps = rng.standard_normal((B, N, 3 + F)).astype(np.float32)
    return eargs, esd, pargs, psd, nm, em, z, eps


_WANT = {}


def _want(name):
    """(guided, unguided) step of the checker, computed once per case."""
    if name not in _WANT:
        from oracle import build_cpu
        from oracle import gaudi_oracle as O
        eargs, esd, pargs, psd, nm, em, z, eps = _setup(name)
        gamma = O.gamma_table("polynomial_2", T_STEPS, 1e-5)
        if build_cpu.cpu_ok():
            port = build_cpu.CpuPort()
            port.load_edm(eargs, esd)
            port.load_predictor(pargs, psd)
            coef = O.step_coefficients(gamma, S_IDX, S_IDX + 1)
            t_val = np.float32(np.float32(S_IDX + 1) / np.float32(T_STEPS))
            guided = port.step(coef, t_val, z, nm, em, eps, target_w=W_TARGET, scale=SCALE)
            unguided = port.step(coef, t_val, z, nm, em, eps)
            port.close()
        else:
            guided = O.step_guided(esd, eargs, psd, pargs, gamma, S_IDX, z, nm[:, :, None], em, eps, W_TARGET, SCALE)
            unguided = O.step_unguided(esd, eargs, gamma, S_IDX, z, nm[:, :, None], em, eps)
        guided.setflags(write=False)
        unguided.setflags(write=False)
        _WANT[name] = (guided, unguided)
    return _WANT[name]


def _per_molecule(got, want):
    B = want.shape[0]
    return np.abs(got - want).reshape(B, -1).max(1) / np.abs(want).reshape(B, -1).max(1)


@pytest.mark.parametrize("name", list(CASES))
def test_guided_and_unguided_step_vs_cpu_port(name):
    from gaudi_amd.engine import Engine
    eargs, esd, pargs, psd, nm, em, z, eps = _setup(name)
    want_g, want_u = _want(name)
    eng = Engine(0)
    eng.load_edm(eargs, esd)
    eng.load_predictor(pargs, psd)
    got_g = eng.step(S_IDX, z, nm, em, eps, target_w=W_TARGET, scale=SCALE)
    shape_g, math_g = eng.last_launch_shape(), eng.edge_math()
    got_u = eng.step(S_IDX, z, nm, em, eps)
    assert eng.kernel_variant()[1] == 8
    eng.close()
    err_g, err_u = _per_molecule(got_g, want_g), _per_molecule(got_u, want_u)
    print(f"{name}: guided {err_g.max():.2e} unguided {err_u.max():.2e} (launch {shape_g}, edge math {math_g})")
    assert err_g.max() < 1e-4, (int(err_g.argmax()), float(err_g.max()))
    assert err_u.max() < 1e-4, (int(err_u.argmax()), float(err_u.max()))
    assert np.all(got_g[nm == 0] == 0) and np.all(got_u[nm == 0] == 0)


def test_guided_chain_in_launches_of_two_steps_repeats_bit_for_bit():
    """A 4-step guided chain of 4 molecules, two steps per launch, run twice: the ring loads of every wave are retired before the
    barrier that opens a trip whichever wave issued them, so two runs give the same bits."""
    from gaudi_amd.engine import Engine
    from oracle import gaudi_oracle as O
    T = 4
    F = synth.num_node_features("cata")
    eargs, pargs = synth.edm_args(dataset="cata", diffusion_steps=T), synth.pred_args(dataset="cata")
    esd = synth.synth_edm_state_dict(eargs, F, seed=21, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=22, amplify_coord=True)
    sizes = [11, 7, 9, 11]
    nm, em = O.build_masks(sizes, 11, False)
    nm = np.asarray(nm, np.float32).reshape(4, 11)
    em = np.asarray(em, np.float32).reshape(4, 11, 11)
    eng = Engine(0)
    eng.load_edm(eargs, esd)
    eng.load_predictor(pargs, psd)
    eng.set_steps_per_launch(2)
    runs = [eng.sample(nm, em, seed=5, sample_offset=2, target_w=W_TARGET, scale=SCALE, return_z0=True) for _ in range(2)]
    eng.close()
    assert np.isfinite(runs[0][0]).all()
    n_arrays = 0
    for u, v in zip(*runs):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v)
            n_arrays += 1
    assert n_arrays >= 2
