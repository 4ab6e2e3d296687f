"""The side job of the resident N1 fused kernel: where no workgroup of a launch has an edge tile for its last wave (at most 7 tiles:
11 fully connected nodes), that wave computes the h half of the predictor's node-MLP first Linear during the edge phase, and the
GEMM behind the phase starts from its rows.  No floating-point operation or its order changes: the job must run exactly where it
may, give the bits of a launch without it, and stay within 1e-4 per molecule of the C++ restatement (the cases, seeds and bar of
tests/test_gpu_diet.py, whose references are shared).

The flag: the key of a launch that ran the job ends in " SD=1" (gaudi_last_kernel_key) -- set where the plan placed the job's rows
AND the kernel launched has the job compiled in (a build with GAUDI_SIDE_STAGES=0 never shows it).  The job is a launch parameter
of the N1 fused kernel, so the kernel table and the log of launched keys keep their names."""
import numpy as np
import pytest

from tests import test_gpu_diet as D
from tests import test_gpu_n1 as N
from tests.helpers import TINY, TINY_P

pytestmark = pytest.mark.gpu



SIDE = " SD=1"


@pytest.mark.parametrize("name", ["default_n11", "default_n3"])
def test_side_job_runs_and_gives_the_n1_kernels_bits(name, monkeypatch):
    """default_n11: 11 / 7 / 9 live nodes = 7, 3 and 5 edge tiles -- the full shape, and workgroups in which waves 5-6 (5 tiles) or
    3-6 (3 tiles) idle too."""
    eng = N._engine(name)
    nm, em = D._setup(name)[4:6]
    assert max(eng.pack_plan(nm, em)[2]) <= 7
    (g1, kg1), (u1, ku1) = N._steps(eng, name)
    eng.close()
    print(f"{name}: guided [{kg1}] unguided [{ku1}]")
    assert N.N1 in kg1 and "HPE=192 HPP=208" in kg1 and kg1.endswith(SIDE), kg1
    assert N.N1 in ku1 and "HPE=192 HPP=0" in ku1 and "SD=" not in ku1, ku1  # (the side job is the predictor's)
    N._check_vs_port(name, g1, u1)
    eng = N._engine(name, monkeypatch, GAUDI_NO_SIDE=1)
    (g0, kg0), (u0, ku0) = N._steps(eng, name)
    eng.close()
    assert N.N1 in kg0 and "HPE=192 HPP=208" in kg0 and "SD=" not in kg0 and "SD=" not in ku0, (kg0, ku0)
    assert np.array_equal(g0, g1) and np.array_equal(u0, u1)


def test_a_workgroup_with_eight_tiles_runs_no_side_job():
    """12 nodes with six node pairs masked out: 120 live edge slots = 8 tiles in one round -- the last wave has a tile."""
    from gaudi_amd import synth
    from gaudi_amd.engine import Engine
    from oracle import build_cpu
    from oracle import gaudi_oracle as O
    sizes, n = [12, 11, 12], 12
    F = synth.num_node_features("cata")
    eargs, pargs = synth.edm_args(dataset="cata", diffusion_steps=D.T_STEPS), synth.pred_args(dataset="cata")
    esd = synth.synth_edm_state_dict(eargs, F, seed=21, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=22, amplify_coord=True)
    nm, em = O.build_masks(sizes, n, False)
    nm = np.asarray(nm, np.float32).reshape(3, n)
    em = np.array(em, np.float32).reshape(3, n, n)
    for b in (0, 2):
        for i in range(6):  # pairs (0, 11), (1, 10), ...: every node keeps ten neighbours
            em[b, i, n - 1 - i] = em[b, n - 1 - i, i] = 0.0
    rng = np.random.default_rng(33)
    z = O._combined_noise(rng.standard_normal((3, n, 3 + F)).astype(np.float32), nm[:, :, None])
    eps = rng.standard_normal((3, n, 3 + F)).astype(np.float32)
    eng = Engine(0)
    eng.load_edm(eargs, esd)
    eng.load_predictor(pargs, psd)
    assert sorted(eng.pack_plan(nm, em)[2]) == [7, 8, 8]
    got = eng.step(D.S_IDX, z, nm, em, eps, target_w=D.W_TARGET, scale=D.SCALE)
    key = eng.last_kernel_key()
    eng.close()
    assert N.N1 in key and "HPE=192 HPP=208" in key and "SD=" not in key, key
    if build_cpu.cpu_ok():
        port = build_cpu.CpuPort()
        port.load_edm(eargs, esd)
        port.load_predictor(pargs, psd)
        gamma = O.gamma_table("polynomial_2", D.T_STEPS, 1e-5)
        coef = O.step_coefficients(gamma, D.S_IDX, D.S_IDX + 1)
        t_val = np.float32(np.float32(D.S_IDX + 1) / np.float32(D.T_STEPS))
        want = port.step(coef, t_val, z, nm, em, eps, target_w=D.W_TARGET, scale=D.SCALE)
        port.close()
    else:
        gamma = O.gamma_table("polynomial_2", D.T_STEPS, 1e-5)
        want = O.step_guided(esd, eargs, psd, pargs, gamma, D.S_IDX, z, nm[:, :, None], em, eps, D.W_TARGET, D.SCALE)
    err = D._per_molecule(got, want)
    print(f"eight tiles: guided {err.max():.2e} [{key}]")
    assert err.max() < 1e-4, (int(err.argmax()), float(err.max()))
    assert np.all(got[nm == 0] == 0)


def test_guided_chain_in_launches_of_two_steps_repeats_bit_for_bit(monkeypatch):
    """A 4-step guided chain, two steps per launch, run twice and once more without the side job: the side wave's rows are written
    during a layer's edge phase and read behind its closing barrier, the kept copy of h it reads is rewritten a layer later -- a
    race there would show as runs that differ.  (No two of these molecules share a workgroup of 11 node slots.)"""
    from gaudi_amd import synth
    from gaudi_amd.engine import Engine
    from oracle import gaudi_oracle as O
    F = synth.num_node_features("cata")
    eargs, pargs = synth.edm_args(dataset="cata", diffusion_steps=4), synth.pred_args(dataset="cata")
    esd = synth.synth_edm_state_dict(eargs, F, seed=21, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=22, amplify_coord=True)
    nm, em = O.build_masks([11, 10, 11, 9], 11, False)
    nm = np.asarray(nm, np.float32).reshape(4, 11)
    em = np.asarray(em, np.float32).reshape(4, 11, 11)

    def chain(runs, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        eng = Engine(0)
        for k in env:
            monkeypatch.delenv(k)
        eng.load_edm(eargs, esd)
        eng.load_predictor(pargs, psd)
        eng.set_steps_per_launch(2)
        out = [eng.sample(nm, em, seed=5, sample_offset=2, target_w=D.W_TARGET, scale=D.SCALE, return_z0=True) for _ in range(runs)]
        key = eng.last_kernel_key()
        eng.close()
        return out, key

    (a, b), key = chain(2)
    assert N.N1 in key and key.endswith(SIDE), key
    (c,), key0 = chain(1, GAUDI_NO_SIDE=1)
    assert N.N1 in key0 and "SD=" not in key0, key0
    assert np.isfinite(a[0]).all()
    n_arrays = 0
    for u, v, w in zip(a, b, c):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v) and np.array_equal(u, w)
            n_arrays += 1
    assert n_arrays >= 2


@pytest.mark.parametrize("name", ["pred200_n11", "tiny_n11"])
def test_kernels_without_the_job_keep_theirs(name, monkeypatch):
    """No flag, results unchanged: the bits of a GAUDI_NO_SIDE=1 handle, and the port's to 1e-4."""
    assert D.CASES["tiny_n11"][:2] == (TINY, TINY_P)
    eng = N._engine(name)
    (g, kg), (u, ku) = N._steps(eng, name)
    eng.close()
    print(f"{name}: guided [{kg}] unguided [{ku}]")
    assert "N1=0" in kg and "SD=" not in kg and "SD=" not in ku, (kg, ku)
    N._check_vs_port(name, g, u)
    eng = N._engine(name, monkeypatch, GAUDI_NO_SIDE=1)
    (g0, kg0), (u0, ku0) = N._steps(eng, name)
    eng.close()
    assert kg0 == kg and ku0 == ku
    assert np.array_equal(g0, g) and np.array_equal(u0, u)
