"""The batched per-node sums of the resident N1 fused kernel (GAUDI_LDS_BATCH; w8_common.h: FoldBatch): the reverse pass's du -> dP /
dQ gather, its dx sum and the coordinate update fetch the rows of a run a batch at a time and fold them afterwards -- the same
additions on the same operands in the same order, a slot beyond the run skipped by a select.  The N1 kernel must therefore give
the bits of the plain kernel (GAUDI_NO_N1=1), whose sums read one row per iteration, and stay within 1e-4 per molecule of the
C++ restatement (the seeds and bar of tests/test_gpu_diet.py, whose references are shared).  Runs shorter than a batch (degree
1), of one partial batch (6), of the benchmark's length (10), with masked nodes and with masked node pairs on all eight tiles, and the
longest an N1 launch can hold (15, beside runs of 3 that cross tile borders)."""
import numpy as np
import pytest

from tests import test_gpu_diet as D
from tests import test_gpu_n1 as N

pytestmark = pytest.mark.gpu

# name -> (EDM overrides, predictor overrides, live nodes per molecule); the names (and so the cached references) of
# tests/test_gpu_stash_ride.py
D.CASES.setdefault("ride_n2", ({}, {}, [2, 2]))
D.CASES.setdefault("ride_n7", ({}, {}, [7, 7]))
D.CASES.setdefault("ride_n11", ({}, {}, [11, 11]))
D.CASES.setdefault("ride_mixed", ({}, {}, [11, 9, 7]))
TILES = {"ride_n2": [1, 1], "ride_n7": [3, 3], "ride_n11": [7, 7], "ride_mixed": [7, 5, 3]}


@pytest.mark.parametrize("name", list(TILES))
def test_guided_and_unguided_step_give_the_plain_kernels_bits(name, monkeypatch):
    eng = N._engine(name)
    nm, em = D._setup(name)[4:6]
    assert list(eng.pack_plan(nm, em)[2]) == TILES[name]
    (g1, kg1), (u1, ku1) = N._steps(eng, name)
    eng.close()
    print(f"{name}: guided [{kg1}] unguided [{ku1}]")
    assert N.N1 in kg1 and "HPE=192 HPP=208" in kg1, kg1
    assert N.N1 in ku1, ku1
    N._check_vs_port(name, g1, u1)
    eng = N._engine(name, monkeypatch, GAUDI_NO_N1=1)
    (g0, kg0), (u0, ku0) = N._steps(eng, name)
    eng.close()
    assert N.PLAIN in kg0 and "HPE=192 HPP=208" in kg0, kg0
    assert N.PLAIN in ku0, ku0
    assert np.array_equal(g0, g1) and np.array_equal(u0, u1)


def _masked_pairs():
    """12 nodes with six node pairs masked out in molecules 0 and 2 (the 8-tile case of tests/test_gpu_stash_ride.py): 120 live
    edge slots there, every node of degree 10; molecule 1 has 11 nodes of degree 10 and one masked."""
    from oracle import gaudi_oracle as O
    n = 12
    nm, em = O.build_masks([12, 11, 12], n, False)
    nm = np.asarray(nm, np.float32).reshape(3, n)
    em = np.array(em, np.float32).reshape(3, n, n)
    for b in (0, 2):
        for i in range(6):
            em[b, i, n - 1 - i] = em[b, n - 1 - i, i] = 0.0
    return nm, em, [7, 8, 8]


def _star_and_ring():
    """16 nodes, node 0 joined to all fifteen others, the others joined in a ring: 60 directed edges in 4 tiles, node 0's run of
    15 slots is the longest an N1 launch can hold, the runs of degree 3 behind it cross the tile borders."""
    n = 16
    nm = np.ones((2, n), np.float32)
    em = np.zeros((2, n, n), np.float32)
    for b in range(2):
        for i in range(1, n):
            k = i + 1 if i + 1 < n else 1
            em[b, 0, i] = em[b, i, 0] = 1.0
            em[b, i, k] = em[b, k, i] = 1.0
    assert int(em[0].sum()) == 60 and int(em[0, 0].sum()) == 15 and set(em[0, 1:].sum(1)) == {3.0}
    return nm, em, [4, 4]


@pytest.mark.parametrize("graph", [_masked_pairs, _star_and_ring])
def test_hand_built_graphs_give_the_plain_kernels_bits(graph, monkeypatch):
    from gaudi_amd import synth
    from gaudi_amd.engine import Engine
    from oracle import build_cpu
    from oracle import gaudi_oracle as O
    nm, em, tiles = graph()
    B, n = nm.shape
    F = synth.num_node_features("cata")
    eargs, pargs = synth.edm_args(dataset="cata", diffusion_steps=D.T_STEPS), synth.pred_args(dataset="cata")
    esd = synth.synth_edm_state_dict(eargs, F, seed=21, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=22, amplify_coord=True)
    rng = np.random.default_rng(33)
    z = O._combined_noise(rng.standard_normal((B, n, 3 + F)).astype(np.float32), nm[:, :, None])
    eps = rng.standard_normal((B, n, 3 + F)).astype(np.float32)

    def steps(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        eng = Engine(0)
        for k in env:
            monkeypatch.delenv(k)
        eng.load_edm(eargs, esd)
        eng.load_predictor(pargs, psd)
        assert sorted(eng.pack_plan(nm, em)[2]) == sorted(tiles)
        g = eng.step(D.S_IDX, z, nm, em, eps, target_w=D.W_TARGET, scale=D.SCALE)
        kg = eng.last_kernel_key()
        u = eng.step(D.S_IDX, z, nm, em, eps)
        ku = eng.last_kernel_key()
        eng.close()
        return g, kg, u, ku

    g1, kg1, u1, ku1 = steps()
    g0, kg0, u0, ku0 = steps(GAUDI_NO_N1=1)
    print(f"{graph.__name__}: guided [{kg1}] unguided [{ku1}]")
    assert N.N1 in kg1 and "HPE=192 HPP=208" in kg1 and N.N1 in ku1, (kg1, ku1)
    assert N.PLAIN in kg0 and "HPE=192 HPP=208" in kg0 and N.PLAIN in ku0, (kg0, ku0)
    assert np.array_equal(g0, g1) and np.array_equal(u0, u1)
    gamma = O.gamma_table("polynomial_2", D.T_STEPS, 1e-5)
    if build_cpu.cpu_ok():
        port = build_cpu.CpuPort()
        port.load_edm(eargs, esd)
        port.load_predictor(pargs, psd)
        coef = O.step_coefficients(gamma, D.S_IDX, D.S_IDX + 1)
        t_val = np.float32(np.float32(D.S_IDX + 1) / np.float32(D.T_STEPS))
        want_g = port.step(coef, t_val, z, nm, em, eps, target_w=D.W_TARGET, scale=D.SCALE)
        want_u = port.step(coef, t_val, z, nm, em, eps)
        port.close()
    else:
        want_g = O.step_guided(esd, eargs, psd, pargs, gamma, D.S_IDX, z, nm[:, :, None], em, eps, D.W_TARGET, D.SCALE)
        want_u = O.step_unguided(esd, eargs, gamma, D.S_IDX, z, nm[:, :, None], em, eps)
    err_g, err_u = D._per_molecule(g1, want_g), D._per_molecule(u1, want_u)
    print(f"{graph.__name__}: guided {err_g.max():.2e} unguided {err_u.max():.2e}")
    assert err_g.max() < 1e-4, (int(err_g.argmax()), float(err_g.max()))
    assert err_u.max() < 1e-4, (int(err_u.argmax()), float(err_u.max()))
    assert np.all(g1[nm == 0] == 0) and np.all(u1[nm == 0] == 0)


def test_guided_chain_in_launches_of_two_steps_repeats_bit_for_bit(monkeypatch):
    """A 4-step guided chain, two steps per launch, run twice on the N1 kernel and once on the plain kernel: all arrays bit-equal
    (a batch that read a row before the barrier ahead of it would show as runs that differ)."""
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
    assert N.N1 in key, key
    (c,), key0 = chain(1, GAUDI_NO_N1=1)
    assert N.PLAIN in key0, key0
    assert np.isfinite(a[0]).all()
    n_arrays = 0
    for u, v, w in zip(a, b, c):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v) and np.array_equal(u, w)
            n_arrays += 1
    assert n_arrays >= 2
