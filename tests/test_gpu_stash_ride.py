"""The stash rides of the resident N1 fused kernel's reverse pass: the activation-stash rows a phase reads first are requested
behind the last weight request of the GEMM ahead of it (w8_split.h: RideAt, w8_nodes_f16.h: hook) and one trip barrier leaves
exactly those loads in flight.  No floating-point operation or its order changes: the kernel must give the bits of the plain
kernel (GAUDI_NO_N1=1), which has no ride, and stay within 1e-4 per molecule of the C++ restatement (the seeds and bar of
tests/test_gpu_diet.py, whose references are shared).  A wave without an edge tile must wait for ALL its ring units at the counted
barrier (N = 2: seven such waves); a ride that crossed a barrier it should not cross shows as runs that differ."""
import numpy as np
import pytest

from tests import test_gpu_diet as D
from tests import test_gpu_n1 as N

pytestmark = pytest.mark.gpu

# name -> (EDM overrides, predictor overrides, live nodes per molecule): 1, 3 and 7 edge tiles, and workgroups of 7, 5 and 3 tiles
# in one launch
D.CASES.setdefault("ride_n2", ({}, {}, [2, 2]))
D.CASES.setdefault("ride_n7", ({}, {}, [7, 7]))
D.CASES.setdefault("ride_n11", ({}, {}, [11, 11]))
D.CASES.setdefault("ride_mixed", ({}, {}, [11, 9, 7]))
TILES = {"ride_n2": [1, 1], "ride_n7": [3, 3], "ride_n11": [7, 7], "ride_mixed": [7, 5, 3]}


@pytest.mark.parametrize("name", list(TILES))
def test_guided_step_gives_the_plain_kernels_bits(name, monkeypatch):
    eng = N._engine(name)
    nm, em = D._setup(name)[4:6]
    assert list(eng.pack_plan(nm, em)[2]) == TILES[name]
    (g1, kg1), (u1, ku1) = N._steps(eng, name)
    eng.close()
    print(f"{name}: guided [{kg1}] unguided [{ku1}]")
    assert N.N1 in kg1 and "HPE=192 HPP=208" in kg1, kg1
    N._check_vs_port(name, g1, u1)
    eng = N._engine(name, monkeypatch, GAUDI_NO_N1=1)
    (g0, kg0), (u0, ku0) = N._steps(eng, name)
    eng.close()
    assert N.PLAIN in kg0 and "HPE=192 HPP=208" in kg0, kg0
    assert np.array_equal(g0, g1) and np.array_equal(u0, u1)


def test_eight_tiles_every_wave_rides(monkeypatch):
    """12 nodes with six node pairs masked out (tests/test_gpu_side.py): 120 live edge slots = 8 tiles, no wave without one."""
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
        for i in range(6):
            em[b, i, n - 1 - i] = em[b, n - 1 - i, i] = 0.0
    rng = np.random.default_rng(33)
    z = O._combined_noise(rng.standard_normal((3, n, 3 + F)).astype(np.float32), nm[:, :, None])
    eps = rng.standard_normal((3, n, 3 + F)).astype(np.float32)

    def step(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        eng = Engine(0)
        for k in env:
            monkeypatch.delenv(k)
        eng.load_edm(eargs, esd)
        eng.load_predictor(pargs, psd)
        assert sorted(eng.pack_plan(nm, em)[2]) == [7, 8, 8]
        got = eng.step(D.S_IDX, z, nm, em, eps, target_w=D.W_TARGET, scale=D.SCALE)
        key = eng.last_kernel_key()
        eng.close()
        return got, key

    got, key = step()
    plain, key0 = step(GAUDI_NO_N1=1)
    assert N.N1 in key and N.PLAIN in key0, (key, key0)
    assert np.array_equal(got, plain)
    gamma = O.gamma_table("polynomial_2", D.T_STEPS, 1e-5)
    if build_cpu.cpu_ok():
        port = build_cpu.CpuPort()
        port.load_edm(eargs, esd)
        port.load_predictor(pargs, psd)
        coef = O.step_coefficients(gamma, D.S_IDX, D.S_IDX + 1)
        t_val = np.float32(np.float32(D.S_IDX + 1) / np.float32(D.T_STEPS))
        want = port.step(coef, t_val, z, nm, em, eps, target_w=D.W_TARGET, scale=D.SCALE)
        port.close()
    else:
        want = O.step_guided(esd, eargs, psd, pargs, gamma, D.S_IDX, z, nm[:, :, None], em, eps, D.W_TARGET, D.SCALE)
    err = D._per_molecule(got, want)
    print(f"eight tiles: guided {err.max():.2e} [{key}]")
    assert err.max() < 1e-4, (int(err.argmax()), float(err.max()))
    assert np.all(got[nm == 0] == 0)


def test_guided_chain_in_launches_of_two_steps_repeats_bit_for_bit(monkeypatch):
    """A 4-step guided chain, two steps per launch, run twice and once on the plain kernel: all arrays bit-equal."""
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


def test_nothing_rides_where_nothing_should(monkeypatch):
    """An unguided step (no predictor) and a pred200_n11 step (four tail k-steps: the plain kernel) keep their keys -- the ride adds
    no flag -- and their bits."""
    eng = N._engine("pred200_n11")
    (g, kg), (u, ku) = N._steps(eng, "pred200_n11")
    eng.close()
    print(f"pred200_n11: guided [{kg}] unguided [{ku}]")
    assert "N1=0" in kg and "HPP=0" in ku, (kg, ku)
    assert "SD=" not in kg and "RIDE" not in kg.upper() and "RIDE" not in ku.upper(), (kg, ku)
    N._check_vs_port("pred200_n11", g, u)
    eng = N._engine("pred200_n11", monkeypatch, GAUDI_NO_N1=1)
    (g0, kg0), (u0, ku0) = N._steps(eng, "pred200_n11")
    eng.close()
    assert kg0 == kg
    assert np.array_equal(g0, g) and np.array_equal(u0, u)
