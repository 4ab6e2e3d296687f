"""Tile-slot classes of the N1 kernels (w8_nodes_f16.h): at 12 and 13 output tiles -- the default widths, EDM 192 and predictor
196 -> 208 -- waves 4-7 / 5-7 own one tile of their two slots and run the phases in a body that issues nothing for the other.
No floating-point operation or its order changes, so the N1 kernels must still give the plain kernels' bits (GAUDI_NO_N1=1), stay
within the parity gate's 1e-4 per molecule of the numpy oracle -- a slot or tile mix-up moves whole blocks of 16 output features --
and repeat themselves bit for bit (the weight stream's waits are what the classes touch).

One batch of four fully connected cata molecules, N in {2, 7, 11, 16}: 16 is a full column tile, 2 a nearly empty one.  A guided
launch of 12 or more nodes goes to the kernels with several rounds of edge tiles, so the guided cases use N in {2, 7, 11}."""
import numpy as np
import pytest

from gaudi_amd import synth

pytestmark = pytest.mark.gpu

N1 = "MR=0 GN=0 FR=0 PG=0 N1=1"
PLAIN = "MR=0 GN=0 FR=0 PG=0 N1=0"
W_TARGET = np.array([0.5, -1.0, 0.25, 0.0, 1.0], np.float32)
SCALE = 0.6
T_CHAIN = 4          # diffusion steps of the chain tests, in launches of two
T_STEP = 1000        # ... of the teacher-forced steps (s = T / 2)
S_IDX = T_STEP // 2
SIZES_U = [2, 7, 11, 16]
SIZES_G = [2, 7, 11]


def _nets(T):
    F = synth.num_node_features("cata")
    eargs, pargs = synth.edm_args(dataset="cata", diffusion_steps=T), synth.pred_args(dataset="cata")
    esd = synth.synth_edm_state_dict(eargs, F, seed=21, amplify_coord=True)
    psd = synth.synth_predictor_state_dict(pargs, F, 5, seed=22, amplify_coord=True)
    return F, eargs, esd, pargs, psd


def _masks(sizes):
    from oracle import gaudi_oracle as O
    B, N = len(sizes), max(sizes)
    nm, em = O.build_masks(sizes, N, False)
    return np.asarray(nm, np.float32).reshape(B, N), np.asarray(em, np.float32).reshape(B, N, N)


def _engine(T, monkeypatch=None, **env):
    from gaudi_amd.engine import Engine
    _, eargs, esd, pargs, psd = _nets(T)
    for k, v in env.items():  # (read once, when the handle is created)
        monkeypatch.setenv(k, str(v))
    eng = Engine(0)
    for k in env:
        monkeypatch.delenv(k)
    eng.load_edm(eargs, esd)
    eng.load_predictor(pargs, psd)
    return eng


def _chain(eng, sizes, guided):
    nm, em = _masks(sizes)
    eng.set_steps_per_launch(2)
    kw = dict(target_w=W_TARGET, scale=SCALE) if guided else {}
    out = eng.sample(nm, em, seed=5, sample_offset=2, return_z0=True, **kw)
    return out, eng.last_kernel_key()


def _same_arrays(a, b):
    n = 0
    for u, v in zip(a, b):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v)
            n += 1
    assert n >= 2


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
def test_chain_through_the_n1_kernels_gives_the_plain_kernels_bits(guided, monkeypatch):
    sizes = SIZES_G if guided else SIZES_U
    eng = _engine(T_CHAIN)
    lean, key1 = _chain(eng, sizes, guided)
    eng.close()
    eng = _engine(T_CHAIN, monkeypatch, GAUDI_NO_N1=1)
    plain, key0 = _chain(eng, sizes, guided)
    eng.close()
    print(f"lean [{key1}] plain [{key0}]")
    assert N1 in key1 and "HPE=192" in key1 and ("HPP=208" in key1) == guided, key1
    assert PLAIN in key0, key0
    assert np.isfinite(lean[0]).all()
    _same_arrays(lean, plain)


def test_guided_chain_repeats_bit_for_bit():
    eng = _engine(T_CHAIN)
    runs = [_chain(eng, SIZES_G, True) for _ in range(2)]
    eng.close()
    assert N1 in runs[0][1] and N1 in runs[1][1]
    assert np.isfinite(runs[0][0][0]).all()
    _same_arrays(runs[0][0], runs[1][0])


def _per_molecule(got, want):
    B = want.shape[0]
    return np.abs(got - want).reshape(B, -1).max(1) / np.abs(want).reshape(B, -1).max(1)


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
def test_teacher_forced_step_vs_numpy_oracle(guided):
    from oracle import gaudi_oracle as O
    sizes = SIZES_G if guided else SIZES_U
    F, eargs, esd, pargs, psd = _nets(T_STEP)
    nm, em = _masks(sizes)
    B, N = nm.shape
    rng = np.random.default_rng(31)
    z = O._combined_noise(rng.standard_normal((B, N, 3 + F)).astype(np.float32), nm[:, :, None])
    eps = rng.standard_normal((B, N, 3 + F)).astype(np.float32)
    gamma = O.gamma_table("polynomial_2", T_STEP, 1e-5)
    if guided:
        want = O.step_guided(esd, eargs, psd, pargs, gamma, S_IDX, z, nm[:, :, None], em, eps, W_TARGET, SCALE)
    else:
        want = O.step_unguided(esd, eargs, gamma, S_IDX, z, nm[:, :, None], em, eps)
    eng = _engine(T_STEP)
    got = eng.step(S_IDX, z, nm, em, eps, **(dict(target_w=W_TARGET, scale=SCALE) if guided else {}))
    key = eng.last_kernel_key()
    eng.close()
    err = _per_molecule(got, want)
    print(f"{'guided' if guided else 'unguided'} [{key}]: max|HIP - oracle| / max|oracle| per molecule {err}")
    assert N1 in key, key
    assert err.max() < 1e-4, (int(err.argmax()), float(err.max()))
    assert np.all(got[nm == 0] == 0)
