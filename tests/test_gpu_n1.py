"""The resident full-ring kernel's N1 instantiation (node GEMMs compiled for one column tile and one tail k-step: workgroups of at
most 16 node slots) and the edge aggregation's partial sums added inside the node MLP's split pass.  Neither changes a floating-
point operation or its order: the N1 kernel must run exactly where it may, give the plain kernel's bits there, and every kernel
must stay within 1e-4 per molecule of the C++ restatement (the cases, seeds and bar of tests/test_gpu_diet.py, whose references are
shared)."""
import numpy as np
import pytest

from tests import test_gpu_diet as D
from tests.helpers import TINY, TINY_P

pytestmark = pytest.mark.gpu

# the cases this file adds to the shared table (name -> EDM overrides, predictor overrides, live nodes per molecule): _setup and
# the cached references of _want are keyed by name
D.CASES.setdefault("default_n16", ({}, {}, [16, 12, 15]))          # 16: the last size of one column tile
D.CASES.setdefault("pred200_n11", ({}, dict(nf=200), [11, 7, 9]))  # padded to 208 like nf = 196, but four tail k-steps

N1, PLAIN, FR = "MR=0 GN=0 FR=0 PG=0 N1=1", "MR=0 GN=0 FR=0 PG=0 N1=0", "MR=0 GN=0 FR=1 PG=0 N1=0"
# A fully connected molecule of 12 or more nodes has more than 128 edge slots: the launches that run the predictor then take the
# kernel with several rounds of edge tiles, which has no N1 and no FR form -- at 16 and 17 nodes only the denoiser-only launch of
# the unguided step is on the resident single-round kernel.
ROUNDS = "MR=1 GN=0 FR=0 PG=0 N1=0"


def _engine(name, monkeypatch=None, **env):
    from gaudi_amd.engine import Engine
    eargs, esd, pargs, psd = D._setup(name)[:4]
    for k, v in env.items():  # (read once, when the handle is created)
        monkeypatch.setenv(k, str(v))
    eng = Engine(0)
    for k in env:
        monkeypatch.delenv(k)
    eng.load_edm(eargs, esd)
    eng.load_predictor(pargs, psd)
    return eng


def _steps(eng, name):
    """One teacher-forced guided and one unguided step -> ((z_s, kernel key), (z_s, kernel key))."""
    _, _, _, _, nm, em, z, eps = D._setup(name)
    got_g = eng.step(D.S_IDX, z, nm, em, eps, target_w=D.W_TARGET, scale=D.SCALE)
    key_g = eng.last_kernel_key()
    got_u = eng.step(D.S_IDX, z, nm, em, eps)
    key_u = eng.last_kernel_key()
    assert eng.kernel_variant()[1] == 8
    return (got_g, key_g), (got_u, key_u)


def _check_vs_port(name, got_g, got_u):
    want_g, want_u = D._want(name)
    nm = D._setup(name)[4]
    err_g, err_u = D._per_molecule(got_g, want_g), D._per_molecule(got_u, want_u)
    print(f"{name}: guided {err_g.max():.2e} unguided {err_u.max():.2e}")
    assert err_g.max() < 1e-4, (int(err_g.argmax()), float(err_g.max()))
    assert err_u.max() < 1e-4, (int(err_u.argmax()), float(err_u.max()))
    assert np.all(got_g[nm == 0] == 0) and np.all(got_u[nm == 0] == 0)


@pytest.mark.parametrize("name,guided_key", [("default_n11", N1), ("default_n16", ROUNDS), ("default_n3", N1)])
def test_n1_kernel_runs_where_it_should_and_gives_the_plain_kernels_bits(name, guided_key, monkeypatch):
    eng = _engine(name)
    (g1, kg1), (u1, ku1) = _steps(eng, name)
    eng.close()
    print(f"{name}: guided [{kg1}] unguided [{ku1}]")
    assert guided_key in kg1 and "HPE=192 HPP=208" in kg1, kg1
    assert N1 in ku1 and "HPE=192 HPP=0" in ku1, ku1
    _check_vs_port(name, g1, u1)
    eng = _engine(name, monkeypatch, GAUDI_NO_N1=1)
    (g0, kg0), (u0, ku0) = _steps(eng, name)
    eng.close()
    assert (PLAIN if guided_key == N1 else guided_key) in kg0 and "HPE=192 HPP=208" in kg0, kg0
    assert PLAIN in ku0 and "HPE=192 HPP=0" in ku0, ku0
    assert np.array_equal(g0, g1) and np.array_equal(u0, u1)


def test_more_than_16_node_slots_take_the_fr_kernel():
    eng = _engine("default_n17")
    (g, kg), (u, ku) = _steps(eng, "default_n17")
    eng.close()
    assert ROUNDS in kg and FR in ku, (kg, ku)
    _check_vs_port("default_n17", g, u)


def test_predictor_with_four_tail_steps_takes_the_plain_kernel():
    eng = _engine("pred200_n11")
    (g, kg), (u, ku) = _steps(eng, "pred200_n11")
    eng.close()
    assert PLAIN in kg and "HPP=208" in kg, kg  # (one plan per call family: the denoiser-only launch may or may not be N1)
    _check_vs_port("pred200_n11", g, u)


def test_value_target_step_takes_its_vt_kernel():
    name = "default_n11"
    eng = _engine(name)
    _, _, _, _, nm, em, z, eps = D._setup(name)
    got = eng.step_target(D.S_IDX, z, nm, em, eps, dict(w=D.W_TARGET, scale=D.SCALE))
    key = eng.last_kernel_key()
    eng.close()
    assert PLAIN in key and key.endswith("VT=1"), key
    err = D._per_molecule(got, D._want(name)[0])  # (zero curvature, shared arrays: the affine target)
    print(f"{name} value target: {err.max():.2e}")
    assert err.max() < 1e-4, (int(err.argmax()), float(err.max()))


# ---- the partial sums inside the split pass reach kernels that N1 does not
@pytest.mark.parametrize("name", ["default_n22", "tiny_n11"])
def test_summed_sources_on_the_other_resident_kernels(name):
    assert D.CASES["tiny_n11"][:2] == (TINY, TINY_P)
    eng = _engine(name)
    (g, kg), (u, ku) = _steps(eng, name)
    eng.close()
    print(f"{name}: guided [{kg}] unguided [{ku}]")
    assert "N1=0" in kg and "N1=0" in ku
    _check_vs_port(name, g, u)


def test_guided_chain_in_launches_of_two_steps_repeats_bit_for_bit():
    """A 4-step guided chain of 4 molecules, two steps per launch, run twice: the split pass reads the two partial sums behind the
    edge phase's closing barrier alone (the pass that added them, and its barrier, are gone), and the next layer zeroes them behind
    two more -- a race there would show as runs that differ."""
    from gaudi_amd import synth
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
    runs = [eng.sample(nm, em, seed=5, sample_offset=2, target_w=D.W_TARGET, scale=D.SCALE, return_z0=True) for _ in range(2)]
    assert N1 in eng.last_kernel_key()
    eng.close()
    assert np.isfinite(runs[0][0]).all()
    n_arrays = 0
    for u, v in zip(*runs):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u, v)
            n_arrays += 1
    assert n_arrays >= 2
