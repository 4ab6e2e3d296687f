"""PPP-CIS excited states on the device (csrc/ppp_cis.inc): gaudi_ppp_cis against the kernels' host build, bit for bit in all
twenty-eight outputs -- golden g30 in one call, the tier-edge set in one mixed call and each molecule alone, the batch sizes around
a workgroup, windows 1, 3 and 8, both repulsion formulas, a charge vector, every refusal, the small shapes -- the two profile logs,
and the layers on top through a real Engine.  What the outputs must satisfy is checked on the host build by
tests/test_ppp_cis_cpu.py; equality with it carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests import ppp_helpers as P
from tests.gor2goa_helpers import unpack
from tests.ppp_cis_helpers import (ALL_ARRAYS, CIS_BITS, assert_no_cis_rows, assert_same_bits, device, edge_host, g30_host, host, refusals,
                                   small_shapes)

pytestmark = pytest.mark.gpu
OK, BAD_TABLE = P.OK, P.BAD_TABLE


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def _row(out, i, n_atoms, n_bonds):
    """Molecule i's twenty-eight outputs trimmed to its own sizes: what must not depend on the batch it ran in."""
    r = {k: out[k][i].copy() for k in ALL_ARRAYS}
    r["pi_charge"], r["site_class"], r["pi_bond_order"] = r["pi_charge"][:n_atoms], r["site_class"][:n_atoms], r["pi_bond_order"][:n_bonds]
    return r


def _assert_rows_equal(a, b):
    for k in ALL_ARRAYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_g30_equals_the_host_build(engine):
    mols = P.g30_molecules()
    dev = device(engine, mols)
    assert_same_bits(dev, g30_host())
    assert (dev["status"] == OK).sum() == 155 and (dev["n_states"] > 0).sum() == 155


def test_g30_under_a_charge_vector(engine):
    mols = P.g30_molecules()[::2]
    charged = (np.arange(len(mols), dtype=np.int32) % 3 - 1) * 2
    dev = device(engine, mols, charged)
    assert_same_bits(dev, host(mols, charged))
    assert (dev["n_states"] > 0).sum() >= 60


@pytest.mark.parametrize("k", range(len(P.EDGE_SIZES)), ids=[str(n) for n in P.EDGE_SIZES])
def test_a_tier_edge_molecule_alone(engine, k):
    mols, charge = P.edge_set()
    m = mols[k]
    dev = device(engine, [m], charge[k:k + 1])
    _assert_rows_equal(_row(dev, 0, len(m[0]), len(m[1])), _row(edge_host(), k, len(m[0]), len(m[1])))
    assert dev["n_pi"][0] == P.EDGE_SIZES[k] and dev["status"][0] == OK and dev["n_states"][0] == edge_host()["n_states"][k]


def test_the_tier_edge_set_in_one_mixed_call(engine):
    mols, charge = P.edge_set()
    dev = device(engine, mols, charge)  # three tiers, one CIS launch: the tier, the batch and the place leave no trace
    assert_same_bits(dev, edge_host())
    assert dev["n_pi"].tolist() == list(P.EDGE_SIZES) and (dev["status"] == OK).all()


@pytest.mark.parametrize("B", [1, 2, 3, 129])
def test_batch_sizes(engine, B):
    ref = g30_host()
    good = sorted((i for i in range(len(ref["status"])) if ref["status"][i] == OK), key=lambda i: -ref["n_pi"][i])[:B]
    mols = [P.g30_molecules()[i] for i in good]
    dev = device(engine, mols)
    for j, i in enumerate(good):  # (the host rows of the whole of g30: a molecule's result does not depend on its batch)
        m = mols[j]
        _assert_rows_equal(_row(dev, j, len(m[0]), len(m[1])), _row(ref, i, len(m[0]), len(m[1])))
    assert (dev["status"] == OK).all() and dev["n_states"].min() > 0


@pytest.mark.parametrize("window, repulsion", [(1, 0), (3, 0), (8, 1), (3, 1)])
def test_windows_and_both_formulas(engine, window, repulsion):
    mols = P.g30_molecules()[::4] + [P.phenacene(15, 1), P.benzene()]
    charge = np.array([0] * (len(mols) - 2) + [1, 0], np.int32)
    dev, ref = device(engine, mols, charge, repulsion, window=window), host(mols, charge, repulsion, window=window)
    assert_same_bits(dev, ref)
    assert (dev["status"] == OK).sum() >= 30 and dev["n_pi"][-2] == 63 and dev["n_states"][-2] == window * window
    assert dev["n_active_occ"].max() == min(window, 8)


def test_refusals_and_settings_that_cannot_be_used(engine):
    mols, charge, status = refusals()
    dev = device(engine, mols, charge)
    assert_same_bits(dev, host(mols, charge))
    assert dev["status"].tolist() == status
    for i, st in enumerate(status):
        if st != OK:
            assert_no_cis_rows(dev, i)
    two = [P.benzene(), P.naphthalene()]
    for kw in ({"parameters": {"classes": {"C": {"gamma": 0.0}}}}, {"damping": 1.0}, {"repulsion": 2}, {"window": 0}, {"window": 9}):
        out = device(engine, two, **kw)
        assert out["status"].tolist() == [BAD_TABLE, BAD_TABLE] and not out["levels"].any() and not out["singlet"].any(), kw
        assert_same_bits(out, host(two, **kw))
    t = P.c_tables()
    t.n_elems = 9
    with pytest.raises(_lib.GaudiError):
        engine.ppp_cis(t, *P.pack(two))
    assert_same_bits(device(engine, two), host(two))  # (the engine goes on working)


def test_the_small_shapes(engine):
    shapes = small_shapes()
    for window in sorted({w for _, _, w in shapes.values()}):
        names = [k for k, v in shapes.items() if v[2] == window]
        mols, charge = [shapes[k][0] for k in names], [shapes[k][1] for k in names]
        dev = device(engine, mols, charge, window=window)
        assert_same_bits(dev, host(mols, charge, window=window))
        assert (dev["status"] == OK).all()
    d0 = device(engine, [P.chain_molecule(2)] * 2, [2, -2])
    assert d0["n_states"].tolist() == [0, 0] and d0["status"].tolist() == [OK, OK] and not d0["singlet"].any()


def test_the_profile_logs(engine):
    mixed = [P.benzene(), P.phenacene(10), P.phenacene(7), P.phenacene(17)]  # three tiers: 6, 42, 30 and 70 centres
    engine.profile_reset(True)
    assert engine.ppp_cis_profile_get() == (0, 0.0) and engine.ppp_profile_get() == (0, 0.0)
    P.device(engine, mixed)
    scf = engine.ppp_profile_get()[0]
    assert scf == 3 and engine.ppp_cis_profile_get()[0] == 0
    engine.profile_reset(True)
    device(engine, mixed)
    assert engine.ppp_profile_get()[0] == scf  # the SCF launches are logged where gaudi_ppp's are
    n, ms = engine.ppp_cis_profile_get()
    assert n == 1 and ms > 0.0  # ... and the CIS launch in its own log
    device(engine, [P.benzene()], window=0)  # refused on the host: nothing launched
    assert engine.ppp_profile_get()[0] == scf and engine.ppp_cis_profile_get()[0] == 1
    engine.profile_reset(False)
    device(engine, [P.benzene()])
    assert engine.ppp_cis_profile_get()[0] == 0 and engine.ppp_profile_get()[0] == 0


def test_the_layers_through_an_engine(golden, engine):
    from gaudi_amd import ppp
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    ref = g30_host()
    pick = [i for i in range(len(ref["status"])) if ref["status"][i] == OK][::25]
    mols = [P.g30_molecules()[i] for i in pick]
    states, opt = ppp.excited_states(mols, "hetro", engine=engine), ppp.optical(mols, "hetro", engine=engine)
    for s, i, j in zip(states, pick, range(len(pick))):
        k = ref["n_states"][i]
        assert s["status"] == OK and s["singlet"].tobytes() == ref["singlet"][i, :k].tobytes() and s["osc"].tobytes() == ref["osc"][i, :k].tobytes()
        assert s["t1"] == float(ref["triplet"][i, 0]) == opt["t1"][j] and s["s1"] == opt["s1"][j] and s["flags"] == ref["flags"][i]
        lit = np.flatnonzero(ref["osc"][i, :k] >= np.float32(0.01))
        assert (np.isnan(opt["bright"][j]) and not len(lit)) or opt["bright"][j] == float(ref["singlet"][i, lit[0]])
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "hetro"][:40]
    rings = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    engine.profile_reset(True)
    ppp_recs = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine, ppp=True)
    scf_alone = engine.ppp_profile_get()[0]
    assert engine.ppp_cis_profile_get()[0] == 0
    engine.profile_reset(True)
    both = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine, ppp=True, ppp_cis=True)
    assert engine.ppp_profile_get()[0] <= scf_alone and engine.ppp_cis_profile_get()[0] == 1  # one call serves both
    engine.profile_reset(True)
    recs = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine, ppp_cis=True)
    assert engine.ppp_profile_get()[0] == scf_alone and engine.ppp_cis_profile_get()[0] == 1
    engine.profile_reset(False)
    plain_recs = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine)
    added = {"ppp_s1", "ppp_t1", "ppp_s1_f", "ppp_bright", "ppp_cis_flags"}
    raw = ppp.excited_states(plain_recs, "hetro", engine=engine)
    for r, p, q, b, o in zip(recs, plain_recs, ppp_recs, both, raw):
        assert set(r) == set(p) | added and all(np.array_equal(r[k], p[k]) for k in p)
        assert set(b) == set(q) | added and all(np.array_equal(b[k], q[k]) for k in q)
        assert all(np.array_equal(b[k], r[k], equal_nan=True) for k in added)
        assert np.array_equal([r["ppp_s1"], r["ppp_t1"], r["ppp_s1_f"]], [o["s1"], o["t1"], o["s1_f"]], equal_nan=True)
        assert r["ppp_cis_flags"] == o["flags"] & CIS_BITS and np.isnan(r["ppp_s1"]) == (o["status"] != OK)
    assert sum(0.5 < r["ppp_s1"] < 10.0 and r["ppp_t1"] < r["ppp_s1"] for r in recs) >= 20
    plain, _ = analyze_atoms_for_molecules(rings, 0.1, "hetro", engine=engine)
    d, _ = analyze_atoms_for_molecules(rings, 0.1, "hetro", engine=engine, ppp_cis=True)
    assert set(d) == set(plain) | {"ppp_s1", "ppp_t1", "ppp_bright", "ppp_triplet_unstable_fraction"}
    assert all(np.array_equal(d[k], plain[k]) for k in plain)
    bare = [r for r in rings_to_atoms(rings, "hetro", 0.1, engine=engine, ppp_cis=True) if r["status"] == 0]
    assert np.array_equal(d["ppp_s1"], [r["ppp_s1"] for r in bare], equal_nan=True)
    assert d["ppp_triplet_unstable_fraction"] == sum(bool(r["ppp_cis_flags"] & 128) for r in bare) / len(bare)


def test_design_with_ppp_cis():
    import types

    import torch  # noqa: F401
    from gaudi_amd import generation_guidance, ppp, synth
    from gaudi_amd.models_edm import get_cond_predictor_model, get_model
    from tests.helpers import TINY, TINY_P
    eargs = synth.edm_args(dataset="cata", diffusion_steps=40, **TINY)
    pargs = synth.pred_args(dataset="cata", **TINY_P)
    model, _, _ = get_model(eargs, state_dict=synth.synth_edm_state_dict(eargs, 1, seed=3))
    cp = get_cond_predictor_model(pargs, model=model, state_dict=synth.synth_predictor_state_dict(pargs, 1, 5, seed=4))
    model.seed = 5
    args = types.SimpleNamespace(device="cuda", dataset="cata", max_nodes=9, batch_size=6)

    def tf_gap(z, nm, em, t):
        return -cp(z, nm, em, t)[:, 1]

    plain = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True)
    model.sample_offset = 0
    model.engine.profile_reset(True)
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, ppp=True, ppp_cis=True)
    assert model.engine.ppp_cis_profile_get()[0] == 1 and model.engine.ppp_profile_get()[0] <= 3
    model.engine.profile_reset(False)
    assert set(out) == set(plain) | {"ppp_gap", "ppp_ip", "ppp_ea", "ppp_s1", "ppp_t1", "ppp_bright"}
    for k in ("fingerprints", "mol_unique", "best", "target_function_values"):
        assert np.array_equal(out[k], plain[k]), k
    want, front = ppp.optical(out["atoms"], "cata", engine=model.engine), ppp.frontier(out["atoms"], "cata", engine=model.engine)
    for k in ("s1", "t1", "bright"):
        assert out["ppp_" + k].shape == (6,) and out["ppp_" + k].dtype == np.float64
        assert np.array_equal(out["ppp_" + k], want[k], equal_nan=True)
    for k in ("gap", "ip", "ea"):
        assert np.array_equal(out["ppp_" + k], front[k], equal_nan=True)
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, ppp_cis=True)
    model.engine.close()
