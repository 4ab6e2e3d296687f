"""PPP levels on the device (csrc/ppp.inc): gaudi_ppp against the kernel's host build, bit for bit in all eighteen outputs -- golden
g30 in one call, the tier-edge set in one mixed call and each molecule alone, the batch sizes around a workgroup, both repulsion
formulas, damping 0 and 0.25, a charge vector, every refusal -- and the layers on top through a real Engine.  What the outputs must
satisfy is checked on the host build by tests/test_ppp_cpu.py; equality with it carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import H
from tests.gor2goa_helpers import unpack
from tests.ppp_helpers import (BAD_GEOMETRY, BAD_INPUT, BAD_TABLE, EDGE_SIZES, EMPTY, NOT_CONVERGED, OK, OPEN_SHELL, OVERFLOW,
                               assert_rows_equal, assert_same_bits, benzene, c_tables, chain_molecule, device, edge_host_one, edge_set,
                               g30_host, g30_molecules, host, naphthalene, pack, phenacene, row)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def test_g30_equals_the_host_build(engine):
    mols = g30_molecules()
    dev = device(engine, mols)
    assert_same_bits(dev, g30_host())
    st = np.bincount(dev["status"], minlength=9)
    assert st[OK] >= 150 and st[NOT_CONVERGED] >= 1 and st[OPEN_SHELL] >= 1 and st[BAD_GEOMETRY] >= 1
    charged = (np.arange(len(mols), dtype=np.int32) % 3 - 1) * 2
    assert_same_bits(device(engine, mols, charged), host(mols, charged))


@pytest.mark.parametrize("k", range(len(EDGE_SIZES)), ids=[str(n) for n in EDGE_SIZES])
def test_a_tier_edge_molecule_alone(engine, k):
    mols, charge = edge_set()
    dev = device(engine, [mols[k]], charge[k:k + 1])
    assert_same_bits(dev, edge_host_one(k))
    assert dev["n_pi"][0] == EDGE_SIZES[k] and dev["status"][0] == OK


def test_the_tier_edge_set_in_one_mixed_call(engine):
    mols, charge = edge_set()
    dev = device(engine, mols, charge)  # three tiers in one call: the tier, the batch and the place leave no trace
    assert dev["n_pi"].tolist() == list(EDGE_SIZES) and (dev["status"] == OK).all()
    for k, m in enumerate(mols):
        assert_rows_equal(row(dev, k, len(m[0]), len(m[1])), row(edge_host_one(k), 0, len(m[0]), len(m[1])))


@pytest.mark.parametrize("B", [1, 2, 3, 129])
def test_batch_sizes(engine, B):
    ref = g30_host()
    good = sorted((i for i in range(len(ref["status"])) if ref["status"][i] == OK), key=lambda i: -ref["n_pi"][i])[:B]
    mols = [g30_molecules()[i] for i in good]
    dev = device(engine, mols)
    assert_same_bits(dev, host(mols))
    assert (dev["status"] == OK).all() and dev["n_pi"].min() > 0


@pytest.mark.parametrize("repulsion, damping", [(0, 0.0), (1, 0.25), (1, 0.0)])
def test_the_other_formula_and_no_damping(engine, repulsion, damping):
    mols = g30_molecules()[::4] + [phenacene(15, 1)]
    charge = np.array([0] * (len(mols) - 1) + [1], np.int32)
    dev, ref = device(engine, mols, charge, repulsion, damping), host(mols, charge, repulsion, damping)
    assert_same_bits(dev, ref)
    assert (dev["status"] == OK).sum() >= 30 and dev["status"][-1] == OK and dev["n_pi"][-1] == 63


def test_refusals_and_a_table_that_cannot_be_used(engine):
    e, b, x = benzene()
    he, hb, hx = chain_molecule(2)
    mols = [chain_molecule(3), (e, b, np.where(np.arange(6)[:, None] == 1, x[0] + [0.3, 0.0, 0.0], x)),
            (e, b, np.where(np.arange(6)[:, None] == 4, np.nan, x)), phenacene(32),
            (np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 3))), (he, hb, np.where((he == H)[:, None], 0.0, hx)),
            chain_molecule(3)]
    charge = [0, 0, 0, 0, 0, 0, 5]
    dev = device(engine, mols, charge)
    assert_same_bits(dev, host(mols, charge))
    assert dev["status"].tolist() == [OPEN_SHELL, BAD_GEOMETRY, BAD_GEOMETRY, OVERFLOW, EMPTY, OK, BAD_INPUT]
    two = [benzene(), naphthalene()]
    for kw in ({"parameters": {"classes": {"C": {"gamma": 0.0}}}}, {"damping": 1.0}, {"repulsion": 2}):
        out = device(engine, two, **kw)
        assert out["status"].tolist() == [BAD_TABLE, BAD_TABLE] and not out["levels"].any(), kw
        assert_same_bits(out, host(two, **kw))
    t = c_tables()
    t.n_elems = 9
    with pytest.raises(_lib.GaudiError):
        engine.ppp(t, *pack(two))
    assert_same_bits(device(engine, two), host(two))  # (the engine goes on working)


def test_the_profile_counts_one_launch_per_tier(engine):
    engine.profile_reset(True)
    assert engine.ppp_profile_get() == (0, 0.0)
    device(engine, [benzene(), naphthalene()])
    assert engine.ppp_profile_get()[0] == 1
    device(engine, [benzene(), phenacene(10), phenacene(7), phenacene(9)])
    n, ms = engine.ppp_profile_get()
    assert n == 3 and ms > 0.0
    engine.profile_reset(False)
    device(engine, [benzene()])
    assert engine.ppp_profile_get()[0] == 0


def test_orbitals_gap_and_analyze_through_an_engine(golden, engine):
    from gaudi_amd import ppp
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    ref = g30_host()
    pick = [i for i in range(len(ref["status"])) if ref["status"][i] == OK][::25]
    mols = [g30_molecules()[i] for i in pick]
    orbs, gaps = ppp.orbitals(mols, "hetro", engine=engine), ppp.gap(mols, "hetro", engine=engine)
    for o, g, i, m in zip(orbs, gaps, pick, mols):
        n = ref["n_pi"][i]
        assert o["status"] == OK and o["levels"].tobytes() == ref["levels"][i, :n].tobytes() and g == float(ref["gap"][i]) == o["gap"]
        assert o["pi_charge"].tobytes() == ref["pi_charge"][i, :len(m[0])].tobytes() and o["ip"] == -float(ref["homo"][i])
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "hetro"][:40]
    rings = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    plain_recs = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine)
    engine.profile_reset(True)
    recs = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine, ppp=True)
    assert 1 <= engine.ppp_profile_get()[0] <= 3
    engine.profile_reset(False)
    added = {"ppp_gap", "ppp_homo", "ppp_lumo", "ppp_flags", "ppp_status"}
    raw = ppp.orbitals(plain_recs, "hetro", engine=engine)
    built = np.array([r["status"] == 0 for r in recs])
    assert built.sum() >= 30
    for r, p, o in zip(recs, plain_recs, raw):
        assert set(r) == set(p) | added and all(np.array_equal(r[k], p[k]) for k in p)
        assert (r["ppp_status"], r["ppp_gap"], r["ppp_homo"], r["ppp_lumo"], r["ppp_flags"]) == \
            (o["status"], o["gap"], o["homo"], o["lumo"], o["flags"])
        assert (r["ppp_status"] == EMPTY) == (r["status"] != 0)
    assert sum(r["ppp_status"] == OK and 0.5 < r["ppp_gap"] < 15.0 for r in recs) >= 20
    plain, _ = analyze_atoms_for_molecules(rings, 0.1, "hetro", engine=engine)
    engine.profile_reset(True)
    d, _ = analyze_atoms_for_molecules(rings, 0.1, "hetro", engine=engine, ppp=True)
    assert 1 <= engine.ppp_profile_get()[0] <= 3
    engine.profile_reset(False)
    assert set(d) == set(plain) | {"ppp_gap", "ppp_not_converged_fraction"} and all(np.array_equal(d[k], plain[k]) for k in plain)
    bare = [r for r in rings_to_atoms(rings, "hetro", 0.1, engine=engine, ppp=True) if r["status"] == 0]
    assert np.array_equal(d["ppp_gap"], np.array([r["ppp_gap"] if r["ppp_status"] == 0 else np.nan for r in bare]), equal_nan=True)
    assert d["ppp_not_converged_fraction"] == sum(r["ppp_status"] == NOT_CONVERGED for r in bare) / built.sum()


def test_design_with_ppp():
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
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, ppp=True)
    assert set(out) == set(plain) | {"ppp_gap", "ppp_ip", "ppp_ea"}
    for k in ("fingerprints", "mol_unique", "best", "target_function_values"):
        assert np.array_equal(out[k], plain[k]), k
    want = ppp.frontier(out["atoms"], "cata", engine=model.engine)
    for k in ("gap", "ip", "ea"):
        assert out["ppp_" + k].shape == (6,) and out["ppp_" + k].dtype == np.float64
        assert np.array_equal(out["ppp_" + k], want[k], equal_nan=True)
    for rec, g in zip(out["atoms"], out["ppp_gap"]):
        assert np.isnan(g) == (rec["status"] != 0 or ppp.orbitals([rec], "cata", engine=model.engine)[0]["status"] != OK)
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, ppp=True)
    model.engine.close()
