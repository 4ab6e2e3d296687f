"""PPP for open shells on the device (csrc/ppp_open.inc): gaudi_ppp_open against the kernel's host build, bit for bit in all
twenty-three outputs, the doubles included -- golden g30 under the four state kinds in ONE mixed call, the tier edges as cations in
one call and each alone, the 126- to 128-centre rows against the host build's record, one centre and triplet ethylene, the batch
sizes around a workgroup, every refusal, one launch per tier -- and the keyword ppp_dscf through a real Engine.  What the outputs
must satisfy is checked on the host build by tests/test_ppp_open_cpu.py; equality with it carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests.gor2goa_helpers import unpack
from tests.ppp_helpers import (BAD_GEOMETRY, BAD_INPUT, BAD_TABLE, EMPTY, NOT_CONVERGED, OK, OVERFLOW, benzene, c_tables, chain_molecule,
                               edge_molecule, naphthalene, pack, phenacene)
from tests.ppp_open_helpers import (OPEN_TIE, assert_same_bits, device, g30_rows, host, hosts, long_host, long_rows, one_centre, row)

pytestmark = pytest.mark.gpu
EDGES = (2, 3, 31, 32, 33, 63, 64, 65)


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


_CACHE = {}


def edge_cations():
    mols = [edge_molecule(n) for n in EDGES]
    return [m for m, _ in mols], np.array([q + 1 for _, q in mols], np.int32)


def edge_host():
    """The host build's outputs for the eight cations in one call, computed once."""
    if "edge" not in _CACHE:
        _CACHE["edge"] = host(*edge_cations())
    return _CACHE["edge"]


def test_g30_under_the_four_state_kinds_in_one_mixed_call(engine):
    mols, charge, mult, _ = g30_rows()
    dev = device(engine, mols, charge, mult)
    ref = hosts("g30", g30_rows())
    assert_same_bits(dev, ref)
    assert dev["e_state"].dtype == np.float64 and np.bincount(dev["n_open"], minlength=3).tolist() == [157, 314, 157]
    st = np.bincount(dev["status"], minlength=9)
    assert st[OK] >= 560 and st[NOT_CONVERGED] >= 20 and st[OK] + st[NOT_CONVERGED] == len(mols)
    assert ((dev["flags"] & OPEN_TIE) != 0).sum() >= 30


def test_the_tier_edges_as_cations_in_one_call(engine):
    mols, charge = edge_cations()
    dev = device(engine, mols, charge)  # three tiers in one call: the tier, the batch and the place leave no trace
    assert dev["n_pi"].tolist() == list(EDGES) and (dev["n_open"] == 1).all()
    assert_same_bits(dev, edge_host())


@pytest.mark.parametrize("k", range(len(EDGES)), ids=[str(n) for n in EDGES])
def test_a_tier_edge_cation_alone(engine, k):
    mols, charge = edge_cations()
    dev, together = device(engine, [mols[k]], charge[k:k + 1]), edge_host()
    na, nb = len(mols[k][0]), len(mols[k][1])
    a, b = row(dev, 0, na, nb), row(together, k, na, nb)
    for name in _lib.PPP_OPEN_ARRAYS:
        assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), name
    assert dev["n_pi"][0] == EDGES[k] and dev["status"][0] == OK


def test_the_long_rows(engine):
    """126, 127 and 128 centres with one electron removed, the largest tier: against the host build's recorded results
    (tests/golden/ppp_open_long_jobs.npz, which tests/test_ppp_open_cpu.py holds to the live host build)."""
    mols, charge, mult, _ = long_rows()
    dev = device(engine, mols, charge, mult)
    assert_same_bits(dev, long_host())
    assert dev["n_pi"].tolist() == [126, 127, 128] and dev["status"].tolist() == [NOT_CONVERGED, OK, NOT_CONVERGED]
    for k in (1, 2):  # 127 and 128 centres, one row each: a launch of a single workgroup in the largest tier
        alone = device(engine, [mols[k]], charge[k:k + 1], mult[k:k + 1])
        a, b = row(alone, 0, len(mols[k][0]), len(mols[k][1])), row(dev, k, len(mols[k][0]), len(mols[k][1]))
        assert all(np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes() for name in _lib.PPP_OPEN_ARRAYS), k


def test_one_centre_and_triplet_ethylene(engine):
    mols, charge, mult = [one_centre(), chain_molecule(2), chain_molecule(2), one_centre()], [0, 0, 0, -1], [0, 3, 0, 0]
    dev = device(engine, mols, charge, mult)
    assert_same_bits(dev, host(mols, charge, mult))
    assert dev["status"].tolist() == [OK] * 4 and dev["n_pi"].tolist() == [1, 2, 2, 1] and dev["n_open"].tolist() == [1, 2, 0, 0]
    assert abs(dev["e_state"][0] + 11.16) <= 1e-5 and abs(dev["e_state"][1] + 22.32) <= 1e-5


@pytest.mark.parametrize("B", [1, 2, 3, 129])
def test_batch_sizes(engine, B):
    mols, charge, mult, _ = g30_rows()
    pick = [(7 * i) % len(mols) for i in range(B)]
    ms, q, s = [mols[i] for i in pick], charge[pick], mult[pick]
    dev = device(engine, ms, q, s)
    ref = hosts("g30", g30_rows())
    for j, i in enumerate(pick):
        a, b = row(dev, j, len(ms[j][0]), len(ms[j][1])), row(ref, i, len(ms[j][0]), len(ms[j][1]))
        assert all(np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes() for name in _lib.PPP_OPEN_ARRAYS), (j, i)


def test_refusals_the_other_formula_and_a_table_that_cannot_be_used(engine):
    e, b, x = benzene()
    ethylene, allyl = chain_molecule(2), chain_molecule(3)
    empty = (np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 3)))
    cases = [(ethylene, 0, 2, BAD_INPUT), (allyl, 0, 3, BAD_INPUT), (ethylene, -2, 3, BAD_INPUT), (ethylene, 0, 4, BAD_INPUT),
             (ethylene, 0, -1, BAD_INPUT), ((e, b, x), -7, 0, BAD_INPUT),
             ((e, b, np.where(np.arange(6)[:, None] == 1, x[0] + [0.3, 0.0, 0.0], x)), 1, 0, BAD_GEOMETRY),
             ((e, b, np.where(np.arange(6)[:, None] == 4, np.nan, x)), 0, 3, BAD_GEOMETRY), (phenacene(32), 1, 0, OVERFLOW),
             (empty, 0, 0, EMPTY), (allyl, 0, 0, OK), (ethylene, 0, 3, OK)]
    mols, charge, mult = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    dev = device(engine, mols, charge, mult)
    assert_same_bits(dev, host(mols, charge, mult))
    assert dev["status"].tolist() == [c[3] for c in cases]
    two, q, s = [naphthalene(), phenacene(3, 1)], [1, 0], [2, 0]
    for kw in ({"parameters": {"classes": {"C": {"gamma": 0.0}}}}, {"damping": 1.0}, {"repulsion": 2}):
        out = device(engine, two, q, s, **kw)
        assert out["status"].tolist() == [BAD_TABLE, BAD_TABLE] and not out["levels"].any() and not out["e_state"].any(), kw
        assert_same_bits(out, host(two, q, s, **kw))
    t = c_tables()
    t.n_elems = 9
    with pytest.raises(_lib.GaudiError):
        engine.ppp_open(t, *pack(two))
    for kw in ({"repulsion": 1}, {"damping": 0.0}, {}):  # (the engine goes on working)
        assert_same_bits(device(engine, two, q, s, **kw), host(two, q, s, **kw))


def test_the_profile_counts_one_launch_per_tier(engine):
    engine.profile_reset(True)
    assert engine.ppp_open_profile_get() == (0, 0.0)
    n_closed = engine.ppp_profile_get()[0]
    device(engine, [benzene(), naphthalene()], [1, -1])
    assert engine.ppp_open_profile_get()[0] == 1
    device(engine, [benzene(), phenacene(10), phenacene(7), phenacene(9)], [1, 1, 0, -1], [0, 0, 3, 0])
    n, ms = engine.ppp_open_profile_get()
    assert n == 3 and ms > 0.0 and engine.ppp_profile_get()[0] == n_closed  # (its own kernel and its own counter)
    engine.profile_reset(False)
    device(engine, [benzene()], [1])
    assert engine.ppp_open_profile_get()[0] == 0


def test_states_ionization_and_the_keyword_through_an_engine(golden, engine):
    from gaudi_amd import ppp
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms
    from tests.ppp_open_helpers import HostEngine
    g30 = unpack(golden("g30_gor2goa"))
    idx = [i for i, m in enumerate(g30) if m["dataset"] == "hetro"][:40]
    rings = [(g30[i]["x"], g30[i]["types"]) for i in idx]
    plain_recs = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine)
    engine.profile_reset(True)
    same = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine, ppp_dscf=False)
    assert engine.ppp_open_profile_get()[0] == 0 and all(set(a) == set(b) for a, b in zip(same, plain_recs))  # off: no launch
    recs = rings_to_atoms(rings, "hetro", 0.1, place_hydrogens=True, engine=engine, ppp_dscf=True)
    assert 1 <= engine.ppp_open_profile_get()[0] <= 3  # ONE call of 3B rows
    engine.profile_reset(False)
    added = {"ppp_ip_dscf", "ppp_ea_dscf", "ppp_dscf_status"}
    want, on_host = ppp.ionization(plain_recs, "hetro", engine=engine), ppp.ionization(plain_recs, "hetro", engine=HostEngine())
    for k in want:
        assert np.array_equal(want[k], on_host[k], equal_nan=True), k
    built = np.array([r["status"] == 0 for r in recs])
    assert built.sum() >= 30
    for i, (r, p) in enumerate(zip(recs, plain_recs)):
        assert set(r) == set(p) | added and all(np.array_equal(r[k], p[k]) for k in p)
        assert np.array_equal([r["ppp_ip_dscf"], r["ppp_ea_dscf"]], [want["ip"][i], want["ea"][i]], equal_nan=True)
        assert r["ppp_dscf_status"] == want["status"][:, i].max() and (r["ppp_dscf_status"] == EMPTY) == (r["status"] != 0)
    solved = [r for r in recs if r["ppp_dscf_status"] == OK]
    assert len(solved) >= 20 and all(3.0 < r["ppp_ip_dscf"] < 15.0 and r["ppp_ea_dscf"] < r["ppp_ip_dscf"] for r in solved)
    st_dev, st_host = ppp.states(plain_recs[:6], "hetro", charge=1, engine=engine), ppp.states(plain_recs[:6], "hetro", charge=1, engine=HostEngine())
    for a, b in zip(st_dev, st_host):
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    plain, _ = analyze_atoms_for_molecules(rings, 0.1, "hetro", engine=engine)
    d, _ = analyze_atoms_for_molecules(rings, 0.1, "hetro", engine=engine, ppp_dscf=True)
    assert set(d) == set(plain) | {"mol_ppp_ip_dscf", "mol_ppp_ea_dscf"} and all(np.array_equal(d[k], plain[k]) for k in plain)
    bare = [r for r in rings_to_atoms(rings, "hetro", 0.1, engine=engine, ppp_dscf=True) if r["status"] == 0]
    assert np.array_equal(d["mol_ppp_ip_dscf"], np.array([r["ppp_ip_dscf"] for r in bare]), equal_nan=True)
    assert np.array_equal(d["mol_ppp_ea_dscf"], np.array([r["ppp_ea_dscf"] for r in bare]), equal_nan=True)


def test_design_with_ppp_dscf():
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
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, ppp_dscf=True)
    assert set(out) == set(plain) | {"ppp_ip_dscf", "ppp_ea_dscf"}
    for k in ("fingerprints", "mol_unique", "best", "target_function_values"):
        assert np.array_equal(out[k], plain[k]), k
    want = ppp.ionization(out["atoms"], "cata", engine=model.engine)
    for k in ("ip", "ea"):
        assert out[f"ppp_{k}_dscf"].shape == (6,) and out[f"ppp_{k}_dscf"].dtype == np.float64
        assert np.array_equal(out[f"ppp_{k}_dscf"], want[k], equal_nan=True)
    with pytest.raises(ValueError, match="with_atoms"):
        generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, ppp_dscf=True)
    model.engine.close()
