"""Bond orders and formal charges on the device (gaudi_bond_orders) against the kernel's host build, bit for bit, on golden g32 --
the whole fixture is one launch -- and the layers on top: rings_to_atoms(bond_orders=True), analyze_atoms_for_molecules
(valence_check=True), design(with_atoms=True, valence_check=True).  What the structures must satisfy is checked on the host build
by tests/test_bond_orders_cpu.py; equality with it carries that over."""
import types

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import (BAD_INPUT, CAPPED, DATASET, EMPTY, GAVE_UP, OK, OVERFLOW, budget_molecule, fixture, pack,
                                      six_charge_molecule)
from tests.gor2goa_helpers import unpack

pytestmark = pytest.mark.gpu
ARRAYS = ("status", "n_charged", "order", "charge")


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def tables():
    from gaudi_amd.gor2goa import c_valence_tables
    return c_valence_tables(DATASET)


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


@pytest.fixture(scope="module")
def host(g32, tables):
    return _lib.host_bond_orders(tables, *pack(g32[1]))


@pytest.fixture(scope="module")
def device(g32, tables, engine):
    return engine.bond_orders(tables, *pack(g32[1]))


def test_device_equals_the_host_build(g32, host, device):
    for k in ARRAYS:
        assert device[k].dtype == host[k].dtype and np.array_equal(device[k], host[k]), k
    assert (device["status"] == OK).sum() >= 250
    # the inputs the kernel must reject by status sit inside the batch, between ordinary molecules
    for code in (BAD_INPUT, OVERFLOW, EMPTY):
        i = next(m["index"] for m in g32[1] if m["special"] == code)
        assert device["status"][i] == code and device["n_charged"][i] == 0
        assert not device["order"][i].any() and not device["charge"][i].any()


@pytest.mark.parametrize("B", [1, 3])
def test_small_batches(g32, tables, engine, B):
    """One molecule, and three: a last workgroup with one of its two waves idle."""
    mols = [m for m in g32[1] if m["min_charged"] == 2][:B]
    args = pack(mols)
    dev, ref = engine.bond_orders(tables, *args), _lib.host_bond_orders(tables, *args)
    for k in ARRAYS:
        assert np.array_equal(dev[k], ref[k]), k
    assert (dev["status"] == OK).all() and (dev["n_charged"] == 2).all()


def test_paths_the_fixture_does_not_take(g32, tables, engine):
    """The subset budget runs out (GAVE_UP: undecided), the same molecule renumbered so that the search reaches its structure
    (OK, 4 charges), and a molecule whose only structures have 6 charged atoms (CAPPED), next to an ordinary one."""
    e, b, _, _ = six_charge_molecule()
    args = pack([budget_molecule(), budget_molecule(front=True), (e, b), next(m for m in g32[1] if m["special"] == OK)])
    dev, ref = engine.bond_orders(tables, *args), _lib.host_bond_orders(tables, *args)
    for k in ARRAYS:
        assert np.array_equal(dev[k], ref[k]), k
    assert dev["status"].tolist() == [GAVE_UP, OK, CAPPED, OK] and dev["n_charged"].tolist() == [0, 4, 0, 0]


def test_position_in_the_batch_does_not_matter(g32, tables, engine):
    mols = g32[1]
    probe = next(m for m in mols if m["min_charged"] == 4)
    a = [probe] + mols[10:41]
    b = mols[200:233] + [probe]
    da, db = engine.bond_orders(tables, *pack(a)), engine.bond_orders(tables, *pack(b))
    na, nb = len(probe["elem"]), len(probe["bonds"])
    assert da["status"][0] == db["status"][-1] == OK and da["n_charged"][0] == db["n_charged"][-1] == 4
    assert da["order"][0, :nb].tobytes() == db["order"][-1, :nb].tobytes()
    assert da["charge"][0, :na].tobytes() == db["charge"][-1, :na].tobytes()
    assert not da["order"][0, nb:].any() and not db["order"][-1, nb:].any()


def _g30_by_dataset(golden):
    g30 = unpack(golden("g30_gor2goa"))
    return g30, {ds: [i for i, m in enumerate(g30) if m["dataset"] == ds] for ds in ("cata", "hetro")}


def test_rings_to_atoms_with_bond_orders(golden, g32, device):
    """From the ring level: the statuses and charge counts the fixture's atom-level entries of the same molecules get."""
    from gaudi_amd.gor2goa import rings_to_atoms
    g30, by_ds = _g30_by_dataset(golden)
    entry = {m["g30"]: m["index"] for m in g32[1] if m["kind"] == 0}
    n = 0
    for ds, idx in by_ds.items():
        recs = rings_to_atoms([(g30[i]["x"], g30[i]["types"]) for i in idx], ds, 0.1, bond_orders=True)
        plain = rings_to_atoms([(g30[i]["x"], g30[i]["types"]) for i in idx], ds, 0.1)
        for i, r, p in zip(idx, recs, plain):
            assert set(r) == set(p) | {"kekule_status", "orders", "charges", "n_charged"}
            assert all(np.array_equal(r[k], p[k]) for k in p)
            if g30[i]["threw"]:
                assert r["status"] != 0 and r["kekule_status"] == EMPTY and len(r["orders"]) == 0 and len(r["charges"]) == 0
                continue
            j = entry[i]
            assert r["kekule_status"] == device["status"][j] and r["n_charged"] == device["n_charged"][j], (ds, i)
            assert len(r["orders"]) == len(r["bonds"]) and len(r["charges"]) == len(r["atom_types"])
            if r["kekule_status"] == OK:
                assert set(r["orders"].tolist()) <= {1, 2} and r["charges"].sum() == 0
            n += 1
    assert n == len(entry) >= 150


def test_analyze_atoms_with_valence_check(golden, g32):
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    g30, by_ds = _g30_by_dataset(golden)
    valid = {m["g30"] for m in g32[1] if m["kind"] == 0 and 0 <= m["min_charged"] <= 4}
    for ds, idx in by_ds.items():
        mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
        train = [1, 2, 3]
        plain, built = analyze_atoms_for_molecules(mols, 0.1, ds, train_fingerprints=train)
        d, kept = analyze_atoms_for_molecules(mols, 0.1, ds, train_fingerprints=train, valence_check=True)
        for k in plain:
            assert d[k] == plain[k], k
        assert set(d) == set(plain) | {"mol_valid", "molecule_valid_bool", "mol_unique_valid", "mol_novel_valid"}
        want = [i in valid for i in idx]
        assert d["molecule_valid_bool"] == want
        assert d["mol_valid"] == sum(want) / float(len(idx)) and d["mol_valid"] <= d["mol_built"]
        assert len(kept) == sum(want) <= len(built)
        keys = [k for k, ok in zip(d["fingerprints"], want) if ok]
        assert d["mol_unique_valid"] == len(set(keys)) / float(len(keys)) and d["mol_novel_valid"] == 1.0
    assert len(valid) >= 150


def test_design_with_valence_check():
    import torch  # noqa: F401
    from gaudi_amd import generation_guidance, synth
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

    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, valence_check=True)
    assert {"atoms", "mol_unique", "fingerprints", "mol_valid", "valid", "best_valid", "best", "best_stable"} <= set(out)
    assert len(out["valid"]) == len(out["atoms"]) == 6 and out["valid"].dtype == bool
    assert out["mol_valid"] == out["valid"].sum() / 6.0
    assert set(out["best_valid"].tolist()) == {int(i) for i in out["best"] if out["valid"][i]}
    assert [int(i) for i in out["best"] if out["valid"][i]] == out["best_valid"].tolist()  # the ranking's order is kept
    for rec, ok in zip(out["atoms"], out["valid"]):
        assert ok == (rec["status"] == 0 and rec["kekule_status"] == OK)
        assert len(rec["orders"]) == len(rec["bonds"]) and len(rec["charges"]) == len(rec["atom_types"])
    model.engine.close()
