"""Canonical numbering on the device (gaudi_canonical_order) against the kernel's host build, bit for bit, on golden g32 -- the
whole fixture is one launch, with the 190 / 194-atom acenes that fill the capacities inside it -- and the layers on top:
rings_to_atoms(canonical=True, bond_orders=True) on g30 and its twins, analyze_atoms_for_molecules(exact=True).  What the outputs
must satisfy is checked on the host build by tests/test_canonical_cpu.py; equality with it carries that over."""
import numpy as np
import pytest

from tests.bond_order_helpers import C, H, fixture, pack
from tests.canonical_helpers import ARRAYS, BAD_INPUT, EMPTY, GAVE_UP, N_ELEMS, OK, OVERFLOW, benzenes, host_canon
from tests.gor2goa_helpers import unpack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def device_canon(engine, mols):
    return engine.canonical_order(N_ELEMS, H, C, *pack(mols))


def test_device_equals_the_host_build(g32, engine):
    mols = g32[1]
    assert len(mols) % 2 == 1  # an odd count: the last workgroup has one wave idle
    assert max(len(m["elem"]) for m in mols if m["special"] == 0) >= 190
    dev, ref = device_canon(engine, mols), host_canon(mols)
    for k in ARRAYS:
        assert dev[k].dtype == ref[k].dtype and np.array_equal(dev[k], ref[k]), k
    assert (dev["status"] == OK).sum() >= 500 and dev["nodes"].max() == 469
    for code, special in ((BAD_INPUT, 5), (OVERFLOW, 6), (EMPTY, 7)):
        i = next(m["index"] for m in mols if m["special"] == special)
        assert dev["status"][i] == code and not any(dev[k][i].any() for k in ARRAYS if k != "status")


@pytest.mark.parametrize("B", [1, 3])
def test_small_batches(g32, engine, B):
    """One wave alone, and three: a last workgroup with one of its two waves idle.  The largest molecules of the fixture."""
    mols = sorted((m for m in g32[1] if m["special"] == 0), key=lambda m: -len(m["elem"]))[:B]
    dev, ref = device_canon(engine, mols), host_canon(mols)
    for k in ARRAYS:
        assert np.array_equal(dev[k], ref[k]), k
    assert (dev["status"] == OK).all()


def test_the_search_gives_up_on_the_device_as_on_the_host(g32, engine):
    """Three benzenes run into the node cap next to two (the fixture's largest tree) and an ordinary molecule."""
    mols = [benzenes(3), benzenes(2), next(m for m in g32[1] if m["special"] == 0)]
    dev, ref = device_canon(engine, mols), host_canon(mols)
    for k in ARRAYS:
        assert np.array_equal(dev[k], ref[k]), k
    assert dev["status"].tolist() == [GAVE_UP, OK, OK] and dev["nodes"].tolist()[:2] == [4096, 469]


def test_position_in_the_batch_does_not_matter(g32, engine):
    mols = g32[1]
    probe = next(m for m in mols if m["min_charged"] == 4)
    da, db = device_canon(engine, [probe] + mols[10:41]), device_canon(engine, mols[200:233] + [probe])
    na, A = len(probe["elem"]), min(da["rank"].shape[1], db["rank"].shape[1])
    M = min(da["cbonds"].shape[1], db["cbonds"].shape[1])
    assert da["status"][0] == db["status"][-1] == OK and na <= A
    for k in ("nodes", "n_heavy", "n_hbonds"):
        assert da[k][0] == db[k][-1]
    assert da["rank"][0, :na].tobytes() == db["rank"][-1, :na].tobytes()
    assert da["label"][0, :A].tobytes() == db["label"][-1, :A].tobytes()
    assert da["cbonds"][0, :M].tobytes() == db["cbonds"][-1, :M].tobytes()


def test_the_layers_end_to_end(golden):
    """From the ring level: a molecule and its twin (the same molecule from other ring positions, so with another atom
    numbering) get the same key and the same SMILES; the keys' classes are the fixture's iso_class; the exact counting runs."""
    from gaudi_amd.analyze import analyze_atoms_for_molecules
    from gaudi_amd.gor2goa import rings_to_atoms, smiles
    g30 = unpack(golden("g30_gor2goa"))
    by_key, by_class, n_smiles = {}, {}, 0
    for ds in ("cata", "hetro"):
        idx = [i for i, m in enumerate(g30) if m["dataset"] == ds]
        recs = rings_to_atoms([(g30[i]["x"], g30[i]["types"]) for i in idx], ds, 0.1, canonical=True, bond_orders=True)
        twins = rings_to_atoms([(g30[i]["twin_x"], g30[i]["twin_types"]) for i in idx], ds, 0.1, canonical=True, bond_orders=True)
        plain = rings_to_atoms([(g30[i]["x"], g30[i]["types"]) for i in idx], ds, 0.1, bond_orders=True)
        for i, r, t, p in zip(idx, recs, twins, plain):
            assert set(r) == set(p) | {"canon_status", "canon_rank", "canon_key", "canon_nodes", "canon_kekule_status",
                                       "canon_orders", "canon_charges", "canon_n_charged"}
            assert all(np.array_equal(r[k], p[k]) for k in p)
            if g30[i]["threw"]:
                assert r["canon_status"] == EMPTY and r["canon_key"] is None and smiles(r, ds) is None
                continue
            assert r["canon_status"] == t["canon_status"] == OK and r["canon_key"] == t["canon_key"], (ds, i)
            assert g30[i]["iso_class"] == g30[i]["twin_iso_class"]
            assert r["canon_kekule_status"] == t["canon_kekule_status"] == r["kekule_status"]
            assert smiles(r, ds) == smiles(t, ds) and (smiles(r, ds) is not None) == (r["canon_kekule_status"] == 0)
            n_smiles += smiles(r, ds) is not None
            # the element lists of the two datasets share their first entries, so keys compare across them but for n_elems,
            # which is no part of the key
            by_key.setdefault(r["canon_key"], set()).add(g30[i]["iso_class"])
            by_class.setdefault(g30[i]["iso_class"], set()).add(r["canon_key"])
        mols = [(g30[i]["x"], g30[i]["types"]) for i in idx]
        plain_d, _ = analyze_atoms_for_molecules(mols, 0.1, ds, valence_check=True)
        d, kept = analyze_atoms_for_molecules(mols, 0.1, ds, valence_check=True, exact=True, train_keys=[next(r["canon_key"] for r in recs if r["canon_key"])])
        assert set(d) == set(plain_d) | {"canon_keys", "mol_undecided", "smiles", "mol_novel", "mol_novel_valid"}
        assert d["canon_keys"] == [r["canon_key"] for r in recs] and d["mol_undecided"] == 0.0
        assert d["smiles"] == [smiles(r, ds) for r in recs] and len(kept) == sum(s is not None for s in d["smiles"])
        built = [k for k in d["canon_keys"] if k is not None]
        assert d["mol_unique"] == len(set(built)) / float(len(built)) and 0.0 < d["mol_novel"] < 1.0
    assert all(len(v) == 1 for v in by_key.values()) and all(len(v) == 1 for v in by_class.values())
    assert len(by_key) == 128 and n_smiles >= 100


def test_design_with_exact_keys():
    import types

    import torch  # noqa: F401
    from gaudi_amd import generation_guidance, synth
    from gaudi_amd.gor2goa import smiles
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

    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True, valence_check=True,
                                     exact=True)
    assert {"atoms", "mol_unique", "fingerprints", "mol_valid", "valid", "canon_keys", "smiles"} <= set(out)
    assert len(out["canon_keys"]) == len(out["smiles"]) == len(out["atoms"]) == 6
    for rec, key, text in zip(out["atoms"], out["canon_keys"], out["smiles"]):
        assert (key is None) == (rec["status"] != 0) and text == smiles(rec, "cata")
        if rec["status"] == 0 and rec["canon_status"] == OK:
            assert key == rec["canon_key"] and isinstance(key, bytes)
    built = [k for k in out["canon_keys"] if k is not None]
    assert out["mol_unique"] == (len(set(built)) / float(len(built)) if built else 0.0)
    model.engine.close()
