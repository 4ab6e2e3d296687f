"""Graph of rings -> graph of atoms on the device (gaudi_rings_to_atoms) against the reference's gor2goa (golden g30): the
discrete result exactly, the geometry within a tolerance measured on the reference, the lifted coordinates, frame invariance,
the fingerprint against exact isomorphism, hydrogens, capacity, and design(with_atoms=True)."""
import types

import numpy as np
import pytest

from gaudi_amd._lib import GaudiError
from tests.gor2goa_helpers import n_rings, pdist, tolerances, unpack

pytestmark = pytest.mark.gpu

H, C = 0, 1


@pytest.fixture(scope="module")
def g30(golden):
    return unpack(golden("g30_gor2goa"))


def _run(mols, key_x="x", key_t="types", **kw):
    """One launch per dataset; records in the order of `mols`."""
    from gaudi_amd.gor2goa import rings_to_atoms
    out = [None] * len(mols)
    for ds in ("cata", "hetro"):
        idx = [i for i, m in enumerate(mols) if m["dataset"] == ds]
        if idx:
            for i, r in zip(idx, rings_to_atoms([(mols[i][key_x], mols[i][key_t]) for i in idx], ds, 0.1, **kw)):
                out[i] = r
    return out


@pytest.fixture(scope="module")
def built(g30):
    return _run(g30, fingerprint=True)


@pytest.fixture(scope="module")
def built_h(g30):
    return _run(g30, place_hydrogens=True, fingerprint=True)


@pytest.fixture(scope="module")
def fused_pairs(g30):
    """Number of fused ring pairs of every built molecule, from the device's own positions2adj (one launch per dataset).
    The stability kernel leaves the adjacency empty when the orientation-node test fails (g30 holds a hetero molecule with an odd
    node count, which gor2goa builds all the same), so only the ring nodes go in, each followed by a well-formed orientation node:
    the adjacency does not read those."""
    from gaudi_amd.analyze import _pack, check_stability_batch, rings_list
    out = [0] * len(g30)
    for ds in ("cata", "hetro"):
        idx = [i for i, m in enumerate(g30) if m["dataset"] == ds and not m["threw"]]
        mols = []
        for i in idx:
            nr = n_rings(g30[i])
            x, t = g30[i]["x"][:nr], g30[i]["types"][:nr]
            if ds != "cata":
                x, t = np.concatenate([x, x]), np.concatenate([t, np.full(nr, len(rings_list(ds)) - 1, np.int64)])
            mols.append((x, t))
        X, T, nn = _pack(mols)
        _, _, adj = check_stability_batch(X, T, nn, 0.1, ds, want_adj=True)
        for i, a in zip(idx, adj):
            out[i] = int(np.triu(a).sum())
    return out


def _ring_tables(dataset):
    from gaudi_amd.gor2goa import c_atom_tables
    t = c_atom_tables(dataset)
    return t, [np.array([[t.templ[i][k][0], t.templ[i][k][1]] for k in range(t.ring_size[i])]) for i in range(t.n_types)]


def _plane(points):
    """Least-squares plane through points [n,3] -> (a point on it, its unit normal)."""
    c = points.mean(0)
    return c, np.linalg.svd(points - c)[2][2]


def test_parity_with_the_reference(g30, built):
    """status != 0 exactly where the reference raises; n_atoms, atom types and the sorted bond list EQUAL the reference's; the
    pairwise distances of xy within 4 x the molecule's dist_spread, floored at the fixture's median spread.
    Largest observed ratio error / tolerance on the MI355X: see DESIGN.md (graph of atoms); a float64 device path sits orders of
    magnitude inside."""
    tol, floor = tolerances(g30)
    worst = 0.0
    for m, r, t in zip(g30, built, tol):
        assert (r["status"] != 0) == m["threw"], (m["dataset"], len(m["x"]), r["status"])
        if m["threw"]:
            assert len(r["atom_types"]) == 0 and len(r["bonds"]) == 0 and r["fingerprint"] == 0
            continue
        assert np.array_equal(r["atom_types"], m["ref_types"])
        assert np.array_equal(r["bonds"], m["ref_bonds"])
        err = float(np.abs(pdist(r["atoms"]) - pdist(m["ref_atoms"])).max())
        worst = max(worst, err / t)
        assert err <= t, (m["dataset"], n_rings(m), err, t)
    print(f"g30 parity: largest |distance error| / tolerance = {worst:.3e} (tolerance floor {floor:.2e} A)")


def test_lifted_coordinates(g30, built, fused_pairs):
    """xyz has the pairwise distances of xy, and every atom that is not a merged midpoint (the last two per fused pair) or a
    template H sits on a template vertex of one of the rings: at that vertex's radius from the ring's input centroid projected on
    the fitted plane."""
    tol, _ = tolerances(g30)
    for m, r, t, n_pairs in zip(g30, built, tol, fused_pairs):
        if m["threw"]:
            continue
        assert np.abs(pdist(r["atoms3d"]) - pdist(r["atoms"])).max() <= t
        tab, templ = _ring_tables(m["dataset"])
        nr = n_rings(m)
        ring_t = m["types"][:nr]
        n_merged = 2 * n_pairs
        heavy = r["atom_types"] != H
        p0, nrm = _plane(r["atoms3d"][heavy])
        cen = m["x"][:nr].astype(np.float64)
        cen = cen - ((cen - p0) @ nrm)[:, None] * nrm
        radii = [np.linalg.norm(templ[k], axis=1) for k in ring_t]
        for a in np.nonzero(heavy[: len(heavy) - n_merged])[0]:
            d = np.linalg.norm(cen - r["atoms3d"][a], axis=1)
            assert min(np.abs(d[i] - radii[i]).min() for i in range(nr)) <= t + 1e-9, (m["dataset"], nr, a)


def test_single_molecule_call_agrees_and_raises(g30, built):
    from gaudi_amd.gor2goa import gor2goa
    picks = [next(i for i, m in enumerate(g30) if m["dataset"] == ds and not m["threw"] and n_rings(m) >= 5) for ds in ("cata", "hetro")]
    for i in picks:
        m = g30[i]
        atoms, types_, bonds = gor2goa(m["x"], m["types"], m["dataset"], 0.1)
        assert np.array_equal(np.asarray(atoms), built[i]["atoms"]) and np.asarray(atoms).dtype == np.float64
        assert np.array_equal(np.asarray(types_), built[i]["atom_types"])
        assert bonds == [tuple(b) for b in built[i]["bonds"].tolist()]
    i = next(i for i, m in enumerate(g30) if m["threw"])
    with pytest.raises(GaudiError):
        gor2goa(g30[i]["x"], g30[i]["types"], g30[i]["dataset"])


def test_frame_invariance_on_the_device(g30, built):
    """Rings permuted (orientation nodes with them), the molecule rotated and reflected: same fingerprint, same counts."""
    twins = _run(g30, "twin_x", "twin_types", fingerprint=True)
    n = 0
    for m, r, t in zip(g30, built, twins):
        assert r["status"] == t["status"]
        if m["threw"]:
            continue
        assert len(t["atom_types"]) == len(r["atom_types"]) and len(t["bonds"]) == len(r["bonds"])
        assert t["fingerprint"] == r["fingerprint"] != 0, (m["dataset"], n_rings(m))
        n += 1
    assert n >= 150


def test_fingerprint_partition_equals_exact_isomorphism(g30, built):
    by_key, by_class = {}, {}
    for m, r in zip(g30, built):
        if m["threw"]:
            continue
        by_key.setdefault(r["fingerprint"], set()).add(m["iso_class"])
        by_class.setdefault(m["iso_class"], set()).add(r["fingerprint"])
    assert all(len(v) == 1 for v in by_key.values()), "two non-isomorphic molecules share a fingerprint"
    assert all(len(v) == 1 for v in by_class.values()), "isomorphic molecules with different fingerprints"
    assert len(by_key) == len(by_class) >= 60


def test_hydrogens(g30, built, built_h):
    """place_hydrogens leaves the heavy atoms and their bonds alone; stable cata molecules come out as C(4n+2)H(2n+4) with every
    C-H 1.09 A long, in the molecular plane, pointing away from the ring."""
    n = 0
    for m, r, rh in zip(g30, built, built_h):
        if m["threw"]:
            assert rh["status"] != 0
            continue
        k = len(r["atom_types"])
        assert rh["status"] == 0 and rh["fingerprint"] == r["fingerprint"]
        heavy = r["atom_types"] != H
        assert np.array_equal(rh["atom_types"][:k], r["atom_types"]) and np.all(rh["atom_types"][k:] == H)
        assert np.array_equal(rh["atoms"][:k][heavy], r["atoms"][heavy])  # (template H's move, nothing else does)
        hb = rh["bonds"]
        assert np.array_equal(hb[hb[:, 1] < k], r["bonds"])
        new = hb[hb[:, 1] >= k]
        assert np.array_equal(new[:, 1], np.arange(k, len(rh["atom_types"]))) and np.all(np.diff(new[:, 0]) > 0)  # ascending parents
        if not (m["dataset"] == "cata" and m["stable"]):
            continue
        n += 1
        nr = n_rings(m)
        ty = rh["atom_types"]
        assert (ty == C).sum() == 4 * nr + 2 and (ty == H).sum() == 2 * nr + 4
        p0, nrm = _plane(rh["atoms3d"][ty == C])
        cen = m["x"].astype(np.float64)
        cen = cen - ((cen - p0) @ nrm)[:, None] * nrm
        for c, h in new:
            assert ty[c] == C and ty[h] == H
            assert abs(np.linalg.norm(rh["atoms3d"][h] - rh["atoms3d"][c]) - 1.09) < 1e-9
            assert abs(np.linalg.norm(rh["atoms"][h] - rh["atoms"][c]) - 1.09) < 1e-9
            assert abs((rh["atoms3d"][h] - p0) @ nrm) < 1e-6
            ring = np.argmin(np.linalg.norm(cen - rh["atoms3d"][c], axis=1))
            assert np.linalg.norm(rh["atoms3d"][h] - cen[ring]) > np.linalg.norm(rh["atoms3d"][c] - cen[ring])
    assert n >= 40


def test_hydrogens_on_hetero_template_atoms(g30, built_h):
    """Template H's (Bl / Pl / DhDb) leave the origin: 1.09 A from the ring atom they are bonded to."""
    n = 0
    for m, rh in zip(g30, built_h):
        if m["threw"] or m["dataset"] != "hetro":
            continue
        ty, xy = rh["atom_types"], rh["atoms"]
        for i, j in rh["bonds"]:
            if (ty[i] == H) != (ty[j] == H):
                assert abs(np.linalg.norm(xy[i] - xy[j]) - 1.09) < 1e-9
                n += ty[i] != C and ty[j] != C
    assert n >= 5  # H on B / N


def test_capacity(g30, built):
    from gaudi_amd.gor2goa import rings_to_atoms
    i = next(i for i, m in enumerate(g30) if n_rings(m) == 32)
    assert built[i]["status"] == 0 and len(built[i]["atom_types"]) == 4 * 32 + 2
    x = np.array([[2.45 * k, 0.01 * (k % 3), 0.0] for k in range(33)], np.float32)
    with pytest.raises(GaudiError, match=r"\(-5\)"):
        rings_to_atoms([(x, np.zeros(33, np.int64))], "cata")


def test_design_with_atoms():
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

    parent_keys = {"stability", "best_stable", "x", "one_hot", "node_mask", "edge_mask", "target_function_values", "pred", "best",
                   "seconds", "molecules_per_second"}
    plain = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5)
    assert set(plain) == parent_keys
    out = generation_guidance.design(args, model, cp, tf_gap, None, None, 0.6, 7, n_steps=5, with_atoms=True)
    assert set(out) == parent_keys | {"atoms", "mol_unique", "fingerprints"}
    assert len(out["atoms"]) == len(out["fingerprints"]) == out["x"].shape[0] == 6
    assert 0.0 <= out["mol_unique"] <= 1.0
    for rec, key in zip(out["atoms"], out["fingerprints"]):
        assert rec["fingerprint"] == key and (key != 0) == (rec["status"] == 0)
        assert len(rec["atoms"]) == len(rec["atoms3d"]) == len(rec["atom_types"])
    model.engine.close()
