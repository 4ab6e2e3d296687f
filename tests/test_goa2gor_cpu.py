"""Atoms -> graph of rings without a GPU: the HOST build of the perception routine (gaudi_host_atoms_to_rings, the same source text
the kernel compiles) against the reference's get_connectivity_matrix / get_rings / get_rings_adj / AromaticDataset.get_all as
recorded in tests/golden/g31_goa2gor.npz, plus the host code around it."""
import io
import os
import random
import re

import numpy as np
import pytest

from tests.goa2gor_helpers import BAD_TYPE, NO_RINGS, NOT_A_BASIS, OK, OVERFLOW, HostEngine, compared, fixture, ring_sets, rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results():
    """Every fixture molecule through goa2gor.atoms_to_rings on the host build: one call per (dataset, use_hydrogens)."""
    from gaudi_amd.goa2gor import atoms_to_rings
    _, mols = fixture()
    out = [None] * len(mols)
    for ds in ("cata", "hetro"):
        for use_h in (False, True):
            grp = [m for m in mols if m["ds"] == ds and m["use_h"] == use_h]
            if grp:
                recs = atoms_to_rings([(m["elem"], m["xyz"]) for m in grp], ds, use_hydrogens=use_h, engine=HostEngine())
                for m, r in zip(grp, recs):
                    out[m["index"]] = r
    return out


def test_g31_is_what_the_issue_asks_for():
    z, mols = fixture()
    ok = [m for m in mols if m["basis_ok"] and not m["threw"]]
    assert len(ok) >= 100 and sum(m["ds"] == "hetro" for m in ok) >= 40
    assert sum(not m["basis_ok"] for m in mols) >= 5
    assert min(m["margin"] for m in mols) >= 1e-9
    assert {m["expect"] for m in mols if m["special"]} == {OK, NO_RINGS, BAD_TYPE, NOT_A_BASIS, OVERFLOW}
    assert len(z["ga_hetro_idx"]) >= 8 and len(z["ga_cata_idx"]) >= 4
    g30 = os.path.getsize(os.path.join(ROOT, "tests", "golden", "g30_gor2goa.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g31_goa2gor.npz")) <= g30


def test_statuses(results):
    _, mols = fixture()
    for m, r in zip(mols, results):
        assert r["status"] == m["expect"], (m["index"], r["status"], m["expect"])
        if r["status"] != OK:
            assert len(r["x"]) == 0 and len(r["ring_atoms"]) == 0 and r["orientation"] == []
    sp = [m for m in mols if m["special"]]
    assert [m["expect"] for m in sp[-2:]] == [OK, OVERFLOW]  # the 32-ring row and the 33-ring row
    assert len(results[sp[-2]["index"]]["x"]) == 32


def test_rings_match_the_reference(results):
    _, mols = fixture()
    n = 0
    for m, r in zip(mols, results):
        if not compared(m):
            continue
        n += 1
        # the kernel's order is the fixture's order: ascending by the sorted atom tuple
        got = [tuple(int(a) for a in row if a >= 0) for row in r["ring_atoms"]]
        assert got == sorted(got) and all(list(t) == sorted(t) for t in got)
        assert set(ring_sets(r["ring_atoms"])) == set(ring_sets(m["ring_atoms"])) and len(got) == m["n_rings"]
        assert [set(t) for t in got] == [set(s) for s in ring_sets(m["ring_atoms"])]  # so rings are matched by position
        assert np.array_equal(r["ring_type"], m["ring_type"]), m["index"]
        assert np.array_equal(r["adj"], m["adj"].astype(np.float32)), m["index"]
        assert np.array_equal(r["node_features"].argmax(1), m["ring_type"]) and np.all(r["node_features"].sum(1) == 1)
        tol = 64 * 2.0 ** -53 * np.abs(m["xyz"]).max()
        assert np.abs(r["centres"] - m["centre"]).max() <= tol, m["index"]
        assert np.all(np.abs(r["x"] - m["x32"]) <= np.spacing(np.abs(m["x32"]))), m["index"]
        assert r["x"].dtype == np.float32 and r["centres"].dtype == np.float64
        for k in range(m["n_rings"]):  # orientation candidates are input values: bit-equal, compared as sets
            want = {tuple(m["centre"][k]) if a == -1 else tuple(m["xyz"][a]) for a in m["orient"][k] if a >= -1}
            if -1 in m["orient"][k]:  # the centre itself: the reference's centre, within the centre tolerance
                assert len(r["orientation"][k]) == 1 and np.array_equal(r["orientation"][k][0], r["centres"][k])
            else:
                assert {tuple(p) for p in r["orientation"][k]} == want, (m["index"], k)
    assert n >= 100


def test_hydrogens_decide_db_against_dhdb():
    from gaudi_amd.aromatic_dataloader import RINGS_LIST
    from gaudi_amd.goa2gor import atoms_to_rings
    _, mols = fixture()
    sp = [m for m in mols if m["use_h"]]
    assert len(sp) == 2
    names = [RINGS_LIST["hetro"][int(m["ring_type"][0])] for m in sp]
    assert names == ["Db", "DhDb"]  # what the reference said with the hydrogens in its graph
    pairs = [(m["symbols"], m["xyz"]) for m in sp]
    with_h = atoms_to_rings(pairs, "hetro", use_hydrogens=True, engine=HostEngine())
    assert [RINGS_LIST["hetro"][int(r["ring_type"][0])] for r in with_h] == ["Db", "DhDb"]
    without = atoms_to_rings(pairs, "hetro", engine=HostEngine())
    assert [RINGS_LIST["hetro"][int(r["ring_type"][0])] for r in without] == ["Db", "Db"]  # skip_hydrogen=True: the dataset path


def test_permuting_or_rotating_a_molecule_relabels_its_rings(results):
    from gaudi_amd.goa2gor import atoms_to_rings
    _, mols = fixture()
    rng = np.random.default_rng(31)
    picked = [m for m in mols if compared(m) and m["margin"] >= 1e-3 and not m["use_h"]][::6]
    assert len(picked) >= 15
    for ds in ("cata", "hetro"):
        grp = [m for m in picked if m["ds"] == ds]
        perms = [rng.permutation(len(m["elem"])) for m in grp]
        moved = [(m["elem"][p], (m["xyz"] @ rot(rng) + rng.uniform(-3, 3, 3))[p]) for m, p in zip(grp, perms)]
        for m, p, r in zip(grp, perms, atoms_to_rings(moved, ds, engine=HostEngine())):
            base = results[m["index"]]
            assert r["status"] == OK
            back = {frozenset(int(p[a]) for a in s) for s in ring_sets(r["ring_atoms"])}  # new index a was old atom p[a]
            assert back == set(ring_sets(base["ring_atoms"]))
            key = lambda rec, q=None: sorted((tuple(sorted((q[a] if q is not None else a) for a in row if a >= 0)), int(t))
                                             for row, t in zip(rec["ring_atoms"], rec["ring_type"]))
            assert key(r, p) == key(base)


def test_a_failing_molecule_leaves_its_neighbours_alone(results):
    from gaudi_amd.goa2gor import atoms_to_rings
    _, mols = fixture()
    good = [m for m in mols if compared(m) and m["ds"] == "cata"][:2]
    for bad in [m for m in mols if m["ds"] == "cata" and m["expect"] in (NO_RINGS, NOT_A_BASIS, OVERFLOW)]:
        recs = atoms_to_rings([(good[0]["elem"], good[0]["xyz"]), (bad["elem"], bad["xyz"]), (good[1]["elem"], good[1]["xyz"])],
                              "cata", engine=HostEngine())
        assert recs[1]["status"] == bad["expect"]
        for r, m in ((recs[0], good[0]), (recs[2], good[1])):
            base = results[m["index"]]
            for k in ("x", "centres", "ring_type", "adj", "ring_atoms", "node_features"):
                assert np.array_equal(r[k], base[k])
            assert all(np.array_equal(a, b) for a, b in zip(r["orientation"], base["orientation"]))


@pytest.mark.parametrize("ds", ["hetro", "cata"])
def test_dataset_rows_against_get_all(results, ds):
    from gaudi_amd.aromatic_dataloader import RingsDataset, batches
    z, mols = fixture()
    idx = [int(i) for i in z[f"ga_{ds}_idx"]]
    mn = int(z[f"ga_{ds}_max_nodes"])
    dset = RingsDataset([results[i] for i in idx], z[f"ga_{ds}_targets"], ds, mn, normalize=True)
    assert len(dset) == len(idx) and dset.skipped == {}
    assert np.array_equal(dset.mean, z[f"ga_{ds}_mean"]) and np.array_equal(dset.std, z[f"ga_{ds}_std"])
    random.seed(5)
    for row, i in enumerate(idx):
        x, nm, em, nf, y = dset[row]
        n = mols[i]["n_rings"]
        assert np.array_equal(nm, z[f"ga_{ds}_node_mask"][row]) and np.array_equal(em, z[f"ga_{ds}_edge_mask"][row])
        assert np.array_equal(y, z[f"ga_{ds}_y"][row])
        # the reference laid its rings out in networkx's order: match them by centre (the fixture's x32, in sorted order)
        ref_x, ref_nf = z[f"ga_{ds}_x"][row], z[f"ga_{ds}_node_features"][row]
        order = [int(np.argmin(np.abs(ref_x[:n] - mols[i]["x32"][k]).sum(1))) for k in range(n)]
        assert sorted(order) == list(range(n))
        assert np.all(np.abs(x[:n] - ref_x[order]) <= np.spacing(np.abs(ref_x[order])))
        assert np.array_equal(nf[:n], ref_nf[order]) and np.array_equal(nf[n:mn], ref_nf[n:mn])
        if ds == "hetro":
            assert np.array_equal(nf[mn:mn + n], ref_nf[mn:mn + n][order]) and np.all(nf[mn:mn + n, -1] == 1)
            assert np.all(x[n:mn] == 0) and np.all(x[mn + n:] == 0)
            for k in range(n):  # each orientation row is one of that ring's candidates (cast as torch.tensor casts them)
                cands = [np.asarray(c, np.float64).astype(np.float32) for c in results[i]["orientation"][k]]
                assert any(np.array_equal(x[mn + k], c) for c in cands)
                ref_cands = [mols[i]["centre"][k] if a == -1 else mols[i]["xyz"][a] for a in mols[i]["orient"][k] if a >= -1]
                assert any(np.all(np.abs(ref_x[mn + order[k]] - np.asarray(c).astype(np.float32)) <= np.spacing(np.float32(8)))
                           for c in ref_cands)
    got = list(batches(dset, 3))
    assert [len(b[0]) for b in got] == [3] * (len(idx) // 3) + ([len(idx) % 3] if len(idx) % 3 else [])
    assert all(len(b) == 5 and b[0].shape[1:] == ((2 * mn if ds == "hetro" else mn), 3) for b in got)


def test_dataset_leaves_out_what_it_cannot_lay_out(results):
    from gaudi_amd.aromatic_dataloader import RingsDataset
    _, mols = fixture()
    cata = [m for m in mols if m["ds"] == "cata"]
    dset = RingsDataset([results[m["index"]] for m in cata], None, "cata", 11)
    want = {}
    for m in cata:
        name = {OK: None, NO_RINGS: "NO_RINGS", BAD_TYPE: "BAD_TYPE", NOT_A_BASIS: "NOT_A_BASIS", OVERFLOW: "OVERFLOW"}[m["expect"]]
        if name is None and m["n_rings"] > 11:
            name = "TOO_MANY_RINGS"
        if name:
            want[name] = want.get(name, 0) + 1
    assert dset.skipped == want and len(dset) == len(cata) - sum(want.values()) and "TOO_MANY_RINGS" in want
    assert dset[0][4].shape == (0,)


def test_read_xyz_inverts_write_xyz(tmp_path):
    from gaudi_amd._lib import GaudiError
    from gaudi_amd.goa2gor import read_xyz
    from gaudi_amd.gor2goa import write_xyz
    rng = np.random.default_rng(7)
    xyz = np.round(rng.uniform(-9, 9, (7, 3)), 8)  # write_xyz keeps 8 decimals
    types = np.array([1, 0, 2, 3, 4, 5, 1])
    path = str(tmp_path / "m.xyz")
    write_xyz(path, xyz, types, "hetro", comment="a comment")
    sym, back = read_xyz(path)
    assert sym == ["C", "H", "B", "N", "O", "S", "C"] and back.dtype == np.float64 and np.array_equal(back, xyz)
    sym, back = read_xyz(io.StringIO("2\n\n6 0.5 1 -2\nh 0 0 1e-3\n"))  # atomic numbers and lower case, as load_xyz takes them
    assert sym == ["C", "H"] and np.array_equal(back, [[0.5, 1, -2], [0, 0, 1e-3]])
    with pytest.raises(GaudiError):
        read_xyz(io.StringIO("1\n\nC 0 0\n"))


def test_goa2gor_and_errors():
    from gaudi_amd._lib import GaudiError
    from gaudi_amd.goa2gor import atoms_to_rings, goa2gor
    _, mols = fixture()
    m = next(m for m in mols if compared(m) and m["ds"] == "hetro" and m["n_rings"] >= 3)
    x, adj, nf, orientation = goa2gor(m["symbols"], m["xyz"], "hetro", engine=HostEngine())
    assert tuple(x.shape) == (m["n_rings"], 3) and tuple(adj.shape) == (m["n_rings"],) * 2 and nf.shape[1] == 12
    assert len(orientation) == m["n_rings"] and all(1 <= len(o) <= 2 and len(o[0]) == 3 for o in orientation)
    seven = next(m for m in mols if m["special"] and m["expect"] == NOT_A_BASIS)
    with pytest.raises(GaudiError, match="NOT_A_BASIS"):
        goa2gor(seven["symbols"], seven["xyz"], "cata", engine=HostEngine())
    with pytest.raises(GaudiError, match="ATOMS_LIST"):
        atoms_to_rings([(["C", "N"], np.zeros((2, 3)))], "cata", engine=HostEngine())
    with pytest.raises(GaudiError, match="ATOMS_LIST"):
        atoms_to_rings([(np.array([1, 2]), np.zeros((2, 3)))], "cata", engine=HostEngine())
    assert atoms_to_rings([], "cata", engine=HostEngine()) == []


def test_entry_points_are_declared_and_bound():
    from gaudi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    for name, nargs in (("gaudi_atoms_to_rings", 19), ("gaudi_host_atoms_to_rings", 18), ("gaudi_rings_profile_get", 3)):
        assert re.search(rf"\bint {name}\(", hdr) and len(_lib.EXPORTS[name][1]) == nargs
    assert "#define GAUDI_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7
    for macro, val in (("MAX_ATOMS", _lib.RINGS_MAX_ATOMS), ("MAX_HEAVY", _lib.RINGS_MAX_HEAVY), ("MAX_RINGS", _lib.RINGS_MAX_RINGS),
                       ("USE_H", _lib.RINGS_USE_H), ("OK", 0), ("NO_RINGS", 1), ("BAD_TYPE", 2), ("NOT_A_BASIS", 3), ("OVERFLOW", 4)):
        assert re.search(rf"#define GAUDI_RINGS_{macro} {val}\b", hdr), macro
    assert _lib.RINGS_MAX_ATOMS >= _lib.ATOMS_MAX_ATOMS and _lib.RINGS_MAX_HEAVY >= 192 and _lib.RINGS_MAX_RINGS >= 32
    lib = _lib.load_library()
    assert all(hasattr(lib, n) for n in _lib._RINGS_EXPORTS + ("gaudi_host_atoms_to_rings",))


def test_a_library_without_the_export_group_still_loads(monkeypatch):
    from gaudi_amd import _lib
    real = _lib.load_library()
    hidden = set(_lib._RINGS_EXPORTS) | {"gaudi_host_atoms_to_rings"}

    class Older:
        """The library as it was before this export group existed."""

        def __getattr__(self, name):
            if name in hidden:
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setenv("GAUDI_LIB", _lib.LIB_PATH)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Older())
    monkeypatch.setattr(_lib, "_lib", None)
    lib = _lib.load_library()
    assert isinstance(lib, Older) and not hasattr(lib, "gaudi_atoms_to_rings") and hasattr(lib, "gaudi_rings_to_atoms")
    monkeypatch.delenv("GAUDI_LIB")
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(AttributeError):  # and outside the diagnostic mode a missing entry point is an error
        _lib.load_library()


def test_ring_tables_carry_the_radii():
    from gaudi_amd.analyze import ring_tables
    from gaudi_amd.goa2gor import c_perception_tables
    radii = ring_tables()["goa"]["cov_radii"]
    assert set(radii) == {"H", "B", "C", "N", "O", "S"} and radii["C"] == 0.76 and radii["S"] == 1.05
    t = c_perception_tables("hetro")
    assert (t.n_elems, t.n_types, t.h_elem, t.c_elem, t.b_elem) == (6, 12, 0, 1, 2) and t.ring_size[11] == 0
    assert t.dhdb_type == 8 and t.db_type == 9 and [t.no_orientation[i] for i in (0, 10)] == [1, 1]
    c = c_perception_tables("cata")
    assert (c.n_elems, c.n_types, c.b_elem, c.db_type, c.dhdb_type) == (2, 1, -1, -1, -1)
