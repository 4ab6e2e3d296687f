"""Circular count fingerprints and nearest-neighbour similarity (csrc/fp.inc) through the HOST builds,
gaudi_host_circular_fingerprint and gaudi_host_fp_nearest: the fingerprint equals a Python restatement of its definition, does
not depend on the numbering nor on placed hydrogens, separates exactly the isomorphism classes of g32 at radius 2, carries the
statuses and saturates; the nearest rows are numpy's by the total order; and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import C as C_ELEM, H, fixture, pack, relabel
from tests.canonical_helpers import N_ELEMS, strip_implied_hydrogens
from tests.gor2goa_helpers import unpack
from tests.similarity_helpers import (BAD_INPUT, EMPTY, OK, OVERFLOW, g32_fingerprints, g32_keys, host_fp, numpy_nearest,
                                      restated_counts, restated_fingerprint, stars)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gaudi_circular_fingerprint", "gaudi_host_circular_fingerprint", "gaudi_fp_library_set", "gaudi_fp_nearest",
       "gaudi_fp_common", "gaudi_host_fp_nearest", "gaudi_fp_profile_get")


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def ordinary(g32):
    """The molecules of g32 that have a fingerprint: all but the three refused specials."""
    st = g32_fingerprints()["status"]
    mols = [m for m in g32[1] if st[m["index"]] == OK]
    assert len(mols) == 504
    return mols


@pytest.mark.parametrize("radius,n_bins", [(0, 256), (2, 1024), (3, 512)])
def test_host_build_equals_the_restatement(ordinary, radius, n_bins):
    out = host_fp(ordinary, radius, n_bins)
    assert (out["status"] == OK).all() and out["fp"].shape == (len(ordinary), n_bins) and out["fp"].dtype == np.uint8
    for i, m in enumerate(ordinary):
        row, total = restated_fingerprint(m["elem"], m["bonds"], radius, n_bins)
        assert np.array_equal(out["fp"][i], row), (i, radius, n_bins)
        assert out["total"][i] == total == int(out["fp"][i].astype(np.int64).sum())
    heavy = np.array([(m["elem"] != H).sum() for m in ordinary])
    assert np.array_equal(out["total"], heavy * (radius + 1))  # nothing saturates in the fixture: every feature is counted


def test_renumbering_changes_nothing(ordinary):
    rng = np.random.default_rng(3501)
    mols = ordinary[::7][:64]
    assert len(mols) == 64
    a, b = host_fp(mols), host_fp([relabel(m, rng) for m in mols])
    assert np.array_equal(a["fp"], b["fp"]) and np.array_equal(a["total"], b["total"]) and (b["status"] == OK).all()


def test_placed_hydrogens_change_nothing(ordinary):
    stripped = [strip_implied_hydrogens(m["elem"], m["bonds"]) for m in ordinary]
    assert sum(n for _, _, n in stripped) > 1000
    a, b = host_fp(ordinary), host_fp([(e, bd) for e, bd, _ in stripped])
    assert np.array_equal(a["fp"], b["fp"]) and np.array_equal(a["total"], b["total"])


def test_isomorphic_molecules_of_g30_get_the_same_row(golden):
    """g30 on the atoms and bonds the reference built, through the layer on top: the 160 molecules fall into 128 isomorphism
    classes, and within a class -- the same molecule sampled twice, with another atom numbering -- the row is the same.  (A
    molecule's twin is given as rings, and only the device builds atoms from rings: tests/test_gpu_similarity.py has that.)"""
    from gaudi_amd.similarity import fingerprints
    from tests.similarity_helpers import HostEngine
    mols = [m for m in unpack(golden("g30_gor2goa")) if not m["threw"]]
    pairs = [(m["ref_types"].astype(np.int32), m["ref_bonds"].astype(np.int32)) for m in mols]
    by_class, by_row = {}, {}
    out = fingerprints(pairs, "hetro", engine=HostEngine())  # (the element list of "cata" is a prefix of this one)
    assert (out["status"] == OK).all() and len(mols) == 160
    for m, row in zip(mols, out["fp"]):
        by_class.setdefault(m["iso_class"], set()).add(row.tobytes())
        by_row.setdefault(row.tobytes(), set()).add(m["iso_class"])
    assert all(len(v) == 1 for v in by_class.values()) and len(by_class) == 128
    assert all(len(v) == 1 for v in by_row.values())
    # an unbuilt record gives EMPTY and a zero row
    rec = fingerprints([dict(status=3, atom_types=np.zeros(0, np.int64), bonds=np.zeros((0, 2), np.int64)), pairs[0]], "hetro",
                       engine=HostEngine())
    assert rec["status"].tolist() == [EMPTY, OK] and not rec["fp"][0].any() and np.array_equal(rec["fp"][1], out["fp"][0])


@pytest.mark.parametrize("n_bins", [256, 1024])
def test_rows_separate_exactly_the_isomorphism_classes(g32, n_bins):
    fp, keys = g32_fingerprints(2, n_bins), g32_keys()
    by_key, by_row = {}, {}
    for m in g32[1]:
        k = keys[m["index"]]
        if k is None:
            continue
        row = fp["fp"][m["index"]].tobytes()
        by_key.setdefault(k, set()).add(row)
        by_row.setdefault(row, set()).add(k)
    assert len(by_key) == 432
    assert all(len(v) == 1 for v in by_key.values())  # equal keys, equal rows
    assert all(len(v) == 1 for v in by_row.values()) and len(by_row) == 432  # different keys, different rows


def test_statuses_and_saturation(g32):
    out = g32_fingerprints()
    seen = set()
    for m in g32[1]:
        want = {5: BAD_INPUT, 6: OVERFLOW, 7: EMPTY}.get(m["special"])
        if want is not None:
            i = m["index"]
            assert out["status"][i] == want and not out["fp"][i].any() and out["total"][i] == 0
            seen.add(want)
    assert seen == {BAD_INPUT, OVERFLOW, EMPTY}
    e, b = stars()
    raw = restated_counts(e, b, 3, 256)
    assert raw.max() == 304  # more than 255 equal-bin features: two of the leaves' ids share a bin
    sat = host_fp([(e, b), g32[1][0]], 3, 256)
    assert sat["status"][0] == OK and sat["fp"][0].max() == 255 and np.array_equal(sat["fp"][0], np.minimum(raw, 255))
    assert sat["total"][0] == int(np.minimum(raw, 255).sum()) == raw.sum() - 49


def _same(out, ref):
    for name, a in zip(("idx", "common", "union"), ref):
        assert out[name].dtype == np.int32 and np.array_equal(out[name], a), name


def test_nearest_on_g32_against_numpy():
    fp = g32_fingerprints()["fp"]  # queries and library alike, the three zero rows of the refused specials inside
    out = _lib.host_fp_nearest(fp, fp, 3)
    _same(out, numpy_nearest(fp, fp, 3))
    built = g32_fingerprints()["status"] == OK
    assert (out["common"][built, 0] == out["union"][built, 0]).all()  # similarity 1 with itself or an earlier isomer
    ties = sum(out["common"][b, 1] * out["union"][b, 2] == out["common"][b, 2] * out["union"][b, 1] for b in np.nonzero(built)[0])
    assert ties > 0  # the fixture itself exercises the tie rule


def test_nearest_edge_cases():
    fp = np.array(g32_fingerprints(2, 256)["fp"])
    rows = fp[g32_fingerprints(2, 256)["status"] == OK]
    rows = rows[np.sort(np.unique(rows, axis=0, return_index=True)[1])]  # one row per isomorphism class, in fixture order
    assert len(rows) == 432
    # duplicated rows: the lower index wins
    lib = np.concatenate([rows[:20], rows[:20], rows[5:6]])
    out = _lib.host_fp_nearest(rows[:20], lib, 4)
    _same(out, numpy_nearest(rows[:20], lib, 4))
    assert out["idx"][:, 0].tolist() == list(range(20)) and out["idx"][5, :3].tolist() == [5, 25, 40]
    # k = 16 > M = 5
    out = _lib.host_fp_nearest(rows[:7], rows[30:35], 16)
    _same(out, numpy_nearest(rows[:7], rows[30:35], 16))
    assert (out["idx"][:, 5:] == -1).all() and not out["common"][:, 5:].any() and not out["union"][:, 5:].any()
    assert sorted(out["idx"][0, :5].tolist()) == [0, 1, 2, 3, 4]
    # an all-zero query: every similarity is 0, the rows come in index order
    zero = np.zeros((1, 256), np.uint8)
    out = _lib.host_fp_nearest(zero, rows[:6], 3)
    _same(out, numpy_nearest(zero, rows[:6], 3))
    assert out["idx"].tolist() == [[0, 1, 2]] and not out["common"].any()
    # an all-zero library row: behind every row that shares something, ahead of nothing but the padding
    lib = np.concatenate([zero, rows[:3], zero])
    out = _lib.host_fp_nearest(np.concatenate([rows[:2], zero]), lib, 5)
    _same(out, numpy_nearest(np.concatenate([rows[:2], zero]), lib, 5))
    assert out["idx"][0, 3:].tolist() == [0, 4] and out["idx"][2].tolist() == [0, 1, 2, 3, 4] and out["union"][2, 0] == 0
    # M = 1 and B = 1
    out = _lib.host_fp_nearest(rows[3:4], rows[9:10], 2)
    _same(out, numpy_nearest(rows[3:4], rows[9:10], 2))
    assert out["idx"].tolist() == [[0, -1]]


def test_declarations_and_argument_checks():
    header = open(os.path.join(ROOT, "include", "gaudi_hip.h")).read()
    assert "#define GAUDI_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7 and _lib.load_library().gaudi_abi_version() == 7
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(_lib.EXPORTS[name][1]) == m.group(1).count(",") + 1, name
        assert header.index("(Entry points ADDED since") < header.index(name) < header.index("#define GAUDI_ABI_VERSION")
    assert _lib.EXPORTS["gaudi_fp_nearest"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, _lib.U8P, C.c_int, _lib.U8P, C.c_int,
                                                          _lib.IP, _lib.IP, _lib.IP])
    lib = _lib.load_library()
    elem, na, bonds, nb = pack([fixture()[1][0]])
    ok = _lib.fp_outputs(1, 1024)
    for radius, n_bins in ((4, 1024), (-1, 1024), (2, 128), (2, 2048), (2, 1000)):
        args = _lib.fp_args(N_ELEMS, H, C_ELEM, elem, na, bonds, nb, radius, n_bins, ok)
        assert lib.gaudi_host_circular_fingerprint(*args) == -1, (radius, n_bins)  # GAUDI_E_INVALID
    q = np.zeros((2, 256), np.uint8)
    out = _lib.nearest_outputs(2, 16)
    ptrs = [out[n].ctypes.data_as(_lib.IP) for n in ("idx", "common", "union")]
    u8 = lambda a: a.ctypes.data_as(_lib.U8P)
    assert lib.gaudi_host_fp_nearest(256, 2, u8(q), 2, u8(q), 16, *ptrs) == 0
    for k in (0, 17, -1):
        assert lib.gaudi_host_fp_nearest(256, 2, u8(q), 2, u8(q), k, *ptrs) == -1
    assert lib.gaudi_host_fp_nearest(128, 2, u8(q), 2, u8(q), 1, *ptrs) == -1
    assert lib.gaudi_host_fp_nearest(256, 2, u8(q), 0, u8(q), 1, *ptrs) == -1
