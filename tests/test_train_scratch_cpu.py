"""The chunk scratch of the two training passes, on the CPU: the host code counts the floats one molecule takes with the same
list that hands out the pointers (csrc/train_host.inc: Carver; pt_carve / et_carve), and gaudi_host_train_floats_per_mol returns
that count.  Here it is held to the polynomials of tests/train_shapes.py, which are written independently of the list, at every
case of the table: an array added to the list and not to the restatement (or the reverse) fails here, before a device runs."""
import ctypes as C

import pytest

from tests import train_shapes as TS


def _count(lib, *shape):
    out = C.c_int64(-1)
    assert lib.gaudi_host_train_floats_per_mol(*shape, C.byref(out)) == 0
    return out.value


def _lib():
    from gaudi_amd import _lib, build
    build.build()
    return _lib.load_library()


@pytest.mark.parametrize("name", list(TS.BY_NAME))
def test_carver_count_matches_the_restated_formula(name):
    case = TS.BY_NAME[name]
    net, N, H, L, S, F, K, A = TS.shape_of(case)
    got = _count(_lib(), net, N, H, L, S, F, K, A)
    assert got == TS.floats_per_mol(case)
    # against the polynomials the two host files kept by hand before the carver counted
    if case.net == "pred":  # ... less one [N][H] and one [N][4] array: the running gradient went between two buffers then
        E = N * N
        before = (L + 1) * N * (H + 4) + N * (F + 1) + E + 10 * N * H + 8 * N + N * K + 8 * E * H + 8 * E + 6 * E
        assert got == before - (N * H + 4 * N)
        assert TS.pt_floats_per_mol_two_buffers(N, H, L, F + 1, K) == before
    else:
        E, F1, D = N * N, F + 1, 3 + F
        before = ((L * (S + 1) + 1) * N * H + (L + 1) * N * 4 + N * F1 + N * D + E * (A // 2) + E * A + 8 * E + 2 * E + 9 * N * H
                  + 4 * N + N * F1 + 6 * E * H + 5 * E)
        assert got == before


def test_count_refuses_bad_arguments_and_ignores_what_a_network_does_not_have():
    lib = _lib()
    out = C.c_int64(0)
    assert lib.gaudi_host_train_floats_per_mol(2, 5, 32, 2, 1, 3, 5, 2, C.byref(out)) != 0
    assert lib.gaudi_host_train_floats_per_mol(0, 0, 32, 2, 1, 3, 5, 2, C.byref(out)) != 0
    assert lib.gaudi_host_train_floats_per_mol(1, 5, 32, 2, 1, 3, 5, 2, None) != 0
    assert _count(lib, 0, 11, 36, 2, 1, 3, 5, 2) == _count(lib, 0, 11, 36, 2, 4, 3, 5, 24)  # the predictor has no S, and A = 2
    assert _count(lib, 1, 11, 32, 2, 1, 3, 5, 2) == _count(lib, 1, 11, 32, 2, 1, 3, 1, 2)    # the EDM has no K
    assert _count(lib, 1, 11, 32, 2, 1, 3, 5, 24) > _count(lib, 1, 11, 32, 2, 1, 3, 5, 2)
