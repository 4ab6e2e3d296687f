"""The PPP SCF with Pulay's DIIS on the device (csrc/ppp_scf.inc): gaudi_ppp_scf against the kernel's host build, bit for bit in all
twenty-five outputs, the doubles included -- the small rows, the first 32 molecules of g30 under the four state kinds in ONE mixed
call, the 126- to 128-centre rows against the host build's record, a call that splits into more than one launch at the 128 tier (with
the default and with the longest history), run to run.  What the outputs must satisfy is checked on the host build by
tests/test_ppp_scf_cpu.py; equality with it carries that over."""
import numpy as np
import pytest

from gaudi_amd import _lib
from tests.ppp_helpers import BAD_INPUT, NOT_CONVERGED, OK, benzene, edge_molecule, naphthalene
from tests.ppp_open_helpers import g30_rows, small_rows
from tests.ppp_scf_helpers import assert_same_bits, device, host, hosts, long_host, long_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from gaudi_amd.engine import Engine
    return Engine.default()


def mixed_rows():
    mols, charge, mult, kind = g30_rows()
    return mols[:128], charge[:128], mult[:128], kind[:128]


def test_the_small_rows(engine):
    mols, charge, mult, _ = small_rows()
    dev = device(engine, mols, charge, mult)
    assert_same_bits(dev, hosts("small", small_rows()))
    assert (dev["status"] == OK).all() and dev["n_extrapolated"].max() >= 5 and dev["diis_error"].dtype == np.float32


def test_thirty_two_of_g30_under_the_four_state_kinds_in_one_mixed_call(engine):
    mols, charge, mult, _ = mixed_rows()
    dev = device(engine, mols, charge, mult)
    assert_same_bits(dev, hosts("g30 mixed", mixed_rows()))
    assert np.bincount(dev["n_open"], minlength=3).tolist() == [32, 64, 32] and (dev["status"] <= NOT_CONVERGED).all()
    assert dev["n_extrapolated"].min() <= 4 and dev["n_extrapolated"].max() >= 10  # short and long histories in one launch
    again = device(engine, mols, charge, mult)  # run to run
    assert_same_bits(again, dev)


def test_the_long_rows(engine):
    """126, 127 and 128 centres with one electron removed: against the host build's recorded results
    (tests/golden/ppp_scf_long_jobs.npz, which tests/test_ppp_scf_cpu.py holds to the live host build)."""
    mols, charge, mult, _ = long_rows()
    dev = device(engine, mols, charge, mult)
    assert_same_bits(dev, long_host())
    assert dev["n_pi"].tolist() == [126, 127, 128]


@pytest.mark.parametrize("diis_size", [6, 8])
def test_a_call_that_splits_into_launches_at_the_largest_tier(engine, diis_size):
    """700 rows of one 128-centre molecule (the tier-edge one, a zig-zag chain of 31 fused rings with a two-carbon tail, one electron
    removed: it is at rest after 12 iterations, where a polyene chain of 128 carbons runs all 64): 630 rows of the default history
    (481 of the longest) fill 512 MiB of scratch, so the tier runs as two launches that share it.  Every row has the bits of a
    one-row call."""
    mol, q = edge_molecule(128)
    engine.profile_reset(True)
    alone = device(engine, [mol], [q + 1], [0], diis_size=diis_size)
    assert engine.ppp_scf_profile_get()[0] == 1 and alone["n_pi"][0] == 128 and alone["status"][0] == OK
    dev = device(engine, [mol] * 700, [q + 1] * 700, [0] * 700, diis_size=diis_size)
    assert engine.ppp_scf_profile_get()[0] == 3
    engine.profile_reset(False)
    for name in _lib.PPP_SCF_ARRAYS:
        want = np.broadcast_to(alone[name], dev[name].shape)
        assert dev[name].tobytes() == np.ascontiguousarray(want).tobytes(), name


def test_refused_settings_and_the_other_settings(engine):
    two, q, s = [naphthalene(), benzene()], [1, 0], [2, 3]
    for kw in ({"diis_size": 0}, {"diis_size": 9}, {"diis_start": 1}):
        out = device(engine, two, q, s, **kw)
        assert out["status"].tolist() == [BAD_INPUT] * 2 and not out["levels"].any(), kw
        assert_same_bits(out, host(two, q, s, **kw))
    for kw in ({"diis_size": 2}, {"diis_start": 2}, {"diis_start": 5, "repulsion": 1}):
        assert_same_bits(device(engine, two, q, s, **kw), host(two, q, s, **kw))
