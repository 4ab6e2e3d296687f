"""The kernel table against the census (tests/kernel_census.py), without a device: every registered instantiation is claimed by a
case that launches it on the GPU (tests/test_gpu_kernel_census.py) or is listed, with its reason, as unreachable."""
import re

from tests import kernel_census as KC

KEY = re.compile(r"waves=(4|8) SP=[012] MR=[01] GN=[012] FR=[01] PG=[01] N1=[01] EF=(2|24) HPE=\d+ HPP=\d+ VT=[01]")


def _registered():
    from gaudi_amd import _lib, build
    build.build()
    return _lib.registered_kernel_keys()


def _claimed():
    return set().union(*(c.keys for c in KC.CASES))


def test_every_registered_kernel_has_a_case_or_a_reason():
    reg = _registered()
    assert len(reg) == len(set(reg)) > 0 and all(KEY.fullmatch(k) for k in reg), "a duplicate or malformed key"
    missing = sorted(set(reg) - _claimed() - set(KC.LEFT_OUT))
    assert not missing, "kernel-table entries no census case launches (add a case to tests/kernel_census.py):\n" + "\n".join(missing)


def test_no_key_is_both_covered_and_left_out():
    both = sorted(_claimed() & set(KC.LEFT_OUT))
    assert not both, both


def test_no_case_or_reason_names_a_kernel_that_is_not_registered():
    reg = set(_registered())
    for c in KC.CASES:
        assert c.keys and c.keys <= reg, (c.name, sorted(c.keys - reg))
    assert set(KC.LEFT_OUT) <= reg, sorted(set(KC.LEFT_OUT) - reg)


def test_left_out_stays_within_what_may_be_left_out():
    """Only 8-wave kernels below a padded width of 128 whose reason is written down, or 8-wave predictor-only value-target twins
    (which have no caller at any width): never a 4-wave kernel, never a fused or denoiser-only kernel of width 128 or more."""
    for k, why in KC.LEFT_OUT.items():
        f = dict(kv.split("=") for kv in k.split())
        assert f["waves"] == "8" and len(why) > 40, k
        no_caller = f["HPE"] == "0" and f["VT"] == "1"
        assert no_caller or max(int(f["HPE"]), int(f["HPP"])) < 128, k
    half_tiny = [k for k in KC.LEFT_OUT if not (" HPE=0 " in k and k.endswith("VT=1"))]
    assert len(half_tiny) <= 23 - 3  # (three of the issue's 23 are predictor-only VT twins, counted with those)


def test_case_names_are_unique_and_shapes_are_the_census_shapes():
    names = [c.name for c in KC.CASES]
    assert len(names) == len(set(names))
    for c in KC.CASES:
        assert len(c.sizes) == 3 and min(c.sizes) * (2 if c.dataset == "hetro" else 1) <= 3, c.name
        assert set(c.env) <= {"GAUDI_WAVES", "GAUDI_FORCE_GN", "GAUDI_EDGE_MATH", "GAUDI_FORCE_GN8", "GAUDI_GN8_PQ", "GAUDI_PAIRS",
                              "GAUDI_NO_N1", "GAUDI_NO_FR"}, c.name
    assert {c.dataset for c in KC.CASES} == {"cata", "hetro"}


def test_every_left_out_half_ring_kernel_has_its_full_ring_twin_registered():
    """The half-ring argument of LEFT_OUT rests on the planner finding the full-ring kernel first: a removed twin would make the
    half-ring key reachable."""
    reg = set(_registered())
    half = [k for k in KC.LEFT_OUT if " SP=2 " in k]
    assert half
    for k in half:
        assert k.replace(" SP=2 ", " SP=1 ") in reg, k
