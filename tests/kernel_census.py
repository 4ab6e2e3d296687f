"""The census of the kernel table: every instantiation of sampler_kernel_v<V, HPE, HPP, VT> that a kern*_*.hip registers
(csrc/kernel_table.h) is either launched by a case of CASES -- which says exactly which keys its calls run -- or listed in LEFT_OUT
with the reason no input reaches it.  tests/test_kernel_census_cpu.py holds the two against gaudi_host_kernel_keys (no device);
tests/test_gpu_kernel_census.py runs every case against the float64 oracle and asserts the keys it launched.

A case is one engine: environment switches (read at gaudi_create), the two architectures, three molecules of mixed size, and the
calls below.  Which key a call reaches is read from plan_kernel / launch / stage_graph8 / stage_graph (csrc/gaudi_hip.hip):

  phi, unguided step       (HPE, 0)          form `edm`
  predictor_grad           (0, HPP, VT=0)    form `pred`
  guided step              (HPE, HPP, VT=0)  form `fused`; a two-launch plan (a pair of forms): (HPE, 0) + (0, HPP, VT=0)
  step_target (affine)     (HPE, HPP, VT=1)  form `target` (default: `fused`); two launches: (HPE, 0) + (0, HPP, VT=1)
  sample (the PG case)     (HPE, HPP, VT=0)  form `fused`: only a sampling call packs molecules into wide groups

A new entry<...>() line fails the CPU census until a case here claims its key ("The kernel census")."""
from collections import namedtuple

WIDTHS = (32, 48, 64, 128, 192, 208, 256)  # gaudi_hip.hip: round_hidden


def padded(nf):
    return next(w for w in WIDTHS if w >= nf)


def key(form, hpe, hpp, vt=0):
    f = dict(waves=8, sp=0, mr=0, gn=0, fr=0, pg=0, n1=0, ef=2)
    f.update(form)
    if not hpe:
        f["ef"] = 2  # (a predictor-only launch has no sin_embedding)
    return (f"waves={f['waves']} SP={f['sp']} MR={f['mr']} GN={f['gn']} FR={f['fr']} PG={f['pg']} N1={f['n1']} EF={f['ef']} "
            f"HPE={hpe} HPP={hpp} VT={vt}")


# the forms (sampler_kernel.h: V4T / V8T)
V4, V4G, V4S, V4GS = dict(waves=4), dict(waves=4, gn=1), dict(waves=4, ef=24), dict(waves=4, gn=1, ef=24)
V8, V8S, V8H = dict(sp=0), dict(sp=1), dict(sp=2)                        # resident: fp32 instructions, full ring, half ring
MR0, MR1, MR2 = dict(sp=0, mr=1), dict(sp=1, mr=1), dict(sp=2, mr=1)     # several rounds of edge tiles
GN1, GN2 = dict(sp=1, mr=1, gn=1), dict(sp=1, mr=1, gn=2)                # node buffers global: all of them, all but P / Q
FR, N1, PG = dict(sp=1, fr=1), dict(sp=1, n1=1), dict(sp=1, mr=1, pg=1)

Case = namedtuple("Case", "name env edm pred dataset sizes mask calls keys")

CALLS = ("phi", "pgrad", "guided", "unguided", "target")


def case(name, env, nf_e, nf_p, sizes, edm, pred, fused, target=None, mask=0, dataset="cata", layers=(2, 2), sin=False,
         calls=CALLS):
    """sizes: live nodes per molecule (hetro: rings; a molecule then has twice as many nodes).  mask: 0 = fully connected, k > 0 =
    every node tied to its k neighbours on either side of a cycle (a sparse, symmetric, legal edge mask).  edm / pred / fused /
    target: the forms the calls must reach; a pair of forms = a guided step of two launches."""
    hpe, hpp = padded(nf_e), padded(nf_p)
    target = fused if target is None else target
    keys = set()
    if "phi" in calls or "unguided" in calls:
        keys.add(key(edm, hpe, 0))
    if "pgrad" in calls:
        keys.add(key(pred, 0, hpp))
    for call, form, vt in (("guided", fused, 0), ("sample", fused, 0), ("target", target, 1)):
        if call in calls:
            keys |= {key(form[0], hpe, 0), key(form[1], 0, hpp, vt)} if isinstance(form, tuple) else {key(form, hpe, hpp, vt)}
    e = dict(nf=nf_e, n_layers=layers[0], dataset=dataset)
    if sin:
        e["sin_embedding"] = True
    p = dict(nf=nf_p, n_layers=layers[1], dataset=dataset)
    assert len(sizes) == 3 and min(sizes) <= 3
    return Case(name, dict(env), e, p, dataset, tuple(sizes), mask, tuple(calls), frozenset(keys))


W4, GN4 = {"GAUDI_WAVES": 4}, {"GAUDI_FORCE_GN": 1}
F32 = {"GAUDI_EDGE_MATH": "fp32"}
G8, G8A = {"GAUDI_FORCE_GN8": 1}, {"GAUDI_FORCE_GN8": 1, "GAUDI_GN8_PQ": 0}

# (nf of the denoiser, nf of the predictor) per padded width pair: never the padded width itself where a smaller nf exists in the
# suite, so the padding and the tail blocks run -- 244 -> 256 and 196 -> 208 are the one-k-step tails (has_ktail), 200 has four
TINY_PAIRS = {"32_48": (32, 36), "32_32": (20, 32), "48_48": (40, 48), "64_64": (60, 64)}

CASES = []

# ---- the 4-wave family (GAUDI_WAVES=4): every fused pair with its denoiser-only and predictor-only kernels
for tag, (ne, np_), sizes, ds in (("32_48", TINY_PAIRS["32_48"], [5, 1, 3], "hetro"), ("32_32", TINY_PAIRS["32_32"], [11, 3, 7], "cata"),
                                  ("48_48", TINY_PAIRS["48_48"], [11, 2, 8], "cata"), ("64_64", TINY_PAIRS["64_64"], [6, 1, 4], "hetro"),
                                  ("128_128", (120, 120), [11, 3, 7], "cata"), ("192_192", (180, 180), [11, 3, 9], "cata"),
                                  ("192_208", (192, 196), [11, 3, 7], "cata"), ("208_208", (200, 200), [11, 1, 6], "cata"),
                                  ("256_256", (250, 250), [11, 3, 7], "cata")):
    CASES.append(case("w4_" + tag, W4, ne, np_, sizes, V4, V4, V4, dataset=ds))

# ---- sin_embedding denoisers (4-wave kernels whatever the family): fused at two width pairs, two launches everywhere else -- the
# second launch is the ordinary 4-wave predictor-only kernel, and the only caller of its VT twin
for tag, (ne, np_), sizes, ds in (("32_48", (32, 36), [11, 3, 7], "cata"), ("192_208", (192, 196), [5, 1, 3], "hetro")):
    CASES.append(case("se_" + tag, W4, ne, np_, sizes, V4S, V4, V4S, dataset=ds, sin=True))
for tag, (ne, np_), sizes, ds in (("32_32", (20, 20), [11, 3, 7], "cata"), ("48_48", (40, 40), [5, 1, 3], "hetro"),
                                  ("64_64", (60, 60), [11, 2, 8], "cata"), ("128_128", (120, 120), [11, 3, 7], "cata"),
                                  ("192_192", (180, 180), [11, 3, 7], "cata"), ("208_208", (200, 200), [11, 3, 7], "cata"),
                                  ("256_256", (250, 250), [11, 3, 7], "cata")):
    CASES.append(case("se2_" + tag, W4, ne, np_, sizes, V4S, V4, (V4S, V4), dataset=ds, sin=True))

# ---- 4 waves, node buffers in global memory (GAUDI_FORCE_GN=1): no fused kernel, a guided step is always two launches
for tag, (ne, np_), sizes, ds, sin in (("32_48", (32, 36), [11, 3, 7], "cata", False), ("192_208", (192, 196), [5, 1, 3], "hetro", False),
                                       ("se_32_48", (32, 36), [5, 1, 3], "hetro", True), ("se_192_208", (192, 196), [11, 3, 7], "cata", True)):
    CASES.append(case("gn4_" + tag, GN4, ne, np_, sizes, V4GS if sin else V4G, V4G, (V4GS if sin else V4G, V4G), dataset=ds, sin=sin))

# ---- 8 waves, the default configuration (192 / 196 features, 9 / 12 layers): 11 nodes take the N1 kernels; the value target has
# no N1 twin and the predictor-only launch no N1 form, both run the plain full-ring kernel
CASES.append(case("default_n11", {}, 192, 196, [11, 3, 7], N1, V8S, N1, target=V8S, layers=(9, 12)))
# 16 node slots: the last size of one column tile; GAUDI_NO_N1 keeps the plain kernel (180 features: padding at 192)
CASES.append(case("plain_n11", {"GAUDI_NO_N1": 1}, 180, 196, [11, 3, 7], V8S, V8S, V8S))
CASES.append(case("n1_n16_sparse", {}, 192, 196, [16, 3, 12], N1, V8S, N1, target=V8S, mask=2))
# 17 node slots on at most 128 edge slots: two column tiles, the FR kernels (predictor-only: no FR form)
CASES.append(case("fr_n17_sparse", {}, 192, 196, [17, 3, 12], FR, V8S, FR, mask=1))
# ... and GAUDI_NO_FR keeps the plain kernel at two column tiles
CASES.append(case("plain_n17_sparse", {"GAUDI_NO_FR": 1}, 192, 196, [17, 3, 12], V8S, V8S, V8S, mask=1))
# a fully connected molecule of 12 nodes has 132 edges: the launches that run the predictor take the multi-round kernels
CASES.append(case("mr_n12", {}, 192, 196, [12, 3, 9], N1, MR1, MR1))
# 22 fully connected nodes: five node buffers leave no room for the full ring
CASES.append(case("half_n22", {}, 192, 196, [22, 3, 15], V8H, MR2, MR2))
# ... and 24 nodes on a sparse mask of one round: the resident half-ring kernel (the denoiser alone still fits the full ring;
# the predictor alone has no resident half-ring kernel and runs on fp32 instructions)
CASES.append(case("half_n24_sparse", {}, 192, 196, [24, 3, 15], FR, V8, V8H, mask=2))
# 23 fully connected nodes fit no resident plan with the predictor: without any switch those launches keep three of the five node
# buffers in global memory (the denoiser alone still fits the half ring)
CASES.append(case("gn8_unforced_n23", {}, 192, 196, [23, 3, 14], V8H, GN2, GN2))

# ---- 8 waves at the small widths: full ring, FR, rounds
for tag, (ne, np_) in TINY_PAIRS.items():
    ds, sizes = ("hetro", [5, 1, 3]) if tag in ("32_48", "64_64") else ("cata", [11, 3, 7])
    CASES.append(case("tiny_" + tag, {}, ne, np_, sizes, V8S, V8S, V8S, dataset=ds))
    CASES.append(case("tiny_mr_" + tag, {}, ne, np_, [12, 3, 9], V8S, MR1, MR1))
for tag in ("32_48", "64_64"):
    CASES.append(case("tiny_fr_" + tag, {}, *TINY_PAIRS[tag], [17, 2, 12], V8S, V8S, FR, mask=1))

# ---- 8 waves at the widths that have fp32-instruction fused kernels only (the denoiser-only / predictor-only launches take the
# full-ring kernels where those exist: 128 both, 192 the denoiser, 208 the predictor)
CASES.append(case("w8_128_128", {}, 120, 120, [11, 3, 7], V8S, V8S, V8))
CASES.append(case("w8_192_192", {}, 180, 180, [11, 3, 7], N1, V8, V8))
CASES.append(case("w8_208_208", {}, 200, 200, [11, 3, 7], V8, V8S, V8))
CASES.append(case("w8_256_256", {}, 250, 250, [11, 3, 7], V8, V8, V8))
CASES.append(case("w8_256_256_ktail", {}, 244, 244, [5, 1, 3], V8, V8, V8, dataset="hetro"))

# ---- 8 waves, fp32 instructions everywhere (GAUDI_EDGE_MATH=fp32)
for tag, (ne, np_) in dict(TINY_PAIRS, **{"128_128": (120, 120), "192_208": (180, 200)}).items():
    ds, sizes = ("hetro", [5, 1, 3]) if tag in ("32_32", "48_48") else ("cata", [11, 3, 7])
    CASES.append(case("fp32_" + tag, F32, ne, np_, sizes, V8, V8, V8, dataset=ds))
    if tag != "128_128":  # (no multi-round kernel at 128)
        CASES.append(case("fp32_mr_" + tag, F32, ne, np_, [12, 3, 9], V8, MR0, MR0))

# ---- 8 waves, node buffers in global memory (GAUDI_FORCE_GN8=1): 18 nodes = two column tiles, rounds of edge tiles
CASES.append(case("gn8pq_32_48", G8, 32, 36, [18, 3, 11], GN2, GN2, GN2))
CASES.append(case("gn8pq_192_208", G8, 192, 196, [18, 3, 11], GN2, GN2, GN2))
for tag, (ne, np_) in dict(TINY_PAIRS, **{"192_208": (180, 200)}).items():
    ds, sizes = ("hetro", [9, 1, 5]) if tag == "48_48" else ("cata", [18, 3, 11])
    CASES.append(case("gn8_" + tag, G8A, ne, np_, sizes, GN1, GN1, GN1, dataset=ds))

# ---- wide groups (GAUDI_PAIRS=2): two 11-node molecules share a workgroup of 22 node slots on the full ring, the predictor's
# fifth node buffer in global memory -- a sampling call (only those pack), a chain of three steps
CASES.append(case("pg_pairs", {"GAUDI_PAIRS": 2}, 192, 196, [11, 11, 3], None, None, PG, calls=("sample",)))


def _hpp0_vt1(form, widths):
    return {key(form, 0, w, 1): "8 waves: run_chain (the only place a value target is attached) launches (HPE, HPP) in one piece; "
            "the (0, HPP) launch of a two-launch plan exists in stage_graph's 4-wave plans only (plan.two), and "
            "gaudi_predictor_grad carries no value target" for w in widths}


_HALF_TINY = ("plan_for (stage_graph8) tries the half ring only after the full ring was refused; every full-ring twin of these kernels "
              "is registered (V8S fused, V8T<1,true> fused and 0/HPP: have_kernel8 cannot be the refusal) and node_f16_fits admits "
              "the full ring at 32 / 48 / 64 for every N <= 32 (nh_split_floats of one or two column tiles is at most the ring's "
              "free half, with equality at 48 and 64 on two tiles -- a larger nh_split_floats or a removed twin would change "
              "this), which leaves plan_pub8; with a predictor the room "
              "plan_pub8 leaves the publish buffer does not depend on the ring (own and base both hold it), so the refusal must be "
              "base > cap, i.e. cap - base(half) < 2048 floats at widths <= 64 -- then fewer than 8448 floats / 20 per edge slot "
              "allow pub_ch >= 1, S <= 422, where base is far below cap for the <= 32 node slots node_f16_fits admits")

LEFT_OUT = {}
# a value target on a predictor-only 8-wave launch: no caller
for form, widths in ((V8, (32, 48, 64, 128, 192, 208, 256)), (V8S, (32, 48, 64, 128, 208)), (MR0, (32, 48, 64, 208)),
                     (MR1, (32, 48, 64, 208)), (MR2, (32, 48, 64, 208)), (GN1, (32, 48, 64, 208)), (GN2, (48, 208))):
    LEFT_OUT.update(_hpp0_vt1(form, widths))
# the half ring at the small widths: the full ring always fits
for hpe, hpp in ((32, 48), (32, 32), (48, 48), (64, 64)):
    for vt in (0, 1):
        LEFT_OUT[key(V8H, hpe, hpp, vt)] = _HALF_TINY
        LEFT_OUT[key(MR2, hpe, hpp, vt)] = _HALF_TINY
for hpp in (32, 48, 64):
    LEFT_OUT[key(MR2, 0, hpp, 0)] = _HALF_TINY
    LEFT_OUT[key(MR2, 0, hpp, 1)] += "; and " + _HALF_TINY
LEFT_OUT[key(PG, 32, 48)] = ("stage_graph8 takes the PG kernel only for a wide group whose resident plan is the half ring "
                             "(p2.mode == 2), which no launch at these widths is: " + _HALF_TINY)
