"""The shapes the two training passes (gaudi_edm_loss_grad / gaudi_predictor_loss_grad) are held to oracle/train_oracle.py at: one
table for tests/test_train_oracle_cpu.py (which checks, with the oracle alone, that every case is a meaningful comparison: a small
float32-to-float64 spread, live gradients, no saturated tanh, an L1 sign margin) and tests/test_gpu_train_shapes.py (which runs the
kernels).  DESIGN.md, "Training kernels against the autograd oracle", gives the reason for each shape.

A case is one network ('edm' or 'pred'), its overrides, the padded N, the live nodes per molecule (B = len(live)), t_int and, for
the EDM, the loss type and the per-molecule weights.  Inputs are seeded: ring-like coordinates (a random walk with bonded-length
steps, as tests/test_gpu_stability.py draws them), one-hot ring types, raw noise.  reference() evaluates a case once per process in
float64 and float32 and keeps the result."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from gaudi_amd import synth
from oracle import train_oracle as TO
from tests.helpers import rel_err

T_TINY = 50
EDM_TINY = dict(nf=32, n_layers=2, diffusion_steps=T_TINY)
PRED_TINY = dict(nf=36, n_layers=2)

PRED_NMAX = 53

Case = namedtuple("Case", "name net dataset edm pred N live t_int loss_type weight K no_edges env draw")

CASES = []


def _add(name, nets, N, live, *, edm=None, pred=None, dataset="cata", t_int=None, loss_type="l2", weight=None, K=5,
         no_edges=False, env=None, draw=0):
    """draw: which seeded draw of weights and inputs the case takes.  A draw at which some scalar gradient (an att_mlp bias, say)
    nearly cancels has a float32 oracle several times further from the float64 one than its neighbours, and by an amount that
    depends on the machine's summation order: such a draw is replaced, the bar is not."""
    for net in nets:
        e = dict(EDM_TINY, **(edm or {}))
        p = dict(PRED_TINY, **(pred or {}))
        CASES.append(Case(f"{net}_{name}", net, dataset, e, p, N, tuple(live), None if t_int is None else tuple(t_int), loss_type,
                          None if weight is None else tuple(weight), K, no_edges, env, draw))


BOTH = ("edm", "pred")
# large molecules: the aggregation of up to 127 edge messages is divided (normalization_factor), as a run at that size would set
# it; the predictor has no such switch (its agg is a plain sum).  Not by more than 10: the float32 kl_prior of 128 nodes carries
# an absolute error of about 3e-5 (one rounding of dof * sigma_T^2 = 381), which a loss well below 1 would not hide
BIG = dict(normalization_factor=10.0)

# ---- no live edge at all, and the smallest molecules (one row in all; then B = 3 each)
_add("n1_b1", BOTH, 1, [1], no_edges=True)
_add("n1_single", BOTH, 1, [1, 1, 1], no_edges=True)
_add("n1_one_live", BOTH, 5, [1, 1, 1], no_edges=True)
_add("n1_full", BOTH, 5, [5, 5, 5])
_add("n2", ("edm",), 2, [2])
_add("n2", ("pred",), 2, [2], draw=1)
# ---- the N ladder
_add("n16", BOTH, 16, [16])
_add("n17", BOTH, 17, [17, 3])
_add("n33", BOTH, 33, [33], edm=BIG)
_add("n64", ("edm",), 64, [64, 7], edm=BIG)
_add("n128", ("edm",), 128, [128, 5], edm=dict(BIG, n_layers=1))
# the predictor's forward is the sampler launch (gaudi_predict_noised): a fully connected molecule of more than PRED_NMAX nodes is
# refused there at nf 36 (its edge list no longer fits the workgroup's LDS), so the predictor's ladder ends at that size
_add("nmax", ("pred",), PRED_NMAX, [PRED_NMAX, 7])
_add("nmax_l1", ("pred",), PRED_NMAX, [PRED_NMAX, 5], pred=dict(n_layers=1), draw=2)
_add("rows", BOTH, 20, [20 - (i % 7) for i in range(64)])
# ---- widths
_add("h256", BOTH, 5, [5, 3], edm=dict(nf=256, n_layers=1), pred=dict(nf=256, n_layers=2))
_add("h250", BOTH, 5, [5, 3], edm=dict(nf=250, n_layers=1), pred=dict(nf=250, n_layers=2))
_add("h20_hetro", BOTH, 12, [12, 5], dataset="hetro", edm=dict(nf=20), pred=dict(nf=20))
# ---- depth
_add("deep", ("edm",), 11, [11, 4], edm=dict(n_layers=3, inv_sublayers=3))
_add("deep_l1", ("pred",), 11, [11, 4], pred=dict(n_layers=1))
_add("deep_l3", ("pred",), 11, [11, 4], pred=dict(n_layers=3))
# ---- switches, off the fixtures' shape
_add("plain", BOTH, 17, [17, 9], edm=dict(attention=False, tanh=False), pred=dict(attention=False, tanh=False))
_add("mean", ("edm",), 17, [17, 9], edm=dict(aggregation_method="mean"))
_add("sin", ("edm",), 17, [17, 9], edm=dict(sin_embedding=True))
_add("vlb_t", ("edm",), 17, [17, 9, 17, 12], edm=dict(diffusion_loss_type="vlb"), loss_type="vlb",
     t_int=(0, 1, T_TINY, T_TINY // 2), weight=(0.5, -1.0, 0.0, 2.0))
_add("t_k1", ("pred",), 17, [17, 9, 12], t_int=(0, T_TINY, 7), K=1)
_add("t_k5", ("pred",), 17, [17, 9, 12], t_int=(0, T_TINY, 7), K=5)
# ---- every element at the default widths
_add("default_elementwise", BOTH, 11, [11, 7, 11], edm=dict(nf=192, n_layers=2, diffusion_steps=1000), pred=dict(nf=196, n_layers=2))
# ---- several scratch chunks (2 / 2 / 1) against the oracle
_add("chunks", ("edm",), 33, [33, 20, 33, 5, 28], edm=BIG, env="GAUDI_EDM_TRAIN_SCRATCH_KB")
_add("chunks", ("pred",), 17, [17, 3, 12, 17, 9], env="GAUDI_PRED_TRAIN_SCRATCH_KB", draw=1)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _seed(case):
    return zlib.crc32(case.name.encode()) % (1 << 30) + 1000 * case.draw


def ring_walk(rng, n):
    """n ring centres: each one bonded-length step (1.9 - 2.7) from an earlier one, nearly planar; mean-free."""
    pos = [np.zeros(3)]
    for k in range(1, n):
        d = rng.standard_normal(3)
        d[2] *= 0.15
        pos.append(pos[int(rng.integers(k))] + d / np.linalg.norm(d) * rng.uniform(1.9, 2.7))
    x = np.array(pos)
    return x - x.mean(0, keepdims=True)


def models(case):
    """-> (edm args, edm state dict, predictor args, predictor state dict); the EDM of a predictor case only lends its schedule."""
    F = synth.num_node_features(case.dataset)
    s = _seed(case)
    eargs = synth.edm_args(dataset=case.dataset, **case.edm)
    esd = synth.synth_edm_state_dict(eargs, F, seed=s, amplify_coord=True)
    pargs = synth.pred_args(dataset=case.dataset, **case.pred)
    psd = synth.synth_predictor_state_dict(pargs, F, case.K, seed=s + 1, amplify_coord=True)
    return eargs, esd, pargs, psd


def inputs(case):
    """-> dict of float32 arrays x [B,N,3], h [B,N,F], node_mask [B,N], edge_mask [B,N,N], noise [B,N,3+F] and t_int [B]."""
    rng = np.random.default_rng(_seed(case) + 2)
    B, N, F = len(case.live), case.N, synth.num_node_features(case.dataset)
    T = int(case.edm["diffusion_steps"])
    x = np.zeros((B, N, 3), np.float32)
    nm = np.zeros((B, N), np.float32)
    for b, n in enumerate(case.live):
        x[b, :n] = ring_walk(rng, n)
        nm[b, :n] = 1
    h = (np.eye(F, dtype=np.float32)[rng.integers(0, F, (B, N))] * nm[:, :, None]).astype(np.float32)
    em = (nm[:, :, None] * nm[:, None, :] * (1 - np.eye(N, dtype=np.float32))[None]).astype(np.float32)
    t_int = rng.integers(1, T + 1, B) if case.t_int is None else np.array(case.t_int)
    noise = rng.standard_normal((B, N, 3 + F)).astype(np.float32)
    return dict(x=x, h=h, node_mask=nm, edge_mask=em, t_int=t_int.astype(np.int32), noise=noise)


def targets(case, pred64):
    """The predictor's targets: the float64 prediction plus an offset of random sign, at least half of max(1, |pred|), so that
    the sign of pred - y is the same in every precision."""
    rng = np.random.default_rng(_seed(case) + 3)
    sgn = np.where(rng.random(pred64.shape) < 0.5, -1.0, 1.0)
    return (pred64 + sgn * (0.5 + rng.random(pred64.shape)) * np.maximum(1.0, np.abs(pred64))).astype(np.float32)


def run_oracle(case, dtype, y=None, aux=None):
    """-> (loss, net or pred, grads) of the oracle in `dtype`."""
    eargs, esd, pargs, psd = models(case)
    i = inputs(case)
    if case.net == "edm":
        return TO.edm_train(esd, eargs, i["x"], i["h"], i["t_int"], i["node_mask"], i["edge_mask"], i["noise"],
                            loss_type=case.loss_type, weight=case.weight, dtype=dtype, aux=aux)
    return TO.pred_train(eargs, psd, pargs, i["x"], i["h"], i["t_int"], i["node_mask"], i["edge_mask"], y, i["noise"], dtype=dtype,
                         aux=aux)


Ref = namedtuple("Ref", "loss out grads loss32 out32 grads32 spread y tanh")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's float64 and float32 evaluations of a case, once per process: read-only."""
    import torch
    case = BY_NAME[name]
    y = None
    if case.net == "pred":
        y = targets(case, run_oracle(case, torch.float64)[1])
    aux = {}
    l64, o64, g64 = run_oracle(case, torch.float64, y, aux)
    l32, o32, g32 = run_oracle(case, torch.float32, y)
    spread = {"loss": rel_err(l32, l64), "out": rel_err(o32, o64)}
    for k, v in g64.items():
        if v is not None:
            spread[k] = rel_err(g32[k], v)
    return Ref(l64, o64, g64, l32, o32, g32, spread, y, aux["tanh"])


def bar(ref):
    """The bound a kernel result is held to: 1e-4, or twice the oracle's own float32 spread where that is larger (only
    sin_embedding may be: tests/test_train_oracle_cpu.py holds every other case to a spread of 5e-5)."""
    return max(1e-4, 2.0 * max(ref.spread.values()))


# ---- the scratch of the two host files, restated: the chunk a knob value gives.  The host code counts the floats with the list
# that carves them (csrc/train_host.inc: Carver); these polynomials are written independently of it, and
# tests/test_train_scratch_cpu.py holds gaudi_host_train_floats_per_mol to them at every case of the table.

def pt_floats_per_mol(N, H, L, F1, K):
    """csrc/pred_train_host.inc: pt_carve.  (L+1) node stashes of h and x, the input, d0, 9 node arrays (the running dh among
    them, updated in place), dx, the readout gradient, 8 edge arrays, coord_diff and its gradient, 6 edge scalars."""
    E = N * N
    return (L + 1) * N * (H + 4) + N * F1 + E + 9 * N * H + 4 * N + N * K + 8 * E * H + 8 * E + 6 * E


def pt_floats_per_mol_two_buffers(N, H, L, F1, K):
    """What the predictor's scratch took while its running gradient went between two buffers (dh0 / dh1, dx0 / dx1): one
    [N][H] and one [N][4] array more.  A library built from such a revision needs this to turn a chunk size into a knob value."""
    return pt_floats_per_mol(N, H, L, F1, K) + N * H + 4 * N


def et_floats_per_mol(N, H, L, S, F, A):
    """csrc/edm_train_host.inc: et_carve."""
    E, F1, D = N * N, F + 1, 3 + F
    return ((L * (S + 1) + 1) * N * H + (L + 1) * N * 4 + N * F1 + N * D + E * (A // 2) + E * A + 8 * E + 2 * E + 9 * N * H + 4 * N
            + N * F1 + 6 * E * H + 5 * E)


def shape_of(case):
    """-> (net, N, H, L, S, F, K, A): the arguments of gaudi_host_train_floats_per_mol for a case (net 0: predictor, 1: EDM)."""
    F = synth.num_node_features(case.dataset)
    if case.net == "pred":
        return 0, case.N, case.pred["nf"], case.pred["n_layers"], 1, F, case.K, 2
    e = case.edm
    return 1, case.N, e["nf"], e["n_layers"], e.get("inv_sublayers", 1), F, case.K, 24 if e.get("sin_embedding") else 2


def floats_per_mol(case):
    net, N, H, L, S, F, K, A = shape_of(case)
    return pt_floats_per_mol(N, H, L, F + 1, K) if net == 0 else et_floats_per_mol(N, H, L, S, F, A)


def chunk_of(case, kb):
    """Molecules per chunk for a knob value of kb KiB (Bc of the host code)."""
    return max(1, min(len(case.live), kb * 1024 // 4 // floats_per_mol(case)))


def knob_kb(case, mols):
    """A knob value that gives chunks of `mols` molecules."""
    kb = (mols * floats_per_mol(case) * 4 + 1023) // 1024
    assert chunk_of(case, kb) == mols
    return kb
