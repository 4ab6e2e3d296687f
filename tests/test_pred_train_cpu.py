"""Device-free pieces of predictor training: the autograd hand-off of compute_loss in train mode, the no-gradient-path rule
as the reference's fixture records it, and the C ABI binding of the new entry points."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loss_backward_fills_grad_and_leaves_none():
    import torch
    from gaudi_amd.cond_prediction import _L1
    a = torch.nn.Parameter(torch.zeros(2, 3))
    b = torch.nn.Parameter(torch.ones(4))
    ga = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    loss = _L1.apply(torch.tensor(0.75), [ga, None], a, b)
    assert float(loss) == 0.75
    loss.backward()
    assert torch.equal(a.grad, ga) and b.grad is None
    opt = torch.optim.AdamW([a, b], lr=0.1, amsgrad=True, weight_decay=0.5)
    opt.step()
    assert torch.equal(b.detach(), torch.ones(4))  # no .grad: AdamW skips it, weight decay included
    assert not torch.equal(a.detach(), torch.zeros(2, 3))


@pytest.mark.parametrize("fixture,name", [("g26_pred_grad", "cata"), ("g26_pred_grad_plain", "plain"),
                                          ("g26_pred_grad", "full"), ("g26_pred_grad_hetro", "hetro")])
def test_no_gradient_path_rule(golden, fixture, name):
    """torch leaves .grad None for exactly the last layer's coord_mlp (gaudi_predictor_loss_grad's has_grad rule)."""
    g = golden(fixture)
    cfg = json.loads(str(g[name + "_cfg"]))
    L = cfg["over"]["n_layers"]
    want = {n for n in cfg["names"] if n.startswith(f"egnn.gcl_{L - 1}.coord_mlp.")}
    assert len(want) == 3
    for tag in cfg["tags"]:
        assert set(json.loads(str(g[f"{name}_{tag}_nograd"]))) == want
        if name != "full":
            have = {n for n in cfg["names"] if f"{name}_{tag}_g.{n}" in g}
            assert have == set(cfg["names"]) - want
    if not cfg["over"].get("attention", True):
        assert not any("att_mlp" in n for n in cfg["names"])


def test_abi_declares_training_entry_points():
    from gaudi_amd import _lib
    with open(os.path.join(ROOT, "include", "gaudi_hip.h")) as f:
        hdr = f.read()
    for fn in ("gaudi_predictor_loss_grad", "gaudi_predictor_grad_size"):
        assert f"int {fn}(" in hdr and fn in _lib.EXPORTS
    assert len(_lib.EXPORTS["gaudi_predictor_loss_grad"][1]) == 16
    assert _lib.ABI_VERSION == 7


ROLES = ["edge_mlp.0.weight", "edge_mlp.0.bias", "edge_mlp.2.weight", "edge_mlp.2.bias", "att_mlp.0.weight", "att_mlp.0.bias",
         "coord_mlp.0.weight", "coord_mlp.0.bias", "coord_mlp.2.weight", "node_mlp.0.weight", "node_mlp.0.bias",
         "node_mlp.2.weight", "node_mlp.2.bias"]


def _layout(args, sd):
    import ctypes as C
    from gaudi_amd import _lib
    lib = _lib.load_library()
    names = list(sd)
    arrs = [np.ascontiguousarray(sd[k], np.float32) for k in names]
    n = len(names)
    F = sd["egnn.embedding.weight"].shape[1] - 1
    K = sd["egnn.embedding_out.weight"].shape[0]
    cfg = _lib.PredConfig(F, K, int(args["nf"]), int(args["n_layers"]), int(bool(args["attention"])), int(bool(args["tanh"])),
                          float(args["coords_range"]))
    total = sum(a.size for a in arrs)
    off = np.zeros(4 + 13 * int(args["n_layers"]), np.int32)
    has = np.zeros(n, np.int32)
    wt = np.zeros(total, np.float32)
    rc = lib.gaudi_host_pred_train_layout(C.byref(cfg), n, (C.c_char_p * n)(*[k.encode() for k in names]),
                                          (_lib.FP * n)(*[_lib.fptr(a) for a in arrs]),
                                          (C.c_int64 * n)(*[a.size for a in arrs]), off.ctypes.data_as(_lib.IP),
                                          has.ctypes.data_as(_lib.IP), _lib.fptr(wt))
    return rc, names, arrs, off, has, wt


@pytest.mark.parametrize("nf,attention", [(36, True), (196, True), (36, False)])
def test_layout_table_and_transposes(nf, attention):
    """gaudi_host_pred_train_layout -- the table gaudi_predictor_loss_grad reads the weights through: every role at its
    tensor's offset in names order, the no-gradient-path rule, and each matrix transposed in place (round trip)."""
    from gaudi_amd import synth
    L = 3
    args = synth.pred_args(dataset="cata", nf=nf, n_layers=L, attention=attention, tanh=True)
    sd = synth.synth_predictor_state_dict(args, 1, 5, seed=7)
    sd = dict(reversed(list(sd.items())))  # any order of names: offsets follow the order given
    rc, names, arrs, off, has, wt = _layout(args, sd)
    assert rc == 0
    start = dict(zip(names, np.cumsum([0] + [a.size for a in arrs])[:-1].tolist()))
    head = ["egnn.embedding.weight", "egnn.embedding.bias", "egnn.embedding_out.weight", "egnn.embedding_out.bias"]
    want = [start[n] for n in head]
    for l in range(L):
        for r in ROLES:
            n = f"egnn.gcl_{l}.{r}"
            want.append(start[n] if n in start else -1)
    assert off.tolist() == want
    assert (not attention) == all(v == -1 for l in range(L) for v in off[4 + 13 * l + 4: 4 + 13 * l + 6])
    for n, a, g in zip(names, arrs, has):
        assert g == (0 if n.startswith(f"egnn.gcl_{L - 1}.coord_mlp.") else 1), n
        block = wt[start[n]:start[n] + a.size]
        if a.ndim == 2 and min(a.shape) > 1:
            assert np.array_equal(block.reshape(a.shape[1], a.shape[0]).T, a), n
        else:
            assert np.array_equal(block, a.reshape(-1)), n


def test_layout_refuses_misshaped_tensor():
    from gaudi_amd import synth
    args = synth.pred_args(dataset="cata", nf=36, n_layers=2)
    sd = synth.synth_predictor_state_dict(args, 1, 5, seed=7)
    sd["egnn.gcl_1.node_mlp.2.weight"] = sd["egnn.gcl_1.node_mlp.2.weight"][:, :35].copy()
    assert _layout(args, sd)[0] == -4  # GAUDI_E_MISSING
