"""Host mirror of the EDM's validation loss: compute_loss / val_epoch of train_edm.py:36-143, on top of gaudi_edm_nll (both
network passes of the eval-mode NLL in one launch).  Evaluation only: there is no backward pass through the weights here
(training is out of scope), and the `epoch % 50` chain pictures of val_epoch are left to the caller."""
from __future__ import annotations

import numpy as np

from .models_edm import _like_ref, _to_numpy, assert_correctly_masked, assert_mean_zero_with_mask


def remove_mean_with_mask(x, node_mask):
    """utils.py:33-44."""
    x = _to_numpy(x).astype(np.float32)
    nm = _to_numpy(node_mask).astype(np.float32).reshape(x.shape[0], x.shape[1], 1)
    return x - (x * nm).sum(1, keepdims=True) / np.maximum(nm.sum(1, keepdims=True), 1) * nm


def compute_loss(model, x, h, node_mask, edge_mask):
    """train_edm.py:36-50 -> the batch mean of the NLL (a 0-d torch tensor)."""
    import torch
    xn = _to_numpy(x)
    bs, n_nodes = xn.shape[0], xn.shape[1]
    assert_correctly_masked(xn, node_mask)
    edge_mask = _to_numpy(edge_mask).reshape(bs, n_nodes * n_nodes)
    h = {"categorical": h, "integer": torch.zeros(0)}
    loss = model(x, h, node_mask, edge_mask)
    return loss.mean(0)


def val_epoch(tag, epoch, model, nodes_dist, prop_dist, dataloader, args, writer=None):
    """train_edm.py:97-143 over a loader of (x, node_mask, edge_mask, node_features, y) batches -> mean NLL per batch."""
    model.eval()
    losses = []
    for x, node_mask, edge_mask, node_features, y in dataloader:
        nm = _to_numpy(node_mask).astype(np.float32)
        nm = nm.reshape(nm.shape[0], nm.shape[1], 1)
        x = remove_mean_with_mask(x, nm)
        h = _to_numpy(node_features).astype(np.float32)
        for v in (x, h):
            if v.shape[-1] != 0:
                assert_correctly_masked(v, nm)
        assert_mean_zero_with_mask(x, nm)
        loss = compute_loss(model, _like_ref(x), _like_ref(h), _like_ref(nm), edge_mask)
        losses.append(float(loss))
    print(f"[{epoch}|{tag}] loss: {np.mean(losses):.3f}+-{np.std(losses):.3f}")
    if writer is not None:
        writer.add_scalar(f"{tag} loss", np.mean(losses), epoch)
    return np.mean(losses)
