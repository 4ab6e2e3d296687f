"""Host mirror of the EDM's training and validation loops: compute_loss / train_epoch / val_epoch of train_edm.py:36-143 and
Queue / gradient_clipping of edm/utils.py:31-70.  In train mode GaudiModel(...) returns the train-mode loss per molecule
(gaudi_edm_loss_grad: the network and its reverse pass in HIP), whose backward() fills every dynamics.* .grad; in eval mode
it is the eval-mode NLL (gaudi_edm_nll).  Tensorboard / tqdm and the `epoch % 50` chain pictures are left to the caller."""
from __future__ import annotations

import numpy as np

from .models_edm import _like_ref, _to_numpy, assert_correctly_masked, assert_mean_zero_with_mask


def remove_mean_with_mask(x, node_mask):
    """utils.py:33-44."""
    x = _to_numpy(x).astype(np.float32)
    nm = _to_numpy(node_mask).astype(np.float32).reshape(x.shape[0], x.shape[1], 1)
    return x - (x * nm).sum(1, keepdims=True) / np.maximum(nm.sum(1, keepdims=True), 1) * nm


def compute_loss(model, x, h, node_mask, edge_mask):
    """train_edm.py:36-50 -> the batch mean of the model's loss (a 0-d torch tensor): the eval-mode NLL, or in train mode
    the training loss, differentiable in the model's parameters."""
    import torch
    xn = _to_numpy(x)
    bs, n_nodes = xn.shape[0], xn.shape[1]
    assert_correctly_masked(xn, node_mask)
    edge_mask = _to_numpy(edge_mask).reshape(bs, n_nodes * n_nodes)
    h = {"categorical": h, "integer": torch.zeros(0)}
    loss = model(x, h, node_mask, edge_mask)
    return loss.mean(0)


class Queue:
    """edm/utils.py:31-50: the recent gradient norms gradient_clipping bounds the next one by."""

    def __init__(self, max_len=50):
        self.items = []
        self.max_len = max_len

    def __len__(self):
        return len(self.items)

    def add(self, item):
        self.items.insert(0, item)
        if len(self) > self.max_len:
            self.items.pop()

    def mean(self):
        return np.mean(self.items)

    def std(self):
        return np.std(self.items)


def gradient_clipping(flow, gradnorm_queue):
    """edm/utils.py:53-70: clip to 1.5 x the recent mean + 2 x its std (torch's clip_grad_norm_ over flow.parameters())."""
    import torch
    max_grad_norm = 1.5 * gradnorm_queue.mean() + 2 * gradnorm_queue.std()
    grad_norm = torch.nn.utils.clip_grad_norm_(flow.parameters(), max_norm=max_grad_norm, norm_type=2.0)
    if float(grad_norm) > max_grad_norm:
        gradnorm_queue.add(float(max_grad_norm))
        print(f"Clipped gradient with value {grad_norm:.1f} while allowed {max_grad_norm:.1f}")
    else:
        gradnorm_queue.add(float(grad_norm))
    return grad_norm


def train_epoch(epoch, model, dataloader, optimizer, args, writer=None, gradnorm_queue=None):
    """train_edm.py:52-94 over a loader of (x, node_mask, edge_mask, node_features, y) batches -> (losses, grad norms)."""
    import time
    a = args if isinstance(args, dict) else vars(args)
    model.train()
    start = time.time()
    losses, grad_norms = [], []
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
        optimizer.zero_grad()
        loss.backward()
        if a.get("clip_grad", True):
            grad_norm = gradient_clipping(model, gradnorm_queue)
            grad_norms.append(grad_norm.item())
        optimizer.step()
        losses.append(loss.item())
    print(f"[{epoch}|train] loss: {np.mean(losses):.3f}+-{np.std(losses):.3f}, "
          f"GradNorm: {np.mean(grad_norms) if grad_norms else float('nan'):.1f},  in {int(time.time() - start)} secs")
    if writer is not None:
        writer.add_scalar("Train loss", np.mean(losses), epoch)
        writer.add_scalar("Train grad norm", np.mean(grad_norms), epoch)
    return losses, grad_norms


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
