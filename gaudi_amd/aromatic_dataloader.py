"""Host mirror of data/aromatic_dataloader.py: molecules given as atoms -> the batches the training loops take.

``RingsDataset`` lays a molecule out exactly as ``AromaticDataset.get_all`` does (data/aromatic_dataloader.py:175-245) and
``batches`` yields the ``(x, node_mask, edge_mask, node_features, y)`` tuples that ``train_edm.train_epoch`` / ``val_epoch`` and
the predictor's training loop consume.  The rings come from ``goa2gor.atoms_to_rings``: one kernel launch for the whole dataset
where the reference perceives rings per molecule in Python and caches them on disk.

Not mirrored: the pandas CSV splits (``get_splits``), ``from_rdkit`` (``.pkl`` input) and torch ``DataLoader`` workers -- a
dataset here is built from records or xyz paths the caller chose, and ``batches`` is a plain generator."""
from __future__ import annotations

import random

import numpy as np

from ._lib import GaudiError
from .analyze import rings_list
from .goa2gor import STATUS_NAMES, atoms_to_rings, read_xyz
from .gor2goa import atoms_list

ATOMS_LIST = {ds: atoms_list(ds) for ds in ("cata", "peri", "hetro")}   # data/aromatic_dataloader.py:26-30
RINGS_LIST = {ds: rings_list(ds) for ds in ("cata", "peri", "hetro")}   # :31-35


class RingsDataset:
    """``records``: what ``atoms_to_rings`` returns.  ``targets`` [M,K] (one row per record) or None.  Molecules with a status
    other than OK or with more than ``max_nodes`` rings are left out and counted in ``skipped`` by status name ("TOO_MANY_RINGS"
    for the latter, the reference's ``df.n_rings <= max_nodes``); ``kept`` holds the indices of the records that stayed.
    normalize: y = (y - mean) / std with the given train-set ``mean`` / ``std``, or those of the targets kept here."""

    def __init__(self, records, targets=None, dataset="cata", max_nodes=11, normalize=False, mean=None, std=None):
        if dataset not in RINGS_LIST:
            raise GaudiError(f"no ring list for dataset {dataset!r}")
        records = list(records)
        if targets is not None:
            targets = np.asarray(targets, np.float32).reshape(len(records), -1)
        self.dataset, self.max_nodes, self.normalize = dataset, int(max_nodes), bool(normalize)
        self.orientation = dataset != "cata"
        self.skipped, self.kept, self.records = {}, [], []
        for i, rec in enumerate(records):
            why = None
            if rec["status"]:
                why = STATUS_NAMES.get(rec["status"], str(rec["status"]))
            elif len(rec["x"]) > self.max_nodes:
                why = "TOO_MANY_RINGS"
            if why is not None:
                self.skipped[why] = self.skipped.get(why, 0) + 1
                continue
            self.kept.append(i)
            self.records.append(rec)
        self.targets = None if targets is None else targets[self.kept]
        if self.normalize:
            if self.targets is None:
                raise GaudiError("normalize=True needs targets")
            self.mean = np.asarray(self.targets.mean(0) if mean is None else mean, np.float32)
            self.std = np.asarray(self.targets.std(0) if std is None else std, np.float32)
        else:
            self.mean, self.std = np.zeros(1, np.float32), np.ones(1, np.float32)
        self.num_node_features = len(RINGS_LIST[dataset])
        self.num_targets = 0 if self.targets is None else self.targets.shape[1]

    @classmethod
    def from_xyz(cls, paths, targets=None, dataset="cata", max_nodes=11, normalize=False, mean=None, std=None, engine=None):
        """Read the xyz files and perceive their rings in ONE batched call."""
        return cls(atoms_to_rings([read_xyz(p) for p in paths], dataset, engine=engine), targets, dataset, max_nodes, normalize,
                   mean, std)

    def __len__(self):
        return len(self.records)

    def rescale_loss(self, x):
        return x * self.std.mean() if self.normalize else x

    def __getitem__(self, idx):
        """-> (x, node_mask, edge_mask, node_features, y) as float32 arrays, AromaticDataset.get_all's layout."""
        rec, mn = self.records[idx], self.max_nodes
        y = np.zeros(0, np.float32) if self.targets is None else self.targets[idx].copy()
        if self.normalize:
            y = (y - self.mean) / self.std
        n, F = len(rec["x"]), rec["node_features"].shape[1]
        N = 2 * mn if self.orientation else mn
        x = np.zeros((N, 3), np.float32)
        node_mask = np.zeros(N, np.float32)
        feats = np.zeros((N, F), np.float32)
        x[:n] = rec["x"]
        node_mask[:n] = 1
        feats[:n] = rec["node_features"]
        ring_block = node_mask[:mn, None] * node_mask[None, :mn] * (1 - np.eye(mn, dtype=np.float32))
        if not self.orientation:
            return x, node_mask, ring_block.astype(np.float32), feats, y
        # one orientation candidate per ring, drawn as the reference draws it (random.sample on the module's generator)
        x[mn:mn + n] = np.asarray([random.sample(list(o), 1)[0] for o in rec["orientation"]], np.float64).reshape(n, 3)
        node_mask[mn:mn + n] = 1
        feats[mn:mn + n, -1] = 1  # the orientation nodes as an additional ring type
        edge_mask = np.zeros((N, N), np.float32)
        edge_mask[:mn, :mn] = ring_block
        i = np.arange(mn)
        edge_mask[i, mn + i] = edge_mask[mn + i, i] = 1  # every slot pair, as get_edge_mask_orientation sets them
        return x, node_mask, edge_mask, feats, y


def batches(dataset, batch_size, shuffle=False, seed=0):
    """Yield (x [B,N,3], node_mask [B,N], edge_mask [B,N,N], node_features [B,N,F], y [B,K]) float32 torch tensors, the last
    batch short: what a DataLoader over AromaticDataset yields."""
    import torch
    order = np.arange(len(dataset))
    if shuffle:
        np.random.default_rng(seed).shuffle(order)
    for s in range(0, len(order), int(batch_size)):
        rows = [dataset[int(i)] for i in order[s:s + int(batch_size)]]
        yield tuple(torch.from_numpy(np.stack([r[k] for r in rows])) for k in range(5))
