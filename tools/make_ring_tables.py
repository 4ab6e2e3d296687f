#!/usr/bin/env python3
"""Dump the graph-of-rings geometry tables of the REFERENCE into gaudi_amd/data/ring_tables.json.

Runs only in the build container.  The tables are data measured on the reference's datasets (quantiles of ring-ring
distances, 3-ring angles, 4-ring dihedrals; utils/helpers.py:11-196, data/aromatic_dataloader.py:31-35, data/ring.py:6-18)
and are needed verbatim for parity of the stability check; they are exported in array form, indexed by the ring-type
index the one-hot node features use:

    rings[dataset]            ring symbols, index = class index of the one-hot features
    dist_lo/hi[dataset][i][j] bonded-distance window of ring types (i, j), 0/0 when the pair never bonds
    a3[dataset][i]            list of (low, high) windows for the 3-ring angle centred on ring type i
    a4[dataset]               {"0": q, "180": q} dihedral thresholds;   n_nodes[dataset]: ring-count histogram

and the constants of the graph-of-rings -> graph-of-atoms conversion (data/gor2goa.py:18-51,133-198, data/ring.py:6-18,
utils/ring_graph.py:9, data/aromatic_dataloader.py:26-30), keyed by ring symbol:

    goa.templates[name]       2-D ring templates (hexagon, pentagon, square), one [x, y] per ring atom
    goa.ring_template[sym]    which template a ring type uses;   goa.ring_atoms[sym]: its elements (RINGS_DICT)
    goa.no_orientation        ring types turned towards a fused ring instead of an orientation node
    goa.extra_angle[sym]      what gor2goa adds to that angle;   goa.template_h[sym]: ring atoms that carry a template H
    goa.atoms[dataset]        ATOMS_LIST;   goa.h_bond: X-H distance used when hydrogens are placed (ours, not the reference's)
    goa.cov_radii[element]    covalent radii (utils/const.py) of the elements of ATOMS_LIST: bond perception of atoms -> rings

and the valence options of the bond-order assignment (gaudi_bond_orders), from the allowed valences and the charge function of
data/xyz2mol.py:136-164,312-326:

    valence.options[element]  per sigma degree 0..4 the list of [added bonds, formal charge] for every allowed valence v >= degree
                              with v - degree <= 1 (the rule is ours: DESIGN.md section 8h), the neutral option first
"""
import json
import os
import sys
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")
for m in ["rdkit", "rdkit.Chem", "rdkit.Chem.Draw", "rdkit.Chem.rdmolops", "rdkit.Chem.rdchem", "rdkit.Chem.AllChem",
          "imageio", "torch.utils.tensorboard"]:
    sys.modules[m] = MagicMock()

import math  # noqa: E402

from data import gor2goa as G  # noqa: E402
from data import xyz2mol as X  # noqa: E402
from data.aromatic_dataloader import ATOMS_LIST, RINGS_LIST  # noqa: E402
from data.ring import RINGS_DICT  # noqa: E402
from utils.ring_graph import NO_ORIENTATION_RINGS  # noqa: E402
from utils.const import __COV_RADII__  # noqa: E402
from utils import helpers as H  # noqa: E402

out = dict(rings={}, dist_lo={}, dist_hi={}, a3={}, a4={}, n_nodes={}, min_dist={})
for ds in ("cata", "hetro"):
    rings = list(RINGS_LIST[ds])
    R = len(rings)
    lo = [[0.0] * R for _ in range(R)]
    hi = [[0.0] * R for _ in range(R)]
    for i, si in enumerate(rings):
        for j, sj in enumerate(rings):
            # the lookup order of positions2adj (utils/helpers.py:178-182): "si-sj" first, then "sj-si"
            key = f"{si}-{sj}"
            if key not in H.ring_distances[ds]:
                key = f"{sj}-{si}"
            if key in H.ring_distances[ds]:
                lo[i][j], hi[i][j] = H.ring_distances[ds][key]
    out["rings"][ds] = rings
    out["dist_lo"][ds], out["dist_hi"][ds] = lo, hi
    out["min_dist"][ds] = min(r[0] for r in H.ring_distances[ds].values())
    out["a3"][ds] = [[list(w) for w in H.angels3_dict[ds][s].values()] if s in H.angels3_dict[ds] else [] for s in rings]
    out["a4"][ds] = H.angels4_dict[ds]
    out["n_nodes"][ds] = {str(k): v for k, v in H.analyzed_rings[ds]["n_nodes"].items()}
templates = {"hexagon": G.hexagon, "pentagon": G.pentagon, "square": G.square}
out["goa"] = dict(
    templates={k: [[float(c) for c in row] for row in v] for k, v in templates.items()},
    ring_template={sym: next(k for k, v in templates.items() if v is arr) for sym, arr in G.rings.items()},
    ring_atoms={sym: list(elems) for sym, elems in RINGS_DICT.items()},
    no_orientation=list(NO_ORIENTATION_RINGS),
    # the two rules below are literals inside gor2goa's body (data/gor2goa.py:161-164 and :189-198), restated here
    extra_angle={"Bn": math.pi / 6, "Cbd": math.pi / 4},
    template_h={"Bl": [4], "Pl": [4], "DhDb": [2, 5]},
    atoms={ds: list(ATOMS_LIST[ds]) for ds in ("cata", "peri", "hetro")},
    h_bond=1.09,
    cov_radii={e: float(__COV_RADII__[e]) for e in ATOMS_LIST["hetro"]},
)


def valence_options(sym, degree):
    z = X.int_atom(sym)
    opts = [[v - degree, int(X.get_atomic_charge(z, X.atomic_valence_electrons[z], v))] for v in X.atomic_valence[z]
            if 0 <= v - degree <= 1]
    return sorted(opts, key=lambda o: (abs(o[1]), o[0]))


out["valence"] = dict(degrees=5, options={e: [valence_options(e, d) for d in range(5)] for e in ATOMS_LIST["hetro"]})
path = os.path.join(ROOT, "gaudi_amd", "data", "ring_tables.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print(path, os.path.getsize(path), "bytes")
