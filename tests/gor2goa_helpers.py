"""Shared by tests/test_gor2goa_cpu.py and tests/test_gpu_gor2goa.py: the g30 fixture unpacked into per-molecule lists."""
import numpy as np


def unpack(g):
    """g30_gor2goa.npz -> list of dicts (dataset, x, types, threw, stable, ref atoms / types / bonds, iso_class, spread, twin)."""
    out = []
    for m in range(len(g["n"])):
        n = int(g["n"][m])
        a0, a1, b0, b1 = int(g["atom_off"][m]), int(g["atom_off"][m + 1]), int(g["bond_off"][m]), int(g["bond_off"][m + 1])
        out.append(dict(dataset="hetro" if g["hetro"][m] else "cata", x=g["x"][m, :n], types=g["types"][m, :n].astype(np.int64),
                        threw=bool(g["threw"][m]), stable=bool(g["stable"][m]), ref_atoms=g["ref_atoms"][a0:a1],
                        ref_types=g["ref_types"][a0:a1].astype(np.int64), ref_bonds=g["ref_bonds"][b0:b1].astype(np.int64),
                        iso_class=int(g["iso_class"][m]), spread=float(g["dist_spread"][m]), twin_x=g["twin_x"][m, :n],
                        twin_types=g["twin_types"][m, :n].astype(np.int64), twin_iso_class=int(g["twin_iso_class"][m])))
    return out


def n_rings(mol):
    return len(mol["x"]) if mol["dataset"] == "cata" else len(mol["x"]) // 2


def pdist(a):
    a = np.asarray(a, np.float64)
    return np.sqrt(((a[:, None] - a[None]) ** 2).sum(-1))


def tolerances(mols):
    """Per molecule: 4 x its dist_spread (an fp32 implementation makes about four rounding steps of the size dist_spread
    measures: alignment, rotation, translation, midpoint), floored at the fixture's median spread over the built molecules."""
    spreads = np.array([m["spread"] for m in mols if not m["threw"]])
    floor = float(np.median(spreads))
    return [max(4.0 * m["spread"], floor) for m in mols], floor
