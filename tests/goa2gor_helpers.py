"""Shared by test_goa2gor_cpu.py and test_gpu_goa2gor.py: the g31 fixture as a list of molecules, and an engine-shaped object
that runs the perception routine's HOST build (gaudi_host_atoms_to_rings) so that gaudi_amd.goa2gor can be driven without a device."""
import os

import numpy as np

from gaudi_amd import _lib
from gaudi_amd.gor2goa import atoms_list

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, NO_RINGS, BAD_TYPE, NOT_A_BASIS, OVERFLOW = range(5)


class HostEngine:
    """Engine.atoms_to_rings through the host export: test surface, the package itself never takes this path."""

    def atoms_to_rings(self, tables, xyz, elem, n_atoms, flags=0, covalency_factor=1.3, max_rings=_lib.RINGS_MAX_RINGS):
        return _lib.host_atoms_to_rings(tables, xyz, elem, n_atoms, flags, covalency_factor, max_rings)


_CACHE = {}


def fixture():
    """-> (npz, molecules): one dict per molecule with its inputs, flags and the reference's rings (sorted by atom tuple)."""
    if "g31" in _CACHE:
        return _CACHE["g31"]
    z = np.load(os.path.join(GOLDEN, "g31_goa2gor.npz"))
    ao, ro, jo = z["atom_off"], z["ring_off"], z["adj_off"]
    mols = []
    for m in range(len(z["expect"])):
        ds = "hetro" if z["hetro"][m] else "cata"
        xyz = z["xyz"][ao[m]:ao[m + 1]].astype(np.float64)
        elem = z["elem"][ao[m]:ao[m + 1]].astype(np.int32)
        k = int(ro[m + 1] - ro[m])
        sl = slice(ro[m], ro[m + 1])
        expect = int(z["expect"][m])
        if expect < 0:
            expect = NOT_A_BASIS if not z["basis_ok"][m] else BAD_TYPE if z["threw"][m] else OK
        mols.append(dict(index=m, ds=ds, xyz=xyz, elem=elem, symbols=[atoms_list(ds)[e] for e in elem], use_h=bool(z["use_h"][m]),
                         special=int(z["expect"][m]) >= 0, expect=expect, threw=bool(z["threw"][m]), basis_ok=bool(z["basis_ok"][m]),
                         margin=float(z["margin"][m]), n_rings=k, ring_atoms=z["ring_atoms"][sl].astype(np.int64),
                         ring_type=z["ring_type"][sl].astype(np.int64), centre=z["centre"][sl], x32=z["x32"][sl],
                         orient=z["orient"][sl].astype(np.int64), adj=z["adj"][jo[m]:jo[m + 1]].reshape(k, k)))
    _CACHE["g31"] = (z, mols)
    return _CACHE["g31"]


def compared(mol):
    """The reference's rings are compared where it returned some and the basis criterion holds."""
    return mol["basis_ok"] and not mol["threw"] and mol["expect"] == OK and mol["n_rings"] > 0


def ring_sets(ring_atoms):
    return [frozenset(int(a) for a in row if a >= 0) for row in ring_atoms]


def rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q
