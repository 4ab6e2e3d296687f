"""Shared by test_bond_orders_cpu.py and test_gpu_bond_orders.py: the g32 fixture as a list of molecules, packed arrays for the two
entry points, and a verifier of a returned structure that knows nothing of how it was found."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, NO_STRUCTURE, CAPPED, NOT_CONNECTED, BAD_VALENCE, BAD_INPUT, OVERFLOW, EMPTY, GAVE_UP = range(9)
H, C = 0, 1  # in ATOMS_LIST["hetro"], the element list of every molecule of the fixture (ATOMS_LIST["cata"] is its prefix)
DATASET = "hetro"

_CACHE = {}


def fixture():
    """-> (npz, molecules): one dict per molecule with its elements, bonds and the fixture's flags."""
    if "g32" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "g32_bond_orders.npz"))
        ao, bo = z["atom_off"], z["bond_off"]
        mols = [dict(index=m, elem=z["elem"][ao[m]:ao[m + 1]].astype(np.int32), bonds=z["bonds"][bo[m]:bo[m + 1]].astype(np.int32),
                     kind=int(z["kind"][m]), special=int(z["special"][m]), g30=int(z["g30"][m]), ref_ran=bool(z["ref_ran"][m]),
                     ref_valid=bool(z["ref_valid"][m]), ref_stable=bool(z["ref_stable"][m]),
                     ref_cumulated=bool(z["ref_cumulated"][m]), min_charged=int(z["min_charged"][m]),
                     odd_cycle=bool(z["odd_cycle"][m])) for m in range(len(z["kind"]))]
        _CACHE["g32"] = (z, mols)
    return _CACHE["g32"]


def pack(mols):
    """[(elem, bonds)] or fixture molecules -> elem [B,A], n_atoms [B], bonds [B,M,2], n_bonds [B] (int32, zero padded)."""
    pairs = [(m["elem"], m["bonds"]) if isinstance(m, dict) else m for m in mols]
    B = len(pairs)
    A, M = max(1, max(len(e) for e, _ in pairs)), max(1, max(len(b) for _, b in pairs))
    elem, bonds = np.zeros((B, A), np.int32), np.zeros((B, M, 2), np.int32)
    na, nb = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for i, (e, b) in enumerate(pairs):
        elem[i, :len(e)], na[i], nb[i] = e, len(e), len(b)
        bonds[i, :len(b)] = np.asarray(b, np.int32).reshape(-1, 2)
    return elem, na, bonds, nb


def relabel(mol, rng):
    """The same molecule with its atoms renumbered and its bond list shuffled and randomly flipped."""
    n = len(mol["elem"])
    perm = rng.permutation(n)
    elem = np.zeros(n, np.int32)
    elem[perm] = mol["elem"]
    bonds = perm[mol["bonds"]].astype(np.int32).reshape(-1, 2)
    bonds = bonds[rng.permutation(len(bonds))]
    flip = rng.random(len(bonds)) < 0.5
    bonds[flip] = bonds[flip][:, ::-1]
    return elem, bonds


def verify(table_n, table_opt, elem, bonds, orders, charges, n_charged):
    """A structure is right when: orders are 1 or 2; with the sigma degree of the rule (bonds, one more for a carbon with exactly
    two), every atom's (sum of orders - bonds, charge) is one of the options the table has for its (element, degree); the charges
    sum to zero; n_charged counts the nonzero ones."""
    elem, bonds = np.asarray(elem), np.asarray(bonds).reshape(-1, 2)
    orders, charges = np.asarray(orders, np.int64), np.asarray(charges, np.int64)
    assert len(orders) == len(bonds) and len(charges) == len(elem)
    assert np.isin(orders, (1, 2)).all()
    n = len(elem)
    deg, added = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for (i, j), o in zip(bonds, orders):
        deg[i] += 1
        deg[j] += 1
        added[i] += o - 1
        added[j] += o - 1
    deg += (elem == C) & (deg == 2)
    for a in range(n):
        assert deg[a] <= 4, (a, deg[a])
        opts = [tuple(table_opt[elem[a], deg[a], k]) for k in range(table_n[elem[a], deg[a]])]
        assert (added[a], charges[a]) in opts, (a, int(elem[a]), int(deg[a]), int(added[a]), int(charges[a]), opts)
    assert charges.sum() == 0
    assert n_charged == np.count_nonzero(charges)


def budget_molecule(n=192, front=False):
    """A ladder of alternating B / N atoms of degree 3 (188 atoms with a neutral and a charged option each) between two pairs of
    carbons that add a bond and find no partner in the first matching.  It HAS a structure with 4 charged atoms: the ladder atoms
    next to the four carbons, 2 and n - 3 (N+) and 3 and n - 4 (B-), each take the double bond of their carbon.  In the order of
    this numbering that subset comes after more than 16 384 others of size 4, so the search gives up (GAVE_UP: undecided).
    front=True renumbers the last four ladder-and-carbon atoms to the front, where the same search reaches the structure: the one
    status that may depend on the numbering, as DESIGN.md section 8h and the header say."""
    B, N = 2, 3
    e = [B if k % 4 in (0, 3) else N for k in range(n)]
    b = [(k, k + 1) for k in range(2, n - 2, 2)]
    for k in range(0, n - 2, 2):
        b += [(k, k + 2), (k + 1, k + 3)]
    for c in (0, 1, n - 2, n - 1):
        e[c] = C
        b.append((c, len(e)))
        e.append(H)
    e, b = np.array(e, np.int32), np.array(b, np.int32)
    if front:
        order = list(range(n - 4, n)) + list(range(n - 4)) + list(range(n, len(e)))  # new index -> old index
        new = np.zeros(len(e), np.int32)
        new[order] = np.arange(len(e))
        e, b = e[order], new[b]
    return e, b


def budget_structure(n=192):
    """The 4-charge structure of budget_molecule(n) in its own numbering -> (orders, charges)."""
    e, b = budget_molecule(n)
    double = {(0, 2), (1, 3), (n - 4, n - 2), (n - 3, n - 1)}
    orders = np.array([2 if (min(i, j), max(i, j)) in double else 1 for i, j in b])
    charges = np.zeros(len(e), np.int64)
    for a in (2, 3, n - 4, n - 3):
        charges[a] = 1 if e[a] == 3 else -1
    return orders, charges


def six_charge_molecule():
    """A saturated chain of six carbons, each carrying a heteroatom X_i (N, N, N, B, B, B; bonds: chain carbon, H, C_i) whose
    C_i is a CH2 with three bonds.  C_i must take a double bond and X_i is its only partner that can, which X_i can only when
    charged: every structure has all six X charged (3 N+, 3 B-), none has fewer.  -> (elem, bonds, orders, charges) with that
    structure: beyond the cap of 4, within the 6 the search still looks at, so the status is CAPPED."""
    N, B = 3, 2
    e, b, double = [], [], set()

    def atom(el, *nbrs):
        e.append(el)
        for o in nbrs:
            b.append((o, len(e) - 1))
        return len(e) - 1

    chain = []
    for i in range(6):
        c = atom(C, *chain[-1:])
        chain.append(c)
        for _ in range(2 if i in (0, 5) else 1):
            atom(H, c)
    xs = []
    for i, c in enumerate(chain):
        x = atom(N if i < 3 else B, c)
        atom(H, x)
        ci = atom(C, x)
        atom(H, ci)
        atom(H, ci)
        xs.append(x)
        double.add((x, ci))
    charges = np.zeros(len(e), np.int64)
    for x in xs:
        charges[x] = 1 if e[x] == N else -1
    orders = np.array([2 if (i, j) in double else 1 for i, j in b])
    return np.array(e, np.int32), np.array(b, np.int32), orders, charges
