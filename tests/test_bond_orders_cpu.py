"""Bond orders and formal charges from connectivity (csrc/bonds.inc) through the kernel's HOST build, gaudi_host_bond_orders,
against golden g32: the valence table, every returned structure checked by an independent verifier, the fewest-charges claim
against the generator's exhaustive search, the verdict against the reference's AC2BO, the specials, relabelling, write_molfile."""
import io

import numpy as np
import pytest

from gaudi_amd import _lib
from tests.bond_order_helpers import (BAD_INPUT, BAD_VALENCE, CAPPED, DATASET, EMPTY, NO_STRUCTURE, NOT_CONNECTED, OK, OVERFLOW,
                                      GAVE_UP, budget_molecule, budget_structure, fixture, pack, relabel, six_charge_molecule, verify)


@pytest.fixture(scope="module")
def g32():
    return fixture()


@pytest.fixture(scope="module")
def host(g32):
    """The whole fixture in one call of the host twin."""
    from gaudi_amd.gor2goa import c_valence_tables
    return _lib.host_bond_orders(c_valence_tables(DATASET), *pack(g32[1]))


def test_valence_section_equals_the_fixture_table(g32):
    """ring_tables.json "valence" (what the package ships) against the table the fixture's generator derived from the reference's
    valence lists and charge function; and the C struct built from it."""
    from gaudi_amd.analyze import ring_tables
    from gaudi_amd.gor2goa import atoms_list, c_valence_tables
    z = g32[0]
    V = ring_tables()["valence"]
    names = atoms_list(DATASET)
    assert V["degrees"] == z["table_n"].shape[1] == 5 and len(names) == z["table_n"].shape[0]
    t = c_valence_tables(DATASET)
    for e, sym in enumerate(names):
        for d in range(5):
            want = [[int(v) for v in z["table_opt"][e, d, k]] for k in range(z["table_n"][e, d])]
            assert V["options"][sym][d] == want, (sym, d)
            assert t.n_options[e][d] == len(want)
            assert [[t.option[e][d][k][0], t.option[e][d][k][1]] for k in range(len(want))] == want
            assert len(want) <= 2 and all(a in (0, 1) for a, _ in want)
    c = c_valence_tables("cata")  # the same rows for the shorter element list
    assert c.n_elems == 2 and [c.n_options[1][d] for d in range(5)] == [t.n_options[1][d] for d in range(5)]


def test_every_structure_passes_the_verifier(g32, host):
    z, mols = g32
    n = 0
    for m, st in zip(mols, host["status"]):
        i = m["index"]
        na, nb = len(m["elem"]), len(m["bonds"])
        if st != OK:
            assert not host["order"][i].any() and not host["charge"][i].any() and host["n_charged"][i] == 0
            continue
        verify(z["table_n"], z["table_opt"], m["elem"], m["bonds"], host["order"][i, :nb], host["charge"][i, :na], host["n_charged"][i])
        assert not host["order"][i, nb:].any() and not host["charge"][i, na:].any()
        n += 1
    assert n >= 250


def _why_none(table_n, m):
    """The status of a molecule without a structure, from the fixture's table alone: an atom without an option first, then pieces."""
    n = len(m["elem"])
    deg = np.bincount(m["bonds"].reshape(-1), minlength=n)
    deg = deg + ((m["elem"] == 1) & (deg == 2))
    if any(d > 4 or table_n[e, d] == 0 for e, d in zip(m["elem"], deg)):
        return BAD_VALENCE
    label = np.arange(n)
    for _ in range(n):
        for i, j in m["bonds"]:
            label[i] = label[j] = min(label[i], label[j])
    return NOT_CONNECTED if len(set(label.tolist())) > 1 else NO_STRUCTURE


def test_fewest_charges_against_the_exhaustive_search(g32, host):
    """OK <=> min_charged in 0..4, with n_charged = min_charged; NO_STRUCTURE exactly where the search (up to 6) found none, CAPPED
    where it found one with 5 or 6.  The molecules the reference cannot take (bad index, overflow, empty) have statuses of their own."""
    counts = {}
    for m, st, nc in zip(g32[1], host["status"], host["n_charged"]):
        if not m["ref_ran"]:
            continue
        mc = m["min_charged"]
        counts[mc] = counts.get(mc, 0) + 1
        assert (st == OK) == (0 <= mc <= 4), (m["index"], st, mc)
        if st == OK:
            assert nc == mc, (m["index"], nc, mc)
        elif mc > 4:
            assert st == CAPPED, (m["index"], st, mc)
        else:  # (a molecule with an atom without an option, or in several pieces, has no structure either)
            assert st == _why_none(g32[0]["table_n"], m), (m["index"], st)
    assert counts[0] >= 100 and counts[2] >= 10 and counts[4] >= 1 and counts[-1] >= 50
    assert sum(m["odd_cycle"] for m in g32[1]) >= 10  # matchings in non-bipartite selected subgraphs are in


def test_verdict_equals_the_reference(g32, host):
    """OK <=> the reference's AC2BO verdict, on every molecule whose verdict does not depend on the atom numbering
    (ref_stable), that the reference did not reach through an atom with two added bonds (ref_cumulated) and that it can take
    at all (ref_ran: not the bad-index, overflow and empty specials).  No exceptions; at most 5 % may stand outside."""
    mols = g32[1]
    compared = [m for m in mols if m["ref_ran"] and m["ref_stable"] and not m["ref_cumulated"]]
    assert (len(mols) - len(compared)) * 100 <= 5 * len(mols)
    wrong = [m["index"] for m in compared if (host["status"][m["index"]] == OK) != m["ref_valid"]]
    assert not wrong, wrong
    assert sum(m["ref_valid"] for m in compared) >= 250 and sum(not m["ref_valid"] for m in compared) >= 50


def test_specials(g32, host):
    seen = set()
    for m in g32[1]:
        if m["special"] >= 0:
            assert host["status"][m["index"]] == m["special"], (m["index"], len(m["elem"]))
            seen.add(m["special"])
    assert seen == {OK, NO_STRUCTURE, NOT_CONNECTED, BAD_VALENCE, BAD_INPUT, OVERFLOW, EMPTY}
    big = [m for m in g32[1] if m["special"] == OK and (m["elem"] != 0).sum() == 190]
    assert len(big) == 1 and host["n_charged"][big[0]["index"]] == 0  # the capacity edge has a neutral Kekule structure


def test_relabelling_keeps_status_and_charge_count(g32, host):
    """On the fixture, whose molecules never exhaust the search budget (no GAVE_UP among the statuses): for such molecules the
    status and n_charged are functions of the molecule, whatever its numbering."""
    assert GAVE_UP not in host["status"]
    from gaudi_amd.gor2goa import c_valence_tables
    z, mols = g32
    t = c_valence_tables(DATASET)
    for seed in (1, 2):
        rng = np.random.default_rng(3210 + seed)
        twins = [relabel(m, rng) if m["special"] not in (BAD_INPUT,) else (m["elem"], m["bonds"]) for m in mols]
        out = _lib.host_bond_orders(t, *pack(twins))
        assert np.array_equal(out["status"], host["status"])
        assert np.array_equal(out["n_charged"], host["n_charged"])
        for (e, b), m in zip(twins, mols):
            i = m["index"]
            if out["status"][i] == OK:
                verify(z["table_n"], z["table_opt"], e, b, out["order"][i, :len(b)], out["charge"][i, :len(e)], out["n_charged"][i])


def test_matching_against_networkx_on_random_graphs():
    """The matching alone, odd cycles included: random connected graphs of degree <= 4 whose atoms have ONE option each -- sulfur
    at degree 1 and carbon at 2 and 3 add a bond, carbon at 4 does not -- so a structure exists iff the atoms of degree <= 3 have
    a perfect matching among themselves.  Against networkx's maximum-cardinality matching."""
    import networkx as nx
    from gaudi_amd.gor2goa import atoms_list, c_valence_tables
    names = atoms_list(DATASET)
    S, C = names.index("S"), names.index("C")
    rng = np.random.default_rng(3220)
    mols, want, odd = [], [], 0
    while len(mols) < 600:
        n = int(rng.integers(4, 40))
        g = nx.Graph()
        g.add_nodes_from(range(n))
        for a in range(1, n):
            g.add_edge(a, int(rng.integers(a)))
        for _ in range(int(rng.integers(0, n))):
            a, b = (int(v) for v in rng.integers(n, size=2))
            if a != b and g.degree(a) < 3 and g.degree(b) < 3:
                g.add_edge(a, b)
        if max(d for _, d in g.degree()) > 4:
            continue
        sel = [a for a in range(n) if g.degree(a) <= 3]
        h = g.subgraph(sel)
        want.append(2 * len(nx.max_weight_matching(h, maxcardinality=True)) == len(sel))
        odd += want[-1] and not nx.is_bipartite(h)
        mols.append((np.array([S if g.degree(a) == 1 else C for a in range(n)], np.int32), np.array(list(g.edges()), np.int32)))
    out = _lib.host_bond_orders(c_valence_tables(DATASET), *pack(mols))
    assert set(out["status"].tolist()) <= {OK, NO_STRUCTURE}
    assert ((out["status"] == OK) == np.array(want)).all()
    assert sum(want) >= 50 and odd >= 20 and not out["n_charged"].any()


def test_the_search_gives_up_within_its_budget(g32):
    """GAVE_UP is 'undecided', not a verdict: the molecule has a structure with 4 charged atoms (checked by the verifier), the
    search does not reach it in this numbering and says so, and it does reach it when the four atoms come first.  Its neighbour
    in the batch is untouched."""
    from gaudi_amd.gor2goa import c_valence_tables
    z = g32[0]
    t = c_valence_tables(DATASET)
    e, b = budget_molecule()
    verify(z["table_n"], z["table_opt"], e, b, *budget_structure(), 4)
    benzene = next(m for m in g32[1] if m["special"] == OK)
    out = _lib.host_bond_orders(t, *pack([(e, b), benzene]))
    assert out["status"].tolist() == [GAVE_UP, OK] and not out["order"][0].any() and not out["charge"][0].any()
    assert out["n_charged"][0] == 0 and set(out["order"][1, :len(benzene["bonds"])].tolist()) == {1, 2}
    e2, b2 = budget_molecule(front=True)
    out = _lib.host_bond_orders(t, *pack([(e2, b2)]))
    assert out["status"][0] == OK and out["n_charged"][0] == 4
    verify(z["table_n"], z["table_opt"], e2, b2, out["order"][0, :len(b2)], out["charge"][0, :len(e2)], 4)


def test_a_structure_beyond_the_cap_is_capped(g32):
    """Six charged atoms are needed and six exist (the hand-built structure passes the verifier): none within the cap, one within
    the search -> CAPPED, under any numbering."""
    from gaudi_amd.gor2goa import c_valence_tables
    z = g32[0]
    e, b, orders, charges = six_charge_molecule()
    verify(z["table_n"], z["table_opt"], e, b, orders, charges, 6)
    mol = dict(elem=e, bonds=b)
    rng = np.random.default_rng(3230)
    out = _lib.host_bond_orders(c_valence_tables(DATASET), *pack([(e, b), relabel(mol, rng), relabel(mol, rng)]))
    assert out["status"].tolist() == [CAPPED] * 3 and not out["n_charged"].any() and not out["order"].any() and not out["charge"].any()


def test_a_failing_molecule_leaves_the_others_alone(g32, host):
    """Single-molecule calls give the bytes the whole-fixture call gave, on a sample that includes every special."""
    from gaudi_amd.gor2goa import c_valence_tables
    t = c_valence_tables(DATASET)
    mols = g32[1]
    picks = [m for m in mols if m["special"] >= 0] + mols[:12] + [m for m in mols if m["min_charged"] == 4]
    for m in picks:
        i, na, nb = m["index"], len(m["elem"]), len(m["bonds"])
        one = _lib.host_bond_orders(t, *pack([m]))
        assert one["status"][0] == host["status"][i] and one["n_charged"][0] == host["n_charged"][i]
        assert np.array_equal(one["order"][0, :nb], host["order"][i, :nb]) and np.array_equal(one["charge"][0, :na], host["charge"][i, :na])


def test_bad_tables_are_refused(g32):
    from gaudi_amd.gor2goa import c_valence_tables
    t = c_valence_tables(DATASET)
    t.option[2][3][0][1] = -1  # of two options the first must be neutral
    with pytest.raises(_lib.GaudiError):
        _lib.host_bond_orders(t, *pack(g32[1][:1]))
    elem, na, bonds, nb = pack(g32[1][:1])
    nb[0] = bonds.shape[1] + 1
    with pytest.raises(_lib.GaudiError):
        _lib.host_bond_orders(c_valence_tables(DATASET), elem, na, bonds, nb)


def _legacy_molfile(atoms3d, atom_types, bonds, dataset, comment):
    """The molfile text as the writer produced it before it knew orders and charges, restated."""
    from gaudi_amd.gor2goa import atoms_list
    names = atoms_list(dataset)
    sym = [names[int(t)] for t in atom_types]
    xyz = np.asarray(atoms3d, np.float64)
    out = [f"{comment}\n  gaudi_amd\n\n", f"{len(xyz):3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000\n"]
    for s, p in zip(sym, xyz):
        out.append(f"{p[0]:10.4f}{p[1]:10.4f}{p[2]:10.4f} {s:<3s} 0  0  0  0  0  0  0  0  0  0  0  0\n")
    for i, j in bonds:
        out.append(f"{i + 1:3d}{j + 1:3d}{1 if 'H' in (sym[i], sym[j]) else 4:3d}  0\n")
    return "".join(out) + "M  END\n"


def test_write_molfile(g32, host):
    from gaudi_amd.gor2goa import write_molfile
    mols = g32[1]
    m = next(m for m in mols if m["kind"] == 0 and (m["elem"] > 1).any() and host["status"][m["index"]] == OK)
    rng = np.random.default_rng(5)
    xyz = rng.standard_normal((len(m["elem"]), 3))
    f = io.StringIO()
    write_molfile(f, xyz, m["elem"], m["bonds"], DATASET, comment="g32")
    assert f.getvalue() == _legacy_molfile(xyz, m["elem"], m["bonds"], DATASET, "g32")
    # with orders and charges: a molecule with ten charged atoms' worth of lines is not in the fixture, so the charges are made up
    i, nb = m["index"], len(m["bonds"])
    charges = np.zeros(len(m["elem"]), np.int64)
    charges[:10] = [1, -1] * 5
    f = io.StringIO()
    write_molfile(f, xyz, m["elem"], m["bonds"], DATASET, comment="g32", orders=host["order"][i, :nb], charges=charges)
    lines = f.getvalue().splitlines()
    bond_lines = lines[4 + len(m["elem"]): 4 + len(m["elem"]) + nb]
    assert [int(l[6:9]) for l in bond_lines] == host["order"][i, :nb].tolist() and {int(l[6:9]) for l in bond_lines} == {1, 2}
    chg = [l for l in lines if l.startswith("M  CHG")]
    assert chg == ["M  CHG  8   1   1   2  -1   3   1   4  -1   5   1   6  -1   7   1   8  -1", "M  CHG  2   9   1  10  -1"]
    assert lines[-1] == "M  END"
    # a real charged structure: the CHG entries are its nonzero charges
    q = next(m for m in mols if m["min_charged"] == 2)
    j = q["index"]
    f = io.StringIO()
    write_molfile(f, np.zeros((len(q["elem"]), 3)), q["elem"], q["bonds"], DATASET, orders=host["order"][j, :len(q["bonds"])],
                  charges=host["charge"][j, :len(q["elem"])])
    entry = next(l for l in f.getvalue().splitlines() if l.startswith("M  CHG")).split()
    assert int(entry[2]) == 2 and sorted(int(v) for v in entry[4::2]) == [-1, 1]
