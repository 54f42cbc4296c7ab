"""CPU tests of tests/boo_model.py, the restatement of the bond-orientational order contract (aztot_boo_*), and of the 'boo' directive of control.txt.

The independent oracle is the addition theorem, q_l(i)^2 = (1 / n_i^2) sum_{j, k in N(i)} P_l(u_j . u_k): it never touches a spherical harmonic, so it
catches normalisation and phase mistakes.  Known answers (quoted to six decimals) are held to 5e-7."""
import ctypes as C
import math
import os

import mpmath
import numpy as np
import pytest

from aztotmd_amd import api, inputs

import boo_model as bm

ORDERS = tuple(range(1, 13))


def legendre(l, x):
    p0, p1 = mpmath.mpf(1), x
    for k in range(2, l + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    return p1 if l else p0


def addition_theorem(vectors, l):
    with mpmath.workdps(50):
        u = [[mpmath.mpf(float(c)) for c in v] for v in vectors]
        u = [[c / mpmath.sqrt(sum(d * d for d in v)) for c in v] for v in u]
        s = sum(legendre(l, sum(a * b for a, b in zip(p, q))) for p in u for q in u)
        return mpmath.sqrt(max(s, 0)) / len(u)


def fcc_lattice(n, a=4.0):
    base = np.array([(0, 0, 0), (0.5, 0.5, 0), (0.5, 0, 0.5), (0, 0.5, 0.5)])
    cells = np.array([(i, j, k) for i in range(n) for j in range(n) for k in range(n)])
    return ((cells[:, None, :] + base[None, :, :]).reshape(-1, 3) * a + 0.25), (n * a,) * 3


def test_harmonics_are_the_standard_ones():
    """Y_lm of single bonds against mpmath.spherharm (orthonormal, Condon-Shortley phase), bonds along +-z and in the xy-plane included"""
    rng = np.random.default_rng(11)
    worst = mpmath.mpf(0)
    with mpmath.workdps(50):
        for v in list(rng.normal(size=(3, 3))) + [[0, 0, 2.5], [0, 0, -1.25], [1.5, 0, 0], [-0.75, 0, 0], [0.6, -0.8, 0]]:
            v = np.asarray(v, dtype=np.float64)
            B = bm.shell([v])
            x = [mpmath.mpf(float(c)) for c in v]
            r = mpmath.sqrt(sum(c * c for c in x))
            theta, phi = mpmath.acos(x[2] / r), mpmath.atan2(x[1], x[0])
            for l in ORDERS:
                re, im = bm.exact_qlm(B, l)
                for m in range(l + 1):
                    y = mpmath.spherharm(l, m, theta, phi)
                    worst = max(worst, abs(mpmath.mpf(int(re[0, m])) / bm.ONE - y.real), abs(mpmath.mpf(int(im[0, m])) / bm.ONE - y.imag))
    print("worst |Y_lm - mpmath|", mpmath.nstr(worst, 5))
    assert worst < mpmath.mpf(10) ** -45


def test_addition_theorem_on_random_shells():
    rng = np.random.default_rng(5)
    worst = 0.0
    for n in (1, 2, 3, 5, 8, 12, 14):
        v = rng.normal(size=(n, 3)) * rng.uniform(0.5, 3.0, size=(n, 1))
        B = bm.shell(v)
        for l in ORDERS:
            re, im = bm.exact_qlm(B, l)
            q = bm.exact_invariant(re, im, l)
            with mpmath.workdps(50):
                worst = max(worst, float(abs(mpmath.mpf(int(q[0])) / bm.ONE - addition_theorem(v, l))))
    print("worst |q_l - addition theorem|", worst)
    assert worst < 1e-40


@pytest.mark.parametrize("name", sorted(bm.KNOWN))
def test_known_answers(name):
    make, want = bm.KNOWN[name]
    got = [bm.shell_q(make(), l) for l in bm.KNOWN_ORDERS]
    print(name, got)
    for g, w in zip(got, want):
        assert abs(g - w) <= bm.KNOWN_TOL
    # and through the fp64 route
    B = bm.shell(make())
    for l, w in zip(bm.KNOWN_ORDERS, want):
        assert abs(bm.invariant(bm.route_qlm(B, l), l)[0] - w) <= bm.KNOWN_TOL


def test_simple_cubic_exact_values():
    assert abs(bm.shell_q(bm.sc_shell(), 4) - math.sqrt(7.0 / 12.0)) < 1e-15 and abs(bm.shell_q(bm.sc_shell(), 6) - math.sqrt(1.0 / 8.0)) < 1e-15


def test_single_and_opposite_neighbours():
    """one neighbour in any direction (exactly +-z and in the xy-plane included): q_l = 1 for every l; two opposite ones: 1 for even l, 0 for odd l"""
    for v in ([0, 0, 1.5], [0, 0, -2.0], [1.0, 0, 0], [0.3, -0.4, 0], [0.1, 0.7, -0.2]):
        for l in ORDERS:
            assert abs(bm.shell_q([v], l) - 1.0) < 1e-15, (v, l)
            assert abs(bm.invariant(bm.route_qlm(bm.shell([v]), l), l)[0] - 1.0) < bm.Q_TOL
            both = bm.shell_q([v, [-c for c in v]], l)
            assert abs(both - (1.0 if l % 2 == 0 else 0.0)) < 1e-30, (v, l)


def test_fcc_lattice_average_equals_plain():
    """a perfect FCC lattice, R between the first and the second shell: every atom has 12 neighbours, q-bar_l = q_l = the known answer"""
    pos, box = fcc_lattice(3)
    types = np.zeros(len(pos), dtype=np.int64)
    B = bm.bonds(pos, types, box, 0.5 * (4.0 / math.sqrt(2.0) + 4.0), 1, 1)
    assert (B.n == 12).all()
    for l, w in zip(bm.KNOWN_ORDERS, bm.KNOWN["fcc"][1]):
        q, qbar = bm.exact_q(B, l)
        assert np.abs(q - w).max() <= bm.KNOWN_TOL and np.abs(qbar - q).max() < 1e-15
        qlm = bm.route_qlm(B, l)
        assert np.abs(bm.invariant(bm.averaged(B, qlm), l) - w).max() <= bm.KNOWN_TOL


def test_route_matches_the_exact_values():
    rng = np.random.default_rng(2)
    pos = np.round(rng.random((400, 3)) * 12.0, 6)
    types = np.arange(400) % 2
    B = bm.bonds(pos, types, (12.0, 12.0, 12.0), 2.4, 3, 3)
    assert 3 < B.n.mean() < 20
    err = bm.route_error(B, ORDERS)
    print("route error", err, "bound", bm.QLM_TOL)
    assert err <= bm.QLM_TOL
    for l in (4, 12):
        qlm = bm.route_qlm(B, l)
        q, qbar = bm.exact_q(B, l)
        assert np.abs(bm.invariant(qlm, l) - q).max() <= bm.Q_TOL and np.abs(bm.invariant(bm.averaged(B, qlm), l) - qbar).max() <= bm.Q_TOL


def test_route_worst_is_the_measured_figure():
    """the case that sets ROUTE_WORST, measured again: the constant is that figure, not a guess (every operation of the route is correctly rounded, so
    the figure does not depend on the machine)"""
    import boo_cases as bc
    c = [c for c in bc.mask_cases() if c["name"] == "order12_alone"][0]
    pos, types = bc.positions_of(c["case"])
    err = bm.route_error(bm.bonds(pos, types, c["box"], c["R"], c["central"], c["ligand"]), c["orders"])
    print("measured", err, "ROUTE_WORST", bm.ROUTE_WORST, "QLM_TOL", bm.QLM_TOL)
    assert 0.99 * bm.ROUTE_WORST <= err <= bm.ROUTE_WORST and bm.QLM_TOL == 4.0 * bm.ROUTE_WORST


def mutation_case():
    """a cluster near a box face (so that the minimum image matters), one partner exactly at distance R, two species"""
    box = (10.0, 10.0, 10.0)
    pos = np.array([(0.5, 5.0, 5.0), (9.5, 5.0, 5.0), (0.5, 6.5, 5.0), (1.5, 5.0, 6.0), (0.5, 5.0, 3.0), (2.0, 6.0, 5.5), (9.0, 4.0, 4.5), (1.25, 4.25, 5.5)])
    types = np.array([0, 0, 0, 1, 0, 1, 0, 0])
    return pos, types, box, 2.0           # atom 4 is exactly 2.0 from atom 0


@pytest.mark.parametrize("mutate", ["no_factor2", "inverted_factorial", "inclusive", "self", "div_by_C", "no_image"])
def test_mutations_are_caught(mutate):
    pos, types, box, R = mutation_case()
    B, Bm = bm.bonds(pos, types, box, R, 1, 3), bm.bonds(pos, types, box, R, 1, 3, mutate=mutate)
    assert B.n[0] == 6 and B.n[3] == -1
    moved = 0.0
    for l in (4, 6):
        q, qbar = bm.exact_q(B, l)
        qm, qbarm = bm.exact_q(Bm, l, mutate)
        moved = max(moved, np.abs(qbarm - qbar).max() if mutate == "div_by_C" else np.abs(qm - q).max())
    print(mutate, "moves a value by", moved)
    assert moved > 1e-3
    if mutate in ("no_factor2", "inverted_factorial"):      # and the known answers notice
        assert abs(bm.shell_q(bm.fcc_shell(), 6, mutate) - bm.KNOWN["fcc"][1][1]) > 1e-2


def test_bins_sums_and_values():
    q = np.zeros((6, 1, 2))
    q[:, 0, 0] = [0.0, 0.25, 0.5, 0.999999, 1.0, 0.3]
    q[:, 0, 1] = [0.1, 0.1, 0.2, 0.2, 0.3, 0.9]
    n = np.array([3, 1, 0, 2, 4, -1])
    types = np.array([0, 1, 0, 1, 0, 1])
    assert list(bm.bin_of(q[:, 0, 0], 4)) == [0, 1, 2, 3, 3, 1]
    hist, sums, entered = bm.totals(n, q, types, 2, 4)
    assert list(entered) == [2, 2] and hist.sum() == 8
    assert list(hist[0, 0, 0]) == [1, 0, 0, 1] and list(hist[0, 0, 1]) == [0, 1, 0, 1]
    assert sums[0, 0, 0] == 0.0 + 1.0 and sums[0, 0, 1] == 0.25 + 0.999999
    centre, dens, mean = bm.values(hist, sums, entered)
    assert list(centre) == [0.125, 0.375, 0.625, 0.875] and np.allclose(dens.sum(axis=-1) / 4, 1.0) and mean[0, 0, 0] == 0.5


# ---- the 'boo' directive of control.txt through the library's parser ----
def lj2(**kw):
    return dict(inputs.lj_case((4, 4, 4), charges=(0.0, 0.0)), **kw)


def control_with(tmp_path, block):
    d = inputs.write_input_files(lj2(), str(tmp_path / "d"))
    with open(os.path.join(d, "control.txt"), "a") as f:
        f.write(block + "\n")
    return d


def test_directive_round_trips(tmp_path):
    d = inputs.write_input_files(lj2(boo=(4.5, 100, 10, [4, 6], ["A"], ["A", "B"])), str(tmp_path / "d"))
    # R, n_bins, every, central_mask, ligand_mask, n_orders, the orders
    assert list(api.Model.from_dir(d).query("boo")) == [4.5, 100, 10, 1, 3, 2, 4, 6]
    plain = inputs.write_input_files(lj2(), str(tmp_path / "p"))
    assert list(api.Model.from_dir(plain).query("boo")) == [0, 0, 0, 0, 0, 0]
    ctl = open(os.path.join(plain, "control.txt")).read()
    assert "boo" not in ctl and ctl == "".join(l for l in open(os.path.join(d, "control.txt")) if not l.startswith("boo"))
    assert list(api.Model.from_case(lj2()).query("boo")) == [0, 0, 0, 0, 0, 0]
    # free format, every == 0, four orders, the lists in any order
    m = api.Model.from_dir(control_with(tmp_path, "boo 3.25 1 0\n4 12 1 6 2\n1 B\n2 B A"))
    assert list(m.query("boo")) == [3.25, 1, 0, 2, 3, 4, 12, 1, 6, 2]


@pytest.mark.parametrize("block,code", [
    ("boo x 100 10 1 6 1 A 1 A", "ERROR[419]"),                 # R is no number
    ("boo 4.5 100 10 1 6 1 A", "ERROR[419]"),                   # the ligand list is missing
    ("boo 4.5 100 10 2 6 1 A 1 A", "ERROR[419]"),               # an order short: 'A' is no number
    ("boo -4.5 100 10 1 6 1 A 1 A", "ERROR[419]"),              # out-of-range numbers
    ("boo 4.5 0 10 1 6 1 A 1 A", "ERROR[419]"),
    ("boo 4.5 4097 10 1 6 1 A 1 A", "ERROR[419]"),
    ("boo 4.5 100 10 0 1 A 1 A", "ERROR[419]"),
    ("boo 4.5 100 10 5 1 2 3 4 5 1 A 1 A", "ERROR[419]"),
    ("boo 4.5 100 10 1 0 1 A 1 A", "ERROR[419]"),
    ("boo 4.5 100 10 1 13 1 A 1 A", "ERROR[419]"),
    ("boo 4.5 100 10 1 6 0 1 A", "ERROR[419]"),
    ("boo 4.5 100 10 1 6 3 A B A 1 A", "ERROR[419]"),           # more names than species
    ("boo 4.5 100 -1 1 6 1 A 1 A", "ERROR[419]"),               # negative period
    ("boo 4.5 100 10 2 6 6 1 A 1 A", "ERROR[419]"),             # repeated order
    ("boo 4.5 100 10 1 6 1 Xe 1 A", "ERROR[420]"),              # unknown species
    ("boo 4.5 100 10 1 6 1 A 1 Xe", "ERROR[420]"),
    ("boo 4.5 100 10 1 6 1 A 2 B B", "ERROR[420]"),             # repeated species
])
def test_bad_directives_are_refused(tmp_path, block, code):
    with pytest.raises(api.AztotError) as e:
        api.Model.from_dir(control_with(tmp_path, block))
    assert code in str(e.value)


def test_entry_points_refuse_null_handles():
    L = api.lib()
    p = api._BooParams()
    assert L.aztot_boo_setup(None, C.byref(p)) == -4
    for f in (L.aztot_boo_sample, L.aztot_boo_reset):
        assert f(None) == -4
    assert L.aztot_boo_shape(None, None, None, None, None, None) == -4
    assert L.aztot_boo_per_atom(None, None, None, 0) == -4 and L.aztot_boo_qlm(None, None, 0) == -4
    assert L.aztot_boo_counts(None, None, None, None, None, 0) == -4 and L.aztot_boo_values(None, None, None, None, 0) == -4


def test_exports_and_struct():
    for n in ("setup", "sample", "reset", "shape", "per_atom", "qlm", "counts", "values"):
        assert "aztot_boo_" + n in api.EXPORTS and hasattr(api.lib(), "aztot_boo_" + n)
    assert C.sizeof(api._BooParams) == 48
