"""CPU tests of the bond-angle distribution contract (tests/adf_model.py, include/aztot.h 'bond-angle distributions'): the edge table, the bin rule against
the exact angle, designed exact cases, mutations of the model that it must notice, and the 'adf' block of control.txt with its model query."""
import ctypes as C
import os

import mpmath
import numpy as np
import pytest

from aztotmd_amd import api, inputs

import adf_model as am

BINS = (1, 7, 8, 180, 3600)
EDGE_DEG = 1e-9


def ulp_distance(a, exact):
    a = float(a)
    if a == 0.0:
        return abs(exact) / mpmath.mpf(5e-324)
    return abs(mpmath.mpf(a) - exact) / mpmath.mpf(float(np.spacing(abs(a))))


@pytest.mark.parametrize("n_bins", BINS)
def test_edge_table(n_bins):
    T = am.edges(n_bins)
    assert T.shape == (n_bins + 1,) and T.dtype == np.float64
    assert (np.diff(T) < 0).all()                       # strictly decreasing
    assert T[0] == 1.0 and T[-1] == -1.0
    if n_bins % 2 == 0:
        assert T[n_bins // 2] == 0.0
    worst = 0.0
    with mpmath.workdps(50):
        for b in range(1, n_bins):
            if 2 * b == n_bins:                         # exactly 0, asserted above (a 50-digit cos(pi / 2) is 1e-51, not 0)
                continue
            c = mpmath.cos(mpmath.pi * b / n_bins)
            worst = max(worst, float(ulp_distance(T[b], c * abs(c))))
    print("n_bins", n_bins, "worst distance from the 50-digit value, ulp:", worst)
    assert worst <= 2.0


def random_triplets(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3)) * rng.uniform(0.5, 4.5, size=(n, 1))
    v = rng.normal(size=(n, 3)) * rng.uniform(0.5, 4.5, size=(n, 1))
    return u, v


def rule_bins(u, v, T):
    dot = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
    r2u = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
    r2v = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return dot * np.abs(dot), r2u * r2v


@pytest.mark.parametrize("n_bins", BINS)
def test_rule_is_floor_of_the_angle(n_bins):
    """fp64 acos on 20 000 triplets and the 50-digit angle on 400 of them: the seed is one for which no triplet lies within 1e-9 degrees of an edge
    (asserted), so fp64 acos (good to about 1e-13 degrees here) decides every one of them and none is left out"""
    T = am.edges(n_bins)
    width = 180.0 / n_bins
    u, v = random_triplets(20000, seed=1000 + n_bins)
    s, p = rule_bins(u, v, T)
    got = am.bin_of(s, p, T)
    dot = (u * v).sum(axis=1)
    theta = np.degrees(np.arccos(np.clip(dot / np.sqrt((u * u).sum(axis=1) * (v * v).sum(axis=1)), -1.0, 1.0)))
    inner = np.arange(1, n_bins) * width
    gap = np.abs(theta[:, None] - inner[None, :]).min() if n_bins > 1 else np.inf
    print("n_bins", n_bins, "closest triplet to an edge, degrees:", gap)
    assert gap > EDGE_DEG
    assert np.array_equal(got, np.minimum(np.floor(theta / width).astype(np.int64), n_bins - 1))
    assert np.array_equal(got[:3000], am.bin_of_plain(s[:3000], p[:3000], T))           # the corrected estimate is the literal count
    for k in range(400):
        e = am.exact_angle(u[k], v[k])
        assert got[k] == min(int(mpmath.floor(e / width)), n_bins - 1), (k, float(e))


@pytest.mark.parametrize("n_bins", [8, 100, 180, 3600])
def test_designed_exact_cases(n_bins):
    """0, 60, 90, 120 and 180 degrees on a lattice of multiples of 0.5.  0, 90 and 180 sit on forced edges and fall into bins 0, n / 2 and n - 1 whatever
    n_bins; 60 and 120 are inside a bin for n_bins = 8 and 100"""
    T = am.edges(n_bins)
    assert am.rule_bin((1.0, 0.5, 0.0), (2.0, 1.0, 0.0), T) == 0
    assert am.rule_bin((1.5, 0.0, 0.0), (0.0, 0.0, 2.5), T) == n_bins // 2
    assert am.rule_bin((0.5, 0.5, 0.0), (0.5, -0.5, 3.0), T) == n_bins // 2
    assert am.rule_bin((1.0, 0.5, 0.0), (-2.0, -1.0, 0.0), T) == n_bins - 1
    if n_bins in (8, 100):
        assert am.rule_bin((1.0, 1.0, 0.0), (1.0, 0.0, 1.0), T) == int(60 * n_bins // 180)
        assert am.rule_bin((0.5, 0.5, 0.0), (0.0, -1.5, 1.5), T) == int(120 * n_bins // 180)
        assert am.rule_bin((1.0, 1.0, 0.0), (-1.0, 0.0, 1.0), T) == int(120 * n_bins // 180)


def designed_system():
    """random atoms of two species in a small box (every shell reaches across a face), plus designed atoms around atom 0 (species 0, at (2, 2, 2)):
    a partner at exactly R = 2.5 (inclusive shell test), partners at exactly 90 degrees (< instead of <= in the bin rule), an atom coincident
    with atom 0, and a species-1 partner between the two radii of the mixed column"""
    rng = np.random.default_rng(77)
    box = (7.0, 7.5, 8.0)
    pos = np.round(rng.random((160, 3)) * np.asarray(box), 3)
    types = (np.arange(160) % 2).astype(np.int32)
    pos[0] = (2.0, 2.0, 2.0)
    pos[1] = (4.5, 2.0, 2.0); types[1] = 0          # exactly 2.5 along x
    pos[2] = (2.0, 3.5, 2.0); types[2] = 0          # 90 degrees with atom 4
    pos[4] = (2.0, 2.0, 3.0); types[4] = 0
    pos[6] = (2.0, 2.0, 2.0); types[6] = 0          # coincident with atom 0
    pos[3] = (2.0, 2.0, 5.25); types[3] = 1         # 3.25 from atom 0: inside R_b = 3.5, outside R_a = 2.5
    cols = [(0, 0, 0, 2.5, 2.5), (0, 1, 0, 3.5, 2.5), (1, 0, 1, 2.0, 3.0)]
    return pos, types, box, cols


def test_model_basics():
    pos, types, box, cols = designed_system()
    T = am.edges(8)
    counts, neigh = am.host_adf(pos, types, box, cols, T)
    # both orders of the ligands name the same column
    swapped = [(c, b, a, rb, ra) for c, a, b, ra, rb in cols]
    c2, n2 = am.host_adf(pos, types, box, swapped, T)
    assert np.array_equal(counts, c2) and np.array_equal(neigh, n2)
    # totals: pairs of neighbours per central atom
    L = np.asarray(box)
    for k, (c, a, b, ra, rb) in enumerate(am.normalise(cols)):
        tot = 0
        for i in np.flatnonzero(types == c):
            d = pos - pos[i]
            d = np.where(d > L / 2, d - L, np.where(d < -L / 2, d + L, d))
            r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            na = int(((r2 > 0) & (r2 < ra * ra) & (types == a)).sum())
            nb = int(((r2 > 0) & (r2 < rb * rb) & (types == b)).sum())
            tot += na * (na - 1) // 2 if a == b else na * nb
        assert counts[:, k].sum() == tot and tot > 0
    assert (neigh >= 0).all() and neigh.max() < am.MAX_NEIGHBOURS
    theta, p = am.values(counts)
    assert np.allclose(p.sum(axis=0), 8 / 180.0) and theta[0] == 11.25


@pytest.mark.parametrize("mutation", ["twice", "inclusive", "no_image", "strict_bin", "ra_both", "coincident"])
def test_mutations_are_caught(mutation):
    pos, types, box, cols = designed_system()
    T = am.edges(8)
    counts, neigh = am.host_adf(pos, types, box, cols, T)
    c2, n2 = am.host_adf(pos, types, box, cols, T, mutate=mutation)
    print(mutation, "cells that differ:", int((counts != c2).sum()), "atoms whose neighbour count differs:", int((neigh != n2).sum()))
    assert not np.array_equal(counts, c2)


def test_single_species_no_atoms_of_a_column():
    pos, types, box, _ = designed_system()
    counts, neigh = am.host_adf(pos, types, box, [(2, 0, 1, 3.0, 3.0), (0, 2, 2, 3.0, 3.0)], am.edges(8))
    assert not counts.any() and (neigh[types == 0] == 0).all() and (neigh[types == 1] == -1).all()


# ---- the 'adf' block of control.txt and the model query ----
def lj2(**kw):
    case = inputs.lj_case((4, 4, 4), charges=(0.0, 0.0))
    return dict(case, **kw)


def control_with(tmp_path, block):
    d = inputs.write_input_files(lj2(), str(tmp_path / "d"))
    with open(os.path.join(d, "control.txt"), "a") as f:
        f.write(block + "\n")
    return d


def test_block_round_trips(tmp_path):
    cols = [("A", "A", "A", 3.5, 3.5), ("A", "B", "A", 4.25, 3.0), ("B", "A", "B", 2.5, 4.0)]
    d = inputs.write_input_files(lj2(adf=(180, 10, cols)), str(tmp_path / "d"))
    m = api.Model.from_dir(d)
    # n_bins, every, n, then per line central, ligand_a, ligand_b, R_a, R_b (the ligands in the order of the line)
    assert list(m.query("adf")) == [180, 10, 3, 0, 0, 0, 3.5, 3.5, 0, 1, 0, 4.25, 3.0, 1, 0, 1, 2.5, 4.0]
    plain = inputs.write_input_files(lj2(), str(tmp_path / "p"))
    assert list(api.Model.from_dir(plain).query("adf")) == [0, 0, 0]
    ctl = open(os.path.join(plain, "control.txt")).read()
    assert "adf" not in ctl
    assert ctl == "".join(l for l in open(os.path.join(d, "control.txt")) if not l.startswith(("adf", "A A", "A B", "B A")))
    assert list(api.Model.from_case(lj2()).query("adf")) == [0, 0, 0]
    # every == 0: one sample of the final configuration
    m = api.Model.from_dir(control_with(tmp_path, "adf 1 0 1\nB B B 2.0 2.0"))
    assert list(m.query("adf")) == [1, 0, 1, 1, 1, 1, 2.0, 2.0]


@pytest.mark.parametrize("block,code", [
    ("adf x 10 1\nA A A 3.0 3.0", "ERROR[416]"),                    # n_bins is no number
    ("adf 180 10\nA A A 3.0 3.0", "ERROR[416]"),                    # the number of lines is missing
    ("adf 0 10 1\nA A A 3.0 3.0", "ERROR[416]"),                    # n_bins outside [1, 3600]
    ("adf 3601 10 1\nA A A 3.0 3.0", "ERROR[416]"),
    ("adf 180 -1 1\nA A A 3.0 3.0", "ERROR[416]"),                  # negative every
    ("adf 180 10 0", "ERROR[416]"),                                  # no line
    ("adf 180 10 65\nA A A 3.0 3.0", "ERROR[416]"),                 # more than AZTOT_ADF_MAX_COLUMNS
    ("adf 180 10 2\nA A A 3.0 3.0", "ERROR[416]"),                  # a line short
    ("adf 180 10 1\nA A A 3.0", "ERROR[416]"),
    ("adf 180 10 1\nA A A 3.0 -3.0", "ERROR[416]"),                 # a radius that is not positive
    ("adf 180 10 1\nXe A A 3.0 3.0", "ERROR[417]"),                 # unknown species
    ("adf 180 10 1\nA A Xe 3.0 3.0", "ERROR[417]"),
    ("adf 180 10 2\nA A B 3.0 3.5\nA B A 3.5 3.0", "ERROR[417]"),   # the same column twice (ligands swapped)
    ("adf 180 10 1\nA B B 3.0 3.5", "ERROR[417]"),                  # unequal radii for equal ligands
])
def test_bad_blocks_are_refused(tmp_path, block, code):
    with pytest.raises(api.AztotError) as e:
        api.Model.from_dir(control_with(tmp_path, block))
    assert code in str(e.value)


def test_entry_points_refuse_null_handles():
    L = api.lib()
    col = api._AdfColumn(0, 0, 0, 0, 3.5, 3.5)
    assert L.aztot_adf_setup(None, 8, C.byref(col), 1) == -4
    for f in (L.aztot_adf_sample, L.aztot_adf_reset):
        assert f(None) == -4
    assert L.aztot_adf_shape(None, None, None, None) == -4
    assert L.aztot_adf_edges(None, None, 0) == -4 and L.aztot_adf_counts(None, None, None, 0) == -4
    assert L.aztot_adf_values(None, None, None, 0) == -4 and L.aztot_adf_neighbours(None, None, 0) == -4


def test_exports_and_struct():
    for n in ("setup", "sample", "reset", "shape", "edges", "counts", "values", "neighbours"):
        assert "aztot_adf_" + n in api.EXPORTS and hasattr(api.lib(), "aztot_adf_" + n)
    assert C.sizeof(api._AdfColumn) == 32
