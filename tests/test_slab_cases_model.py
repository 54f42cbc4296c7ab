"""The replicated boxes of tests/slab_cases.py are what they claim to be (CPU, numpy only): exact translates with ids and bonded lists copied by offset, the
cell grid the slab engine will choose, slabs one period wide and no atom on a slab boundary."""
import numpy as np
import pytest

import slab_cases as sc

SYSTEMS = ("lj", "fennell", "hot", "mol")
RANKS = (2, 3, 4)


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("interleaved", [False, True])
def test_copies_are_exact_translates(name, n, interleaved):
    per, box = sc.period(name), sc.replicate(sc.period(name), n, interleaved)
    if interleaved == sc.INTERLEAVED:
        assert all(np.array_equal(box[k], sc.box_case(name, n)[k]) for k in ("x", "y", "z", "vx", "types"))
    n0, L = len(per["types"]), n * sc.P
    assert box["box"] == [L, sc.P, sc.P] and len(box["types"]) == n * n0
    for k in ("x", "y", "z"):                             # every coordinate, p and n p are multiples of 2^-20 A: x + k p is exact
        v = np.asarray(per[k]) * sc.Q
        assert np.array_equal(v, np.round(v)), k
    assert sc.P * sc.Q == round(sc.P * sc.Q)
    x0 = np.mod(np.asarray(per["x"]), L)
    for k in range(n):
        s = sc.copy_ids(n, n0, k, interleaved)
        assert np.array_equal(s, np.arange(k * n0, (k + 1) * n0) if not interleaved else np.arange(n0) * n + k)
        assert np.array_equal(np.mod(box["x"][s] - k * sc.P, L), x0), (name, n, k)
        for key in ("y", "z", "vx", "vy", "vz", "types"):
            assert np.array_equal(box[key][s], np.asarray(per[key])), (name, n, k, key)
    for key in ("x", "y", "z"):
        assert box[key].min() >= 0.0 and box[key].max() < box["box"]["xyz".index(key)]
    # a full-box state made of exact copies has no divergence at all, one copy moved by an ulp has one
    state = {k: box[k] for k in ("x", "y", "z", "vx", "vy", "vz")}
    assert set(sc.divergence(state, n, sc.P, box["box"], interleaved).values()) == {0.0}
    moved = dict(state, x=box["x"].copy())
    one = sc.copy_ids(n, n0, 1, interleaved)
    j = one[int(np.argmax(box["x"][one]))]
    moved["x"][j] = np.nextafter(moved["x"][j], 0.0)
    d = sc.divergence(moved, n, sc.P, box["box"], interleaved)
    assert 0.0 < d["x"] < 1e-15 and d["y"] == 0.0


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("n", RANKS)
def test_bonds_and_angles_are_copied_with_the_id_offset(n, interleaved):
    per, box = sc.period("mol"), sc.replicate(sc.period("mol"), n, interleaved)
    n0, nb, na = len(per["types"]), len(per["bonds"]), len(per["angles"])
    assert len(box["bonds"]) == n * nb and len(box["angles"]) == n * na
    for k in range(n):
        b, a = box["bonds"][k * nb:(k + 1) * nb], box["angles"][k * na:(k + 1) * na]
        if interleaved:
            assert np.array_equal(b[:, :2], per["bonds"][:, :2] * n + k) and np.array_equal(a[:, :3], per["angles"][:, :3] * n + k)
        else:
            assert np.array_equal(b[:, :2], per["bonds"][:, :2] + k * n0) and np.array_equal(a[:, :3], per["angles"][:, :3] + k * n0)
        assert np.array_equal(b[:, 2], per["bonds"][:, 2]) and np.array_equal(a[:, 3], per["angles"][:, 3])
    # every bond of the box is a bond: about 1 A long to the nearest image, also across the seams and the periodic wall
    pos = np.stack([box["x"], box["y"], box["z"]], axis=1)
    d = pos[box["bonds"][:, 0]] - pos[box["bonds"][:, 1]]
    d -= np.array(box["box"]) * np.round(d / np.array(box["box"]))
    r = np.sqrt((d ** 2).sum(1))
    assert 0.9 < r.min() and r.max() < 1.1, (r.min(), r.max())
    # ... and some molecules straddle every slab boundary (their atoms have different owners)
    own = sc.owner(box["x"], n, box["box"][0])
    across = own[box["bonds"][:, 0]] != own[box["bonds"][:, 1]]
    for r_ in range(n):
        ends = np.stack([own[box["bonds"][across, 0]], own[box["bonds"][across, 1]]], axis=1)
        assert (np.sort(ends, axis=1) == sorted((r_, (r_ + 1) % n))).all(axis=1).sum() >= 10, (n, r_)


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("name", SYSTEMS)
def test_grid_and_slab_width(name, n):
    box = sc.box_case(name, n)
    dims, hw, width = sc.expected_grid(box, n)
    assert dims == (n * sc.K, 3, 3) and sc.K >= 3
    assert hw == 1                                        # so every rank has K - 2 >= 1 interior layers for the overlapped exchange
    assert width == sc.P
    assert box["cell_list"] == sc.CELL_SIZE
    # the margin of the cell size: a size of exactly p / 3 could come out one layer short, this one cannot, and it adds none either
    for m in RANKS:
        assert int(np.floor(m * sc.P / sc.CELL_SIZE)) == m * sc.K


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("name", SYSTEMS)
def test_no_atom_starts_on_a_slab_boundary(name, n):
    box = sc.box_case(name, n)
    L = box["box"][0]
    assert sc.seam_distance(box["x"], n, L).min() > 1e-6
    # the seam plane: atoms on both sides of every boundary, within reach of it
    d = np.mod(box["x"], sc.P)
    near = 0.05 if name != "mol" else 0.12
    assert ((d < near).sum() >= 10 * n) and ((d > sc.P - near).sum() >= 10 * n)
    # owner() agrees with the boundaries
    own = sc.owner(box["x"], n, L)
    lo = sc.boundaries(n, L)
    assert np.all(box["x"] >= lo[own]) and np.all(box["x"] < lo[own] + sc.P)
    assert np.array_equal(np.bincount(own, minlength=n), np.full(n, len(box["types"]) // n))


def test_owner_at_the_boundaries_themselves():
    for n in RANKS:
        L = n * sc.P
        lo = sc.boundaries(n, L)
        assert np.array_equal(sc.owner(lo, n, L), np.arange(n))
        assert np.array_equal(sc.owner(np.nextafter(lo[1:], 0.0), n, L), np.arange(n - 1))
        assert sc.owner(np.nextafter(L, 0.0), n, L) == n - 1


def test_the_stray_bond_reaches_past_the_halo():
    c, j, partner = sc.stray_bond_case()
    n = 3
    dims, hw, _ = sc.expected_grid(c, n)
    csz = c["box"][0] / dims[0]
    assert partner == j + 1 and j % n == 0                   # copies 0 and 1 of one atom, interleaved numbering
    lj, lp = int(c["x"][j] // csz), int(c["x"][partner] // csz)
    assert sc.owner(c["x"][j], n, c["box"][0]) == 0 and lj == 1 and lp == 4
    resident = set(range(0, sc.K)) | {sc.K, dims[0] - 1}           # rank 0: its own layers and hw = 1 ghost layer on either side
    assert hw == 1 and lp not in resident
