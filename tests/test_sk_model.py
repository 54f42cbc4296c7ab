"""CPU tests of tests/sk_model.py, the numpy restatement of the structure-factor contract (aztot_sk_*, include/aztot.h): the vector set against a brute-force
enumeration, the fp64 route of the kernels against 50-digit amplitudes, known answers, the six mutations the checks must catch, and the 'strfac' directive
with its model query (host code of the library: no GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

from aztotmd_amd import api, inputs

import sk_model as sm

CUBE = (11.0, 11.0, 11.0)
BRICK = (7.0, 14.0, 21.0)                   # 1 : 2 : 3


# ---- the vector set ----
@pytest.mark.parametrize("box,kmax,dk,H", [(CUBE, 3.3, 0.25, 6), (BRICK, 2.75, 0.2, 10)])
def test_set_equals_brute_force(box, kmax, dk, H):
    vs = sm.vector_set(box, kmax, dk)
    assert np.abs(vs["lmn"]).max() < H                                      # the cube of the enumeration holds the whole sphere
    lmn, b = sm.brute_force_set(box, kmax, dk, H)
    assert len(lmn) > 300
    assert np.array_equal(vs["lmn"], lmn) and np.array_equal(vs["bin"], b)
    assert vs["n_bins"] == int(kmax * (1.0 / dk)) and np.array_equal(vs["n_in_bin"], np.bincount(b, minlength=vs["n_bins"]))
    # one of each +-k: no vector's negative is in the set
    have = {tuple(v) for v in lmn.tolist()}
    assert not any((-l, -m, -n) in have for l, m, n in have)
    # the order is lexicographic
    assert lmn.tolist() == sorted(lmn.tolist())


@pytest.mark.parametrize("box,kmax,dk", [(CUBE, 3.3, 0.25), (BRICK, 2.75, 0.2)])
@pytest.mark.parametrize("M", [3, 8, 64])
def test_thinning(box, kmax, dk, M):
    full = sm.vector_set(box, kmax, dk, 0)
    thin = sm.vector_set(box, kmax, dk, M)
    c = full["n_in_bin"].astype(np.int64)
    assert np.array_equal(full["unthinned"], c) and np.array_equal(thin["unthinned"], c)        # M = 0 changes no bin count
    assert (c > M).any() and ((c <= M) & (c > 0)).any()
    assert np.array_equal(thin["n_in_bin"], np.minimum(c, M))               # exactly M in every over-full bin, the others untouched
    # a subset, still in lexicographic order, each vector in its old bin
    where = {tuple(v): int(b) for v, b in zip(full["lmn"].tolist(), full["bin"].tolist())}
    assert all(where[tuple(v)] == int(b) for v, b in zip(thin["lmn"].tolist(), thin["bin"].tolist()))
    assert thin["lmn"].tolist() == sorted(thin["lmn"].tolist())
    # the rule itself on one over-full bin
    b = int(np.argmax(c))
    j = np.arange(c[b])
    keep = (j + 1) * M // c[b] > j * M // c[b]
    assert np.array_equal(thin["lmn"][thin["bin"] == b], full["lmn"][full["bin"] == b][keep])


def test_set_refusals():
    for kmax, dk, M in ((0.0, 0.1, 0), (-1.0, 0.1, 0), (3.0, 0.0, 0), (3.0, -0.1, 0), (3.0, 3.5, 0), (3.0, 3.0 / 4097.5, 0), (3.0, 0.1, -1), (0.5, 0.1, 0)):
        with pytest.raises(ValueError):
            sm.vector_set(CUBE, kmax, dk, M)                                # (0.5 < 2 pi / 11: empty)
    g = sm.TWO_PI / 21.0
    assert np.abs(sm.vector_set(BRICK, 48.5 * g, 0.5)["lmn"][:, 2]).max() == 48
    with pytest.raises(ValueError) as e:
        sm.vector_set(BRICK, 49.0 * g * (1 + 1e-12), 1.0, 4)
    assert "axis z" in str(e.value)
    assert sm.vector_set(CUBE, 3.0, 3.0 / 4096.5, 1)["n_bins"] == 4096


# ---- accuracy of the kernels' route ----
def random_atoms(n, box, nspec, seed):
    rng = np.random.default_rng(seed)
    pos = np.round(rng.random((n, 3)) * np.asarray(box), 6)
    pos[0] = 0.0
    pos[1] = np.nextafter(np.asarray(box), 0.0)                             # the last doubles below L
    return pos, (np.arange(n) % nspec).astype(np.int32)


LONG = (3.0, 3.5, 90.0)


def long_box_set():
    g = sm.TWO_PI / LONG[2]
    vs = sm.vector_set(LONG, 48.5 * g, 48.5 * g / 6)
    assert np.abs(vs["lmn"][:, 2]).max() == 48 and (vs["lmn"][:, 2] < 0).any() and (vs["lmn"][:, 1] < 0).any()
    return vs


_REF = {}


def long_box_case():
    """100 atoms of two species in a long thin box, harmonic 48 along z; the 50-digit amplitudes are computed once"""
    if not _REF:
        vs = long_box_set()
        pos, types = random_atoms(100, LONG, 2, 5)
        _REF.update(vs=vs, pos=pos, types=types, ref=sm.amplitudes_mp(pos, types, LONG, vs["lmn"], 2))
    return _REF["vs"], _REF["pos"], _REF["types"], _REF["ref"]


def test_fp64_route_within_the_bound():
    vs, pos, types, ref = long_box_case()
    n = sm.numbers_of(types, 2)
    r = sm.worst_ratio(sm.restate_fp64(pos, types, LONG, vs["lmn"], 2), ref, n)
    rl = sm.worst_ratio(sm.amplitudes_ld(pos, types, LONG, vs["lmn"], 2).astype(np.float64), ref, n)
    print("fp64 route: worst |rho - ref| / n_s = %.3g; longdouble route rounded to double: %.3g; TAU = %g" % (r, rl, sm.TAU))
    assert r <= sm.TAU
    # the longdouble engine, the reference of the large GPU cases, agrees with the 50-digit one far below the bound
    d = np.abs(sm.amplitudes_ld(pos, types, LONG, vs["lmn"], 2) - ref).max()
    assert float(d) < 1e-3 * sm.TAU * n.min()


def test_rows_and_fold_follow_the_contract():
    """the tree on integers small enough to be exact in any order, and on a case where the order shows: 16 385 terms fill 256 rows, row 0 takes a second tile"""
    rng = np.random.default_rng(1)
    for N in (1, 63, 64, 65, 16385, 40000):
        t = rng.integers(-1000, 1000, N).astype(np.float64)
        assert sm.fold(sm.row_sums(t)) == t.sum()
    t = rng.random(16385) * 2.0 ** rng.integers(-30, 30, 16385)
    rows = sm.row_sums(t)
    want0 = 0.0
    for v in np.concatenate([t[:64], t[16384:]]):
        want0 = want0 + v
    assert rows[0] == want0 and rows.shape == (256,)
    a = rows.copy()
    h = 128
    while h:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    assert sm.fold(rows) == a[0]


# ---- known answers ----
def sums_of(rho):
    return sm.accumulate(np.zeros((rho.shape[0], rho.shape[1] * (rho.shape[1] + 1) // 2)), rho)


def test_one_atom_gives_one():
    vs = sm.vector_set(BRICK, 2.75, 0.2, 8)
    pos, types = np.array([[1.234567, 9.87, 20.5]]), np.zeros(1, dtype=np.int32)
    rho = sm.restate_fp64(pos, types, BRICK, vs["lmn"], 1)
    _, cnt, tot, part = sm.values(sums_of(rho), 1, vs["bin"], vs["n_bins"], [1], 0.2)
    assert np.abs(tot[cnt > 0] - 1.0).max() <= 4 * sm.TAU and np.abs(part[cnt > 0, 0] - 1.0).max() <= 4 * sm.TAU
    assert not tot[cnt == 0].any()


def lattice(n, a):
    g = np.arange(n) * a
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 0.25


def test_simple_cubic_lattice():
    n, a = 4, 2.5
    box = (n * a,) * 3
    pos, types = lattice(n, a), np.zeros(n ** 3, dtype=np.int32)
    N = n ** 3
    vs = sm.vector_set(box, 5.5, 0.25)
    acc = sums_of(sm.restate_fp64(pos, types, box, vs["lmn"], 1))[:, 0]
    bragg = (vs["lmn"] % n == 0).all(1)
    assert bragg.sum() >= 3 and (~bragg).sum() > 100
    assert np.abs(acc[bragg] - N * N).max() <= 4 * sm.TAU * N * N            # |rho|^2 = N^2 on the reciprocal lattice
    assert np.abs(acc[~bragg]).max() <= 4 * sm.TAU * N * N                   # and nothing elsewhere


def two_atoms():
    box = (10.0, 11.0, 12.0)
    pos = np.array([[1.5, 3.0, 4.0], [6.5, 3.0, 4.0]])                        # half a box apart along x
    return box, pos, np.array([0, 1], dtype=np.int32), sm.vector_set(box, 3.0, 0.25)


def test_two_species_half_a_box_apart():
    box, pos, types, vs = two_atoms()
    acc = sums_of(sm.restate_fp64(pos, types, box, vs["lmn"], 2))
    sign = np.where(vs["lmn"][:, 0] % 2 == 0, 1.0, -1.0)
    assert np.abs(acc[:, sm.pair_index(0, 1, 2)] - sign).max() <= 4 * sm.TAU
    assert np.abs(acc[:, 0] - 1.0).max() <= 4 * sm.TAU and np.abs(acc[:, 2] - 1.0).max() <= 4 * sm.TAU
    # per vector S_01 = (-1)^l with sqrt(n_0 n_1) = 1: bins of dk = 0.25 mix both signs, a set of one bin per vector does not
    for v in range(0, len(acc), 37):
        _, cnt, tot, part = sm.values(acc[v:v + 1], 1, np.zeros(1, dtype=np.int32), 1, [1, 1], 3.0)
        assert abs(part[0, 1] - sign[v]) <= 4 * sm.TAU and abs(tot[0] - (1.0 + sign[v])) <= 8 * sm.TAU


def three_species_case():
    box = (9.0, 10.0, 11.0)
    pos, types = random_atoms(60, box, 3, 9)
    types[:] = np.repeat([0, 1, 2], [30, 20, 10])
    vs = sm.vector_set(box, 3.0, 0.5, 16)
    return box, pos, types, vs


def test_total_is_the_weighted_sum_of_the_partials():
    box, pos, types, vs = three_species_case()
    numbers = sm.numbers_of(types, 3)
    rho = sm.restate_fp64(pos, types, box, vs["lmn"], 3)
    acc = sm.accumulate(sums_of(rho), rho)                                  # two equal samples
    k, cnt, tot, part = sm.values(acc, 2, vs["bin"], vs["n_bins"], numbers, 0.5)
    w = np.array([(1.0 if a == b else 2.0) * np.sqrt(numbers[a] * numbers[b]) for a, b in sm.pairs(3)])
    assert np.allclose(tot, part @ w / 60.0, rtol=1e-13, atol=1e-15) and np.array_equal(k, (np.arange(6) + 0.5) * 0.5)
    # and the total is |sum over all atoms|^2 / N
    whole = rho.sum(1)
    direct = (whole ** 2).sum(1) / 60.0
    mean = np.array([direct[vs["bin"] == b].mean() if c else 0.0 for b, c in enumerate(cnt)])
    assert np.allclose(tot, mean, rtol=1e-12, atol=1e-13)
    # an empty species: its partials are 0, the others unchanged
    rho4 = np.concatenate([rho, np.zeros_like(rho[:, :1])], 1)
    _, _, tot4, part4 = sm.values(sums_of(rho4), 1, vs["bin"], vs["n_bins"], list(numbers) + [0], 0.5)
    assert not part4[:, [sm.pair_index(a, 3, 4) for a in range(4)]].any() and np.allclose(tot4, tot, rtol=1e-13)


# ---- the mutations: each one fails a check above ----
def test_mutations_are_caught():
    caught = []
    # the set
    lmn, b = sm.brute_force_set(CUBE, 3.3, 0.25, 6)
    for mut in ("full_space", "bins_from_kk"):
        vs = sm.vector_set(CUBE, 3.3, 0.25, mutate=mut)
        if not (np.array_equal(vs["lmn"], lmn) and np.array_equal(vs["bin"], b)):
            caught.append(mut)
    # the route
    vs, pos, types, ref = long_box_case()
    n = sm.numbers_of(types, 2)
    for mut in ("no_conjugation_for_negative_m", "harmonics_shifted_by_one"):
        r = sm.worst_ratio(sm.restate_fp64(pos, types, LONG, vs["lmn"], 2, mutate=mut), ref, n)
        print(mut, "worst ratio %.3g" % r)
        if r > sm.TAU:
            caught.append(mut)
    # the pair index: three species, the total against the weighted sum of the partials
    box, pos, types, vs = three_species_case()
    numbers = sm.numbers_of(types, 3)
    rho = sm.restate_fp64(pos, types, box, vs["lmn"], 3)
    acc = sm.accumulate(np.zeros((len(rho), 6)), rho, mutate="transposed_pair_index")
    _, cnt, tot, _ = sm.values(acc, 1, vs["bin"], vs["n_bins"], numbers, 0.5)
    direct = (rho.sum(1) ** 2).sum(1) / 60.0
    mean = np.array([direct[vs["bin"] == bb].mean() if c else 0.0 for bb, c in enumerate(cnt)])
    if not np.allclose(tot, mean, rtol=1e-12, atol=1e-13):
        caught.append("transposed_pair_index")
    # the normalisation: the two atoms of different species
    box, pos, types, vs = two_atoms()
    acc = sums_of(sm.restate_fp64(pos, types, box, vs["lmn"], 2))
    _, _, _, part = sm.values(acc[:1], 1, np.zeros(1, dtype=np.int32), 1, [1, 1], 3.0, mutate="normalised_by_N")
    sign = 1.0 if vs["lmn"][0, 0] % 2 == 0 else -1.0
    if abs(part[0, 1] - sign) > 4 * sm.TAU:
        caught.append("normalised_by_N")
    assert sorted(caught) == sorted(sm.MUTATIONS)


# ---- the 'strfac' line of control.txt and the model query ----
def lj2(**kw):
    return dict(inputs.lj_case((4, 4, 4), charges=(0.0, 0.0)), **kw)


def control_with(tmp_path, block):
    d = inputs.write_input_files(lj2(), str(tmp_path / "d"))
    with open(os.path.join(d, "control.txt"), "a") as f:
        f.write(block + "\n")
    return d


def test_directive_round_trips(tmp_path):
    d = inputs.write_input_files(lj2(strfac=(6.25, 0.05, 20, 64)), str(tmp_path / "d"))
    assert list(api.Model.from_dir(d).query("sk")) == [6.25, 0.05, 20, 64]
    plain = inputs.write_input_files(lj2(), str(tmp_path / "p"))
    assert list(api.Model.from_dir(plain).query("sk")) == [0, 0, 0, 0]
    ctl = open(os.path.join(plain, "control.txt")).read()
    assert "strfac" not in ctl and ctl == "".join(l for l in open(os.path.join(d, "control.txt")) if not l.startswith("strfac"))
    assert list(api.Model.from_case(lj2()).query("sk")) == [0, 0, 0, 0]
    assert list(api.Model.from_dir(control_with(tmp_path, "strfac 1e1 .5 0 0")).query("sk")) == [10.0, 0.5, 0, 0]


def test_directive_is_a_whole_word(tmp_path):
    """inside or at the head of another token the word does not fire"""
    for k, block in enumerate(("xstrfac 6.0 0.1 5 8", "strfacs 6.0 0.1 5 8", "nostrfac6.0 0.1 5 8")):
        assert list(api.Model.from_dir(control_with(tmp_path / str(k), block)).query("sk")) == [0, 0, 0, 0], block


@pytest.mark.parametrize("block", [
    "strfac x 0.1 5 8",                     # kmax is no number
    "strfac 6.0x 0.1 5 8",                  # ... or only starts like one
    "strfac 6.0 0.1 5",                     # a value short
    "strfac 6.0 0.1 five 8",
    "strfac 0 0.1 5 8",                     # kmax, dk not positive
    "strfac -6.0 0.1 5 8",
    "strfac 6.0 0 5 8",
    "strfac 6.0 -0.1 5 8",
    "strfac 6.0 0.1 -1 8",                  # negative period
    "strfac 6.0 0.1 5 -8",                  # negative cap
])
def test_bad_directives_are_refused(tmp_path, block):
    with pytest.raises(api.AztotError) as e:
        api.Model.from_dir(control_with(tmp_path, block))
    assert "ERROR[418]" in str(e.value)


def test_entry_points_refuse_null_handles():
    L = api.lib()
    assert L.aztot_sk_setup(None, 3.0, 0.1, 0) == -4
    for f in (L.aztot_sk_sample, L.aztot_sk_reset):
        assert f(None) == -4
    assert L.aztot_sk_shape(None, None, None, None, None) == -4 and L.aztot_sk_vectors(None, None, None, 0) == -4
    assert L.aztot_sk_amplitudes(None, None, 0) == -4 and L.aztot_sk_sums(None, None, None, 0) == -4
    assert L.aztot_sk_values(None, None, None, None, None, 0) == -4


def test_exports():
    for n in ("setup", "sample", "reset", "shape", "vectors", "amplitudes", "sums", "values"):
        assert "aztot_sk_" + n in api.EXPORTS and hasattr(api.lib(), "aztot_sk_" + n)
    assert C.sizeof(C.c_int32) == 4
