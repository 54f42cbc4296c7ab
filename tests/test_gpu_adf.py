"""GPU tests of the bond-angle distributions (aztot_adf_*, adf.hip.h) against the numpy restatement of the contract in tests/adf_model.py, which reads the
edge table through aztot_adf_edges.  Counts and neighbour counts are compared exactly, cell by cell and atom by atom: the device and the host evaluate
the same correctly rounded operations in the same order, and every total is an integer.

Which path a case takes.  Histogram: n_bins * n_cols <= 5120 cells (kAdfHistBudget) uses the uint32 sub-histogram in LDS, more goes through 64-bit
global atomics: 3600 bins x 3 columns and 180 bins x 64 columns are the global path, everything else here the LDS path.  Lanes per central atom
(Samplers::adf_sample): the fewest, from 4, with atoms * lanes >= 65536 and histogram + tiles (256 / lanes tiles of 36 bytes per neighbour of the
busiest atom) <= 36 KiB; test_every_lane_count_exact forces each choice, the other docstrings say which one a case gets."""
import os
import subprocess

import mpmath
import numpy as np
import pytest

from aztotmd_amd import api, inputs

import adf_model as am
from test_gpu_cn import GEOMETRIES, positions, random_case, run_cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(eng, box, n_bins, cols, setup=True, before=None):
    """one sample compared with the model; `before`: (samples, counts) the totals held before it"""
    if setup:
        assert eng.adf_setup(n_bins, cols) == n_bins
    T = eng.adf_edges()
    eng.adf_sample()
    pos, types = positions(eng)
    counts, neigh = am.host_adf(pos, types, box, cols, T)
    samples, got = eng.adf_counts()
    gn = eng.adf_neighbours()
    base = 0 if before is None else before[1].astype(np.int64)
    print("bins", n_bins, "cols", len(cols), "triplets", int(counts.sum()), "cells that differ", int((got.astype(np.int64) - base != counts).sum()),
          "neighbour mismatches", int((gn != neigh).sum()), "neighbours max / mean", int(neigh.max()), float(neigh[neigh >= 0].mean()) if (neigh >= 0).any() else 0.0)
    assert got.dtype == np.uint64 and got.shape == (n_bins, len(cols))
    assert np.array_equal(gn, neigh)
    assert np.array_equal(got.astype(np.int64) - base, counts)
    assert samples == (1 if before is None else before[0] + 1)
    assert eng.adf_shape() == (n_bins, len(cols), samples)
    return counts, neigh


def test_edge_table_of_the_library():
    """the table the device uses is the model's, and every entry is within 2 ulp of the 50-digit value"""
    eng = api.Engine(api.Model.from_case(random_case(2, 64, (12.0, 12.0, 12.0), seed=3)))
    for n_bins in (1, 7, 8, 180, 3600):
        eng.adf_setup(n_bins, [(0, 0, 0, 3.0, 3.0)])
        T = eng.adf_edges()
        assert T.shape == (n_bins + 1,) and (np.diff(T) < 0).all() and T[0] == 1.0 and T[-1] == -1.0
        assert n_bins % 2 or T[n_bins // 2] == 0.0
        assert np.array_equal(T, am.edges(n_bins))
        with mpmath.workdps(50):
            for b in range(1, n_bins):
                if 2 * b == n_bins:
                    continue
                c = mpmath.cos(mpmath.pi * b / n_bins)
                assert abs(mpmath.mpf(float(T[b])) - c * abs(c)) <= 2 * mpmath.mpf(float(np.spacing(abs(T[b])))), (n_bins, b)


# radii per geometry (the columns are (0,0,0,r0), (0,0,1,r1,r2), (1,0,1,r3,r4)), all inside 2.5 - 4.5 A.  With 3000 atoms the four small boxes are dense
# (0.37 - 1.37 atoms / A^3): their radii stay at the low end so that no atom passes AZTOT_ADF_MAX_NEIGHBOURS = 256, which leaves them 2 - 6 cells per axis.
# The cell shapes the geometries were made for (one cell per axis, 1 / 2 / 3 cells, R > L / 2, R > L_x) are run by test_sparse_geometries_exact below
# with the coordination-number tests' own radii and fewer atoms.
RADII = [(4.5, 3.0, 4.5, 4.0, 2.5), (4.5, 3.0, 4.5, 4.0, 2.5), (2.5, 2.5, 2.75, 2.625, 2.5), (3.0, 2.5, 3.0, 2.75, 2.5), (3.75, 2.5, 3.5, 3.0, 2.5),
         (4.5, 2.5, 3.5, 3.0, 2.5)]


def three_columns(r):
    return [(0, 0, 0, r[0], r[0]), (0, 0, 1, r[1], r[2]), (1, 0, 1, r[3], r[4])]        # (1, 1, 1) is left out


@pytest.mark.parametrize("g", range(6))
def test_geometries_exact(g):
    """3000 atoms: 32 lanes per atom from N, 64 in the two densest boxes (157 and 174 neighbours on the busiest atom)"""
    nspec, box, _, faces = GEOMETRIES[g]
    eng = api.Engine(api.Model.from_case(random_case(nspec, 3000, box, seed=700 + g, faces=faces)))
    counts, neigh = check(eng, box, 180, three_columns(RADII[g]))
    assert counts.sum(axis=0).min() > 0 and neigh.max() <= am.MAX_NEIGHBOURS
    if nspec == 3:
        assert (neigh[positions(eng)[1] == 2] == -1).all()          # S2 is central to nothing


@pytest.mark.parametrize("g,n", [(2, 200), (3, 300), (4, 500), (5, 250)])
def test_sparse_geometries_exact(g, n):
    """the radii of test_gpu_cn.py (8 and 12 A: one cell per axis, 1 / 2 / 3 cells, R > L / 2, R > L_x) on so few atoms that the neighbour cap holds;
    every partner is seen once, through its nearest image"""
    nspec, box, R, faces = GEOMETRIES[g]
    eng = api.Engine(api.Model.from_case(random_case(nspec, n, box, seed=800 + g, faces=faces)))
    _, neigh = check(eng, box, 8, [(0, 0, 0, R, R), (0, 0, 1, 0.5 * R, R), (1, 0, 1, 0.75 * R, 0.625 * R)])
    assert neigh.max() > 0.3 * n


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 769])
def test_atom_counts_exact(n):
    box = (10.0, 11.0, 12.0) if n < 100 else (20.0, 21.0, 22.0)
    eng = api.Engine(api.Model.from_case(random_case(2, n, box, seed=n)))
    check(eng, box, 8, three_columns((4.5, 3.0, 4.5, 4.0, 2.5)))


def test_fifteen_species_all_columns():
    """15 species and AZTOT_ADF_MAX_COLUMNS = 64 columns; 180 x 64 cells: the global-atomics path"""
    box = (30.0, 30.0, 30.0)
    eng = api.Engine(api.Model.from_case(random_case(15, 2500, box, seed=15)))
    cols = []
    for k in range(64):
        c, a = k % 15, (k * 7) % 15
        b = (a + k // 15) % 15
        cols.append((c, a, b, 4.5, 4.5) if a == b else (c, a, b, 3.5 + 0.015 * k, 4.5 - 0.015 * k))
    assert len({(c, min(a, b), max(a, b)) for c, a, b, _, _ in cols}) == 64
    counts, _ = check(eng, box, 180, cols)
    assert (counts.sum(axis=0) > 0).sum() > 50
    with pytest.raises(api.AztotError) as e:
        eng.adf_setup(180, cols + [(14, 14, 14, 3.0, 3.0)])
    assert e.value.code == -4


@pytest.mark.parametrize("n_bins", [1, 8, 180, 3600])
def test_bin_counts_exact(n_bins):
    """3600 bins x 3 columns = 10 800 cells: past the LDS budget of 5120 cells, the global path; the others use the LDS sub-histogram"""
    box = (24.0, 25.0, 26.0)
    eng = api.Engine(api.Model.from_case(random_case(2, 1500, box, seed=41)))
    counts, _ = check(eng, box, n_bins, three_columns((4.5, 3.0, 4.5, 4.0, 2.5)))
    theta, p = eng.adf_values()
    mt, mp_ = am.values(counts)
    assert np.array_equal(theta, mt) and np.array_equal(p, mp_)
    assert np.allclose(p.sum(axis=0) * 180.0 / n_bins, 1.0)


@pytest.mark.parametrize("lanes", [4, 8, 16, 32, 64])
def test_every_lane_count_exact(monkeypatch, lanes):
    """the measurement switch AZTOT_ADF_LANES puts every lanes-per-atom choice on one case (so sparse that the 64 tiles of the 4-lane form fit:
    at most 25 neighbours on an atom, asserted); the counts do not depend on it"""
    box = (28.0, 29.0, 30.0)
    eng = api.Engine(api.Model.from_case(random_case(2, 1500, box, seed=41)))
    monkeypatch.setenv("AZTOT_ADF_LANES", str(lanes))
    counts, neigh = check(eng, box, 36, three_columns((3.0, 2.5, 3.0, 2.75, 2.5)))
    assert 2 <= neigh.max() <= 25
    monkeypatch.delenv("AZTOT_ADF_LANES")
    eng.adf_sample()
    assert np.array_equal(eng.adf_counts()[1].astype(np.int64), 2 * counts)


def sphere(n, r, centre):
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    t = np.pi * (1 + 5 ** 0.5) * k
    return np.round(np.stack([np.cos(t) * np.sin(phi), np.sin(t) * np.sin(phi), np.cos(phi)], axis=1) * r, 6) + np.asarray(centre)


def test_neighbour_cap():
    """a central atom (the only atom of species 1) with exactly 256 neighbours on a sphere of radius 2 passes and matches (32 640 pairs; one wave per
    atom); when the 257th joins them the sample is refused with AZTOT_ERR_INPUT and nothing changes: totals, sample count, the steps that follow"""
    box = (40.0, 40.0, 40.0)
    centre = (20.0, 20.0, 20.0)
    pos = np.concatenate([[centre], sphere(257, 2.0, centre)])
    far = pos.copy()
    far[257] = np.round(centre + (pos[257] - centre) * 1.5, 6)      # at 3 A: outside the shell
    case = random_case(2, 258, box, seed=1)
    case["vdw"] = [(a, b, t, rc, [1e-9, 1.0]) for a, b, t, rc, _ in case["vdw"]]       # (atoms 0.4 A apart: keep the forces small)
    types = np.zeros(258, dtype=np.int32)
    types[0] = 1
    case.update(types=types, x=far[:, 0].copy(), y=far[:, 1].copy(), z=far[:, 2].copy())
    eng, twin = api.Engine(api.Model.from_case(case)), api.Engine(api.Model.from_case(case))
    cols = [(1, 0, 0, 2.5, 2.5)]
    counts, neigh = check(eng, box, 180, cols)
    assert neigh[0] == 256 and (neigh[1:] == -1).all() and counts.sum() == 256 * 255 // 2
    held = eng.adf_counts()
    for e in (eng, twin):
        e.set_state(x=pos[:, 0], y=pos[:, 1], z=pos[:, 2])
    with pytest.raises(api.AztotError) as err:
        eng.adf_sample()
    print(err.value)
    assert err.value.code == -2 and "atom 0 " in str(err.value) and "257" in str(err.value)
    again = eng.adf_counts()
    assert again[0] == held[0] == 1 and np.array_equal(again[1], held[1])
    assert eng.adf_neighbours()[0] == 257                      # the counts of the refused sample
    eng.step(3)
    twin.step(3)
    sa, sb = eng.state(), twin.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(sa[k], sb[k]), k
    ta, tb = eng.stats(), twin.stats()
    for k in ta:
        assert ta[k] == tb[k], k
    # and the sampler works on: back under the cap
    eng.set_state(x=far[:, 0], y=far[:, 1], z=far[:, 2])
    eng.adf_sample()
    assert eng.adf_counts()[0] == 2


@pytest.mark.parametrize("n", [10, 30])        # 4 000 atoms: 32 lanes per atom (from N); 108 000: 4 at R = 4.5 (tiles of 12), 8 at R = 6.5 (tiles of 18)
def test_fcc_known_answers(n):
    """FCC on exactly representable coordinates (a = 6, offset 0.25): 12 nearest neighbours at 6 / sqrt 2, per atom 24 / 12 / 24 / 6 pairs at
    60 / 90 / 120 / 180 degrees; with the second shell (6 more at a = 6) the 153 pairs are at 45, 60, 90, 120, 135 and 180 degrees.  8 and 100 bins:
    60 and 120 are inside a bin, 90 and 180 are forced edges and must land in bins n / 2 and n - 1"""
    case = inputs.lj_case((n, n, n), a=6.0, jitter=0.0, seed=1)
    eng = api.Engine(api.Model.from_case(case))
    N = 4 * n ** 3
    for n_bins in (8, 100):
        eng.adf_setup(n_bins, [(0, 0, 0, 4.5, 4.5)])
        eng.adf_sample()
        _, c = eng.adf_counts()
        want = np.zeros(n_bins, dtype=np.int64)
        for deg, k in ((60, 24), (90, 12), (120, 24), (180, 6)):
            want[min(deg * n_bins // 180, n_bins - 1)] += k * N
        print(n, n_bins, c[:, 0][c[:, 0] > 0])
        assert np.array_equal(c[:, 0].astype(np.int64), want)
        assert (eng.adf_neighbours() == 12).all()
    eng.adf_setup(8, [(0, 0, 0, 6.5, 6.5)])
    eng.adf_sample()
    assert (eng.adf_neighbours() == 18).all()
    _, c = eng.adf_counts()
    assert c.sum() == 153 * N and c[4, 0] % N == 0 and c[7, 0] == 9 * N          # 180 degrees: 6 + 3 straight lines through the atom
    if n == 10:
        pos, types = positions(eng)
        counts, _ = am.host_adf(pos, types, case["box"], [(0, 0, 0, 6.5, 6.5)], eng.adf_edges())
        assert np.array_equal(c.astype(np.int64), counts)


def test_accumulate_reset_and_second_setup():
    box = (22.0, 23.0, 24.0)
    eng = api.Engine(api.Model.from_case(random_case(2, 1200, box, seed=52)))
    cols = three_columns((4.5, 3.0, 4.5, 4.0, 2.5))
    counts, _ = check(eng, box, 36, cols)
    check(eng, box, 36, cols, setup=False, before=eng.adf_counts())
    assert np.array_equal(eng.adf_counts()[1].astype(np.int64), 2 * counts)          # two samples accumulate to twice one
    eng.adf_reset()
    s, c = eng.adf_counts()
    assert s == 0 and not c.any()
    check(eng, box, 36, cols, setup=False)
    eng.step(4)
    check(eng, box, 36, cols, setup=False, before=eng.adf_counts())                   # a moved configuration adds its own triplets
    check(eng, box, 12, [(1, 1, 1, 4.0, 4.0), (1, 1, 0, 3.5, 3.0)])                   # a second set-up replaces columns and bins and zeroes
    with pytest.raises(api.AztotError):
        eng.adf_setup(12, [(0, 0, 0, 4.0, 3.0)])                                      # a refused set-up leaves the earlier one
    assert eng.adf_shape()[:2] == (12, 2)


def test_column_totals_at_scale():
    """100 000 random atoms (about 11 neighbours inside 3 A, 4 or 8 lanes per atom), no brute force: every column total is sum_i n_a(i) n_b(i), or
    sum_i n_a (n_a - 1) / 2 for equal ligands, with the n from the coordination numbers of kind 'nuclei' (strict radii, i != j)"""
    box = (100.0, 100.0, 100.0)
    eng = api.Engine(api.Model.from_case(random_case(2, 100000, box, seed=99)))
    cols = [(0, 0, 0, 2.5, 2.5), (0, 0, 1, 2.5, 3.0), (1, 0, 1, 3.0, 2.0), (1, 1, 1, 2.75, 2.75)]
    eng.adf_setup(180, cols)
    eng.adf_sample()
    _, counts = eng.adf_counts()
    neigh = eng.adf_neighbours()
    types = positions(eng)[1]
    for k, (c, a, b, ra, rb) in enumerate(cols):
        cn = [(c, a, ra)] + ([(c, b, rb)] if a != b else [])
        eng.cn_setup("nuclei", cn)
        eng.cn_sample("nuclei")
        per = eng.cn_per_atom("nuclei").astype(np.int64)
        per = per[types == c]
        want = int((per[:, 0] * (per[:, 0] - 1) // 2).sum()) if a == b else int((per[:, 0] * per[:, 1]).sum())
        print(cols[k], "total", int(counts[:, k].sum()), "from the coordination numbers", want)
        assert int(counts[:, k].sum()) == want and want > 0
    # neighbours: inside the largest radius of the species' columns (3.0 for both), both ligand species
    eng.cn_setup("nuclei", [(0, 0, 3.0), (0, 1, 3.0), (1, 0, 3.0), (1, 1, 3.0)])
    eng.cn_sample("nuclei")
    per = eng.cn_per_atom("nuclei")
    assert np.array_equal(neigh, np.where(types == 0, per[:, 0] + per[:, 1], per[:, 2] + per[:, 3]))


@pytest.mark.parametrize("kw", [{}, {"sort_every": 1}, {"use_graph": 0, "pair_variant": 1}])
def test_sampling_does_not_perturb(kw):
    case = inputs.config("F2")
    case = dict(case, vx=np.sin(np.arange(len(case["x"]))) * 3.0, vy=np.cos(np.arange(len(case["x"]))) * 3.0)
    a = api.Engine(api.Model.from_case(case), **kw)
    b = api.Engine(api.Model.from_case(case), **kw)
    b.adf_setup(90, [(0, 0, 0, 4.2, 4.2)])
    a.stats()
    b.adf_sample()                          # right after init, no step
    for _ in range(5):
        a.step(7)
        a.stats()
        b.step(7)
        b.adf_sample()
    assert b.adf_shape()[2] == 6
    sa, sb = a.state(), b.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(sa[k], sb[k]), k
    ta, tb = a.stats(), b.stats()
    for k in ta:
        assert ta[k] == tb[k], k


def replay(d, nstep, stat, every_rdf, n_bins, every, cols, nequil=0):
    """the CLI's call boundaries (main.cpp): aztot_step up to the next stat row, RDF sample or ADF sample"""
    m = api.Model.from_dir(d)
    eng = api.Engine(m, initial_forces=0)
    eng.adf_setup(n_bins, cols)
    done = taken = 0
    while done < nstep:
        n = min(stat - done % stat, nstep - done)
        nxt = 1 if done < 1 else done + 1 + (every_rdf - done % every_rdf) % every_rdf
        n = min(n, nxt - done)
        if every > 0:
            n = min(n, (max(done, nequil) // every + 1) * every - done)
        eng.step(n)
        done += n
        if every > 0 and done > nequil and done % every == 0:
            eng.adf_sample()
            taken += 1
        if done % stat == 0 or done == nstep:
            eng.stats()
    if not taken:
        eng.adf_sample()
    return eng


def render(eng, header, raw):
    theta, p = eng.adf_values()
    _, c = eng.adf_counts()
    lines = ["theta" + "".join("\t" + h for h in header)]
    for b in range(len(theta)):
        lines.append("%f" % theta[b] + "".join(("\t%d" % v) if raw else ("\t%f" % v) for v in (c[b] if raw else p[b])))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("every,samples", [(60, 3), (0, 1), (500, 1)])
def test_cli_files(tmp_path, every, samples):
    """200 steps: samples after steps 60, 120 and 180; every = 0 and a period longer than the run: one sample of the final configuration"""
    case = inputs.lj_case((6, 6, 6), a=5.26, seed=3, charges=(0.0, 0.0), vel_T=85.0)      # two neutral species A, B
    case["nsteps"] = 200
    adf = (36, every, [("A", "A", "A", 4.5, 4.5), ("A", "B", "A", 4.0, 4.5), ("B", "A", "B", 4.25, 3.75)])
    d = inputs.write_input_files(dict(case, adf=adf), str(tmp_path / "n"), stat=70)
    run_cli(d)
    rdf_every = int(api.Model.from_dir(d).query("rdf")[3]) or 1000000
    eng = replay(d, 200, 70, rdf_every, 36, every, [(0, 0, 0, 4.5, 4.5), (0, 1, 0, 4.0, 4.5), (1, 0, 1, 4.25, 3.75)])
    assert eng.adf_shape() == (36, 3, samples)
    header = ["A-A-A", "B-A-A", "A-B-B"]
    got, got_n = open(os.path.join(d, "adf.dat")).read(), open(os.path.join(d, "adf_n.dat")).read()
    assert got.splitlines()[0] == "theta\tA-A-A\tB-A-A\tA-B-B" and got.splitlines()[1].startswith("2.500000\t")
    assert got_n == render(eng, header, True)
    assert got == render(eng, header, False)
    if every == 60:
        plain = inputs.write_input_files(case, str(tmp_path / "p"), stat=70)
        run_cli(plain)
        assert not os.path.exists(os.path.join(plain, "adf.dat")) and not os.path.exists(os.path.join(plain, "adf_n.dat"))
        for f in ("stat.dat", "revcon.xyz", "velocities.dat", "msd.dat"):
            assert open(os.path.join(d, f)).read() == open(os.path.join(plain, f)).read(), f


def test_cli_sample_over_the_cap_is_fatal(tmp_path):
    case = inputs.lj_case((6, 6, 6), a=5.26, seed=3, charges=(0.0, 0.0))
    case["nsteps"] = 2
    d = inputs.write_input_files(dict(case, adf=(36, 1, [("A", "A", "B", 14.0, 14.0)])), str(tmp_path / "n"), stat=5)
    exe = os.path.join(ROOT, "aztotmd_amd", "aztotmd")
    r = subprocess.run([exe, d, "--out", d], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "AZTOT_ADF_MAX_NEIGHBOURS" in r.stderr and "adf sample" in r.stderr
    assert not os.path.exists(os.path.join(d, "adf.dat"))


def test_slab_handle_refused():
    case = inputs.lj_case((42, 5, 5), a=5.735, seed=31, rc=8.5, vel_T=8.0)
    eng = api.Engine(api.Model.from_case(case), slab={"rank": 1, "nranks": 2, "loopback": True})
    with pytest.raises(api.AztotError) as e:
        eng.adf_setup(180, [(0, 0, 0, 4.0, 4.0)])
    assert e.value.code == -2 and "slab" in str(e.value)
    with pytest.raises(api.AztotError) as e:
        eng.adf_sample()
    assert e.value.code == -4
    eng.step(3)                                 # the handle steps on


def test_errors():
    case = inputs.lj_case((5, 5, 5), a=5.26, seed=3, charges=(0.0, 0.0))
    eng = api.Engine(api.Model.from_case(case))
    L = api.lib()
    for call in (eng.adf_sample, eng.adf_reset, eng.adf_shape, eng.adf_edges, eng.adf_counts, eng.adf_values, eng.adf_neighbours):
        with pytest.raises(api.AztotError) as e:
            call()
        assert e.value.code == -4, call
    ok = (0, 0, 1, 4.0, 3.5)
    for n_bins, cols in ((0, [ok]), (-3, [ok]), (3601, [ok]), (8, []), (8, [ok] * 65), (8, [(2, 0, 0, 4.0, 4.0)]), (8, [(0, -1, 0, 4.0, 4.0)]),
                         (8, [(0, 0, 2, 4.0, 4.0)]), (8, [(0, 0, 1, 0.0, 4.0)]), (8, [(0, 0, 1, 4.0, -1.0)]), (8, [(0, 0, 1, float("nan"), 4.0)]),
                         (8, [(0, 1, 1, 4.0, 3.5)]), (8, [ok, (0, 1, 0, 3.5, 4.0)]), (8, [ok, ok])):
        with pytest.raises(api.AztotError) as e:
            eng.adf_setup(n_bins, cols)
        assert e.value.code == -4, (n_bins, cols)
    col = api._AdfColumn(0, 0, 1, 7, 4.0, 3.5)                          # a non-zero `reserved`
    assert L.aztot_adf_setup(eng.h, 8, col, 1) == -4
    assert L.aztot_adf_setup(eng.h, 8, None, 1) == -4
    assert eng.adf_setup(3600, [ok]) == 3600 and eng.adf_setup(8, [ok, (1, 1, 1, 3.0, 3.0)]) == 8
    with pytest.raises(api.AztotError) as e:
        eng.adf_neighbours()                                            # set up, not sampled yet
    assert e.value.code == -4
    assert eng.adf_shape() == (8, 2, 0) and not eng.adf_counts()[1].any() and not eng.adf_values()[1].any()
    eng.adf_sample()
    # sizes by a null buffer; a cap too small for a buffer is refused and writes nothing
    assert L.aztot_adf_edges(eng.h, None, 0) == 9 and L.aztot_adf_counts(eng.h, None, None, 0) == 16
    assert L.aztot_adf_values(eng.h, None, None, 0) == 16 and L.aztot_adf_neighbours(eng.h, None, 0) == 500
    small = np.full(4, 77.0)
    assert L.aztot_adf_edges(eng.h, small.ctypes.data_as(api._dp), 4) == -4
    assert L.aztot_adf_values(eng.h, None, small.ctypes.data_as(api._dp), 4) == -4 and (small == 77.0).all()
    smalli = np.full(4, 77, dtype=np.int32)
    assert L.aztot_adf_neighbours(eng.h, smalli.ctypes.data_as(api._ip), 4) == -4 and (smalli == 77).all()
    smallu = np.full(4, 77, dtype=np.uint64)
    assert L.aztot_adf_counts(eng.h, None, smallu.ctypes.data_as(api.C.POINTER(api.C.c_uint64)), 4) == -4 and (smallu == 77).all()
