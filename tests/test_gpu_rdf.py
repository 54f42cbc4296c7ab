"""GPU tests of the radial distribution functions (aztot_rdf_*, rdf.hip.h) against an fp64 host restatement of the rules in include/aztot.h:
every unordered pair i < j, minimum image by delta_periodic (one shift by L where |d| > L / 2), r * r < rmax * rmax, bin = (int)(r * (1 / dr)) < n_bins,
pair index mn * (n - 1) + mn * (1 - mn) / 2 + mx.  Totals must match exactly; a pair may sit in a neighbouring bin only where the host check itself puts
it within 1e-9 relative of a bin edge (that allowance is computed, not a free tolerance)."""
import os
import subprocess

import numpy as np
import pytest

from aztotmd_amd import api, inputs

import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERA = 4.0 * 3.14159265359 / 3.0          # const.h:11,15
EDGE = 1e-9


def pair_index(a, b, n):
    mn, mx = np.minimum(a, b), np.maximum(a, b)
    return mn * (n - 1) + mn * (1 - mn) // 2 + mx


def host_rdf(pos, groups, ngroups, box, rmax, dr, nbins):
    """exact counts [bin][pair] and, per bin edge k = 1..nbins, the number of pairs within EDGE relative of it (the allowance)"""
    L = np.asarray(box, dtype=np.float64)
    half = L * 0.5
    idr = 1.0 / dr
    npair = ngroups * (ngroups + 1) // 2
    counts = np.zeros((nbins, npair), dtype=np.int64)
    near = np.zeros(nbins + 1, dtype=np.int64)
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    N = len(x)
    for i in range(N - 1):
        d = []
        for c, k in ((x, 0), (y, 1), (z, 2)):
            v = c[i] - c[i + 1:]
            v = np.where(v > half[k], v - L[k], np.where(v < -half[k], v + L[k], v))
            d.append(v)
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        m = r2 < rmax * rmax
        if not m.any():
            continue
        s = np.sqrt(r2[m]) * idr
        b = s.astype(np.int64)
        ok = b < nbins
        p = pair_index(groups[i], groups[i + 1:][m], ngroups)
        np.add.at(counts, (b[ok], p[ok]), 1)
        e = np.rint(s).astype(np.int64)
        close = (np.abs(s - e) <= EDGE * s) & (e >= 1) & (e <= nbins)
        np.add.at(near, e[close], 1)
    return counts, near


def assert_matches(got, want, near):
    """totals per pair exact; the running sum over bins may differ only by pairs that sit on the edge in between"""
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == want.shape
    assert (got.sum(axis=0) == want.sum(axis=0)).all(), (got.sum(axis=0), want.sum(axis=0))
    diff = np.abs(np.cumsum(got - want, axis=0)).sum(axis=1)            # after bin k: pairs moved across edge k + 1
    assert (diff[:-1] <= near[1:-1]).all(), np.nonzero(diff[:-1] > near[1:-1])


def host_g(counts, samples, numbers, box, dr):
    V = box[0] * box[1] * box[2]
    n = len(numbers)
    nb, npair = counts.shape
    g = np.zeros((nb, npair))
    C1 = 2.0 / (SPHERA * dr * dr * dr * samples)
    for i in range(nb):
        C2 = 1.0 / (3.0 * i * (i + 1.0) + 1.0)
        p = 0
        for a in range(n):
            for b in range(a, n):
                nAnB = float(numbers[a]) * float(numbers[b])
                if nAnB:
                    g[i, p] = float(counts[i, p]) * V / nAnB * C1 * C2 * (1.0 if a == b else 0.5)
                p += 1
    return g


def random_case(nspec, N, box, seed, faces=False):
    rng = np.random.default_rng(seed)
    pos = rng.random((N, 3)) * np.asarray(box)
    pos = np.round(pos, 6)
    if faces:                                        # atoms on the box faces and edges
        pos[:40, 0] = 0.0
        pos[20:60, 1] = 0.0
        pos[50:70, 2] = 0.0
    for k in range(3):
        pos[pos[:, k] >= box[k], k] = 0.0
    types = (np.arange(N) % nspec).astype(np.int32)
    rc = min(3.0, 0.45 * min(box))
    vdw = [(a, b, 1, rc, [0.001, 1.0]) for a in range(nspec) for b in range(a, nspec)]
    return {"box": list(box), "dt": 0.001, "species": [(39.9, 0.0)] * nspec, "names": ["S%d" % k for k in range(nspec)], "types": types,
            "vdw": vdw, "x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": np.zeros(N), "vy": np.zeros(N), "vz": np.zeros(N),
            "cell_list": rc, "use_clist": 1, "elec_type": 0}


def positions(eng):
    s = eng.state(("x", "y", "z"))
    return np.stack([s["x"], s["y"], s["z"]], axis=1), s["types"]


def check_engine(eng, box, rmax, dr, nuclei_of=None, samples=1):
    """sample `samples` times and compare species (and, with nuclei_of, nuclei) histograms and g(r) with the host"""
    nb = eng.rdf_setup(rmax, dr, nuclei=nuclei_of is not None)
    assert nb == int(min(rmax, box[0]) * (1.0 / dr))
    for _ in range(samples):
        eng.rdf_sample()
    pos, types = positions(eng)
    nspec = int(eng.model.query("n_species")[0])
    kinds = [("species", types, nspec)]
    if nuclei_of is not None:
        nuc = np.asarray(nuclei_of)[types]
        kinds.append(("nuclei", nuc, int(nuc.max()) + 1))
    out = {}
    for kind, groups, ng in kinds:
        want, near = host_rdf(pos, groups, ng, box, rmax, dr, nb)
        s, got = eng.rdf_counts(kind)
        assert s == samples
        assert_matches(got, want * samples, near)
        numbers = np.bincount(groups, minlength=ng)
        r, g, names = eng.rdf(kind)
        assert len(names) == ng * (ng + 1) // 2
        assert np.array_equal(r, (np.arange(nb) + 0.5) * dr)
        gw = host_g(got.astype(np.int64), samples, numbers, box, dr)
        assert np.allclose(g, gw, rtol=1e-12, atol=0.0)
        out[kind] = got
    return out


@pytest.mark.parametrize("nspec,box,rmax,dr,faces", [
    (2, (35.0, 35.0, 35.0), 8.0, 0.02, False),       # half shell, 4 LDS copies
    (3, (33.0, 36.0, 31.0), 7.5, 0.02, True),        # half shell, one LDS copy (species + nuclei histograms above a quarter of the budget)
    (2, (12.0, 13.0, 14.0), 8.0, 0.05, False),       # rmax > L / 2 on every axis: one cell per axis
    (3, (8.2, 17.0, 26.0), 8.0, 0.05, True),         # 1, 2 and 3 cells per axis: each distinct cell once
    (2, (17.0, 26.0, 17.0), 8.0, 0.1, False),        # 2 and 3 cells
    (2, (9.0, 30.0, 30.0), 12.0, 0.05, False),       # rmax > L_x: bins from L_x
])
def test_small_systems_exact(nspec, box, rmax, dr, faces):
    case = random_case(nspec, 3000, box, seed=int(rmax * 100) + nspec, faces=faces)
    eng = api.Engine(api.Model.from_case(case))
    check_engine(eng, box, rmax, dr, nuclei_of=list(range(nspec)))


def test_global_histogram_path_15_species():
    """15 species: 120 pairs x 400 bins do not fit the LDS budget, every pair adds into the uint64 totals directly"""
    box = (30.0, 30.0, 30.0)
    case = random_case(15, 2500, box, seed=15)
    eng = api.Engine(api.Model.from_case(case))
    check_engine(eng, box, 8.0, 0.02, nuclei_of=list(range(15)), samples=2)


def test_shared_nucleus_is_sum_of_species_pairs(tmp_path):
    box = (30.0, 31.0, 32.0)
    case = random_case(3, 3000, box, seed=7)
    d = str(tmp_path / "m")
    inputs.write_input_files(case, d)
    fld = open(os.path.join(d, "field.txt")).read().replace("S1\tS1\t", "S1\tS0\t", 1)      # S0 and S1 share nucleus 'S0'
    open(os.path.join(d, "field.txt"), "w").write(fld)
    m = api.Model.from_dir(d)
    assert list(m.query("nuclei")) == [0, 0, 1] and m.nucleus_name(0) == "S0" and m.nucleus_name(1) == "S2"
    eng = api.Engine(m)
    out = check_engine(eng, box, 8.0, 0.02, nuclei_of=[0, 0, 1])
    s, n = out["species"], out["nuclei"]
    # species pairs 00 01 02 11 12 22 -> nuclei pairs 00 01 11
    assert np.array_equal(n[:, 0], s[:, 0] + s[:, 1] + s[:, 3])
    assert np.array_equal(n[:, 1], s[:, 2] + s[:, 4])
    assert np.array_equal(n[:, 2], s[:, 5])


def test_accumulation_reset_and_variants():
    case = inputs.config("F2")
    ref = None
    for kw in ({}, {"pair_variant": 1}, {"pair_variant": 2}, {"sort_every": 1}, {"use_graph": 0}):
        eng = api.Engine(api.Model.from_case(case), **kw)
        eng.rdf_setup(8.0, 0.02, nuclei=True)
        eng.rdf_sample()
        s1, one = eng.rdf_counts()
        for _ in range(4):
            eng.rdf_sample()
        s5, five = eng.rdf_counts()
        assert s1 == 1 and s5 == 5 and np.array_equal(five, 5 * one)
        _, nuc = eng.rdf_counts("nuclei")
        assert np.array_equal(nuc, five)
        if ref is None:
            ref = one
        assert np.array_equal(one, ref), kw
        eng.rdf_reset()
        s0, zero = eng.rdf_counts()
        assert s0 == 0 and not zero.any()
        assert not eng.rdf()[1].any()
        # after steps: exact against the host on the state the engine hands out
        eng.step(12)
        check_engine(eng, case["box"], 8.0, 0.02)


@pytest.mark.parametrize("kw", [{}, {"sort_every": 1}, {"use_graph": 0, "pair_variant": 1}])
def test_sampling_does_not_perturb(kw):
    case = inputs.config("F2")
    case = dict(case, vx=np.sin(np.arange(len(case["x"]))) * 3.0, vy=np.cos(np.arange(len(case["x"]))) * 3.0)
    a = api.Engine(api.Model.from_case(case), **kw)
    b = api.Engine(api.Model.from_case(case), **kw)
    b.rdf_setup(8.0, 0.02, nuclei=True)
    a.stats()
    b.rdf_sample()                       # right after init, no step
    for _ in range(5):
        a.step(7)
        a.stats()
        b.step(7)
        b.rdf_sample()
    sa, sb = a.state(), b.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(sa[k], sb[k]), k
    ta, tb = a.stats(), b.stats()
    for k in ta:
        assert ta[k] == tb[k], k
    assert b.rdf_counts()[0] == 6


def kdtree_cumulative(pos, box, radii):
    """unordered pairs i < j with periodic distance <= each radius (scipy's periodic cKDTree)"""
    from scipy.spatial import cKDTree
    radii = np.asarray(radii)
    order = np.argsort(radii)
    t = cKDTree(pos, boxsize=np.asarray(box))
    c = np.empty(len(radii), dtype=np.int64)
    c[order] = t.count_neighbors(t, radii[order], cumulative=True).astype(np.int64)
    return (c - len(pos)) // 2                          # ordered pairs include i == i


def check_kdtree(eng, box, rmax, dr, kind="species"):
    nb = eng.rdf_setup(rmax, dr, nuclei=(kind == "nuclei"))
    eng.rdf_sample()
    pos, _ = positions(eng)
    pos = np.where(pos >= np.asarray(box), 0.0, pos)
    _, got = eng.rdf_counts(kind)
    got = got[:, 0].astype(np.int64)
    edges = np.arange(1, nb + 1) * dr
    c = kdtree_cumulative(pos, box, np.concatenate([edges, edges * (1 - EDGE), edges * (1 + EDGE)]))
    mid, lo, hi = c[:nb], c[nb:2 * nb], c[2 * nb:]
    cum = np.cumsum(got)                                # pairs with r < (k + 1) dr
    assert ((cum >= lo) & (cum <= hi)).all(), np.nonzero((cum < lo) | (cum > hi))
    assert (cum == mid).mean() > 0.99
    return got


def test_fullsize_fcc_shells():
    case = inputs.lj_case((63, 63, 63), a=5.735, jitter=0.0, seed=1)
    eng = api.Engine(api.Model.from_case(case))
    nb = eng.rdf_setup(8.5, 0.02)
    eng.rdf_sample()
    _, got = eng.rdf_counts()
    N = 4 * 63 ** 3
    a = 5.735
    want = np.zeros(nb, dtype=np.int64)
    for shell, n in ((a / np.sqrt(2), 12), (a, 6), (a * np.sqrt(1.5), 24), (a * np.sqrt(2), 12)):
        want[int(shell / 0.02)] += N * n // 2
    assert np.array_equal(got[:, 0].astype(np.int64), want)


def test_fullsize_c4_against_kdtree():
    case = inputs.config("C4")
    eng = api.Engine(api.Model.from_case(case))
    got = check_kdtree(eng, case["box"], 8.5, 0.02)
    assert got.sum() > 27_000_000


def test_case_study_2_through_api(tmp_path):
    d = util.materialise_case_study(2, str(tmp_path / "cs2"))
    m = api.Model.from_dir(d)
    eng = api.Engine(m, initial_forces=0)
    eng.step(5)
    box = list(m.query("box"))
    check_engine(eng, box, 8.0, 0.02)


def test_case_study_1_through_api(tmp_path):
    d = util.materialise_case_study(1, str(tmp_path / "cs1"))
    m = api.Model.from_dir(d)
    assert m.query("rdf")[5] == 1
    eng = api.Engine(m, initial_forces=0)
    eng.step(5)
    box = list(m.query("box"))
    got = check_kdtree(eng, box, 14.0, 0.02, kind="nuclei")
    _, sp = eng.rdf_counts("nuclei")
    assert got.sum() > 0 and np.array_equal(sp[:, 0].astype(np.int64), got)


def run_cli(d):
    exe = os.path.join(ROOT, "aztotmd_amd", "aztotmd")
    r = subprocess.run([exe, d, "--out", d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def replay_rdf(d, nstep, stat, every, kinds):
    """the CLI's call boundaries (main.cpp): aztot_step up to the next stat row or RDF sample, samples after steps c with (c - 1) % every == 0"""
    m = api.Model.from_dir(d)
    eng = api.Engine(m, initial_forces=0)
    eng.rdf_setup(m.query("rdf")[1], m.query("rdf")[2], nuclei="nuclei" in kinds)
    done = 0
    while done < nstep:
        n = min(stat - done % stat, nstep - done)
        nxt = 1 if done < 1 else done + 1 + (every - done % every) % every
        n = min(n, nxt - done)
        eng.step(n)
        done += n
        if (done - 1) % every == 0:
            eng.rdf_sample()
        if done % stat == 0 or done == nstep:
            eng.stats()
    return eng


def render(r, g, names):
    lines = ["r" + "".join("\t" + p for p in names)]
    lines += ["%f" % r[i] + "".join("\t%f" % v for v in g[i]) for i in range(len(r))]
    return "\n".join(lines) + "\n"


def test_cli_case_study_2(tmp_path):
    d = util.materialise_case_study(2, str(tmp_path / "cs2"), nstep=25)
    run_cli(d)
    assert not os.path.exists(os.path.join(d, "rdf_n.dat"))
    text = open(os.path.join(d, "rdf.dat")).read()
    rows = text.splitlines()
    assert rows[0] == "r\tAr-Ar" and len(rows) == 1 + 400
    assert os.path.exists(os.path.join(d, "rdf0.dat")) and not os.path.exists(os.path.join(d, "rdf10.dat"))
    eng = replay_rdf(d, 25, 200, 10, ("species",))
    assert eng.rdf_counts()[0] == 3                    # after steps 1, 11, 21
    assert text == render(*eng.rdf("species"))
    stat = open(os.path.join(d, "stat.dat")).read().splitlines()
    assert len(stat) == 2 + 1 and int(stat[-1].split("\t")[1]) == 25


def test_cli_nuclei_files(tmp_path):
    case = inputs.lj_case((8, 8, 8), a=5.26, seed=3, charges=(0.0, 0.0), vel_T=85.0)      # two neutral species A, B
    case["nsteps"] = 12
    d = str(tmp_path / "n")
    inputs.write_input_files(case, d, stat=5)
    ctl = open(os.path.join(d, "control.txt")).read().replace("rdf\t8.0\t0.02\t1000000\t1000000\tnucl", "rdf\t8.0\t0.02\t5\t10\tnucl")
    open(os.path.join(d, "control.txt"), "w").write(ctl)
    run_cli(d)
    for f in ("rdf.dat", "rdf_n.dat", "rdf0.dat", "rdf_n0.dat", "rdf10.dat", "rdf_n10.dat"):
        assert os.path.exists(os.path.join(d, f)), f
    assert not os.path.exists(os.path.join(d, "rdf5.dat"))
    eng = replay_rdf(d, 12, 5, 5, ("species", "nuclei"))
    assert eng.rdf_counts()[0] == 3                    # after steps 1, 6, 11
    assert open(os.path.join(d, "rdf.dat")).read() == render(*eng.rdf("species"))
    assert open(os.path.join(d, "rdf_n.dat")).read() == render(*eng.rdf("nuclei"))
    head = open(os.path.join(d, "rdf_n10.dat")).readline()
    assert head == "r\tA-A\tA-B\tB-B\n"
    assert len(open(os.path.join(d, "rdf10.dat")).read().splitlines()) == 401


def test_errors():
    case = inputs.config("F1")
    eng = api.Engine(api.Model.from_case(case))
    for call in (eng.rdf_sample, eng.rdf_reset, eng.rdf_counts, eng.rdf):
        with pytest.raises(api.AztotError) as e:
            call()
        assert e.value.code == -4
    for rmax, dr in ((0.0, 0.02), (-1.0, 0.02), (8.0, 0.0), (8.0, -0.1), (8.0, 100.0)):
        with pytest.raises(api.AztotError) as e:
            eng.rdf_setup(rmax, dr)
        assert e.value.code == -4, (rmax, dr)
    eng.rdf_setup(6.0, 0.05)
    with pytest.raises(api.AztotError) as e:
        eng.rdf_counts("nuclei")
    assert e.value.code == -4
    eng.rdf_sample()
    assert eng.rdf_counts()[0] == 1
    assert eng.rdf_setup(6.0, 0.05, nuclei=True) == 120 and eng.rdf_counts()[0] == 0    # set up again: zeroed


def test_slab_handle_refused():
    case = inputs.lj_case((42, 5, 5), a=5.735, seed=31, rc=8.5, vel_T=8.0)
    eng = api.Engine(api.Model.from_case(case), slab={"rank": 1, "nranks": 2, "loopback": True})
    with pytest.raises(api.AztotError) as e:
        eng.rdf_setup(8.0, 0.02)
    assert e.value.code == -2 and "slab" in str(e.value)
