"""GPU tests of the coordination numbers (aztot_cn_*, cn.hip.h) against an fp64 host restatement of the rules in include/aztot.h.  The reference's
out_cn / out_ncn are not in the oracle's build, so the pin is this restatement, each rule with its reference line:

  r2      sqr_distance (box.cpp:297-305): delta_periodic (one shift by L where |d| > L / 2) on the positions the engine hands out, (dx*dx + dy*dy) + dz*dz
  species R * R >= r2 (out_md.cpp:434), every ordered pair INCLUDING j == i (the loop at out_md.cpp:429 does not skip it), rows CN = 0 .. max
  nuclei  r2 < R * R (out_md.cpp:313,318), pairs i != j only (out_md.cpp:301-304), rows min(10, smallest) .. max(0, largest) (out_md.cpp:300), with
          min / max over ALL atoms (the reference leaves the last atom out, out_md.cpp:301: a bug we do not copy)

Comparison is exact, per atom and per table cell: the device and the host evaluate the same correctly rounded operations in the same order."""
import os
import subprocess

import numpy as np
import pytest

from aztotmd_amd import api, inputs

import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = 1e-9


def host_cn(pos, groups, box, cols, kind):
    """(per_atom[N, ncols] with -1 where the atom is not of the column's central group, cn_min, cn_max, table[cn - cn_min, col])"""
    L = np.asarray(box, dtype=np.float64)
    half = L * 0.5
    N = len(pos)
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    per = np.full((N, len(cols)), -1, dtype=np.int64)
    mine = [[c for c, col in enumerate(cols) if col[0] == g] for g in range(int(max(groups.max(), max(c[0] for c in cols))) + 1)]
    for i in range(N):
        live = mine[groups[i]]
        if not live:
            continue
        d = []
        for c, k in ((x, 0), (y, 1), (z, 2)):
            v = c[i] - c
            v = np.where(v > half[k], v - L[k], np.where(v < -half[k], v + L[k], v))
            d.append(v)
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        for c in live:
            _, lig, R = cols[c]
            if kind == "species":
                hit = (R * R >= r2) & (groups == lig)
            else:
                hit = (r2 < R * R) & (groups == lig)
                hit[i] = False
            per[i, c] = int(hit.sum())
    livev = per[per >= 0]
    if kind == "species":
        mn, mx = 0, int(max(0, livev.max())) if livev.size else 0
    else:
        mn = int(min(10, livev.min())) if livev.size else 10
        mx = int(max(0, livev.max())) if livev.size else 0
    table = np.zeros((max(mx - mn + 1, 0), len(cols)), dtype=np.int64)
    for c in range(len(cols)):
        v = per[:, c][per[:, c] >= 0]
        if v.size:
            table[:, c] = np.bincount(v - mn, minlength=table.shape[0])
    return per, mn, mx, table


def positions(eng):
    s = eng.state(("x", "y", "z"))
    return np.stack([s["x"], s["y"], s["z"]], axis=1), s["types"]


def check(eng, box, kind, cols, nuclei_of=None, setup=True):
    if setup:
        eng.cn_setup(kind, cols)
    eng.cn_sample(kind)
    pos, types = positions(eng)
    groups = types if kind == "species" else np.asarray(nuclei_of)[types]
    per, mn, mx, table = host_cn(pos, groups, box, cols, kind)
    got = eng.cn_per_atom(kind)
    print(kind, cols, "rows", mn, mx, "device rows", eng.cn_shape(kind), "per-atom mismatches", int((got != per).sum()))
    assert eng.cn_shape(kind) == (len(cols), mn, mx)
    assert got.shape == per.shape and np.array_equal(got, per)
    gmn, gt = eng.cn_table(kind)
    assert gmn == mn and gt.shape == table.shape and np.array_equal(gt, table)
    return per, table


def random_case(nspec, N, box, seed, faces=False, used=None):
    """as tests/test_gpu_rdf.py::random_case; `used`: only the first `used` species have atoms"""
    rng = np.random.default_rng(seed)
    pos = rng.random((N, 3)) * np.asarray(box)
    pos = np.round(pos, 6)
    if faces:                                        # atoms on the box faces and edges
        pos[:40, 0] = 0.0
        pos[20:60, 1] = 0.0
        pos[50:70, 2] = 0.0
    for k in range(3):
        pos[pos[:, k] >= box[k], k] = 0.0
    types = (np.arange(N) % (used or nspec)).astype(np.int32)
    rc = min(3.0, 0.45 * min(box))
    vdw = [(a, b, 1, rc, [0.001, 1.0]) for a in range(nspec) for b in range(a, nspec)]
    return {"box": list(box), "dt": 0.001, "species": [(39.9, 0.0)] * nspec, "names": ["S%d" % k for k in range(nspec)], "types": types,
            "vdw": vdw, "x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": np.zeros(N), "vy": np.zeros(N), "vz": np.zeros(N),
            "cell_list": rc, "use_clist": 1, "elec_type": 0}


def shared_nucleus_model(case, d):
    """the case through its input files, with S0 and S1 sharing nucleus 'S0'"""
    inputs.write_input_files(case, d)
    fld = open(os.path.join(d, "field.txt")).read().replace("S1\tS1\t", "S1\tS0\t", 1)
    open(os.path.join(d, "field.txt"), "w").write(fld)
    m = api.Model.from_dir(d)
    assert list(m.query("nuclei"))[:2] == [0, 0]
    return m


GEOMETRIES = [
    (2, (35.0, 35.0, 35.0), 8.0, False),       # 4 x 4 x 4 cells
    (3, (33.0, 36.0, 31.0), 7.5, True),        # 4 x 4 x 4 cells, atoms on faces and edges, two species on one nucleus
    (2, (12.0, 13.0, 14.0), 8.0, False),       # R > L / 2 on every axis: one cell per axis
    (3, (8.2, 17.0, 26.0), 8.0, True),         # 1, 2 and 3 cells per axis: each distinct cell once
    (2, (17.0, 26.0, 17.0), 8.0, False),       # 2 and 3 cells
    (2, (9.0, 30.0, 30.0), 12.0, False),       # R > L_x
]


@pytest.mark.parametrize("nspec,box,R,faces", GEOMETRIES)
def test_small_systems_exact(tmp_path, nspec, box, R, faces):
    case = random_case(nspec, 3000, box, seed=int(R * 100) + nspec, faces=faces)
    if nspec == 3:
        eng = api.Engine(shared_nucleus_model(case, str(tmp_path / "m")))
        nuc = [0, 0, 1]
        # S0 central and ligand (itself counted), S2 central only, S1 ligand only
        scols = [(0, 0, R), (0, 1, R), (2, 0, R), (2, 1, R)]
    else:
        eng = api.Engine(api.Model.from_case(case))
        nuc = [0, 1]
        scols = [(0, 0, R), (0, 1, R), (1, 0, R), (1, 1, R)]
    # directed columns with their own radii; (1, 1) is left out
    ncols = [(0, 0, R), (0, 1, 0.8 * R), (1, 0, 0.6 * R)]
    check(eng, box, "species", scols)
    check(eng, box, "nuclei", ncols, nuc)
    # both kinds live side by side: the species sample is still there, untouched by the nuclei one
    per, _, _, table = host_cn(positions(eng)[0], positions(eng)[1], box, scols, "species")
    assert np.array_equal(eng.cn_per_atom("species"), per) and np.array_equal(eng.cn_table("species")[1], table)
    # set-up again replaces the columns: A -> B without B -> A, one column only
    check(eng, box, "nuclei", [(0, 1, 0.5 * R)], nuc)
    check(eng, box, "species", [(1, 0, 0.7 * R)])


def test_min_rule_of_nuclei_rows():
    """smallest count above 10: the file starts at 10 (mn = 10, out_md.cpp:300); below 10: at the smallest"""
    box = (30.0, 30.0, 30.0)
    eng = api.Engine(api.Model.from_case(random_case(2, 3000, box, seed=5)))
    _, table = check(eng, box, "nuclei", [(0, 0, 9.0), (1, 0, 9.0)], [0, 1])        # ~ 170 neighbours each
    assert eng.cn_shape("nuclei")[1] == 10 and not table[0].any()
    check(eng, box, "nuclei", [(0, 1, 2.5)], [0, 1])                                   # ~ 3.6 neighbours: zeros occur
    assert eng.cn_shape("nuclei")[1] == 0


def test_empty_central_group(tmp_path):
    box = (30.0, 31.0, 32.0)
    case = random_case(3, 3000, box, seed=9, used=2)            # S2 is declared and has no atom
    d = inputs.write_input_files(case, str(tmp_path / "m"))
    eng = api.Engine(api.Model.from_dir(d))
    _, table = check(eng, box, "species", [(2, 0, 6.0), (0, 2, 6.0), (0, 1, 6.0)])
    assert not table[:, 0].any() and table[0, 1] == 1500 and table[:, 2].sum() == 1500
    _, table = check(eng, box, "nuclei", [(2, 0, 6.0), (1, 0, 6.0)], [0, 1, 2])
    assert not table[:, 0].any() and table[:, 1].sum() == 1500
    check(eng, box, "nuclei", [(2, 0, 6.0)], [0, 1, 2])          # nothing but an empty group: mn = 10 > mx = 0, no row
    assert eng.cn_shape("nuclei") == (1, 10, 0) and eng.cn_table("nuclei")[1].shape == (0, 1)


def test_fifteen_species_all_columns():
    """15 x 15 species columns: every atom keeps 15 counters"""
    box = (30.0, 30.0, 30.0)
    eng = api.Engine(api.Model.from_case(random_case(15, 2500, box, seed=15)))
    check(eng, box, "species", [(a, b, 7.0) for a in range(15) for b in range(15)])
    check(eng, box, "nuclei", [(a, (a * 7 + k) % 15, 5.0 + 0.2 * k) for a in range(15) for k in range(5)], list(range(15)))


@pytest.mark.parametrize("n", [10, 14, 20, 30])       # 4 000 ... 108 000 atoms: 32, 8, 4 and 1 lanes per atom
def test_fcc_known_answers(n):
    case = inputs.lj_case((n, n, n), a=5.735, jitter=0.0, seed=1)
    eng = api.Engine(api.Model.from_case(case))
    N = 4 * n ** 3
    for R, shell in ((4.5, 12), (5.8, 18)):
        eng.cn_setup("species", [(0, 0, R)])
        eng.cn_setup("nuclei", [(0, 0, R)])
        eng.cn_sample("species")
        eng.cn_sample("nuclei")
        s, u = eng.cn_per_atom("species"), eng.cn_per_atom("nuclei")
        print(n, R, np.unique(s), np.unique(u))
        assert (s == shell + 1).all() and (u == shell).all()            # 12 (18) neighbours + the atom itself under the species rules
        assert eng.cn_shape("species") == (1, 0, shell + 1) and eng.cn_shape("nuclei") == (1, 10, shell)
        mn, t = eng.cn_table("species")
        assert mn == 0 and t[-1, 0] == N and t.sum() == N
        mn, t = eng.cn_table("nuclei")
        assert mn == 10 and t[-1, 0] == N and t.sum() == N


def kdtree_counts(pos, box, R):
    from scipy.spatial import cKDTree
    t = cKDTree(pos, boxsize=np.asarray(box))
    return [t.query_ball_point(pos, r, return_length=True, workers=16).astype(np.int64) for r in (R * (1 - EDGE), R * (1 + EDGE))]


def check_kdtree(eng, box, R):
    """per atom against scipy's periodic KD-tree (which counts the atom itself), bracketed by R (1 -+ 1e-9): every atom whose brackets agree must match"""
    eng.cn_setup("species", [(0, 0, R)])
    eng.cn_setup("nuclei", [(0, 0, R)])
    eng.cn_sample("species")
    eng.cn_sample("nuclei")
    pos, _ = positions(eng)
    pos = np.where(pos >= np.asarray(box), 0.0, pos)
    lo, hi = kdtree_counts(pos, box, R)
    sure = lo == hi
    s, u = eng.cn_per_atom("species")[:, 0], eng.cn_per_atom("nuclei")[:, 0]
    print("R", R, "atoms compared", int(sure.sum()), "of", len(sure), "species mismatches", int((s[sure] != lo[sure]).sum()),
          "nuclei mismatches", int((u[sure] != lo[sure] - 1).sum()), "counts", np.unique(s)[[0, -1]])
    assert sure.mean() >= 0.999
    assert np.array_equal(s[sure], lo[sure]) and np.array_equal(u[sure], lo[sure] - 1)
    assert ((s >= lo) & (s <= hi)).all() and ((u >= lo - 1) & (u <= hi - 1)).all()
    for kind, v in (("species", s), ("nuclei", u)):
        nc, mn, mx = eng.cn_shape(kind)
        assert mx == v.max() and mn == (0 if kind == "species" else min(10, v.min()))
        gmn, t = eng.cn_table(kind)
        assert np.array_equal(t[:, 0], np.bincount(v - mn, minlength=mx - mn + 1))
    return s


def test_fullsize_c4_against_kdtree():
    case = inputs.config("C4")
    eng = api.Engine(api.Model.from_case(case))
    s = check_kdtree(eng, case["box"], 4.055)           # inside the first shell's jitter band (a / sqrt 2): counts spread from 1 to 13
    assert s.min() < 5 and s.max() >= 12
    s = check_kdtree(eng, case["box"], 4.5)
    assert (s == 13).all()


def test_case_study_2_through_api(tmp_path):
    d = util.materialise_case_study(2, str(tmp_path / "cs2"))
    m = api.Model.from_dir(d)
    eng = api.Engine(m, initial_forces=0)
    eng.step(5)
    box = list(m.query("box"))
    check(eng, box, "species", [(0, 0, 8.0)])           # 62 atoms per cell: the dense end
    check(eng, box, "nuclei", [(0, 0, 8.0)], [0])


def test_case_study_1_through_api(tmp_path):
    d = util.materialise_case_study(1, str(tmp_path / "cs1"))
    m = api.Model.from_dir(d)
    eng = api.Engine(m, initial_forces=0)
    eng.step(5)
    box = list(m.query("box"))
    s = check_kdtree(eng, box, 14.0)                    # the dilute end (40 000 atoms in 1141.5 A): the grid is capped at about N cells
    assert s.min() == 1 and s.max() > 1


def test_sample_is_a_snapshot():
    case = inputs.config("F2")
    eng = api.Engine(api.Model.from_case(case))
    cols = [(0, 0, 4.2)]
    per0, t0 = check(eng, case["box"], "species", cols)
    eng.cn_sample("species")                                # nothing accumulates
    assert np.array_equal(eng.cn_per_atom("species"), per0) and np.array_equal(eng.cn_table("species")[1], t0)
    eng.step(12)
    assert np.array_equal(eng.cn_per_atom("species"), per0)            # the old snapshot stays until the next sample
    check(eng, case["box"], "species", cols, setup=False)
    check(eng, case["box"], "nuclei", [(0, 0, 3.9)], [0])
    check(eng, case["box"], "species", [(0, 0, 6.0)])                   # set-up again replaces the columns
    with pytest.raises(api.AztotError):
        eng.cn_setup("species", [(0, 0, 6.0), (0, 0, 7.0)])            # a failed set-up leaves the old one in place
    assert eng.cn_shape("species")[0] == 1


@pytest.mark.parametrize("kw", [{}, {"sort_every": 1}, {"use_graph": 0, "pair_variant": 1}])
def test_sampling_does_not_perturb(kw):
    case = inputs.config("F2")
    case = dict(case, vx=np.sin(np.arange(len(case["x"]))) * 3.0, vy=np.cos(np.arange(len(case["x"]))) * 3.0)
    a = api.Engine(api.Model.from_case(case), **kw)
    b = api.Engine(api.Model.from_case(case), **kw)
    b.cn_setup("species", [(0, 0, 4.2)])
    b.cn_setup("nuclei", [(0, 0, 5.5)])
    a.stats()
    b.cn_sample("species")                  # right after init, no step
    b.cn_sample("nuclei")
    for _ in range(5):
        a.step(7)
        a.stats()
        b.step(7)
        b.cn_sample("species")
        b.cn_sample("nuclei")
    sa, sb = a.state(), b.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(sa[k], sb[k]), k
    ta, tb = a.stats(), b.stats()
    for k in ta:
        assert ta[k] == tb[k], k


def run_cli(d):
    exe = os.path.join(ROOT, "aztotmd_amd", "aztotmd")
    r = subprocess.run([exe, d, "--out", d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def replay(d, nstep, stat, every):
    """the CLI's call boundaries (main.cpp): aztot_step up to the next stat row or RDF sample, samples after steps c with (c - 1) % every == 0"""
    m = api.Model.from_dir(d)
    eng = api.Engine(m, initial_forces=0)
    eng.rdf_setup(m.query("rdf")[1], m.query("rdf")[2], nuclei=bool(m.query("rdf")[5]))
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
    return m, eng


def render(eng, kind, cols, names):
    eng.cn_setup(kind, cols)
    eng.cn_sample(kind)
    mn, t = eng.cn_table(kind)
    lines = ["CN" + "".join("\t%s-%s" % (names[a], names[b]) for a, b, _ in cols)]
    lines += ["%d" % (mn + i) + "".join("\t%d" % v for v in t[i]) for i in range(len(t))]
    return "\n".join(lines) + "\n"


def test_cli_files(tmp_path):
    case = inputs.lj_case((8, 8, 8), a=5.26, seed=3, charges=(0.0, 0.0), vel_T=85.0)      # two neutral species A, B
    case["nsteps"] = 12
    plain = inputs.write_input_files(case, str(tmp_path / "p"), stat=5)
    run_cli(plain)
    assert not os.path.exists(os.path.join(plain, "CN.dat")) and not os.path.exists(os.path.join(plain, "nCN.dat"))
    d = inputs.write_input_files(dict(case, outCN=(4.0, ["A", "B"], ["B"]), ncn=[("A", "B", 4.0), ("B", "B", 5.5), ("B", "A", 3.8)]), str(tmp_path / "n"), stat=5)
    run_cli(d)
    m, eng = replay(d, 12, 5, 1000000)
    names = [m.species_name(i) for i in range(2)]
    cn = open(os.path.join(d, "CN.dat")).read()
    assert cn.splitlines()[0] == "CN\tA-B\tB-B" and cn.splitlines()[1].startswith("0\t")
    assert cn == render(eng, "species", [(0, 1, 4.0), (1, 1, 4.0)], names)
    ncn = open(os.path.join(d, "nCN.dat")).read()
    assert ncn.splitlines()[0] == "CN\tA-B\tB-B\tB-A"
    assert ncn == render(eng, "nuclei", [(0, 1, 4.0), (1, 1, 5.5), (1, 0, 3.8)], [m.nucleus_name(i) for i in range(2)])
    # the files hold every atom of each column's central group
    rows = np.array([[int(v) for v in l.split("\t")] for l in cn.splitlines()[1:]])
    assert rows[:, 1].sum() == 1024 and rows[:, 2].sum() == 1024
    # the other outputs are those of the run without the directives
    for f in ("stat.dat", "revcon.xyz", "velocities.dat", "rdf.dat"):
        assert open(os.path.join(d, f)).read() == open(os.path.join(plain, f)).read(), f


def test_cli_case_study_2_writes_the_same_files(tmp_path):
    d = util.materialise_case_study(2, str(tmp_path / "cs2"), nstep=25)
    before = set(os.listdir(d))
    run_cli(d)
    made = set(os.listdir(d)) - before
    assert made - {"tchars.dat"} == {"stat.dat", "msd.dat", "revcon.xyz", "velocities.dat", "rdf.dat", "rdf0.dat"}, made


def test_cli_unusable_directive_warns_and_skips(tmp_path):
    case = inputs.lj_case((6, 6, 6), a=5.26, seed=3, charges=(0.0, 0.0))
    case["nsteps"] = 2
    d = inputs.write_input_files(dict(case, outCN=(-4.0, ["A"], ["B"]), ncn=[("A", "B", 4.0)]), str(tmp_path / "n"), stat=5)
    r = run_cli(d)
    assert "WARNING: outCN directive not usable" in r.stderr
    assert not os.path.exists(os.path.join(d, "CN.dat")) and os.path.exists(os.path.join(d, "nCN.dat"))


def test_errors():
    case = inputs.config("F1")
    eng = api.Engine(api.Model.from_case(case))
    L = api.lib()
    for kind in ("species", "nuclei"):
        for call in (eng.cn_sample, eng.cn_shape, eng.cn_per_atom, eng.cn_table):
            with pytest.raises(api.AztotError) as e:
                call(kind)
            assert e.value.code == -4
        for cols in ([], [(1, 0, 4.0)], [(0, 1, 4.0)], [(-1, 0, 4.0)], [(0, 0, 0.0)], [(0, 0, -2.0)], [(0, 0, float("nan"))], [(0, 0, 4.0), (0, 0, 4.0)]):
            with pytest.raises(api.AztotError) as e:
                eng.cn_setup(kind, cols)
            assert e.value.code == -4, cols
        eng.cn_setup(kind, [(0, 0, 4.0)])
        for call in (eng.cn_shape, eng.cn_per_atom, eng.cn_table):          # set up, not sampled yet
            with pytest.raises(api.AztotError) as e:
                call(kind)
            assert e.value.code == -4
        eng.cn_sample(kind)
        assert eng.cn_per_atom(kind).shape == (500, 1)
    col = api._CnColumn(0, 0, 4.0)
    assert L.aztot_cn_setup(eng.h, 2, col, 1) == -4 and L.aztot_cn_sample(eng.h, -1) == -4
    assert L.aztot_cn_setup(eng.h, 0, None, 1) == -4
    # sizes by cap = 0, nothing written below the size
    assert L.aztot_cn_per_atom(eng.h, 0, None, 0) == 500 and L.aztot_cn_table(eng.h, 0, None, 0) == eng.cn_shape("species")[2] + 1
    small = np.full(4, 77, dtype=np.int32)
    assert L.aztot_cn_per_atom(eng.h, 0, small.ctypes.data_as(api._ip), 4) == 500 and (small == 77).all()


def test_species_kind_needs_one_radius():
    case = inputs.lj_case((5, 5, 5), a=5.26, seed=3, charges=(0.0, 0.0))
    eng = api.Engine(api.Model.from_case(case))
    with pytest.raises(api.AztotError) as e:
        eng.cn_setup("species", [(0, 0, 4.0), (0, 1, 4.5)])
    assert e.value.code == -4
    eng.cn_setup("nuclei", [(0, 0, 4.0), (0, 1, 4.5)])


def test_slab_handle_refused():
    case = inputs.lj_case((42, 5, 5), a=5.735, seed=31, rc=8.5, vel_T=8.0)
    eng = api.Engine(api.Model.from_case(case), slab={"rank": 1, "nranks": 2, "loopback": True})
    for kind in ("species", "nuclei"):
        with pytest.raises(api.AztotError) as e:
            eng.cn_setup(kind, [(0, 0, 4.0)])
        assert e.value.code == -2 and "slab" in str(e.value)
