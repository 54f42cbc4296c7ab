"""GPU tests of the bond-orientational order sampler (aztot_boo_*, boo.hip.h) against tests/boo_model.py.

q_lm is held per component to boo_model.QLM_TOL (four times the worst error of the fp64 restatement of the route over the very cases of boo_cases.py,
measured on the CPU); neighbour counts, histograms, sums and entered counts are compared exactly; q_l and q-bar_l are compared with the model applied
to the device's own q_lm read-back (which separates k_boo_average from k_boo_qlm) and with the 60-digit values, both to boo_model.Q_TOL.

Lanes per atom depend on N alone (boo_cases.LANE_COUNTS): the cases lanes64 ... lanes1 are N = 2047, 2048, 4096, 8192, 16384, 32768 and 65536, the first
N of every lane count but the first.  From N = 4096 a sample of the atoms goes through the 60-digit model and the neighbour counts of all atoms
are compared with the coordination-number sampler."""
import os

import numpy as np
import pytest

from aztotmd_amd import api, inputs

import boo_cases as bc
import boo_model as bm
from test_gpu_cn import positions, random_case, run_cli

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in bc.all_cases()}
N_BINS = 40


def compare_counts(eng, before=None):
    """histograms, sums and entered of the handle against the model applied to the per-atom values it hands out; returns what the handle holds"""
    orders, nb, ns, _ = eng.boo_shape()
    n, q = eng.boo_per_atom()
    types = positions(eng)[1]
    hist, sums, entered = bm.totals(n, q, types, ns, nb)
    samples, gh, gs, ge = eng.boo_counts()
    assert gh.dtype == np.uint64 and gh.shape == (2, len(orders), ns, nb) and gs.shape == (2, len(orders), ns)
    if before is None:
        assert np.array_equal(gh.astype(np.int64), hist) and np.array_equal(ge.astype(np.int64), entered)
        assert np.array_equal(gs, sums), (gs, sums)                     # the tree over the ids: to the bit
    else:
        assert np.array_equal(gh.astype(np.int64), before[1].astype(np.int64) + hist) and np.array_equal(ge.astype(np.int64), before[3].astype(np.int64) + entered)
        assert np.array_equal(gs, before[2] + sums)                     # added once per sample in sample order
    assert (q[n <= 0] == 0.0).all() and int(entered.sum()) == int((n > 0).sum())
    return samples, gh, gs, ge


def check_case(c, n_bins=N_BINS):
    eng = api.Engine(api.Model.from_case(c["case"]))
    orders = c["orders"]
    assert eng.boo_setup(c["R"], orders, n_bins, c["central"], c["ligand"]) == n_bins
    eng.boo_sample()
    pos, types = positions(eng)
    N = len(pos)
    B = bm.bonds(pos, types, c["box"], c["R"], c["central"], c["ligand"], atoms=c["atoms"])
    rows = np.arange(N) if c["atoms"] is None else np.asarray(c["atoms"])
    n, q = eng.boo_per_atom()
    qlm = eng.boo_qlm()
    assert n.shape == (N,) and q.shape == (N, len(orders), 2) and qlm.shape == (N, len(orders), 13)
    assert np.array_equal(n[rows], B.n[rows])
    central = ((c["central"] >> types) & 1).astype(bool)
    assert (n[~central] == -1).all() and (n[central] >= 0).all() and not qlm[n <= 0].any() and not q[n <= 0].any()
    if c["atoms"] is not None and N > 1000:     # every atom's count, through the coordination numbers of kind 'nuclei' (strict radius, i != j)
        ns = int(types.max()) + 1
        cols = [(a, b, c["R"]) for a in range(ns) if (c["central"] >> a) & 1 for b in range(ns) if (c["ligand"] >> b) & 1]
        eng.cn_setup("nuclei", cols)
        eng.cn_sample("nuclei")
        assert np.array_equal(n, np.where(central, np.maximum(eng.cn_per_atom("nuclei"), 0).sum(axis=1), -1))
    worst = worst_q = 0.0
    model_q = bm.per_atom(B, qlm, orders)
    for o, l in enumerate(orders):
        assert not qlm[:, o, l + 1:].any()                              # padded to m = 12 with zeros
        re, im = bm.exact_qlm(B, l)
        worst = max(worst, bm.qlm_error(qlm[rows, o], (re[rows], im[rows])))
        are, aim = bm.exact_averaged(B, re, im)
        if c["atoms"] is None:                                          # (the average needs the exact q_lm of every neighbour)
            exact = np.stack([bm.to_float(bm.exact_invariant(re, im, l)), bm.to_float(bm.exact_invariant(are, aim, l))], axis=1)
            worst_q = max(worst_q, float(np.abs(q[:, o, :] - exact).max()) if N else 0.0)
    own = float(np.abs(q[rows] - model_q[rows]).max()) if len(rows) else 0.0
    print(c["name"], "atoms", N, "bonds", len(B.r2), "q_lm error / bound", worst / bm.QLM_TOL, "q error / bound", worst_q / bm.Q_TOL,
          "q against the model on the read-back / bound", own / bm.Q_TOL)
    assert worst <= bm.QLM_TOL and worst_q <= bm.Q_TOL and own <= bm.Q_TOL
    compare_counts(eng)
    return eng, B


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith(("geometry", "sparse"))])
def test_geometries(name):
    """six geometries at 3000 atoms with a handful of neighbours; the sparse variants: one cell per axis, 1 / 2 / 3 cells, R > L / 2, R > L_x; orders (4, 6),
    (1, 2, 12) and (12,); masks equal, overlapping and disjoint"""
    _, B = check_case(CASES[name])
    assert B.n.max() >= 3


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("atoms")])
def test_atom_counts(name):
    check_case(CASES[name])


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("lanes")])
def test_every_lane_count(name):
    check_case(CASES[name])


@pytest.mark.parametrize("name", ["empty_species", "order12_alone"])
def test_masks_and_orders(name):
    eng, B = check_case(CASES[name], n_bins=4096 if name == "order12_alone" else 1)     # 2 * 1 * 2 * 4096 cells: past the LDS budget, global atomics
    if name == "empty_species":
        assert eng.boo_counts()[3][2] == 0 and (B.n[positions(eng)[1] == 1] == -1).all()


def designed_case():
    """bonds exactly along +-z and +-x around atom 0; a pair across the x face and a pair along z on the y = z = 0 edges (isolated: q_l = 1 for every l);
    atom 9 has no neighbour"""
    box = (20.0, 20.0, 20.0)
    pos = np.array([(5.0, 5.0, 5.0), (5.0, 5.0, 6.5), (5.0, 5.0, 3.5), (6.5, 5.0, 5.0), (3.5, 5.0, 5.0),
                    (0.0, 10.0, 10.0), (18.5, 10.0, 10.0), (10.0, 0.0, 0.0), (10.0, 0.0, 18.75), (15.0, 15.0, 15.0)])
    case = random_case(1, len(pos), box, seed=1)
    case.update(x=pos[:, 0].copy(), y=pos[:, 1].copy(), z=pos[:, 2].copy())
    return case, box


def test_designed_atoms():
    case, box = designed_case()
    orders = (1, 4, 6, 12)
    c = {"name": "designed", "case": case, "box": box, "R": 2.0, "central": 1, "ligand": 1, "orders": orders, "atoms": None}
    eng, B = check_case(c)
    n, q = eng.boo_per_atom()
    assert list(n) == [4, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    assert np.abs(q[1:9, :, 0] - 1.0).max() <= bm.Q_TOL                # a single neighbour, along +-z, +-x and through a face: q_l = 1
    assert not q[9].any() and eng.boo_counts()[3][0] == 9               # no neighbour: zeros, not entered
    want = [bm.shell_q([(0, 0, 1.5), (0, 0, -1.5), (1.5, 0, 0), (-1.5, 0, 0)], l) for l in orders]
    assert np.abs(q[0, :, 0] - want).max() <= bm.Q_TOL and q[0, 0, 0] <= bm.Q_TOL      # odd l of an inversion-symmetric shell: 0
    for l in (2, 3, 5, 7, 8, 9, 10, 11):        # the remaining kernels of the template switch, on the same atoms
        eng.boo_setup(2.0, (l,), 8, 1, 1)
        eng.boo_sample()
        got = eng.boo_per_atom()[1]
        assert abs(got[0, 0, 0] - bm.shell_q([(0, 0, 1.5), (0, 0, -1.5), (1.5, 0, 0), (-1.5, 0, 0)], l)) <= bm.Q_TOL and np.abs(got[1:9, 0, 0] - 1.0).max() <= bm.Q_TOL


def test_fcc_and_simple_cubic_blocks():
    """256 atoms of FCC (a = 6, R between the first two shells) and a 6 x 6 x 6 simple-cubic block: every atom's q_l and q-bar_l are the known answers"""
    fcc = inputs.lj_case((4, 4, 4), a=6.0, jitter=0.0, seed=1)
    k = np.arange(6) * 3.0 + 0.5
    sc_pos = np.array([(a, b, c) for a in k for b in k for c in k])
    sc = random_case(1, len(sc_pos), (18.0, 18.0, 18.0), seed=2)
    sc.update(x=sc_pos[:, 0].copy(), y=sc_pos[:, 1].copy(), z=sc_pos[:, 2].copy())
    for name, case, R, nn in (("fcc", fcc, 5.0, 12), ("sc", sc, 3.5, 6)):
        eng = api.Engine(api.Model.from_case(case))
        for orders in ((4, 6, 8, 10), (12,)):
            eng.boo_setup(R, orders, 100, 1, 1)
            eng.boo_sample()
            n, q = eng.boo_per_atom()
            assert len(n) == (256 if name == "fcc" else 216) and (n == nn).all()
            for o, l in enumerate(orders):
                want = bm.KNOWN[name][1][bm.KNOWN_ORDERS.index(l)]
                print(name, l, "worst |q - known|", np.abs(q[:, o, :] - want).max())
                assert np.abs(q[:, o, :] - want).max() <= bm.KNOWN_TOL
                assert eng.boo_counts()[1][:, o, 0].sum(axis=-1).tolist() == [len(n), len(n)]


def test_totals_accumulate_reset_and_values():
    c = CASES["atoms257"]
    eng = api.Engine(api.Model.from_case(c["case"]))
    eng.boo_setup(c["R"], (4, 6), 16, 1, 3)
    eng.boo_sample()
    first = compare_counts(eng)
    eng.step(5)
    eng.boo_sample()
    second = compare_counts(eng, before=first)
    assert second[0] == 2 and eng.boo_shape() == ((4, 6), 16, 2, 2)
    centre, dens, mean = eng.boo_values()
    mc, md, mm = bm.values(second[1].astype(np.int64), second[2], second[3].astype(np.int64))
    assert np.array_equal(centre, mc) and np.array_equal(dens, md) and np.array_equal(mean, mm)
    assert np.allclose(dens[:, :, 0].sum(axis=-1) / 16.0, 1.0) and not dens[:, :, 1].any() and not mean[:, :, 1].any()      # species 1 is not central
    eng.boo_reset()
    s, h, sm, e = eng.boo_counts()
    assert s == 0 and not h.any() and not sm.any() and not e.any()
    eng.boo_sample()
    compare_counts(eng)
    assert eng.boo_setup(c["R"], (6,), 8, 3, 3) == 8                     # a second set-up replaces and zeroes
    assert eng.boo_shape() == ((6,), 8, 2, 0) and not eng.boo_counts()[1].any()
    with pytest.raises(api.AztotError):
        eng.boo_setup(c["R"], (6, 6), 8, 3, 3)                          # a refused set-up leaves the earlier one
    assert eng.boo_shape() == ((6,), 8, 2, 0)


def read_outs(eng):
    n, q = eng.boo_per_atom()
    return (n, q, eng.boo_qlm()) + eng.boo_counts()[1:] + eng.boo_values()


def test_samples_are_a_function_of_the_state_alone():
    case = inputs.lj_case((6, 6, 6), a=5.26, seed=3, charges=(0.0, 0.0), vel_T=85.0)
    keys = ("x", "y", "z", "vx", "vy", "vz")
    src = api.Engine(api.Model.from_case(case))
    src.step(7)
    state = {k: v for k, v in src.state().items() if k in keys}
    a = api.Engine(api.Model.from_case(case))
    b = api.Engine(api.Model.from_case(case), sort_every=1)
    a.set_state(**state)
    b.step(30)                              # the slot order is whatever 30 steps of another schedule left
    b.set_state(**state)
    for e in (a, b):
        e.boo_setup(4.6, (4, 6, 12), 64, 3, 3)
        e.boo_sample()
    ra, rb = read_outs(a), read_outs(b)
    assert ra[0].max() >= 10
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    a.boo_reset()
    a.boo_sample()                          # two samples in a row
    for x, y in zip(read_outs(a), rb):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kw", [{}, {"sort_every": 1}, {"use_graph": 0, "pair_variant": 1}])
def test_sampling_does_not_perturb(kw):
    case = inputs.config("F2")
    case = dict(case, vx=np.sin(np.arange(len(case["x"]))) * 3.0, vy=np.cos(np.arange(len(case["x"]))) * 3.0)
    a = api.Engine(api.Model.from_case(case), **kw)
    b = api.Engine(api.Model.from_case(case), **kw)
    b.boo_setup(4.2, (4, 6), 50, 1, 1)
    a.stats()
    b.boo_sample()                          # right after init, no step
    for _ in range(5):
        a.step(7)
        a.stats()
        b.step(7)
        b.boo_sample()
    assert b.boo_shape()[3] == 6
    sa, sb = a.state(), b.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(sa[k], sb[k]), k
    ta, tb = a.stats(), b.stats()
    for k in ta:
        assert ta[k] == tb[k], k


def replay(d, nstep, stat, every_rdf, setup, every, nequil=0):
    """the CLI's call boundaries (main.cpp): aztot_step up to the next stat row, RDF sample or sample of this sampler"""
    eng = api.Engine(api.Model.from_dir(d), initial_forces=0)
    eng.boo_setup(*setup)
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
            eng.boo_sample()
            taken += 1
        if done % stat == 0 or done == nstep:
            eng.stats()
    if not taken:
        eng.boo_sample()
    return eng


def render(eng, names, central, raw):
    orders, nb, ns, _ = eng.boo_shape()
    centre, dens, mean = eng.boo_values()
    _, hist, _, entered = eng.boo_counts()
    cols = [("%s%d_%s" % ("qbar" if kind else "q", l, names[s]), kind, o, s) for o, l in enumerate(orders) for s in central for kind in range(2)]
    lines = ["q" + "".join("\t" + c[0] for c in cols)]
    for b in range(nb):
        lines.append("%f" % centre[b] + "".join(("\t%d" % hist[k, o, s, b]) if raw else ("\t%f" % dens[k, o, s, b]) for _, k, o, s in cols))
    lines += ["# %s mean %f entered %d" % (name, mean[k, o, s], entered[s]) for name, k, o, s in cols]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("every,samples", [(60, 3), (0, 1)])
def test_cli_files(tmp_path, every, samples):
    """200 steps: samples after steps 60, 120 and 180; every = 0: one sample of the final configuration"""
    case = inputs.lj_case((6, 6, 6), a=5.26, seed=3, charges=(0.0, 0.0), vel_T=85.0)      # two neutral species A, B
    case["nsteps"] = 200
    d = inputs.write_input_files(dict(case, boo=(4.6, 25, every, [4, 6], ["A", "B"], ["A", "B"])), str(tmp_path / "n"), stat=70)
    run_cli(d)
    rdf_every = int(api.Model.from_dir(d).query("rdf")[3]) or 1000000
    eng = replay(d, 200, 70, rdf_every, (4.6, (4, 6), 25, 3, 3), every)
    assert eng.boo_shape() == ((4, 6), 25, 2, samples)
    got, got_n = open(os.path.join(d, "boo.dat")).read(), open(os.path.join(d, "boo_n.dat")).read()
    assert got.splitlines()[0] == "q\tq4_A\tqbar4_A\tq4_B\tqbar4_B\tq6_A\tqbar6_A\tq6_B\tqbar6_B" and got.splitlines()[1].startswith("0.020000\t")
    assert got_n == render(eng, ["A", "B"], (0, 1), True)
    assert got == render(eng, ["A", "B"], (0, 1), False)
    if every == 60:
        plain = inputs.write_input_files(case, str(tmp_path / "p"), stat=70)
        run_cli(plain)
        assert not os.path.exists(os.path.join(plain, "boo.dat")) and not os.path.exists(os.path.join(plain, "boo_n.dat"))
        for f in ("stat.dat", "revcon.xyz", "velocities.dat", "msd.dat"):
            assert open(os.path.join(d, f)).read() == open(os.path.join(plain, f)).read(), f


def test_slab_handle_refused():
    case = inputs.lj_case((42, 5, 5), a=5.735, seed=31, rc=8.5, vel_T=8.0)
    eng = api.Engine(api.Model.from_case(case), slab={"rank": 1, "nranks": 2, "loopback": True})
    with pytest.raises(api.AztotError) as e:
        eng.boo_setup(4.0, (6,), 10, 1, 1)
    assert e.value.code == -2 and "slab" in str(e.value)
    with pytest.raises(api.AztotError) as e:
        eng.boo_sample()
    assert e.value.code == -4
    eng.step(3)                                 # the handle steps on


def test_errors():
    case = inputs.lj_case((5, 5, 5), a=5.26, seed=3, charges=(0.0, 0.0))
    eng = api.Engine(api.Model.from_case(case))
    L = api.lib()
    for call in (eng.boo_sample, eng.boo_reset, eng.boo_shape, eng.boo_per_atom, eng.boo_qlm, eng.boo_counts, eng.boo_values):
        with pytest.raises(api.AztotError) as e:
            call()
        assert e.value.code == -4, call
    good = dict(radius=4.5, orders=(4, 6), n_bins=10, central_mask=1, ligand_mask=3)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(central_mask=0), dict(ligand_mask=0), dict(central_mask=4), dict(ligand_mask=7),
                dict(orders=()), dict(orders=(1, 2, 3, 4, 5)), dict(orders=(0,)), dict(orders=(13,)), dict(orders=(4, 6, 4)), dict(n_bins=0), dict(n_bins=4097),
                dict(reserved=7)):
        with pytest.raises(api.AztotError) as e:
            eng.boo_setup(**dict(good, **bad))
        assert e.value.code == -4, bad
    assert L.aztot_boo_setup(eng.h, None) == -4
    assert eng.boo_setup(**good) == 10 and eng.boo_setup(**dict(good, n_bins=4096, orders=(12, 1, 7, 3))) == 4096 and eng.boo_setup(**good) == 10
    for call in (eng.boo_per_atom, eng.boo_qlm):                        # set up, not sampled yet
        with pytest.raises(api.AztotError) as e:
            call()
        assert e.value.code == -4
    assert eng.boo_shape() == ((4, 6), 10, 2, 0) and not eng.boo_counts()[1].any() and not eng.boo_values()[1].any()
    eng.boo_sample()
    # sizes by a null buffer; a cap too small for a buffer is refused and writes nothing
    assert L.aztot_boo_per_atom(eng.h, None, None, 0) == 500 and L.aztot_boo_qlm(eng.h, None, 0) == 500 * 2 * 26
    assert L.aztot_boo_counts(eng.h, None, None, None, None, 0) == 2 * 2 * 2 * 10 and L.aztot_boo_values(eng.h, None, None, None, 0) == 80
    small, smalli, smallu = np.full(4, 77.0), np.full(4, 77, dtype=np.int32), np.full(4, 77, dtype=np.uint64)
    assert L.aztot_boo_per_atom(eng.h, smalli.ctypes.data_as(api._ip), None, 4) == -4 and (smalli == 77).all()
    assert L.aztot_boo_qlm(eng.h, small.ctypes.data_as(api._dp), 4) == -4
    assert L.aztot_boo_values(eng.h, None, small.ctypes.data_as(api._dp), None, 4) == -4 and (small == 77.0).all()
    assert L.aztot_boo_counts(eng.h, None, smallu.ctypes.data_as(api.C.POINTER(api.C.c_uint64)), None, None, 4) == -4 and (smallu == 77).all()
