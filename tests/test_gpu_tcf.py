"""GPU tests of the time correlation functions (aztot_tcf_*, tcf.hip.h): mean-square displacement and velocity autocorrelation per species over a ring
of time origins.  The contract in include/aztot.h fixes every rounding and the order of every sum, so the raw sums are compared BIT FOR BIT with the
numpy restatement in tests/tcf_model.py, fed with the states the engine hands out."""
import os
import subprocess

import numpy as np
import pytest

from aztotmd_amd import api, inputs

import tcf_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = ("x", "y", "z", "vx", "vy", "vz")
BIG = 1000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def three_species_case():
    """500 atoms of three species, the middle one without atoms"""
    case = inputs.lj_case((5, 5, 5), seed=11, charges=(0.0, 0.0), vel_T=85.0)
    N = len(case["x"])
    p = case["vdw"][0][4]
    case["species"] = [case["species"][0]] * 3
    case["names"] = ["A", "E", "B"]
    case["vdw"] = [(a, b, 1, 8.5, p) for a in range(3) for b in range(a, 3)]
    case["types"] = np.where(np.arange(N) % 3 == 0, 2, 0).astype(np.int32)
    return case


CASES = {
    "108": lambda: inputs.lj_case((3, 3, 3), seed=5, vel_T=85.0),                              # N < 256: one chunk, no fold over chunks
    "500_3spec": three_species_case,                                                           # two chunks, an empty species
    "40000": lambda: inputs.lj_case((25, 20, 20), seed=7, charges=(0.0, 0.0), vel_T=85.0),     # 157 chunks, padded to 256
}


def model_of(eng, M, E):
    st = eng.state(SIX)
    ns = int(eng.model.query("n_species")[0])
    return tcf_model.Sampler(M, E, st["types"], ns, list(eng.model.query("box")))


def assert_same(eng, mod, where):
    nl, ns, samples = eng.tcf_shape()
    assert (nl, ns, samples) == (mod.n_lags, mod.ns, mod.samples), where
    cnt, msd, vaf = eng.tcf_sums()
    assert np.array_equal(cnt, mod.count), where
    assert np.array_equal(bits(msd), bits(mod.msd)), (where, np.abs(msd - mod.msd).max())
    assert np.array_equal(bits(vaf), bits(mod.vaf)), (where, np.abs(vaf - mod.vaf).max())
    m, v = eng.tcf_values()
    wm, wv = mod.values()
    assert np.array_equal(bits(m), bits(wm)) and np.array_equal(bits(v), bits(wv)), where


@pytest.mark.parametrize("name,M,E,nsamp", [
    ("108", 1, BIG, 8), ("108", 1, 1, 6), ("108", 3, 2, 16), ("108", 4, 1, 12),
    ("500_3spec", 1, BIG, 6), ("500_3spec", 3, 2, 16), ("500_3spec", 4, 1, 12),
    ("40000", 3, 2, 14), ("40000", 1, BIG, 4),
])
def test_exact_against_model(name, M, E, nsamp):
    """after every sample the raw sums and the values equal the model's, bit for bit; the ring wraps twice where it can; a reset in mid-run"""
    eng = api.Engine(api.Model.from_case(CASES[name]()))
    assert eng.tcf_setup(M, E) == M * E
    mod = model_of(eng, M, E)
    if name == "500_3spec":
        assert list(mod.number) == [333, 0, 167]
    for c in range(nsamp):
        if c:
            eng.step(3)
        if c == nsamp - 4:
            eng.tcf_reset()
            mod.reset()
            assert eng.tcf_shape()[2] == 0 and not eng.tcf_sums()[0].any() and not eng.tcf_sums()[1].any()
        st = eng.state(SIX)
        eng.tcf_sample()
        mod.sample(st)
        assert_same(eng, mod, (name, M, E, c))
        assert (st["vx"] < 0).any() and (st["vx"] > 0).any()           # a thermalised box: velocities of both signs
    assert mod.count.sum() > 0 and (mod.vaf[0] > 0).any()
    if M * E > 1:
        assert (mod.msd[1:] > 0).any()


@pytest.mark.parametrize("kw", [{"cell_size": 4.3}, {"pair_variant": 1, "sort_every": 1}])
def test_slot_order_independence(kw):
    """two engines whose cell grids (and so the slot order of the atoms) differ give the same bits for the same state"""
    case = inputs.lj_case((6, 6, 6), seed=21, charges=(0.0, 0.0), vel_T=120.0)
    a = api.Engine(api.Model.from_case(case))
    b = api.Engine(api.Model.from_case(case), **kw)
    a.tcf_setup(3, 2)
    b.tcf_setup(3, 2)
    differ = False
    for c in range(9):
        if c:
            a.step(5)
        st = a.state(SIX)
        b.set_state(**{k: st[k] for k in SIX})
        a.tcf_sample()
        b.tcf_sample()
        ia, ib = a.cell_table()[-1], b.cell_table()[-1]
        differ = differ or not np.array_equal(ia, ib)
        ca, ma, va = a.tcf_sums()
        cb, mb, vb = b.tcf_sums()
        assert np.array_equal(ca, cb) and np.array_equal(bits(ma), bits(mb)) and np.array_equal(bits(va), bits(vb)), c
    assert differ, "the two engines kept their atoms in the same order: the test shows nothing"


@pytest.mark.parametrize("kw", [{}, {"sort_every": 1}, {"use_graph": 0, "pair_variant": 1}])
def test_sampling_does_not_perturb(kw):
    """a run that samples is bit-identical to one that calls get_stats at the same points"""
    case = inputs.config("F2")
    case = dict(case, vx=np.sin(np.arange(len(case["x"]))) * 3.0, vy=np.cos(np.arange(len(case["x"]))) * 3.0)
    a = api.Engine(api.Model.from_case(case), **kw)
    b = api.Engine(api.Model.from_case(case), **kw)
    b.tcf_setup(2, 2)
    a.stats()
    b.tcf_sample()                       # right after init, no step
    for _ in range(5):
        a.step(7)
        a.stats()
        b.step(7)
        b.tcf_sample()
    sa, sb = a.state(), b.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(sa[k], sb[k]), k
    ta, tb = a.stats(), b.stats()
    for k in ta:
        assert ta[k] == tb[k], k
    assert b.tcf_shape()[2] == 6


def test_uniform_drift_on_a_perfect_lattice():
    """perfect Ar lattice, every atom with the same velocity, no thermostat: the forces vanish by symmetry, so MSD(l) = |v|^2 (l n dt)^2 and
    VAF(l) = |v|^2 for every species, to the project's trajectory tolerance of 1e-9 relative.  Atoms cross the box walls on the way (those that start
    on the faces at once); the drift over the largest lag stays far below L / 2."""
    v = np.array([3.0, -2.0, 1.5])
    nstep, dt, M, E = 20, 0.001, 3, 2
    case = inputs.lj_case((5, 5, 5), jitter=0.0, charges=(0.0, 0.0), dt=dt)
    N = len(case["x"])
    case = dict(case, vx=np.full(N, v[0]), vy=np.full(N, v[1]), vz=np.full(N, v[2]))
    eng = api.Engine(api.Model.from_case(case))
    eng.tcf_setup(M, E)
    y0 = eng.state(("y",))["y"]
    for c in range(16):
        if c:
            eng.step(nstep)
        eng.tcf_sample()
    assert np.abs(v).max() * M * E * nstep * dt < 0.5 * min(case["box"]) / 10
    moved = eng.state(("y",))["y"] - y0
    assert (np.abs(moved) > 0.5 * case["box"][1]).any(), "no atom crossed a wall"
    cnt, _, _ = eng.tcf_sums()
    assert (cnt > 0).all()
    msd, vaf = eng.tcf_values()
    v2 = float(v @ v)
    for l in range(M * E):
        want = v2 * (l * nstep * dt) ** 2
        for s in range(2):
            print("lag %d species %d: msd %.17g (want %.17g), vaf %.17g (want %.17g)" % (l, s, msd[l, s], want, vaf[l, s], v2))
            assert abs(vaf[l, s] - v2) <= 1e-9 * v2
            assert abs(msd[l, s] - want) <= 1e-9 * want


def run_cli(d):
    exe = os.path.join(ROOT, "aztotmd_amd", "aztotmd")
    r = subprocess.run([exe, d, "--out", d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def replay_cli(d):
    """the program's schedule (main.cpp) through the Python Engine: the rows of displ.dat and vaf.dat as strings"""
    m = api.Model.from_dir(d)
    q = lambda k: int(m.query(k)[0])
    nstep, stat, neq, vaf = q("nstep"), max(1, q("stat")), q("nequil"), q("vaf")
    rdf = m.query("rdf")
    every = int(rdf[3])
    ns = q("n_species")
    eng = api.Engine(m, initial_forces=0)
    eng.rdf_setup(rdf[1], rdf[2], nuclei=bool(rdf[5]))
    stat_row = lambda c: c % stat == 0 or c == nstep
    vaf_row = lambda c: vaf > 0 and c > neq and c % vaf == 0
    due = lambda c: c == 0 or (neq > 0 and c == neq) or stat_row(c) or vaf_row(c)
    eng.tcf_setup(1, sum(1 for c in range(nstep + 1) if due(c)))
    eng.tcf_sample()
    displ, vrows = [], []
    done = 0
    while done < nstep:
        n = min(stat - done % stat, nstep - done)
        n = min(n, (1 if done < 1 else done + 1 + (every - done % every) % every) - done)
        if done < neq:
            n = min(n, neq - done)
        if vaf > 0:
            n = min(n, (max(done, neq) // vaf + 1) * vaf - done)
        eng.step(n)
        done += n
        if (done - 1) % every == 0:
            eng.rdf_sample()
        if not (stat_row(done) or due(done)):
            continue
        st = eng.stats()
        if neq > 0 and done == neq:
            eng.tcf_reset()
        eng.tcf_sample()
        lag = eng.tcf_shape()[2] - 1
        msd, vf = eng.tcf_values(lag, 1)
        head = "%f\t%d" % (st["time"], st["step"])
        if stat_row(done):
            displ.append(head + "".join("\t%f" % v for v in msd[0]))
        if vaf_row(done):
            vrows.append(head + "".join("\t%f" % v for v in vf[0]))
    assert ns == msd.shape[1]
    return displ, vrows


def test_cli_files(tmp_path):
    case = inputs.lj_case((4, 4, 4), a=5.4, seed=3, charges=(0.0, 0.0), vel_T=85.0, nEq=10, freqEq=5, nsteps=60)
    with_vaf = inputs.write_input_files(dict(case, vaf=5), str(tmp_path / "v"), stat=20)
    without = inputs.write_input_files(case, str(tmp_path / "n"), stat=20)
    run_cli(with_vaf)
    run_cli(without)
    assert not os.path.exists(os.path.join(without, "vaf.dat")) and not os.path.exists(os.path.join(without, "displ.dat"))
    displ = open(os.path.join(with_vaf, "displ.dat")).read().splitlines()
    vaf = open(os.path.join(with_vaf, "vaf.dat")).read().splitlines()
    assert displ[0] == "Time\tStep\tA-msd\tB-msd" and vaf[0] == "time,ps\tiStep\tA\tB"
    assert [int(r.split("\t")[1]) for r in displ[1:]] == [20, 40, 60]
    assert [int(r.split("\t")[1]) for r in vaf[1:]] == list(range(15, 61, 5))
    assert all(len(r.split("\t")) == 4 for r in displ + vaf)
    want_displ, want_vaf = replay_cli(with_vaf)
    assert displ[1:] == want_displ and vaf[1:] == want_vaf
    assert float(displ[-1].split("\t")[2]) > 0.0 and float(vaf[1].split("\t")[2]) > 0.0
    # the other files do not know about the directive
    for f in ("msd.dat", "stat.dat", "revcon.xyz"):
        assert open(os.path.join(with_vaf, f), "rb").read() == open(os.path.join(without, f), "rb").read(), f
    assert len(open(os.path.join(with_vaf, "msd.dat")).read().splitlines()) == 1 + 3


def test_cli_origin_is_reset_at_the_end_of_equilibration(tmp_path):
    """a stat row at c == nequil shows 0 (the origin has just been replaced), rows before it are measured from the initial state"""
    case = inputs.lj_case((4, 4, 4), a=5.4, seed=3, charges=(0.0, 0.0), vel_T=85.0, nEq=20, freqEq=5, nsteps=30)
    d = inputs.write_input_files(dict(case, vaf=10), str(tmp_path / "e"), stat=10)
    run_cli(d)
    displ = open(os.path.join(d, "displ.dat")).read().splitlines()
    vaf = open(os.path.join(d, "vaf.dat")).read().splitlines()
    assert [int(r.split("\t")[1]) for r in displ[1:]] == [10, 20, 30] and [int(r.split("\t")[1]) for r in vaf[1:]] == [30]
    assert float(displ[1].split("\t")[2]) > 0.0 and displ[2].split("\t")[2:] == ["0.000000", "0.000000"]
    want_displ, want_vaf = replay_cli(d)
    assert displ[1:] == want_displ and vaf[1:] == want_vaf


def test_errors():
    eng = api.Engine(api.Model.from_case(inputs.config("F1")))
    for call in (eng.tcf_sample, eng.tcf_reset, eng.tcf_shape, eng.tcf_sums, eng.tcf_values):
        with pytest.raises(api.AztotError) as e:
            call()
        assert e.value.code == -4
    for M, E in ((0, 1), (1, 0), (-1, 2), (1 << 13, 1 << 12)):
        with pytest.raises(api.AztotError) as e:
            eng.tcf_setup(M, E)
        assert e.value.code == -4, (M, E)
    assert eng.tcf_setup(2, 3) == 6
    for lag0, n in ((-1, 1), (0, 7), (6, 1), (3, -1)):
        for call in (eng.tcf_sums, eng.tcf_values):
            with pytest.raises(api.AztotError) as e:
                call(lag0, n)
            assert e.value.code == -4, (lag0, n)
    assert eng.tcf_sums(6, 0)[1].shape == (0, 1) and eng.tcf_values(5, 1)[0].shape == (1, 1)
    # too small a buffer is told the size and left alone
    L = api.lib()
    buf = np.full(4, -7.0)
    dp = buf.ctypes.data_as(api._dp)
    assert L.aztot_tcf_sums(eng.h, 0, 6, None, dp, None, 4) == 6 and L.aztot_tcf_values(eng.h, 0, 6, dp, None, 4) == 6 and (buf == -7.0).all()
    eng.tcf_sample()
    eng.step(2)
    eng.tcf_sample()
    cnt, msd, _ = eng.tcf_sums()
    assert list(cnt) == [1, 1, 0, 0, 0, 0] and msd[1, 0] > 0
    # a set-up after a set-up forgets everything
    assert eng.tcf_setup(1, 4) == 4
    cnt, msd, vaf = eng.tcf_sums()
    assert eng.tcf_shape() == (4, 1, 0) and not cnt.any() and not msd.any() and not vaf.any()
    eng.tcf_sample()
    assert list(eng.tcf_sums()[0]) == [1, 0, 0, 0]


def test_setup_without_room_leaves_a_handle_that_steps():
    """a ring far beyond the device's memory: AZTOT_ERR_DEVICE, no sampler, and the handle steps on as one that never asked"""
    case = inputs.lj_case((8, 8, 8), seed=9, vel_T=50.0)
    a = api.Engine(api.Model.from_case(case))
    b = api.Engine(api.Model.from_case(case))
    a.tcf_setup(2, 2)
    a.tcf_sample()
    with pytest.raises(api.AztotError) as e:
        a.tcf_setup(1 << 24, 1)                     # 16 M origins x 48 B x 2 048 ids: 1.6 TB, several times the card's memory
    assert e.value.code == -3
    with pytest.raises(api.AztotError) as e:
        a.tcf_shape()
    assert e.value.code == -4
    a.step(10)
    b.step(10)
    sa, sb = a.state(), b.state()
    for k in ("x", "vx", "fx"):
        assert np.array_equal(sa[k], sb[k]), k
    assert a.tcf_setup(1, 2) == 2
    a.tcf_sample()
    assert list(a.tcf_sums()[0]) == [1, 0]


def test_slab_handle_refused():
    case = inputs.lj_case((42, 5, 5), a=5.735, seed=31, rc=8.5, vel_T=8.0)
    eng = api.Engine(api.Model.from_case(case), slab={"rank": 1, "nranks": 2, "loopback": True})
    with pytest.raises(api.AztotError) as e:
        eng.tcf_setup(1, 1)
    assert e.value.code == -2 and "slab" in str(e.value)
