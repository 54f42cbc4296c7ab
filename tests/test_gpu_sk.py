"""GPU tests of the static structure factors (aztot_sk_*, sk.hip.h) against tests/sk_model.py, the numpy restatement of the contract in include/aztot.h.

Amplitudes are held to |rho_gpu - rho| <= TAU n_s per component (TAU = pair_cases.TAU) against phases evaluated directly at higher precision, and the sums
after one sample to |acc - Re rho_a rho_b*| <= 4 TAU n_a n_b, which follows from the first bound since |rho_s| <= n_s.  The reference is mpmath at 50
digits where it is affordable (up to some ten thousand atom x vector pairs, the long thin box with harmonic 48 among them); the 3000- and 16 385-atom
cases and the 35 143 vectors of the flat box (106 table entries per atom) use the numpy.longdouble route (eps 1.08e-19), which tests/test_sk_model.py
holds to the 50-digit one far below the bound.  The vector set, the accumulation rule and the values are compared exactly.

Which path a case takes.  The LDS tile of k_sk_amplitudes holds 64 atoms up to 48 harmonic entries per atom (l, |m|, |n| tables together), 32 up to 96, 16
beyond: the isotropic boxes here run 64, the long thin box with harmonic 48 runs 32, the flat box with harmonic 48 on two axes runs 16, and
test_tile_and_batches_do_not_change_the_bits forces every choice and a batched walk on one state.  16 385 atoms are 256 tiles plus one atom: row 0 takes a
second tile.  Every case prints its worst ratios before it asserts."""
import os

import numpy as np
import pytest

from aztotmd_amd import api, inputs

import sk_model as sm
from test_gpu_cn import GEOMETRIES, positions, random_case, run_cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(eng, box, nspec, kmax, dk, M=0, engine="mp", setup=True):
    """set-up, the vector set, one sample: amplitudes and sums against the reference.  (vector set, rho)"""
    vs = sm.vector_set(box, kmax, dk, M)
    if setup:
        assert eng.sk_setup(kmax, dk, M) == len(vs["lmn"])
    lmn, b = eng.sk_vectors()
    assert lmn.dtype == np.int32 and np.array_equal(lmn, vs["lmn"]) and np.array_equal(b, vs["bin"])
    npair = nspec * (nspec + 1) // 2
    assert eng.sk_shape() == (len(lmn), vs["n_bins"], npair, 0)
    eng.sk_sample()
    pos, types = positions(eng)
    numbers = sm.numbers_of(types, nspec)
    ref = sm.amplitudes(pos, types, box, lmn, nspec, engine)
    rho = eng.sk_amplitudes()
    assert rho.shape == (len(lmn), nspec, 2)
    r = sm.worst_ratio(rho, ref, numbers)
    samples, acc = eng.sk_sums()
    worst = 0.0
    for a, c in sm.pairs(nspec):
        t = ref[:, a, 0] * ref[:, c, 0] + ref[:, a, 1] * ref[:, c, 1]
        err = np.abs(acc[:, sm.pair_index(a, c, nspec)].astype(LD) - t)
        nn = float(numbers[a]) * float(numbers[c])
        if nn == 0.0:
            assert not err.any()
        else:
            worst = max(worst, float(err.max()) / nn)
    print("N", len(types), "species", list(numbers), "vectors", len(lmn), "harmonics", list(np.abs(lmn).max(0)), "engine", engine,
          "worst |rho - ref| / n_s = %.3g, |acc - ref| / (n_a n_b) = %.3g, TAU = %g" % (r, worst, sm.TAU))
    assert r <= sm.TAU
    assert worst <= 4 * sm.TAU
    assert samples == 1 and eng.sk_shape()[3] == 1
    assert np.array_equal(bits(acc), bits(sm.accumulate(np.zeros_like(acc), rho)))
    return vs, rho


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_atom_counts(n):
    """two species declared; with one atom the second has none: its amplitudes and every sum it takes part in are exactly 0"""
    box = (10.0, 11.0, 12.0)
    eng = api.Engine(api.Model.from_case(random_case(2, n, box, seed=n)))
    vs, rho = check(eng, box, 2, 2.0, 0.25)
    assert len(vs["lmn"]) % 256 != 0 and len(vs["lmn"]) > 64
    if n == 1:
        assert np.abs(np.hypot(rho[:, 0, 0], rho[:, 0, 1]) - 1.0).max() <= 2 * sm.TAU and not rho[:, 1].any()
    check(eng, box, 2, 2.0, 0.25, M=8)                                   # a thinned set, a second set-up


def test_second_tile_of_a_row():
    """16 385 atoms: 256 tiles fill the 256 rows, the last atom is the second tile of row 0.  longdouble reference; a thinned set (M = 8)"""
    box = (60.0, 61.0, 62.0)
    eng = api.Engine(api.Model.from_case(random_case(2, 16385, box, seed=16385)))
    vs, _ = check(eng, box, 2, 1.0, 0.125, M=8, engine="ld")
    assert vs["n_in_bin"].max() == 8 and (vs["unthinned"] > 8).any()


@pytest.mark.parametrize("g", range(6))
def test_geometries(g):
    """3000 atoms in the boxes of test_gpu_cn.py (different harmonic counts per axis; atoms on faces and edges; two or three species).  longdouble reference"""
    nspec, box, _, faces = GEOMETRIES[g]
    eng = api.Engine(api.Model.from_case(random_case(nspec, 3000, box, seed=900 + g, faces=faces)))
    vs, _ = check(eng, box, nspec, 1.2, 0.1, engine="ld")
    assert len(vs["lmn"]) % 256 != 0


def test_three_species_one_empty(tmp_path):
    box = (12.0, 13.0, 14.0)
    d = inputs.write_input_files(random_case(3, 200, box, seed=9, used=2), str(tmp_path / "m"))       # S2 is declared and has no atom
    eng = api.Engine(api.Model.from_dir(d))
    _, rho = check(eng, box, 3, 1.5, 0.25, M=8)
    assert not rho[:, 2].any()
    k, cnt, tot, part = eng.sk_values()
    assert not part[:, [sm.pair_index(a, 2, 3) for a in range(3)]].any() and (tot[cnt > 0] > 0).all()


def test_one_species_one_vector():
    """a set of exactly one vector, (0, 0, 1): one thread of one workgroup has something to do"""
    box = (10.0, 11.0, 12.0)
    eng = api.Engine(api.Model.from_case(random_case(1, 130, box, seed=4)))
    vs, _ = check(eng, box, 1, 0.56, 0.27)
    assert vs["lmn"].tolist() == [[0, 0, 1]] and vs["bin"].tolist() == [1]
    k, cnt, tot, part = eng.sk_values()
    assert cnt.tolist() == [0, 1] and tot[0] == 0.0 and part[0, 0] == 0.0 and tot[1] == part[1, 0]


def test_harmonic_48_in_a_long_thin_box():
    """(3, 3.5, 90): harmonics 1, 1 and 48, 53 table entries per atom: the LDS tile holds 32 atoms.  The whole set, 50 digits"""
    box = (3.0, 3.5, 90.0)
    g = sm.TWO_PI / box[2]
    eng = api.Engine(api.Model.from_case(random_case(2, 100, box, seed=48)))
    vs, _ = check(eng, box, 2, 48.5 * g, 48.5 * g / 6, engine="mp")
    assert np.abs(vs["lmn"]).max(0).tolist() == [1, 1, 48] and (vs["lmn"][:, 1:] < 0).any(0).all()
    with pytest.raises(api.AztotError) as e:
        eng.sk_setup(49.0 * g * (1 + 1e-12), 0.5, 0)
    print(e.value)
    assert e.value.code == -4 and "axis z" in str(e.value) and "%.4f" % (49.0 * g) in str(e.value)
    assert eng.sk_shape()[0] == len(vs["lmn"]) and eng.sk_amplitudes().shape[0] == len(vs["lmn"])      # the refused set-up left the earlier one


def test_harmonic_48_on_two_axes():
    """(60, 60, 9): harmonics 48, 48 and 7, more than 96 table entries per atom: the LDS tile holds 16 atoms.  Three species; longdouble reference"""
    box = (60.0, 60.0, 9.0)
    g = sm.TWO_PI / 60.0
    eng = api.Engine(api.Model.from_case(random_case(3, 60, box, seed=96)))
    vs, _ = check(eng, box, 3, 48.5 * g, 4.82 * g, engine="ld")            # (10 bins that reach past 48 g)
    h = np.abs(vs["lmn"]).max(0)
    assert h[0] == 48 and h[1] == 48 and int(h.sum()) + 3 > 96 and len(vs["lmn"]) > 8192


def md_case():
    return inputs.lj_case((6, 6, 6), a=5.26, seed=3, charges=(0.0, 0.0), vel_T=85.0)          # two neutral species A, B


def test_accumulation_bit_for_bit():
    """three samples with steps in between: the sums grow by fl(fl(re_a re_b) + fl(im_a im_b)) of that sample's amplitudes, the values are the model's from
    the sums, a reset zeroes everything"""
    case = md_case()
    eng = api.Engine(api.Model.from_case(case))
    nk = eng.sk_setup(3.0, 0.125, 16)
    lmn, b = eng.sk_vectors()
    numbers = sm.numbers_of(case["types"], 2)
    acc = np.zeros((nk, 3))
    for c in range(3):
        if c:
            eng.step(6)
        eng.sk_sample()
        rho = eng.sk_amplitudes()
        acc = sm.accumulate(acc, rho)
        samples, got = eng.sk_sums()
        assert samples == c + 1 and np.array_equal(bits(got), bits(acc)), c
        k, cnt, tot, part = eng.sk_values()
        mk, mc, mt, mp_ = sm.values(got, samples, b, eng.sk_shape()[1], numbers, 0.125)
        assert np.array_equal(k, mk) and np.array_equal(cnt, mc) and np.array_equal(bits(tot), bits(mt)) and np.array_equal(bits(part), bits(mp_)), c
    assert (tot[cnt > 0] > 0).all() and cnt.max() == 16
    eng.sk_reset()
    samples, got = eng.sk_sums()
    assert samples == 0 and not got.any() and not eng.sk_values()[2].any() and not eng.sk_values()[3].any()
    eng.sk_sample()
    assert np.array_equal(bits(eng.sk_sums()[1]), bits(sm.accumulate(np.zeros_like(acc), eng.sk_amplitudes())))


def test_slot_order_independence():
    """a second handle made from the first one's state with other cells keeps its atoms in another order and returns the same bits"""
    case = md_case()
    a = api.Engine(api.Model.from_case(case))
    a.step(5)
    st = a.state()
    b = api.Engine(api.Model.from_case(dict(case, **{k: st[k] for k in ("x", "y", "z", "vx", "vy", "vz")})), cell_size=7.3)
    assert not np.array_equal(a.cell_table()[-1], b.cell_table()[-1]), "the two engines keep their atoms in the same order: the test shows nothing"
    for k in ("x", "y", "z"):
        assert np.array_equal(a.state((k,))[k], b.state((k,))[k])
    for e in (a, b):
        e.sk_setup(3.0, 0.125, 0)
        e.sk_sample()
    assert np.array_equal(bits(a.sk_amplitudes()), bits(b.sk_amplitudes())) and np.array_equal(bits(a.sk_sums()[1]), bits(b.sk_sums()[1]))


def test_tile_and_batches_do_not_change_the_bits(monkeypatch):
    """the measurement switches AZTOT_SK_TILE (atoms per LDS tile) and AZTOT_SK_BATCH (vectors per launch) on one state of 3000 atoms: the amplitudes are
    the bits of the default walk (64 atoms per tile, one batch)"""
    box = (30.0, 31.0, 32.0)
    eng = api.Engine(api.Model.from_case(random_case(2, 3000, box, seed=77)))
    nk = eng.sk_setup(2.6, 0.125, 0)
    assert nk > 3 * 1024
    eng.sk_sample()
    base = eng.sk_amplitudes()
    for tile, batch in ((32, None), (16, None), (None, 1024), (None, 1500), (16, 700)):
        if tile:
            monkeypatch.setenv("AZTOT_SK_TILE", str(tile))
        if batch:
            monkeypatch.setenv("AZTOT_SK_BATCH", str(batch))
        eng.sk_sample()
        monkeypatch.delenv("AZTOT_SK_TILE", raising=False)
        monkeypatch.delenv("AZTOT_SK_BATCH", raising=False)
        assert np.array_equal(bits(eng.sk_amplitudes()), bits(base)), (tile, batch)
    assert eng.sk_shape()[3] == 6


@pytest.mark.parametrize("kw", [{}, {"sort_every": 1}])
def test_sampling_does_not_perturb(kw):
    """a run that samples is bit-identical to one that calls get_stats at the same points"""
    case = inputs.config("F2")
    case = dict(case, vx=np.sin(np.arange(len(case["x"]))) * 3.0, vy=np.cos(np.arange(len(case["x"]))) * 3.0)
    a = api.Engine(api.Model.from_case(case), **kw)
    b = api.Engine(api.Model.from_case(case), **kw)
    b.sk_setup(2.0, 0.1, 32)
    a.stats()
    b.sk_sample()                           # right after init, no step
    for _ in range(5):
        a.step(7)
        a.stats()
        b.step(7)
        b.sk_sample()
    assert b.sk_shape()[3] == 6
    sa, sb = a.state(), b.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(sa[k], sb[k]), k
    ta, tb = a.stats(), b.stats()
    for k in ta:
        assert ta[k] == tb[k], k


def test_simple_cubic_lattice():
    """8^3 Ar atoms on a simple-cubic lattice: S = N at the Bragg vectors (l, m, n all multiples of 8), nothing elsewhere"""
    n, a0 = 8, 3.5
    N = n ** 3
    box = (n * a0,) * 3
    g = np.arange(n) * a0 + 0.25
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    case = random_case(1, N, box, seed=1)
    case.update(x=pos[:, 0].copy(), y=pos[:, 1].copy(), z=pos[:, 2].copy(), names=["Ar"])
    eng = api.Engine(api.Model.from_case(case))
    eng.sk_setup(4.0, 0.125, 0)
    eng.sk_sample()
    lmn, b = eng.sk_vectors()
    acc = eng.sk_sums()[1][:, 0]
    bragg = (lmn % n == 0).all(1)
    print("Bragg vectors", int(bragg.sum()), "of", len(lmn), "worst |acc - N^2| / N^2 = %.3g, elsewhere |acc| / N^2 = %.3g" %
          (np.abs(acc[bragg] / N ** 2 - 1).max(), np.abs(acc[~bragg]).max() / N ** 2))
    assert bragg.sum() >= 7
    assert np.abs(acc[bragg] - float(N) ** 2).max() <= 4 * sm.TAU * N * N and np.abs(acc[~bragg]).max() <= 4 * sm.TAU * N * N
    # per vector S = acc / N: bins of one vector each would show N; here the Bragg bins hold other vectors too, so compare the bin means with the model
    k, cnt, tot, part = eng.sk_values()
    mk, mc, mt, mp_ = sm.values(eng.sk_sums()[1], 1, b, eng.sk_shape()[1], [N], 0.125)
    assert np.array_equal(bits(tot), bits(mt)) and np.array_equal(bits(tot), bits(part[:, 0]))
    first = int(b[np.flatnonzero(bragg)[0]])
    assert abs(tot[first] * cnt[first] - N * int((bragg & (b == first)).sum())) <= 1e-9 * N


def test_refusals():
    case = md_case()
    eng = api.Engine(api.Model.from_case(case))
    L = api.lib()
    for call in (eng.sk_sample, eng.sk_reset, eng.sk_shape, eng.sk_vectors, eng.sk_amplitudes, eng.sk_sums, eng.sk_values):
        with pytest.raises(api.AztotError) as e:
            call()
        assert e.value.code == -4, call
    g = sm.TWO_PI / case["box"][0]
    for kmax, dk, M in ((0.0, 0.1, 0), (-1.0, 0.1, 0), (float("nan"), 0.1, 0), (3.0, 0.0, 0), (3.0, -0.1, 0), (3.0, 3.5, 0), (3.0, 3.0 / 4097.5, 0),
                        (3.0, 0.1, -1), (0.5 * g, 0.1 * g, 0), (49.5 * g, 0.5, 8)):
        with pytest.raises(api.AztotError) as e:
            eng.sk_setup(kmax, dk, M)
        assert e.value.code == -4, (kmax, dk, M)
    with pytest.raises(api.AztotError) as e:
        eng.sk_setup(49.5 * g, 0.5, 8)
    assert "axis x" in str(e.value)                                       # a cube: the first axis that needs harmonic 49
    assert eng.sk_setup(3.0, 3.0 / 4096.5, 1) > 0 and eng.sk_shape()[1] == 4096
    nk = eng.sk_setup(2.0, 0.25, 4)
    assert eng.sk_shape() == (nk, 8, 3, 0) and not eng.sk_sums()[1].any() and not eng.sk_values()[3].any()
    with pytest.raises(api.AztotError) as e:
        eng.sk_amplitudes()                                               # set up, not sampled yet
    assert e.value.code == -4
    with pytest.raises(api.AztotError):
        eng.sk_setup(2.0, -0.25, 4)                                       # a refused set-up leaves the earlier one
    assert eng.sk_shape() == (nk, 8, 3, 0)
    eng.sk_sample()
    # sizes by null buffers; a cap too small for a buffer is refused and writes nothing
    assert L.aztot_sk_vectors(eng.h, None, None, 0) == nk and L.aztot_sk_amplitudes(eng.h, None, 0) == nk * 4
    assert L.aztot_sk_sums(eng.h, None, None, 0) == nk * 3 and L.aztot_sk_values(eng.h, None, None, None, None, 0) == 24
    small = np.full(4, 77.0)
    smalli = np.full(4, 77, dtype=np.int32)
    assert L.aztot_sk_amplitudes(eng.h, small.ctypes.data_as(api._dp), 4) == -4 and L.aztot_sk_sums(eng.h, None, small.ctypes.data_as(api._dp), 4) == -4
    assert L.aztot_sk_values(eng.h, None, None, small.ctypes.data_as(api._dp), None, 4) == -4 and (small == 77.0).all()
    assert L.aztot_sk_vectors(eng.h, None, smalli.ctypes.data_as(api._ip), 3) == -4 and (smalli == 77).all()


def test_slab_handle_refused():
    case = inputs.lj_case((42, 5, 5), a=5.735, seed=31, rc=8.5, vel_T=8.0)
    eng = api.Engine(api.Model.from_case(case), slab={"rank": 1, "nranks": 2, "loopback": True})
    with pytest.raises(api.AztotError) as e:
        eng.sk_setup(2.0, 0.1, 0)
    assert e.value.code == -2 and "slab" in str(e.value)
    with pytest.raises(api.AztotError) as e:
        eng.sk_sample()
    assert e.value.code == -4
    eng.step(3)                                 # the handle steps on


def replay(d, nstep, stat, every_rdf, strfac, nequil=0):
    """the CLI's call boundaries (main.cpp): aztot_step up to the next stat row, RDF sample or structure-factor sample"""
    kmax, dk, every, cap = strfac
    eng = api.Engine(api.Model.from_dir(d), initial_forces=0)
    eng.sk_setup(kmax, dk, cap)
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
            eng.sk_sample()
            taken += 1
        if done % stat == 0 or done == nstep:
            eng.stats()
    if not taken:
        eng.sk_sample()
    return eng


@pytest.mark.parametrize("every,samples", [(60, 3), (0, 1)])
def test_cli_file(tmp_path, every, samples):
    """200 steps: samples after steps 60, 120 and 180; every = 0: one sample of the final configuration.  sk.dat parses back to aztot_sk_values of an API
    run with the same call boundaries, at the printed precision; without the line no file is written"""
    case = md_case()
    case["nsteps"] = 200
    strfac = (2.5, 0.125, every, 16)
    d = inputs.write_input_files(dict(case, strfac=strfac), str(tmp_path / "n"), stat=70)
    run_cli(d)
    rdf_every = int(api.Model.from_dir(d).query("rdf")[3]) or 1000000
    eng = replay(d, 200, 70, rdf_every, strfac)
    assert eng.sk_shape()[3] == samples
    k, cnt, tot, part = eng.sk_values()
    lines = open(os.path.join(d, "sk.dat")).read().splitlines()
    assert lines[0] == "k\tn\tS\tA-A\tA-B\tB-B"
    rows = [b for b in range(len(k)) if cnt[b] > 0]
    assert len(lines) == 1 + len(rows) and len(rows) < len(k)             # the first bins hold no vector and have no row
    for line, b in zip(lines[1:], rows):
        assert line == "%f\t%d\t%f" % (k[b], cnt[b], tot[b]) + "".join("\t%f" % v for v in part[b]), b
    if every == 60:
        plain = inputs.write_input_files(case, str(tmp_path / "p"), stat=70)
        run_cli(plain)
        assert not os.path.exists(os.path.join(plain, "sk.dat"))
        for f in ("stat.dat", "revcon.xyz", "velocities.dat", "msd.dat"):
            assert open(os.path.join(d, f)).read() == open(os.path.join(plain, f)).read(), f


def test_cli_unusable_directive_warns(tmp_path):
    """a kmax past 48 harmonics: a WARNING, the run goes on, no sk.dat"""
    case = md_case()
    case["nsteps"] = 2
    d = inputs.write_input_files(dict(case, strfac=(12.0, 0.1, 1, 8)), str(tmp_path / "n"), stat=5)
    r = run_cli(d)
    assert "WARNING: strfac directive not usable" in r.stderr and "axis x" in r.stderr
    assert not os.path.exists(os.path.join(d, "sk.dat")) and os.path.exists(os.path.join(d, "revcon.xyz"))
