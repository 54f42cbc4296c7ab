"""GPU tests of the pressure-tensor sampler (aztot_stress_*, csrc/stress.hip.h) against the contract in include/aztot.h.

Bounds (tests/stress_model.py, tau = pair_cases.TAU = 1e-13 against the condition scales of tests/pair_reference.py):
  |w_i[ab] - ref| <= tau 1/2 sum_j S_F |d_a| |d_b|,  |W[ab] - ref| <= tau sum_pairs S_F |d_a| |d_b|,  |K[ab] - ref| <= tau sum m |v_a| |v_b|,
  the pair energies of the walk within tau sum S_E of the enumeration and within 1e-11 sum |terms| of stats(); integers exact.
Every liquid case asserts that no pair lies within 1e-9 (relative) of rMax^2 or of a per-pair cut-off: the pair set is never in doubt."""
import os
import subprocess

import numpy as np
import pytest

import list_cases
import pair_cases as pc
import stress_model as sm
import tcf_model
import test_gpu_pair_functions as tpf
import util
from aztotmd_amd import api, inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
TOTALS = ("kinetic", "virial", "pressure", "pressure_iso", "eng_vdw", "eng_coul", "pairs", "pairs_dropped", "volume")


def take(e):
    e.stress_sample()
    return e.stress_per_atom(), e.stress()


def same_totals(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in TOTALS)


# ---- 1. isolated pairs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.CASES)
def test_isolated_pairs(name):
    case, pairs, ref = tpf.system(name)
    if "ewald" in name:
        e = api.Engine(api.Model.from_case(case))
        with pytest.raises(api.AztotError) as err:
            e.stress_setup()
        assert err.value.code == -2 and "pme" in str(err.value)
        e.step(2)
        assert e.stats()["step"] == 2
        return
    i, j = pairs["i"], pairs["j"]
    d = np.stack([pairs["dx"], pairs["dy"], pairs["dz"]], 1).astype(LD)
    S = sm.system_from_case(case, state={k: case[k] for k in ("x", "y", "z", "vx", "vy", "vz")} | {"radius": np.zeros(len(case["x"]))})
    n_in = len(sm.fp64_pairs(S)[0])
    assert n_in >= int((pc.r2_fp64(pairs) <= pc.r_max(pc.spec(name)) ** 2).sum())
    for variant in (1, 2):
        e = api.Engine(api.Model.from_case(case), pair_variant=variant)
        radius = e.state()["radius"]
        f, sf, uv, sev = tpf.expected(name, ref, radius, pairs)
        dropped = f * f > 1e10
        e.stress_setup()
        w, tot = take(e)
        N = len(case["x"])
        wr, ws = np.zeros((N, 6), dtype=LD), np.zeros((N, 6), dtype=LD)
        for c, (a, b) in enumerate(sm.COMP):
            t = np.where(dropped, LD(0), LD(0.5) * f.astype(LD) * d[:, a] * d[:, b])
            s = np.where(dropped, LD(0), LD(0.5) * sf.astype(LD) * abs(d[:, a]) * abs(d[:, b]))
            for idx in (i, j):
                wr[idx, c], ws[idx, c] = t, s
        ok, ratio = sm.within(w, wr, ws)
        assert ok, (name, variant, "per atom", ratio)
        assert (w[i[dropped]] == 0.0).all() and (w[j[dropped]] == 0.0).all() and (w[2 * len(i):] == 0.0).all()
        ok, ratio_W = sm.within(tot["virial"], wr.sum(0), ws.sum(0))
        assert ok, (name, variant, "total", ratio_W)
        assert (tot["kinetic"] == 0.0).all()
        assert tot["pairs_dropped"] == int(dropped.sum()) and tot["pairs"] == n_in, (name, tot["pairs"], n_in)
        assert abs(tot["eng_vdw"] - uv.sum()) <= pc.TAU * sev.sum(), (name, tot["eng_vdw"], uv.sum())
        assert abs(tot["eng_coul"] - ref["uc"].sum()) <= pc.TAU * ref["sec"].sum(), (name, tot["eng_coul"], ref["uc"].sum())
        print("%s v%d: per-atom %.3g  W %.3g" % (name, variant, ratio, ratio_W))


# ---- 2. smallest shapes at which the walk or the tree can go wrong ---------------------------------------------------------------------------------
def lattice_case(shape, spacing, n, rc, seed, box=None):
    """the first n sites (in a random order) of a jittered simple-cubic lattice, Maxwell-like random velocities, one LJ species + a frozen one"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sites = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), -1).reshape(-1, 3)
    sites = sites[rng.permutation(len(sites))[:n]]
    box = np.array(box if box is not None else [k * spacing for k in shape], dtype=np.float64)
    pos = (sites + 0.5) * (box / np.array(shape)) + rng.uniform(-0.3, 0.3, size=(n, 3))
    vel = rng.normal(0.0, 1.5, size=(n, 3))
    types = (np.arange(n) % 5 == 4).astype(np.int32) if n > 4 else np.zeros(n, dtype=np.int32)
    return {"box": box.tolist(), "dt": 0.001, "nsteps": 0, "species": [(39.9, 0.0), (20.2, 0.0)], "names": ["A", "F"], "frozen": [0, 1],
            "vdw": [(0, 0, 1, rc, [0.01006, 3.3952]), (0, 1, 1, rc - 0.5, [0.008, 3.1]), (1, 1, 1, rc, [0.012, 3.0])], "types": types,
            "x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": vel[:, 0].copy(), "vy": vel[:, 1].copy(), "vz": vel[:, 2].copy(),
            "elec_type": 0, "rReal": 0.0, "alpha": 0.0, "T": 0.0, "tstat_type": 0, "nEq": 0, "freqEq": 1, "use_clist": 1, "cell_list": rc,
            "center_box": 0, "init_forces": 1, "radii": None, "seed": 12345}


def edge_case():
    """atoms on 0.0 and on the last double below L, partners across the wall"""
    c = lattice_case((5, 5, 5), 3.6, 3, 6.5, 1)
    L = c["box"][0]
    top = np.nextafter(L, 0.0)
    c["x"][:] = [0.0, top, 3.5]
    c["y"][:] = [3.0, 5.5, 0.0]
    c["z"][:] = [3.0, 5.5, top]
    return c


def big_case():
    """70 000 atoms: a dilute cubic lattice (4 A apart, LJ rc 2.5: no lattice pair interacts) with 300 atoms moved next to a neighbour"""
    n, g = 70000, 42
    c = lattice_case((g, g, g), 4.0, n, 2.5, 9)
    rng = np.random.Generator(np.random.PCG64(10))
    c["types"] = np.zeros(n, dtype=np.int32)
    pos = np.stack([c["x"], c["y"], c["z"]], 1)
    box = np.array(c["box"])
    for k in range(0, 600, 2):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        pos[k] = np.mod(pos[k + 1] + u * rng.uniform(2.0, 2.45), box)
    c["x"], c["y"], c["z"] = pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()
    return c


def two_atoms():
    c = lattice_case((5, 5, 5), 3.6, 2, 6.5, 12)
    c["x"][:] = [16.5, 1.25]            # across the wall: 2.75 apart along x
    c["y"][:] = [4.0, 5.5]
    c["z"][:] = [9.0, 7.0]
    return c


SHAPES = {
    "n1": lambda: lattice_case((5, 5, 5), 3.6, 1, 6.5, 11),
    "n2": two_atoms,
    "n63": lambda: lattice_case((5, 5, 5), 3.6, 63, 6.5, 13),
    "n64": lambda: lattice_case((5, 5, 5), 3.6, 64, 6.5, 14),
    "n65": lambda: lattice_case((5, 5, 5), 3.6, 65, 6.5, 15),
    "n769": lambda: lattice_case((10, 10, 8), 3.6, 769, 6.5, 16),
    "cells235": lambda: lattice_case((4, 5, 9), 3.6, 180, 6.5, 17, box=[14.0, 20.0, 33.0]),
    "edges": edge_case,
    "n70000": big_case,
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_small_shapes_against_the_enumeration(shape):
    case = SHAPES[shape]()
    S = sm.system_from_case(case)
    assert sm.near_cutoff(S) == 0
    ref = sm.stress_reference(S, "ld")
    if shape == "n1":
        assert ref["pairs"] == 0
    else:
        assert ref["pairs"] > 0
    if shape == "n70000":
        assert 250 <= ref["pairs"] <= 2000
    first = None
    for variant in ((2,) if shape == "n70000" else (1, 2)):
        e = api.Engine(api.Model.from_case(case), pair_variant=variant)
        e.stress_setup()
        w, tot = take(e)
        sm.check_sample(S, ref, w, tot)
        if shape == "n1":
            assert (tot["virial"] == 0.0).all() and tot["pairs"] == 0 and (w == 0.0).all() and tot["kinetic"][0] > 0.0
        for c in range(6):
            assert tot["virial"][c] == tcf_model.tree_sum(w[:, c]), (shape, c)
        if first is None:
            first = (w, tot)
        else:
            assert np.array_equal(first[0], w) and same_totals(first[1], tot)


# ---- 3. liquids, 4. agreement with the step kernels --------------------------------------------------------------------------------------------------
def fennell_liquid():
    return inputs.lj_case((5, 5, 5), a=5.4, seed=6, rc=6.5, cell_list=6.5, vel_T=120.0, charges=(0.3, -0.3), elec="fenn", r_real=6.5, alpha=0.4)


def surk_liquid():
    c = inputs.lj_case((5, 5, 5), a=3.0, jitter=0.05, seed=8, rc=6.0, cell_list=3.0, T=500.0, tstat="radi", radii=[(2.73, 4.731, 0.2)], vel_T=300.0)
    c["vdw"] = [(0, 0, 7, 6.0, [75.0, 8.0, 1.0, 1.0])]
    return c


def against_stats(e, ref, tot):
    """the walk's energies and kinetic trace against what the step kernels booked for the same state"""
    st = e.stats()
    assert abs(tot["eng_vdw"] - st["engVdW"]) <= 1e-11 * float(ref["eng_vdw_scale"]), (tot["eng_vdw"], st["engVdW"])
    assert abs(tot["eng_coul"] - st["engCoul"]) <= 1e-11 * float(ref["eng_coul_scale"]), (tot["eng_coul"], st["engCoul"])
    return st


@pytest.mark.parametrize("variant", [1, 2])
def test_lj_liquid_after_lazy_steps(variant):
    case = list_cases.liquid("skin_cells")["case"]
    e = api.Engine(api.Model.from_case(case), pair_variant=variant)
    e.stress_setup()
    e.step(20)                          # default schedule: the engine's coordinates are unwrapped by now, the sampler wraps
    w, tot = take(e)
    state = e.state()
    S = sm.system_from_case(case, state)
    assert sm.near_cutoff(S) == 0
    ref = sm.stress_reference(S, "ld")
    sm.check_sample(S, ref, w, tot)
    assert tot["step"] == 20 and tot["time"] == 20 * case["dt"]
    st = against_stats(e, ref, tot)
    # NVE, nothing frozen: tr K = 2 engKin
    trK = tot["kinetic"][0] + tot["kinetic"][1] + tot["kinetic"][2]
    assert abs(trK - 2.0 * st["engKin"]) <= 1e-11 * float(ref["K_scale"][:3].sum()), (trK, st["engKin"])


@pytest.mark.parametrize("variant", [1, 2])
def test_fennell_liquid_against_mpmath(variant):
    case = fennell_liquid()
    e = api.Engine(api.Model.from_case(case), pair_variant=variant)
    e.stress_setup()
    e.step(1)
    w, tot = take(e)
    S = sm.system_from_case(case, e.state())
    assert sm.near_cutoff(S) == 0
    ref = sm.stress_reference(S, "mp")
    sm.check_sample(S, ref, w, tot)
    assert tot["eng_coul"] != 0.0
    st = against_stats(e, ref, tot)
    trK = tot["kinetic"][0] + tot["kinetic"][1] + tot["kinetic"][2]
    assert abs(trK - 2.0 * st["engKin"]) <= 1e-11 * float(ref["K_scale"][:3].sum())


def test_surk_liquid_with_thermostat_radii():
    case = surk_liquid()
    e = api.Engine(api.Model.from_case(case))
    e.stress_setup()
    e.step(10)
    w, tot = take(e)
    state = e.state()
    assert np.ptp(state["radius"]) > 0.0          # the radii differ atom to atom
    S = sm.system_from_case(case, state)
    assert sm.near_cutoff(S) == 0
    ref = sm.stress_reference(S, "ld")
    sm.check_sample(S, ref, w, tot)


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------------------------------
def test_samples_are_a_function_of_the_state_alone():
    case = list_cases.liquid("skin_cells")["case"]
    keys = ("x", "y", "z", "vx", "vy", "vz")
    src = api.Engine(api.Model.from_case(case))
    src.step(7)
    state = {k: v for k, v in src.state().items() if k in keys}
    a = api.Engine(api.Model.from_case(case), pair_variant=1, sort_every=1)
    b = api.Engine(api.Model.from_case(case), pair_variant=2, sort_every=0, cell_size=7.3)
    a.set_state(**state)
    b.step(30)
    b.set_state(**state)                # the rewind: the slot order is whatever 30 steps of another schedule left
    for e in (a, b):
        e.stress_setup()
    wa, ta = take(a)
    wb, tb = take(b)
    assert np.array_equal(wa, wb) and same_totals(ta, tb)
    for c in range(6):
        assert ta["virial"][c] == tcf_model.tree_sum(wa[:, c])
    w2, t2 = take(a)                    # two samples in a row
    assert np.array_equal(wa, w2) and same_totals(ta, t2)
    fresh = sm.fp64_stress(sm.system_from_case(case, state))
    for c in range(6):                  # the kinetic totals are the tree over (m v_a) v_b by id: bit for bit
        assert ta["kinetic"][c] == fresh["K"][c]


# ---- 6. snapshot and non-interference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(sort_every=1), dict(pair_variant=1)])
def test_sampling_does_not_perturb(kw):
    case = inputs.config("F2")
    case = dict(case, vx=np.sin(np.arange(len(case["x"]))) * 3.0, vy=np.cos(np.arange(len(case["x"]))) * 3.0)
    a = api.Engine(api.Model.from_case(case), **kw)
    b = api.Engine(api.Model.from_case(case), **kw)
    b.stress_setup()
    a.stats()
    b.stress_sample()                   # right after init, no step
    for n in (1, 1, 1, 7, 40, 1, 7):
        a.step(n)
        a.stats()
        b.step(n)
        b.stress_sample()
    sa, sb = a.state(), b.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(sa[k], sb[k]), k
    ta, tb = a.stats(), b.stats()
    for k in ta:
        assert ta[k] == tb[k], k


def test_a_second_sample_replaces_the_first():
    case = inputs.config("F1")
    case = dict(case, vx=np.sin(np.arange(len(case["x"]))) * 3.0)
    e = api.Engine(api.Model.from_case(case))
    e.stress_setup()
    w1, t1 = take(e)
    e.step(3)
    w2, t2 = take(e)
    assert t1["step"] == 0 and t2["step"] == 3 and not np.array_equal(w1, w2)
    f = api.Engine(api.Model.from_case(case))
    f.step(3)
    f.stress_setup()
    w3, t3 = take(f)
    assert np.array_equal(w2, w3) and same_totals(t2, t3)


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    eng = api.Engine(api.Model.from_case(inputs.config("F1")))
    L = api.lib()
    for call in (eng.stress_sample, eng.stress, eng.stress_per_atom):
        with pytest.raises(api.AztotError) as e:
            call()
        assert e.value.code == -4 and "aztot_stress_setup" in str(e.value)
    eng.stress_setup()
    for call in (eng.stress, eng.stress_per_atom):          # set up, not sampled yet
        with pytest.raises(api.AztotError) as e:
            call()
        assert e.value.code == -4
    eng.stress_sample()
    assert eng.stress_per_atom().shape == (500, 6)
    out = api._Stress()
    for rc in (L.aztot_stress_setup(None), L.aztot_stress_sample(None), L.aztot_stress_get(None, out), L.aztot_stress_get(eng.h, None),
               L.aztot_stress_per_atom(None, None, 0)):
        assert rc == -4
    assert L.aztot_stress_per_atom(eng.h, None, 0) == 3000
    small = np.full(8, 77.0)
    assert L.aztot_stress_per_atom(eng.h, small.ctypes.data_as(api._dp), 8) == -4 and (small == 77.0).all()
    eng.stress_setup()                                      # a new set-up forgets the sample
    with pytest.raises(api.AztotError):
        eng.stress()


def refused(eng, word):
    with pytest.raises(api.AztotError) as e:
        eng.stress_setup()
    assert e.value.code == -2 and word in str(e.value), str(e.value)
    with pytest.raises(api.AztotError) as e:
        eng.stress_sample()
    assert e.value.code == -4                               # no sampler was left behind
    eng.step(3)
    assert eng.stats()["step"] == 3


def test_slab_handle_refused():
    case = inputs.lj_case((42, 5, 5), a=5.735, seed=31, rc=8.5, vel_T=8.0)
    refused(api.Engine(api.Model.from_case(case), slab={"rank": 1, "nranks": 2, "loopback": True}), "slab")


def test_bonded_model_refused():
    case, mols = pc.build_bonded("bonds")
    refused(api.Engine(api.Model.from_case(case)), "bond")


def test_pme_model_refused():
    case = inputs.lj_case((5, 5, 5), a=5.4, seed=6, rc=6.5, cell_list=6.5, charges=(0.3, -0.3), elec="fenn", r_real=6.5, alpha=0.4)
    case.update(elec_type=2, ewald_k=(4, 4, 4))
    refused(api.Engine(api.Model.from_case(case)), "pme")


# ---- 8. command-line program ----------------------------------------------------------------------------------------------------------------------------
def run_cli(d):
    exe = os.path.join(ROOT, "aztotmd_amd", "aztotmd")
    r = subprocess.run([exe, d, "--out", d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_cli_case_study_1_with_stress(tmp_path):
    plain = util.materialise_case_study(1, str(tmp_path / "plain"), nstep=20)
    d = util.materialise_case_study(1, str(tmp_path / "stress"), nstep=20)
    with open(os.path.join(d, "control.txt"), "ab") as f:
        f.write(b"\r\nstress\t5\r\n")
    before = set(os.listdir(d))
    run_cli(plain)
    run_cli(d)
    made = set(os.listdir(d)) - before
    assert "stress.dat" in made and not os.path.exists(os.path.join(plain, "stress.dat"))
    for fn in made - {"stress.dat"}:
        assert open(os.path.join(d, fn), "rb").read() == open(os.path.join(plain, fn), "rb").read(), fn
    lines = open(os.path.join(d, "stress.dat")).read().splitlines()
    assert lines[0] == "time\tstep\tPxx\tPyy\tPzz\tPxy\tPxz\tPyz\tP" and [l.split("\t")[1] for l in lines[1:]] == ["5", "10", "15", "20"]
    m = api.Model.from_dir(d)
    assert m.query("stress")[0] == 5
    eng = api.Engine(m, initial_forces=0)
    eng.stress_setup()
    for row in lines[1:]:
        eng.step(5)
        eng.stress_sample()
        s = eng.stress()
        want = "%f\t%d" % (s["time"], s["step"]) + "".join("\t%.12g" % v for v in s["pressure"]) + "\t%.12g" % s["pressure_iso"]
        assert row == want


def test_cli_bonded_input_warns_and_skips(tmp_path):
    case, mols = pc.build_bonded("bonds")
    case = dict(case, nsteps=4, stress=2, frozen=[0, 0])
    d = inputs.write_input_files(case, str(tmp_path / "b"), stat=2)
    r = run_cli(d)
    assert "WARNING: stress directive not usable" in r.stderr
    assert not os.path.exists(os.path.join(d, "stress.dat")) and os.path.exists(os.path.join(d, "stat.dat"))


# ---- 9. kernel timers -------------------------------------------------------------------------------------------------------------------------------
def test_kernel_timers_name_the_sampler():
    e = api.Engine(api.Model.from_case(inputs.config("F1")), profile=1)
    e.stress_setup()
    e.step(3)
    e.stats()
    e.reset_kernel_times()
    e.stress_sample()
    e.stress_sample()
    kt = {k: v["calls"] for k, v in e.kernel_times().items() if v["calls"] > 0}
    want = {"k_stress_bin", "k_stress_scan", "k_stress_ids", "k_stress_rank", "k_stress_place", "k_stress_gather", "k_stress_pairs", "k_stress_chunks",
            "k_stress_fold"}
    assert set(kt) == want, kt                      # the sampler's launches and no step kernel
    assert kt["k_stress_pairs"] == 2 and kt["k_stress_fold"] == 2
