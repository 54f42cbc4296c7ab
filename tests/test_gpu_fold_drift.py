"""The next step's drift in the list pair kernel (KICK_DRIFT: fold_drift_atom / fold_drift_finish, csrc/pair_list.hip.h).

Where k_pair_list folds both half-kicks (KICK_BOTH, tests/test_gpu_fold_kick.py) the lane that stores an atom's final velocity can also drift the atom, as
k_drift_plain2 would in a launch of its own: the same operations in the same order with the next step's values, the new position into the second set of
coordinate arrays.  The step behind such a launch opens with no launch at all.  Each test compares two engines on the same system,

    DBG_FOLD_DRIFT | DBG_NO_FUSE_NEXT | DBG_LARGE_KICK_PATH                       KICK_DRIFT
    DBG_FOLD_KICK | DBG_NO_FOLD_DRIFT | DBG_NO_FUSE_NEXT | DBG_LARGE_KICK_PATH    KICK_BOTH and k_drift_plain2 behind it

through the same calls.  Bit for bit: x, y, z, vx, vy, vz, fx, fy, fz, every entry of stats() and the per-species crossing counters - with one exception.
A wall's momentum sum is added up per booking workgroup, and the workgroups differ (the drift kernel's 256 threads of consecutive atoms, the pair kernel's
wave per cell).  Every term of one wall's sum has the same sign (m |v| of a crossing towards that wall), so two orders of adding n terms differ by at most
2 (n - 1) 2^-52 relative; n is the wall's crossing counter, which is compared exactly.  `pressure` is a linear function of the six sums
(Engine::get_stats: sum over the walls of 2 f / (6 A_k dt_w) x (sum now - sum at the last evaluation), f = 1.58e6, dt_w >= dt) and inherits their bound,
twice (now and then), plus 16 ulps of its gross terms for its own roundings.

The systems are the smallest that can still go wrong: 8^3 FCC cells of 5.735 A (2 048 atoms, the smallest box that re-sorts lazily: five cells per axis,
27 whose stencil meets no periodic image - the epilogue's short path - and 98 that take the full one), lattice planes on all six walls and 85 K so that
every wall is crossed many times; two species of unequal masses (table-driven kernel), both moving or one frozen; and the dense liquid with the 7^3
stencil (the five-group kernel and its dense-system loop, several waves per cell).
"""
import numpy as np
import pytest

import list_cases as lc
from aztotmd_amd import api, inputs
from aztotmd_amd.api import DebugBit
from util import on_the_walls, wall_liquid

pytestmark = pytest.mark.gpu

LARGE_PATH = DebugBit.DBG_NO_FUSE_NEXT | DebugBit.DBG_LARGE_KICK_PATH
ON = DebugBit.DBG_FOLD_DRIFT | LARGE_PATH
OFF = DebugBit.DBG_FOLD_KICK | DebugBit.DBG_NO_FOLD_DRIFT | LARGE_PATH
STEP_KERNELS = ("drift", "integrate1", "integrate1_bin")
MOM = ("posMom", "negMom")
CROSS = {"posMom": "posCross", "negMom": "negCross"}
PRESSURE_FACTOR = 1.58e6               # units::pressure_factor (csrc/model.h)
ULP = 2.0 ** -52


def system(name):
    if name == "lj":                 # one species: the one-species LJ kernel
        return wall_liquid()
    if name in ("two_masses", "frozen"):
        # two charged species, LJ + Fennell: the table-driven kernel; the second species 1.7 times as heavy - and, in 'frozen', kicked but never moved
        c = on_the_walls(inputs.lj_case((8, 8, 8), seed=74 if name == "frozen" else 75, vel_T=85.0, charges=(0.2, -0.2), elec="fenn"))
        (m, qa), (_, qb) = c["species"]
        c["species"] = [(m, qa), (1.7 * m, qb)]
        if name == "frozen":
            c["frozen"] = [0, 1]
        return c
    if name == "wide_stencil":       # tests/list_cases.py: 4 000 atoms on cells of 2.75 A, ~460 kept candidates per cell
        return dict(lc.liquid("wide_stencil")["case"])
    raise KeyError(name)


def pair(case, on=ON, off=OFF, **kw):
    kw.setdefault("use_graph", 0)
    return api.Engine(api.Model.from_case(case), debug=on, **kw), api.Engine(api.Model.from_case(case), debug=off, **kw)


def assert_same(a, b, case, what):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), (what, k, int((sa[k] != sb[k]).sum()))
    sta, stb = a.stats(), b.stats()
    L = case["box"]
    area = [L[1] * L[2], L[0] * L[2], L[0] * L[1]]
    tol_p = gross_p = 0.0
    for k in sta:
        if k in MOM:
            for d in range(3):
                n, va, vb = sta[CROSS[k]][d], sta[k][d], stb[k][d]
                bound = 2.0 * max(n - 1, 0) * ULP * abs(vb)
                print("%s %s[%d]: %d crossings, %.17g against %.17g, %.2f ulp (bound %d)" % (what, k, d, n, va, vb, abs(va - vb) / (ULP * abs(vb)) if vb else 0.0, 2 * max(n - 1, 0)))
                assert abs(va - vb) <= bound, (what, k, d, n, va, vb)
                w = 2.0 * PRESSURE_FACTOR / (6.0 * area[d] * case["dt"])
                tol_p += w * 2.0 * bound
                gross_p += w * 2.0 * abs(vb)
        elif k == "pressure":
            continue
        else:
            assert np.array_equal(np.asarray(sta[k]), np.asarray(stb[k]), equal_nan=True), (what, k, sta[k], stb[k])
    print("%s pressure: %.17g against %.17g, allowed %.3g" % (what, sta["pressure"], stb["pressure"], tol_p + 16.0 * ULP * gross_p))
    assert abs(sta["pressure"] - stb["pressure"]) <= tol_p + 16.0 * ULP * gross_p, (what, sta["pressure"], stb["pressure"])
    assert np.array_equal(a.species_crossings(), b.species_crossings()), what
    return sta


def calls_of(e, names=STEP_KERNELS + ("fold_drift",)):
    t = e.kernel_times()
    return {k: (t[k]["calls"] if k in t else 0) for k in names}


PATTERNS = ["single_steps", "one_call", "stats_between", "sort_every_3", "replayed_cycles"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", ["lj", "two_masses", "frozen", "wide_stencil"])
def test_state_and_statistics_agree(name, pattern):
    """one long call (with the looks at 8, 24 and 56 steps inside it), step(1) repeated, step(n) with stats() between the calls, a run across many
    rebuilds with folded steps between them, replayed captured cycles (which hold folded steps like any others)"""
    case = system(name)
    kw = {}
    if pattern == "sort_every_3":
        kw = dict(sort_every=3)
    elif pattern == "replayed_cycles":
        kw = dict(use_graph=1)
    if name == "wide_stencil":
        kw.update(split=2)                        # two waves share a cell's tile and split its atoms (k_pair_list<..., MULTI>)
    a, b = pair(case, **kw)
    both = (a, b)
    if pattern == "single_steps":
        for _ in range(40):
            for e in both:
                e.step(1)
        total = 40
    elif pattern == "one_call":
        for e in both:
            e.step(112)
        total = 112
    elif pattern == "stats_between":
        total = 0
        for n in (7, 33, 2, 30):
            for e in both:
                e.step(n)
            total += n
            assert_same(a, b, case, (name, pattern, total))
    elif pattern == "sort_every_3":
        for e in both:
            e.step(40)
        total = 40
    else:
        for n in (8, 40, 3, 29):
            for e in both:
                e.step(n)
        total = 80
    st = assert_same(a, b, case, (name, pattern, "end"))
    assert st["sort_violations"] == 0 and st["step"] == total, st
    if pattern != "single_steps":
        assert st["pair_lists"] == 1 and st["sort_interval"] > 1, st
    if pattern == "sort_every_3":
        assert st["rebuilds"] >= 10, st                # (far more than two)
    if pattern == "one_call" and name != "wide_stencil":
        # a case without crossings proves nothing: 112 steps at 85 K with lattice planes on the walls cross every wall several times
        assert all(c >= 3 for c in st["posCross"] + st["negCross"]), st
    for e in both:
        e.close()


@pytest.mark.parametrize("name", ["lj", "frozen", "wide_stencil"])
def test_steps_that_open_with_no_launch(name):
    """per-kernel timing counts launches ('fold_drift': pair launches that also drifted).  A step opens with no launch of its own exactly when the step
    before it folded the drift: drift + integrate1 + integrate1_bin of the folding engine plus its folded steps is the other engine's total, one per step"""
    case = system(name)
    a, b = pair(case, **(dict(split=2) if name == "wide_stencil" else {}))
    for e in (a, b):
        e.set_profile(1)
        e.step(8)                                 # the first look: interval measured, lists recorded, the clean-up launch dropped from here on
    K = a.stats()["sort_interval"]
    assert K > 2, K
    folded = 0
    for n in (5, 1, 1, 9, 12):                    # (each inside the 16 steps to the next look: one launched run per call)
        for e in (a, b):
            e.reset_kernel_times()
            e.step(n)
        ka, kb = calls_of(a), calls_of(b)
        assert kb["fold_drift"] == 0 and sum(kb[k] for k in STEP_KERNELS) == n, (n, kb)
        assert ka["drift"] == 0, (n, ka)                                        # nothing is left for k_drift_plain2
        assert sum(ka[k] for k in STEP_KERNELS) + ka["fold_drift"] == n, (n, ka)
        assert ka["fold_drift"] == kb["drift"], (n, ka, kb)                      # the steps that fold are the steps that folded the kicks
        assert ka["integrate1"] == kb["integrate1"] and ka["integrate1_bin"] == kb["integrate1_bin"], (n, ka, kb)
        assert ka["fold_drift"] <= n - 1, (n, ka)                                # the call's last step never folds
        if ka["integrate1_bin"] == 0:
            assert ka["fold_drift"] == n - 1, (n, ka)
        folded += ka["fold_drift"]
    assert folded >= 14, folded
    assert_same(a, b, case, "launch counts")
    for e in (a, b):
        e.close()


def no_fold_case(kind):
    if kind == "energies_every_step":
        return wall_liquid(), dict(energies_every_step=1), LARGE_PATH
    if kind == "radiative":
        return inputs.lj_case((7, 7, 7), a=5.4, seed=82, rc=6.5, cell_list=6.9, T=200.0, tstat="radi", vel_T=150.0, radii=[(2.73, 4.731, 0.2)]), {}, 0
    if kind == "slab":               # one rank of two talking to itself (loopback): 14 cell layers along x
        return inputs.lj_case((42, 5, 5), a=5.735, seed=85, rc=8.5, vel_T=8.0), dict(slab={"rank": 1, "nranks": 2, "loopback": True}), 0
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["energies_every_step", "radiative", "slab"])
def test_runs_that_must_not_fold(kind):
    """energies booked on every step, a thermostat between the two kicks, a slab rank whose neighbours read its state: DBG_FOLD_DRIFT changes nothing -
    no launch drifts, the steps open with the kernels they opened with, the results are equal (the momentum sums too: the same kernels book them)"""
    case, kw, common = no_fold_case(kind)
    a, b = pair(case, on=DebugBit.DBG_FOLD_DRIFT | common, off=DebugBit.DBG_FOLD_KICK | DebugBit.DBG_NO_FOLD_DRIFT | common, **kw)
    for e in (a, b):
        e.set_profile(1)
    for n in (8, 17, 1, 22):
        for e in (a, b):
            e.step(n)
    ka, kb = calls_of(a), calls_of(b)
    assert ka["fold_drift"] == 0 and ka["drift"] == 0 and ka == kb, (kind, ka, kb)
    sa, sb = a.stats(), b.stats()
    for k in MOM:
        assert sa[k] == sb[k], (kind, k, sa[k], sb[k])
    assert sa["pressure"] == sb["pressure"], (kind, sa["pressure"], sb["pressure"])
    assert_same(a, b, case, kind)
    for e in (a, b):
        e.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_window_run_again_from_a_snapshot(seed):
    """the too-fast atoms of tests/test_gpu_fold_kick.py, sort interval held at 16 steps (DBG_FIXED_INTERVAL): looks find skin violations - flagged by the
    pair kernel's drift here - in windows that ran without the clean-up launch and run them again from the snapshot, whose coordinate arrays are those of
    the set that was current when it was taken.  Equal results and equal violation counts."""
    rng = np.random.default_rng(seed)
    kw = dict(a=5.4, seed=100 + seed, rc=6.5, cell_list=6.9, vel_T=float(rng.uniform(6000.0, 12000.0)))
    if seed % 2 == 1:
        kw.update(charges=(0.2, -0.2), elec="fenn", r_real=6.5)
    case = inputs.lj_case((7, 7, 7), **kw)
    case["dt"] = 0.002
    calls = [int(v) for v in rng.integers(1, 40, size=6)]
    a, b = pair(case, on=ON | DebugBit.DBG_FIXED_INTERVAL, off=OFF | DebugBit.DBG_FIXED_INTERVAL, sort_every=16)
    for n in calls:
        a.step(n); b.step(n)
    st = assert_same(a, b, case, (seed, calls))
    assert st["sort_violations"] > 0 and st["step"] == sum(calls), st
    for e in (a, b):
        e.close()
