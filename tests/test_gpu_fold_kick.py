"""Both half-kicks in the list pair kernel (KICK_BOTH, csrc/pair_list.hip.h) and the drift-only plain step behind it (k_drift_plain2, csrc/kernels.hip.h).

On a plain NVE step of a one-GPU run that walks pair lists without the clean-up launch, books no energies and is followed by a plain step of the same
launched run, k_pair_list applies this step's second half-kick and the next step's first and stores the velocity instead of the force; the next step is
then a drift.  Same operations in the same order as k_integrate_plain2 on the stored force: everything a caller can see must be BIT-IDENTICAL to an engine
that does not fold, whatever the pattern of calls - and wherever the host, a snapshot, aztot_forces or a replay can see the state it is the canonical one.

The default folds only above 524 288 atoms.  DBG_FOLD_KICK turns it on whatever the size and DBG_NO_FOLD_KICK off; small systems otherwise fuse the next
step into the pair kernel or kick in the tile kernel's epilogue, other paths whose statistics agree with the large path to summation order only, so both
engines of a comparison are also held on the large path (DBG_NO_FUSE_NEXT | DBG_LARGE_KICK_PATH): folding is then the only difference between them.
Where folding must not happen at all (thermostats, bonded terms, the Ewald sum, slab ranks) the two bits are the only ones set.  Engines launch their steps
one by one (use_graph=0) but for one case that replays captured cycles, which hold folded steps like any others.
"""
import numpy as np
import pytest

from aztotmd_amd import api, inputs
from aztotmd_amd.api import DebugBit
from util import on_the_walls, wall_liquid

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz")
LARGE_PATH = DebugBit.DBG_NO_FUSE_NEXT | DebugBit.DBG_LARGE_KICK_PATH
ON = DebugBit.DBG_FOLD_KICK | LARGE_PATH
OFF = DebugBit.DBG_NO_FOLD_KICK | LARGE_PATH
STEP_KERNELS = ("drift", "integrate1", "integrate1_bin")


def system(name):
    # 8^3 FCC cells of 5.735 A: five cells of rc + skin per axis, the fewest a one-GPU engine re-sorts lazily on (it must be able to widen its stencil by a
    # cell) and so the smallest box that keeps pair lists at rc = 8.5 A (2 048 atoms)
    if name == "lj":                 # one species: the one-species LJ kernel
        return wall_liquid()
    if name == "fennell":            # two charged species, LJ + Fennell: the table-driven kernel
        return on_the_walls(inputs.lj_case((8, 8, 8), seed=72, vel_T=85.0, charges=(0.2, -0.2), elec="fenn"))
    if name == "frozen":             # ... one of them frozen: kicked like any other, never moved
        c = on_the_walls(inputs.lj_case((8, 8, 8), seed=73, vel_T=85.0, charges=(0.2, -0.2), elec="fenn"))
        c["frozen"] = [0, 1]
        return c
    raise KeyError(name)


def pair(case, on=ON, off=OFF, **kw):
    kw.setdefault("use_graph", 0)
    return api.Engine(api.Model.from_case(case), debug=on, **kw), api.Engine(api.Model.from_case(case), debug=off, **kw)


def assert_same(a, b, what):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), (what, k)
    sta, stb = a.stats(), b.stats()
    for k in sta:
        assert np.array_equal(np.asarray(sta[k]), np.asarray(stb[k]), equal_nan=True), (what, k, sta[k], stb[k])
    assert np.array_equal(a.species_crossings(), b.species_crossings()), what
    return sta


def step_kernel_calls(e):
    t = e.kernel_times()
    return {k: (t[k]["calls"] if k in t else 0) for k in STEP_KERNELS}


PATTERNS = ["single_steps", "one_call", "stats_between", "forces_between", "sort_every_3", "looks_inside", "energies_every_step", "replayed_cycles"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", ["lj", "fennell", "frozen"])
def test_state_and_statistics_are_bit_identical(name, pattern):
    """x, v, f, every entry of stats() (wall momenta and crossing counters among them) and species_crossings after each call pattern, folding on against off.
    An engine's first look is spent with the clean-up launch in place, so nothing folds before it: every pattern but 'single_steps' runs on past it."""
    case = system(name)
    kw = {}
    if pattern == "sort_every_3":
        kw = dict(sort_every=3)                   # rebuilds fall between folded steps
    elif pattern == "energies_every_step":
        kw = dict(energies_every_step=1)          # nothing may fold
    elif pattern == "replayed_cycles":
        kw = dict(use_graph=1)
    a, b = pair(case, **kw)
    both = (a, b)
    if pattern == "single_steps":
        for _ in range(40):
            for e in both:
                e.step(1)
    elif pattern in ("one_call", "looks_inside", "sort_every_3", "energies_every_step"):
        for e in both:
            e.step(40)                            # (holds the looks at 8 and at 24 steps)
        if pattern == "looks_inside":
            assert_same(a, b, (name, pattern, 40))
            for e in both:
                e.step(72)                        # ... and the one at 56, with folded steps on either side of it
    elif pattern == "stats_between":
        for e in both:
            e.step(7)
        assert_same(a, b, (name, pattern, 7))
        for e in both:
            e.step(33)
    elif pattern == "forces_between":
        for e in both:
            e.step(5)
            e.forces()
        assert_same(a, b, (name, pattern, 5))
        for e in both:
            e.step(20)
    else:
        for n in (8, 40, 3, 29):
            for e in both:
                e.step(n)
    st = assert_same(a, b, (name, pattern, "end"))
    assert st["sort_violations"] == 0 and st["step"] == {"looks_inside": 112, "replayed_cycles": 80}.get(pattern, 40 if pattern != "forces_between" else 25), st
    if pattern != "single_steps":                 # (calls of one step each end on the step that rebuilt the cells or carry its lists on: nothing to fold either way)
        assert st["pair_lists"] == 1 and st["sort_interval"] > 1, st
    if pattern == "looks_inside":
        # (112 steps at 85 K with lattice planes on the walls: every wall has been crossed, in the frozen case by the moving species)
        assert all(c > 0 for c in st["posCross"] + st["negCross"]), st
    for e in both:
        e.close()


def test_which_kernel_ran():
    """per-kernel timing counts launches: every step opens with exactly one of k_drift_plain2 ('drift'), k_integrate_plain2 ('integrate1') and
    k_integrate1_bin; a step is a drift exactly when the step before it folded"""
    case = system("lj")
    a, b = pair(case)
    c = api.Engine(api.Model.from_case(case), debug=ON, use_graph=0, energies_every_step=1)
    engs = (a, b, c)
    for e in engs:
        e.set_profile(1)
        e.step(8)                                 # the first look: interval measured, lists recorded, the clean-up launch dropped from here on
    K = a.stats()["sort_interval"]
    assert K > 2, K
    taken = 8
    for n in (5, 1, 1, 9, 12):              # (each inside the 16 steps to the next look: one launched run per call)
        for e in engs:
            e.reset_kernel_times()
            e.step(n)
        taken += n
        ka, kb, kc = (step_kernel_calls(e) for e in engs)
        for k in (ka, kb, kc):
            assert sum(k.values()) == n, (n, k)
        assert kb["drift"] == 0 and kc["drift"] == 0, (n, kb, kc)
        # the call's last step never folds, so its first is never a drift: n - 1 at most
        assert ka["drift"] <= n - 1, (n, ka)
        # ... and all the plain steps behind the first are (the clean-up launch is off, no energies are booked before the last step)
        assert ka["integrate1"] <= 1, (n, ka)
        assert ka["drift"] + ka["integrate1"] == kb["integrate1"] and ka["integrate1_bin"] == kb["integrate1_bin"], (n, ka, kb)
        if ka["integrate1_bin"] == 0:             # one look window, no rebuild: all but the first step
            assert ka["drift"] == n - 1, (n, ka)
    assert a.stats()["rebuilds"] < taken / 2      # (most steps were plain ones)
    assert_same(a, b, "kernel counts")
    for e in engs:
        e.close()


def no_fold_case(kind):
    if kind == "nose":
        c = inputs.lj_case((8, 8, 8), seed=81, T=85.0, vel_T=85.0)
        c.update(tstat_type=1, tau=0.08)
        return c, {}
    if kind == "radiative":
        return inputs.lj_case((7, 7, 7), a=5.4, seed=82, rc=6.5, cell_list=6.9, T=200.0, tstat="radi", vel_T=150.0, radii=[(2.73, 4.731, 0.2)]), {}
    if kind == "bonded":
        return inputs.molecular_case((8, 8, 8), seed=83, charges=(-0.2, 0.1), elec="fenn", vel_T=300.0), {}
    if kind == "ewald":
        c = inputs.lj_case((7, 7, 7), a=5.4, seed=84, rc=6.5, cell_list=6.9, charges=(0.4, -0.4), elec="fenn", r_real=6.5, alpha=0.45, vel_T=80.0)
        c.update(elec_type=2, ewald_k=(6, 6, 6))
        return c, {}
    if kind == "slab":               # one rank of two talking to itself (loopback): 14 cell layers along x
        return inputs.lj_case((42, 5, 5), a=5.735, seed=85, rc=8.5, vel_T=8.0), dict(slab={"rank": 1, "nranks": 2, "loopback": True})
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["nose", "radiative", "bonded", "ewald", "slab"])
def test_runs_that_must_not_fold(kind):
    """a thermostat acts between the two kicks, bonded and reciprocal-space forces arrive behind the pair kernel, a slab rank's neighbours read its state:
    DBG_FOLD_KICK changes nothing there"""
    case, kw = no_fold_case(kind)
    a, b = pair(case, on=DebugBit.DBG_FOLD_KICK, off=DebugBit.DBG_NO_FOLD_KICK, **kw)
    for e in (a, b):
        e.set_profile(1)
    for n in (8, 17, 1, 22):
        for e in (a, b):
            e.step(n)
    for e in (a, b):
        assert step_kernel_calls(e)["drift"] == 0, (kind, e.kernel_times())
    assert_same(a, b, kind)
    for e in (a, b):
        e.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_window_run_again_from_a_snapshot(seed):
    """atoms far too fast for a sort interval held at 16 steps (DBG_FIXED_INTERVAL): looks find skin violations in windows that ran without the clean-up launch -
    folded steps among them - and run them again from the snapshot, which holds the canonical state.  The engine's ordinary repair path: equal results and
    equal violation counts, folding on and off."""
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
    st = assert_same(a, b, (seed, calls))
    assert st["sort_violations"] > 0 and st["step"] == sum(calls), st
    for e in (a, b):
        e.close()
