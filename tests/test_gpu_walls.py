"""The first half of a step - half-kick, drift, periodic wrap, wall-crossing counters, wall momenta - in each of its launch forms, atom by atom against the
exact reference of tests/wall_reference.py on the designed gas of tests/wall_cases.py, and the cell sort behind it (k_scan_single, k_scan_totals +
k_scan_apply, k_place, k_rank_gather) against a host prefix sum on a grid of 6 384 cells and on one of 16 929 (odd: no multiple of 4 or of 1024).

  form                               engine                                              evidence (kernel_times of the call)
  k_integrate1_bin<STEP_RESORT>      sort_every=1                                        integrate1_bin == steps
  k_integrate_plain2                 lazy, DBG_NO_FUSE_NEXT | DBG_NO_FOLD_KICK           integrate1 on the plain steps
  k_integrate1_bin<STEP_PLAIN>       ... | DBG_PLAIN_ONE_ATOM                            integrate1; x, v, f, counts bit-equal to the form above
  k_drift_plain2                     DBG_FOLD_KICK                                       drift >= 1
  next_step_atom in k_pair_list      DBG_FUSE_NEXT                                       steps that no integrate kernel opened, pair_lists == 1
  k_boundary_radi                    radiative variant, DBG_NO_FUSE_NEXT                 boundary >= 1
  next_step_atom in k_pair_tile<CLEANUP>   wall-plane liquid, DBG_FUSE_NEXT | DBG_SHORT_LISTS | DBG_ALWAYS_CLEANUP   pair_cleanup on the fused steps

Calls are [1, 4, 7] with stats(), species_crossings() and state() read after each; a twin engine makes one call of 12 steps.  Every engine is held to the
reference under ITS rule: put_periodic every step where the cells are rebuilt every step, the image rule with the rebuild steps the timers show elsewhere
(wall_reference: the two differ for atoms that land on L or start there).  Bounds: |x - x_ref| mod L <= TAU (L + sum |v dt|), |mom - mom_ref| <= TAU sum m |v|,
coordinates whose chain is exact in fp64 EQUAL, counts equal, velocities untouched, forces exactly 0.  Every run prints its worst err / (TAU scale) first.
"""
import numpy as np
import pytest

import wall_cases as wc
import wall_reference as wr
from aztotmd_amd import api
from aztotmd_amd.api import DebugBit
from oracle import oracle
from util import check_cell_table, wall_liquid

pytestmark = pytest.mark.gpu
CALLS = (1, 4, 7)
PLAIN2 = DebugBit.DBG_NO_FUSE_NEXT | DebugBit.DBG_NO_FOLD_KICK
STEP_KERNELS = ("integrate1_bin", "integrate1", "drift", "boundary")
_C = {}


def ref_run(variant, rule, rebuild=None, fold=False, v=None, tag=None):
    key = (variant, rule, tuple(sorted(rebuild)) if rebuild else None, fold, tag)
    if key not in _C:
        g = wc.build()
        _C[key] = wr.run(g["x"], wc.velocities(variant) if v is None else v, g["types"], wc.NSTEPS, rule, set(rebuild) if rebuild else None, fold)
    return _C[key]


def xyz(s, keys=("x", "y", "z")):
    return np.stack([s[k] for k in keys], 1)


def walls(st, what):
    """the six walls in the order Xn Xp Yn Yp Zn Zp from stats()'s neg* / pos* triples"""
    return [st[("neg" if k % 2 == 0 else "pos") + what][k // 2] for k in range(6)]


class Run:
    """an engine on the gas, driven call by call with everything a reader can see kept: per call (steps done, steps of the call, launches, stats,
    species_crossings, state, sort interval before the call)"""

    def __init__(self, variant="plain", **kw):
        self.e = api.Engine(api.Model.from_case(wc.case(variant)), profile=1, **kw)
        self.done, self.obs = 0, []

    def call(self, n):
        K = self.e.stats()["sort_interval"]
        self.e.reset_kernel_times()
        self.e.step(n)
        kt = {k: v["calls"] for k, v in self.e.kernel_times().items() if v["calls"] > 0}
        self.done += n
        st = self.e.stats()
        assert st["step"] == self.done and st["pairs_dropped"] == 0 and st["engVdW"] == 0.0, st
        self.obs.append({"done": self.done, "n": n, "kt": kt, "st": st, "spec": self.e.species_crossings(), "s": self.e.state(), "K": max(int(K), 1)})
        return self.obs[-1]


def rebuild_steps(obs):
    """the steps that rebuilt the cells, from the launches of every call (integrate1_bin) and the sort interval K in force: a step is plain while fewer than
    K - 1 steps have gone by since the last rebuild, and a call either carries the interval of the call before on or opens with a rebuild.  Where the
    number of integrate1_bin launches of a call fits neither, or fits both differently, the schedule is not understood and the test says so."""
    def emulate(K, since, first, n):
        reb = []
        for s in range(first, first + n):
            if since is not None and since < K - 1:
                since += 1
            else:
                reb.append(s)
                since = 0
        return reb, since

    out, since = [], None
    for o in obs:
        first, n, nbin = o["done"] - o["n"] + 1, o["n"], o["kt"].get("integrate1_bin", 0)
        fits = []
        for start in (since, None):
            reb, after = emulate(o["K"], start, first, n)
            if len(reb) == nbin and (reb, after) not in fits:
                fits.append((reb, after))
        assert len(fits) == 1, ("rebuild steps of the call not determined by its launches", o["done"], n, o["K"], since, o["kt"], fits)
        out += fits[0][0]
        since = fits[0][1]
    return out


def judge(label, run, ref, exact, v_expected=None, tie_by_design=None):
    """every call of `run` against the reference steps `ref`; prints the worst ratios, then asserts.  Returns the totals a twin must reproduce.
    tie_by_design: coordinates one ulp from a multiple of L on purpose - no margin asked of them, and no range of the reported value"""
    worst = {"x": 0.0, "mom": 0.0}
    loose = np.zeros_like(exact) if tie_by_design is None else tie_by_design
    assert wr.undecided(ref, exact | loose) == [], (label, "a generic atom within 1e-9 A of a wall decision: no atom may be left unjudged")
    for o in run.obs:
        r, s, st = ref[o["done"]], o["s"], o["st"]
        x = xyz(s)
        rx, unequal = wr.position_ratio(x, r, exact)
        cnt, mom = walls(st, "Cross"), walls(st, "Mom")
        try:
            rm = wr.momentum_ratio(mom, r)
        except AssertionError as err:
            rm = float("inf")
            print(label, "momentum of a wall nobody crossed:", err)
        worst["x"], worst["mom"] = max(worst["x"], rx), max(worst["mom"], rm)
        print("%s steps %d..%d: x %.3e  mom %.3e  exact coordinates not equal %d  crossings %s (reference %s)  launches %s"
              % (label, o["done"] - o["n"] + 1, o["done"], rx, rm, unequal, cnt, list(r["cnt"]), {k: o["kt"][k] for k in STEP_KERNELS if k in o["kt"]}))
        assert all((s[k] == 0.0).all() for k in ("fx", "fy", "fz")), (label, "forces are not exactly 0")
        if v_expected is not None:
            assert np.array_equal(xyz(s, ("vx", "vy", "vz")), v_expected), (label, "a force-free step changed a velocity")
        assert ((x >= 0.0) & (x < np.array(wc.BOX)) | loose).all(), (label, "a reported coordinate outside [0, L)")
        assert rx <= 1.0 and unequal == 0, (label, o["done"], rx, unequal)
        assert cnt == list(r["cnt"]), (label, o["done"], cnt, list(r["cnt"]))
        assert np.array_equal(o["spec"], r["spec"]) and list(o["spec"].sum(0)) == cnt, (label, o["done"], o["spec"], r["spec"])
        assert rm <= 1.0, (label, o["done"], rm)
        for lazy in (True, False):                                # the cell of every atom, on every grid of the tests
            for cell in (wc.CELL_COARSE, wc.CELL_FINE):
                dims = wc.N_CELLS[(cell, lazy)]
                assert np.array_equal(wr.cells(np.where(loose, r["wrapped"], x), dims), wr.cells(r["wrapped"], dims)), (label, o["done"], dims)
    last = run.obs[-1]
    return {"cnt": walls(last["st"], "Cross"), "spec": last["spec"], "ref_cnt": list(ref[last["done"]]["cnt"]), "worst": worst}


def same_totals(label, a, b):
    """a twin that took other calls reports the same totals - wherever its schedule differs in a tie of the two rules, by exactly what the reference says"""
    da = np.array(a["cnt"]) - np.array(a["ref_cnt"])
    db = np.array(b["cnt"]) - np.array(b["ref_cnt"])
    assert not da.any() and not db.any(), (label, a, b)
    if a["ref_cnt"] == b["ref_cnt"]:
        assert a["cnt"] == b["cnt"] and np.array_equal(a["spec"], b["spec"]), (label, a, b)


def n_cells_ok(e, cell, lazy=True):
    dims = wc.N_CELLS[(cell, lazy)]
    n = e.stats()["n_cells"]
    assert n == dims[0] * dims[1] * dims[2], (n, dims)
    assert (n <= 16384) if cell == wc.CELL_COARSE else (n > 16384 and n % 4 != 0 and n % 1024 != 0), n


# ---- cells rebuilt every step --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("cell", [wc.CELL_COARSE, wc.CELL_FINE])
def test_rebuild_every_step(cell, variant):
    """k_integrate1_bin<STEP_RESORT> on both grids with both pair kernels: put_periodic after every drift, the cell table right after every call"""
    ref, ex = ref_run("plain", "every"), wc.exact_axes()
    label = "resort [cells %s, pair_variant %d]" % ("x".join(map(str, wc.N_CELLS[(cell, False)])), variant)
    totals = []
    for calls in (CALLS, (wc.NSTEPS,)):
        r = Run(sort_every=1, pair_variant=variant, cell_size=cell)
        n_cells_ok(r.e, cell, lazy=False)
        check_cell_table(r.e, r.e.state(), wc.BOX)                # the initial sort: atoms ON the upper wall (x == L) among them
        for n in calls:
            o = r.call(n)
            assert o["kt"].get("integrate1_bin") == n and "integrate1" not in o["kt"] and "drift" not in o["kt"], o["kt"]
            check_cell_table(r.e, o["s"], wc.BOX)
        totals.append(judge(label + (" twin" if len(calls) == 1 else ""), r, ref, ex, wc.velocities()))
        r.e.close()
    same_totals(label, *totals)


def test_jumps_of_more_than_a_box_length():
    """+-1.5 L, 2.5 L per step, and per axis an atom that moves nextafter(2 L, 0) from 0.0: where it lands is whatever (int)(x * (1 / L)) makes of it -
    after its first step pinned bit for bit to the CPU oracle, which shares box.cpp's formula (the shift is by 1 L or 2 L there, exact products; later
    steps shift by 3 L, which a fused multiply-add rounds differently, and are held modulo L like every other coordinate)"""
    ref, ex, pinned = ref_run("jump", "every"), wc.exact_axes("jump"), wc.pinned_axes()
    assert pinned.sum() == 3
    r = Run("jump", sort_every=1)
    o = oracle.Oracle(wc.case("jump"))
    for n in CALLS:
        ob = r.call(n)
        assert ob["kt"].get("integrate1_bin") == n, ob["kt"]
        o.step(n)
        gx, ox = xyz(ob["s"]), xyz(o.state())
        print("jump after %d steps: pinned coordinates gpu %s oracle %s" % (ob["done"], gx[pinned].tolist(), ox[pinned].tolist()))
        if ob["done"] == 1:
            assert np.array_equal(gx[pinned], ox[pinned]), "the atom at nextafter(2 L, 0) is not the oracle's, bit for bit"
        check_cell_table(r.e, ob["s"], wc.BOX)
    judge("jump", r, ref, ex, wc.velocities("jump"), tie_by_design=pinned)
    r.e.close()


# ---- the lazy schedule ---------------------------------------------------------------------------------------------------------------------------------
def lazy_pair(label, debug, cell, variant, twin=True, evidence=None):
    """an engine on the lazy schedule through CALLS and a twin through one call of 12 steps, each against the image rule with its own rebuild steps"""
    ex, totals, runs = wc.exact_axes(), [], []
    for calls in ((CALLS, (wc.NSTEPS,)) if twin else (CALLS,)):
        r = Run(debug=debug, pair_variant=variant, cell_size=cell)
        n_cells_ok(r.e, cell)
        for n in calls:
            r.call(n)
        reb = rebuild_steps(r.obs)
        print("%s: calls %s rebuilt the cells at steps %s; sort interval %d" % (label, list(calls), reb, r.obs[-1]["st"]["sort_interval"]))
        ref = ref_run("plain", "image", reb, True)
        totals.append(judge(label + (" twin" if len(calls) == 1 else ""), r, ref, ex, wc.velocities()))
        runs.append(r)
    if twin:
        same_totals(label, *totals)
    main = runs[0]
    assert main.obs[-1]["st"]["sort_interval"] > 1 and main.obs[-1]["st"]["sort_violations"] == 0, main.obs[-1]["st"]
    if evidence is not None:
        evidence(main)
    return runs


def plain_steps_ran(name):
    def check(r):
        later = [o for o in r.obs if o["done"] > 1]
        assert sum(o["kt"].get(name, 0) for o in later) >= 1, [o["kt"] for o in r.obs]
        for o in later:
            assert sum(o["kt"].get(k, 0) for k in STEP_KERNELS) == o["n"], o["kt"]
    return check


def forces_after_a_lazy_call(r, cell):
    """aztot_forces behind plain steps in which atoms crossed: the returned coordinates are in [0, L), the counters are unchanged (STEP_BIN_ONLY counts
    nothing), the cell table is that of the returned state"""
    before, spec = r.e.stats(), r.e.species_crossings()
    assert sum(before["posCross"]) + sum(before["negCross"]) > 100
    r.e.forces()
    after, s = r.e.stats(), r.e.state()
    x = xyz(s)
    assert (x >= 0.0).all() and (x < np.array(wc.BOX)).all()
    for k in ("posCross", "negCross", "posMom", "negMom", "pairs_dropped", "step"):
        assert before[k] == after[k], (k, before[k], after[k])
    assert np.array_equal(spec, r.e.species_crossings())
    assert np.array_equal(x, xyz(r.obs[-1]["s"])), "a force call moved an atom"
    check_cell_table(r.e, s, wc.BOX)
    n_cells_ok(r.e, cell)


@pytest.mark.parametrize("cell,variant", [(wc.CELL_COARSE, 2), (wc.CELL_COARSE, 1), (wc.CELL_FINE, 2)])
def test_plain_steps_two_atoms_per_thread_and_one(cell, variant):
    """k_integrate_plain2 against the image rule, k_integrate1_bin<STEP_PLAIN> (DBG_PLAIN_ONE_ATOM) bit-equal to it in x, v, f and every count (the wall momenta: the same terms summed in
    another order, within the momentum bound of each other); then a
    force call behind the plain steps"""
    label = "plain2 [cells %s, pair_variant %d]" % ("x".join(map(str, wc.N_CELLS[(cell, True)])), variant)
    two = lazy_pair(label, PLAIN2, cell, variant, evidence=plain_steps_ran("integrate1"))
    one = lazy_pair(label.replace("plain2", "plain, one atom per thread"), PLAIN2 | DebugBit.DBG_PLAIN_ONE_ATOM, cell, variant, twin=False, evidence=plain_steps_ran("integrate1"))
    ref_scale = {s_: st["mom_scale"] for s_, st in enumerate(ref_run("plain", "image", rebuild_steps(two[0].obs), True))}
    for a, b in zip(two[0].obs, one[0].obs):
        assert {k: a["kt"].get(k, 0) for k in STEP_KERNELS} == {k: b["kt"].get(k, 0) for k in STEP_KERNELS}
        for k in a["s"]:
            assert np.array_equal(a["s"][k], b["s"][k], equal_nan=True), (label, a["done"], k)
        for k in ("posCross", "negCross", "step"):
            assert a["st"][k] == b["st"][k], (label, a["done"], k, a["st"][k], b["st"][k])
        assert np.array_equal(a["spec"], b["spec"])
        # the wall momenta are sums over the crossings, taken per thread pair and 128 atoms a wave in one kernel and 64 atoms a wave in the other: the same
        # terms in another order (measured: 1 ulp apart, 0.055994280553582645 against 0.05599428055358266) - held to each other by the momentum bound
        ma, mb, scale = np.array(walls(a["st"], "Mom")), np.array(walls(b["st"], "Mom")), ref_scale[a["done"]]
        ratio = float((np.abs(ma - mb) / (wr.TAU * scale)).max())
        print("%s after %d steps: wall momenta of the two kernels apart by %.3e of the bound" % (label, a["done"], ratio))
        assert ratio <= 1.0, (label, a["done"], ma, mb)
    forces_after_a_lazy_call(two[0], cell)
    for r in two + one:
        r.e.close()


def test_drift_only_steps():
    """k_drift_plain2 behind a list kernel that applied both half-kicks (DBG_FOLD_KICK)"""
    def evidence(r):
        assert sum(o["kt"].get("drift", 0) for o in r.obs) >= 1, [o["kt"] for o in r.obs]
    runs = lazy_pair("drift", DebugBit.DBG_FOLD_KICK, wc.CELL_COARSE, 2, evidence=evidence)
    forces_after_a_lazy_call(runs[0], wc.CELL_COARSE)
    for r in runs:
        r.e.close()


@pytest.mark.parametrize("cell", [wc.CELL_COARSE, wc.CELL_FINE])
def test_next_step_opened_by_the_list_kernel(cell):
    """next_step_atom / next_step_finish in the epilogue of k_pair_list (DBG_FUSE_NEXT): on the fused steps no integrate kernel runs at all"""
    def evidence(r):
        fused = 0
        for o in r.obs:
            opened = sum(o["kt"].get(k, 0) for k in STEP_KERNELS)
            assert "drift" not in o["kt"] and opened <= o["n"], o["kt"]
            fused += o["n"] - opened
            if o["done"] > 1:
                assert o["kt"].get("pair_list") == o["n"], o["kt"]
        assert fused >= 1 and r.obs[-1]["st"]["pair_lists"] == 1, [o["kt"] for o in r.obs]
        print("steps opened by the pair kernel: %d" % fused)
    runs = lazy_pair("fused next step [cells %s]" % "x".join(map(str, wc.N_CELLS[(cell, True)])), DebugBit.DBG_FUSE_NEXT, cell, 2, evidence=evidence)
    forces_after_a_lazy_call(runs[0], cell)
    for r in runs:
        r.e.close()


def test_boundary_kernel_of_the_radiative_thermostat():
    """k_boundary_radi closes a step with the thermostat and opens the next: the velocity its drift uses is the one the thermostat left, taken from the states a
    twin that steps one step at a time returns (its own positions and counters are held to the every-step rule with the same velocities)"""
    g = wc.build()
    frozen_only = np.repeat((g["types"] == 2)[:, None], 3, 1)      # the thermostat changes every velocity: only atoms that never move stay exact
    b = Run("radiative", sort_every=1, debug=DebugBit.DBG_NO_FUSE_NEXT)
    vs = [wc.velocities()]
    for _ in range(wc.NSTEPS):
        o = b.call(1)
        assert "boundary" not in o["kt"], o["kt"]
        vs.append(xyz(o["s"], ("vx", "vy", "vz")))
    judge("radiative, one step per call", b, ref_run("radiative", "every", v=vs[:-1], tag="b"), frozen_only)
    a = Run("radiative", debug=DebugBit.DBG_NO_FUSE_NEXT)
    for n in CALLS:
        a.call(n)
    reb = rebuild_steps(a.obs)
    print("k_boundary_radi: rebuilds at steps %s, launches %s" % (reb, [o["kt"] for o in a.obs]))
    assert sum(o["kt"].get("boundary", 0) for o in a.obs) >= 1
    ref = ref_run("radiative", "image", reb, True, v=vs[:-1], tag="a")
    assert wr.undecided(ref, frozen_only) == []
    crossed_in_boundary = sum(int(ref[s]["flags"].sum()) for s in range(2, wc.NSTEPS + 1) if s not in reb)
    assert crossed_in_boundary > 100, crossed_in_boundary
    judge("k_boundary_radi", a, ref, frozen_only)
    for o, s in zip(a.obs, (1, 5, 12)):
        print("  largest |v - v of the step-by-step twin| after step %d: %.3e" % (s, np.abs(xyz(o["s"], ("vx", "vy", "vz")) - vs[s]).max()))
    for r in (a, b):
        r.e.close()


# ---- the wall-plane liquid: atoms that are kicked ----------------------------------------------------------------------------------------------------------
CLEANUP = DebugBit.DBG_SHORT_LISTS | DebugBit.DBG_ALWAYS_CLEANUP


def test_next_step_opened_by_the_clean_up_launch():
    """k_pair_tile<CLEANUP> with next_step_atom: cells whose list overflowed (DBG_SHORT_LISTS) go through the clean-up launch, kept on (DBG_ALWAYS_CLEANUP),
    and under DBG_FUSE_NEXT its epilogue opens the next step for their atoms.  A SCHEDULE-AGAINST-SCHEDULE check, not one against a reference: the same
    engine without fusion must report equal x, v, f, counters and wall momenta over the call pattern [1, 9, 9]."""
    case = wall_liquid()
    a = api.Engine(api.Model.from_case(case), profile=1, debug=DebugBit.DBG_FUSE_NEXT | CLEANUP)
    b = api.Engine(api.Model.from_case(case), profile=1, debug=DebugBit.DBG_NO_FUSE_NEXT | CLEANUP)
    fused = 0
    for n in (1, 9, 9):
        for e in (a, b):
            e.reset_kernel_times()
            e.step(n)
        ka, kb = ({k: v["calls"] for k, v in e.kernel_times().items() if v["calls"] > 0} for e in (a, b))
        sa, sb, sta, stb = a.state(), b.state(), a.stats(), b.stats()
        opened = sum(ka.get(k, 0) for k in STEP_KERNELS)
        print("clean-up launch, call of %d: fused engine %s  cells without a list %d" % (n, {k: ka[k] for k in ka if k.startswith(("pair", "integrate", "drift"))}, sta["cells_without_list"]))
        worst = {k: float(np.abs(sa[k] - sb[k]).max()) for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz")}
        print("  largest differences fused - unfused:", worst, " negMom", np.subtract(sta["negMom"], stb["negMom"]), " posMom", np.subtract(sta["posMom"], stb["posMom"]))
        if n > 1:
            fused += n - opened
            assert n - opened >= 1 and ka.get("pair_cleanup", 0) >= n - opened and sta["cells_without_list"] > 0, (ka, sta)
            assert sum(kb.get(k, 0) for k in STEP_KERNELS) == n, kb
        for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
            assert np.array_equal(sa[k], sb[k]), (n, k, worst[k])
        for k in ("posCross", "negCross", "posMom", "negMom", "step", "pairs_dropped"):
            assert sta[k] == stb[k], (n, k, sta[k], stb[k])
        assert np.array_equal(a.species_crossings(), b.species_crossings())
    assert fused >= 2 and sum(sta["posCross"]) + sum(sta["negCross"]) > 0, (fused, sta)
    for e in (a, b):
        e.close()


@pytest.mark.parametrize("large_kick_path", [False, True])
@pytest.mark.parametrize("form", ["resort", "plain2"])
def test_kicked_atoms_one_step_per_call(form, large_kick_path):
    """calls of ONE step on the liquid: from the states s0, s1 the engine returns, per atom in longdouble, v1 = v0 + rM f0 + rM f1 and
    x1 == x0 + (v0 + rM f0) dt (mod L) within TAU times the sum of the magnitudes of the terms, and the counter increments of the step are what the rule
    decides from x0, v0, f0.  Pins the deferred second half-kick (pendingKick) in every state a reader can see."""
    case = wall_liquid()
    m = api.Model.from_case(case)
    sp = m.query("species").reshape(-1, 10)
    rM, mass, frozen = sp[:, 5].copy(), sp[:, 1].copy(), sp[:, 4] != 0
    types = np.asarray(case["types"])
    debug = (PLAIN2 if form == "plain2" else 0) | (DebugBit.DBG_LARGE_KICK_PATH if large_kick_path else 0)
    e = api.Engine(m, profile=1, debug=debug, sort_every=1 if form == "resort" else 0)
    if form == "plain2":
        e.step(8)                                                 # the look that opens the interval
    pack = lambda s: {"x": xyz(s), "v": xyz(s, ("vx", "vy", "vz")), "f": xyz(s, ("fx", "fy", "fz"))}
    s0, st0, sp0 = pack(e.state()), e.stats(), e.species_crossings()
    worst, plain, crossed, left_out = {"v": 0.0, "x": 0.0, "mom": 0.0}, 0, 0, 0
    for _ in range(12):
        e.reset_kernel_times()
        e.step(1)
        kt = {k: v["calls"] for k, v in e.kernel_times().items() if v["calls"] > 0}
        plain += kt.get("integrate1", 0)
        s1, st1, sp1 = pack(e.state()), e.stats(), e.species_crossings()
        r = wr.one_step_ld(s0, s1, types, rM, mass, frozen, case["box"], case["dt"])
        near = (r["margin"] < wr.MARGIN)
        dc = np.array(walls(st1, "Cross")) - np.array(walls(st0, "Cross"))
        dm = np.array(walls(st1, "Mom"), dtype=wr.LD) - np.array(walls(st0, "Mom"), dtype=wr.LD)
        scale = np.array(walls(st1, "Mom"), dtype=wr.LD)            # the slots accumulate: a sum of positive terms m |v|, rounded at its own magnitude
        rm = max([float(abs(dm[k] - r["mom"][k]) / (wr.LD(wr.TAU) * scale[k])) for k in range(6) if scale[k] > 0] or [0.0])
        worst = {"v": max(worst["v"], r["v"]), "x": max(worst["x"], r["x"]), "mom": max(worst["mom"], rm)}
        crossed += int(r["flags"].sum())
        left_out += int(near.any(1).sum())
        sure = r["flags"] & ~np.repeat(near, 2, 1)                   # crossings the reference is sure of; an atom within 1e-9 A of a wall may go either way
        slack = np.repeat(near.sum(0), 2)
        assert (np.abs(dc - sure.sum(0)) <= slack).all(), (form, st1["step"], dc, sure.sum(0), slack)
        assert np.array_equal((sp1 - sp0).sum(0), dc)
        if not near.any():
            assert rm <= 1.0, (form, st1["step"], rm)
        assert r["v"] <= 1.0 and r["x"] <= 1.0, (form, st1["step"], r["v"], r["x"])
        s0, st0, sp0 = s1, st1, sp1
    print("kicked atoms [%s%s]: v %.3e  x %.3e  mom %.3e  crossings %d  left out %d  plain steps %d" % (form, ", large kick path" if large_kick_path else "", worst["v"], worst["x"], worst["mom"], crossed, left_out, plain))
    assert crossed > 0 and left_out <= 0.01 * crossed
    if form == "plain2":
        assert plain >= 1 and st1["sort_interval"] > 1, (plain, st1)
    e.close()
