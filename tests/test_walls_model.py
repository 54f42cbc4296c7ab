"""CPU side of the wall tests: the designed gas of tests/wall_cases.py holds what it promises, the exact reference of tests/wall_reference.py and the
CPU oracle agree on it within every bound, and the float64 restatement of the kernels' rule is caught by the designed classes when it is mutated.
tests/test_gpu_walls.py holds the HIP kernels to the same reference with the same bounds."""
import numpy as np
import pytest

import wall_cases as wc
import wall_reference as wr
from aztotmd_amd import api
from oracle import oracle
from util import wall_liquid

CALLS = (1, 4, 7)
_C = {}


def ref_run(variant, rule, rebuild=None, fold=False):
    key = (variant, rule, rebuild, fold)
    if key not in _C:
        g = wc.build()
        _C[key] = wr.run(g["x"], wc.velocities(variant), g["types"], wc.NSTEPS, rule, set(rebuild) if rebuild else None, fold)
    return _C[key]


def species_table():
    if "sp" not in _C:
        sp = api.Model.from_case(wc.case()).query("species").reshape(-1, 10)
        _C["sp"] = (sp[:, 5].copy(), sp[:, 1].copy(), sp[:, 4] != 0)          # rMass_hdt, mass, frozen
    return _C["sp"]


def test_the_box_and_the_classes_are_what_the_design_says():
    ints = wc.check_box()
    print("int(nextafter(2 L, 0) * (1 / L)) per box length:", ints)
    g = wc.build()
    assert g["N"] % 2 == 1 and 2800 < g["N"] < 3400
    assert np.array_equal(wc.masses(), species_table()[1]) and list(species_table()[2]) == [False, False, True]
    assert (np.abs(g["v"][g["types"] == 2]).max(1) > 0).all(), "the frozen species is given velocities"
    cc = wc.class_counts()
    for ax in range(3):
        for sp in (0, 1):
            for c, sides in (("cross", (0, 1)), ("stay", (0, 1)), ("land0", (0,)), ("landL", (1,)), ("startL", (1,)), ("ulp", (0, 1)), ("corner", (0, 1))):
                for sd in sides:
                    assert cc.get((c, ax, sd, sp), 0) > 0, (c, ax, sd, sp)
        for sd in (0, 1):
            assert cc.get(("frozen", ax, sd, 2), 0) > 0, ("frozen", ax, sd)
    first = ref_run("plain", "every")[wc.BLOCK_STEP]
    walls = first["flags"].sum(1)
    print("atoms crossing 1 / 2 / 3 walls in step %d: %d / %d / %d" % (wc.BLOCK_STEP, (walls == 1).sum(), (walls == 2).sum(), (walls == 3).sum()))
    every = np.array([st["flags"].sum(1) for st in ref_run("plain", "every")[1:]])
    assert (every == 2).any() and (every == 3).any(), "corners cross two and three walls in one step"
    assert sum(g["jump"] != "") == 12 and set(g["jump"][g["jump"] != ""]) == set(wc.JUMP_KINDS)


def test_the_gas_is_force_free_and_its_designed_chains_are_exact():
    g = wc.build()
    for variant in ("plain", "jump"):
        v = wc.velocities(variant)
        steps = ref_run(variant, "every")
        slow = np.ones(g["N"], dtype=bool) if variant == "plain" else (g["jump"] == "")
        travel = float(np.abs(v[slow] * wc.DT).sum(1).max()) * wc.NSTEPS
        dmin = wc.min_distance(g["x"][slow])
        print("%s: smallest distance %.4f A, longest travel in %d steps %.4f A" % (variant, dmin, wc.NSTEPS, travel))
        assert dmin > wc.RC + 2.0 * travel + 0.05
        assert travel < 0.04, "the lazy schedule must be able to keep its cells"
        box = np.array(wc.BOX)
        for i in np.flatnonzero(~slow):                           # the jump atoms, wherever they land
            for st in steps:
                d = st["wrapped"] - st["wrapped"][i]
                d -= box * np.round(d / box)
                r = np.sqrt((d * d).sum(1))
                r[i] = np.inf
                assert r.min() > wc.RC + 0.1, (variant, i, r.min())
        # exactness: the float64 chain x += v dt, evaluated literally, IS the exact chain on every designed coordinate
        ex = wc.exact_axes(variant)
        frozen = np.array(wc.FROZEN, dtype=bool)[g["types"]]
        x = g["x"].copy()
        for s in range(1, wc.NSTEPS + 1):
            x = x + np.where(frozen[:, None], 0.0, v * wc.DT)
            same = np.array([[int(a) == int(b) for a, b in zip(ra, rb)] for ra, rb in zip(wr.to_int(x), steps[s]["unwrapped"])])
            assert same[ex].all(), (variant, s, np.argwhere(~same & ex)[:5])
        tie_by_design = ex | (wc.pinned_axes() if variant == "jump" else False)
        assert wr.undecided(steps, tie_by_design) == [], "a generic atom within 1e-9 A of a wall decision"
        if variant == "plain":
            assert wr.undecided(ref_run(variant, "image", (1,), True), ex) == []


@pytest.mark.parametrize("cell", [wc.CELL_COARSE, wc.CELL_FINE])
def test_every_layout_occurs_on_both_grids(cell):
    for rule, rebuild, fold in (("every", None, False), ("image", (1,), True)):
        dims = wc.grid_dims(cell, lazy=rule == "image")
        assert dims == wc.N_CELLS[(cell, rule == "image")]
        n = dims[0] * dims[1] * dims[2]
        if cell == wc.CELL_FINE:
            assert n > 16384 and n % 4 != 0 and n % 1024 != 0, n
        else:
            assert n <= 16384, n
        steps = ref_run("plain", rule, rebuild, fold)
        counts = wc.layout_counts(steps, dims, None if rule == "every" else set(rebuild))
        print(dims, rule, counts)
        for k, val in counts.items():
            assert val > 0, (dims, rule, k)
        for lo, hi in wc.populated_wall_layers(steps[0]["wrapped"], dims):
            assert lo > 0 and hi > 0
    order, _ = wc.sorted_order(ref_run("plain", "image", (1,), True)[1]["wrapped"], dims)
    g = wc.build()
    assert tuple(g["site_of_id"][order[-1]]) == (0, 0, 0), "the last atom of the sorted order is the corner atom inside the three upper walls"


def test_the_two_tie_rules_differ_where_the_design_says():
    """an atom that lands exactly on L and moves on: never counted by the every-step rule, counted one step later by the image rule"""
    g = wc.build()
    a, b = ref_run("plain", "every"), ref_run("plain", "image", (1,), True)
    diff = a[-1]["cnt"] - b[-1]["cnt"]
    landL = (g["cls"] == "landL") & (g["when"] < wc.NSTEPS) & (g["when"] > 1)
    startL_out, startL_in = (g["cls"] == "startL") & (g["when"] == 1), (g["cls"] == "startL") & (g["when"] == 0)
    print("every-step minus image rule, per wall:", diff, " landL atoms that move on:", landL.sum(0), " startL outward / inward:", startL_out.sum(0), startL_in.sum(0))
    for ax in range(3):
        # an atom that STARTS on L: the initial force call of a lazy engine has set it to 0.0 (counting nothing), so moving inward it crosses the lower wall
        # in step 1 and moving outward it crosses none; the every-step engine keeps L, counts the outward one in step 1 and the inward one never
        assert diff[2 * ax] == -startL_in[:, ax].sum()
        # ... and the landL atoms are counted by the image rule one step after they land
        assert diff[2 * ax + 1] == startL_out[:, ax].sum() - landL[:, ax].sum()
    assert landL.sum() > 0 and startL_out.sum() > 0 and startL_in.sum() > 0


def oracle_calls(variant):
    o = oracle.Oracle(wc.case(variant))                          # (no force call: the cell binning of the oracle does not take x == L; the forces are 0 anyway)
    out, done = [], 0
    for n in CALLS:
        o.step(n)
        done += n
        s, st = o.state(), o.stats()
        out.append((done, s, st, o.species_crossings()))
    return out


@pytest.mark.parametrize("variant", ["plain", "jump"])
def test_the_cpu_oracle_stays_within_every_bound(variant):
    g = wc.build()
    steps = ref_run(variant, "every")
    ex = wc.exact_axes(variant)
    v = wc.velocities(variant)
    for done, s, st, spec in oracle_calls(variant):
        ref = steps[done]
        x = np.stack([s["x"], s["y"], s["z"]], 1)
        assert all((s[k] == 0.0).all() for k in ("fx", "fy", "fz"))
        assert np.array_equal(np.stack([s["vx"], s["vy"], s["vz"]], 1), v)
        rx, unequal = wr.position_ratio(x, ref, ex)
        cross = [st["cross"][k] for k in range(6)]
        mom = [st["momXn"], st["momXp"], st["momYn"], st["momYp"], st["momZn"], st["momZp"]]
        rm = wr.momentum_ratio(mom, ref)
        print("oracle [%s] after %2d steps: x %.3e  mom %.3e  exact coordinates not equal %d  crossings %s" % (variant, done, rx, rm, unequal, cross))
        assert rx <= 1.0 and rm <= 1.0 and unequal == 0
        assert cross == list(ref["cnt"]) and np.array_equal(spec, ref["spec"]) and list(spec.sum(0)) == cross
        assert (x >= 0).all() and (x < np.array(wc.BOX)).all() or variant == "jump"
        pinned = wc.pinned_axes() if variant == "jump" else np.zeros_like(ex)
        for dims in set(wc.N_CELLS.values()):                        # the cell of every atom
            assert np.array_equal(wr.cells(np.where(pinned, ref["wrapped"], x), dims), wr.cells(ref["wrapped"], dims)), (variant, done, dims)


def restated(rule, body, dims, mutate=None, variant="plain"):
    """the float64 restatement through NSTEPS steps on the launch order of `dims`: per step (x reported, cumulative cnt, mom, spec, flags)"""
    g = wc.build()
    rM, m, frozen = species_table()
    x, v, f = g["x"].copy(), wc.velocities(variant), np.zeros((g["N"], 3))
    box = np.array(wc.BOX)
    if rule == "image":
        x = np.where(x >= box, 0.0, x)                            # the initial force call of a lazy engine
    order, _ = wc.sorted_order(x, dims)
    cnt, mom, spec, out = np.zeros(6, dtype=np.int64), np.zeros(6), np.zeros((3, 6), dtype=np.int64), []
    for s in range(1, wc.NSTEPS + 1):
        wrap = rule == "every" or s == 1
        x, _, c, p, sp = wr.kernel_step(x, v, f, g["types"], rM, m, frozen, order, wrap, body if not wrap else "one", mutate=mutate)
        cnt, mom, spec = cnt + c, mom + p, spec + sp
        rep = x.copy()
        for ax in range(3):
            rep[:, ax] = wr._wrap_fp(x[:, ax], box[ax], 1.0 / box[ax])
        if wrap:
            order, _ = wc.sorted_order(x, dims)
        out.append((rep, cnt.copy(), mom.copy(), spec.copy()))
    return out


def judge(got, ref_steps, exact):
    """the checks of the GPU test, on a restated run: list of (step, what failed)"""
    failed = []
    for s, (x, cnt, mom, spec) in enumerate(got, start=1):
        ref = ref_steps[s]
        rx, unequal = wr.position_ratio(x, ref, exact)
        if rx > 1.0 or unequal:
            failed.append((s, "position"))
        if list(cnt) != list(ref["cnt"]):
            failed.append((s, "counts"))
        if not np.array_equal(spec, ref["spec"]) or list(spec.sum(0)) != list(cnt):
            failed.append((s, "species counts"))
        try:
            if wr.momentum_ratio(mom, ref) > 1.0:
                failed.append((s, "momentum"))
        except AssertionError:
            failed.append((s, "momentum of a wall nobody crossed"))
    return failed


SCHEDULES = {"every": ("every", None, False, "one"), "lazy": ("image", (1,), True, "two")}


@pytest.mark.parametrize("schedule", ["every", "lazy"])
def test_the_restated_rule_is_the_reference(schedule):
    rule, rebuild, fold, body = SCHEDULES[schedule]
    ref = ref_run("plain", rule, rebuild, fold)
    assert judge(restated(rule, body, wc.grid_dims(wc.CELL_COARSE)), ref, wc.exact_axes()) == []


@pytest.mark.parametrize("mutate", [m for m in wr.MUTATIONS if m != "momentum_before_the_kick"])
def test_a_mutated_rule_is_caught(mutate):
    """each mutation of the restated rule fails at least one check of at least one schedule; the structural ones exactly where their structure exists"""
    caught = {}
    for schedule, (rule, rebuild, fold, body) in SCHEDULES.items():
        ref = ref_run("plain", rule, rebuild, fold)
        caught[schedule] = judge(restated(rule, body, wc.grid_dims(wc.CELL_COARSE), mutate), ref, wc.exact_axes())
    print(mutate, {k: sorted(set(w for _, w in v)) for k, v in caught.items()})
    if mutate == "second_atom_of_a_pair_lost":
        assert caught["lazy"] and not caught["every"]
    else:
        assert caught["every"] and caught["lazy"], caught


def test_momentum_before_the_kick_is_caught():
    """the gas is force-free, so this mutation needs forces: one step of the designed atoms with a kick of a thousandth of their velocity, the momenta
    against the longdouble statement of the same step"""
    g = wc.build()
    rM, m, frozen = species_table()
    x, v = g["x"].copy(), wc.velocities()
    x = np.where(x >= np.array(wc.BOX), 0.0, x)
    f = 1e-3 * v / rM[g["types"]][:, None]
    order, _ = wc.sorted_order(x, wc.grid_dims(wc.CELL_COARSE))
    res = {}
    for mutate in (None, "momentum_before_the_kick"):
        x1, v1, cnt, mom, spec = wr.kernel_step(x, v, f, g["types"], rM, m, frozen, order, True, mutate=mutate)
        ref = wr.one_step_ld({"x": x, "v": v, "f": f}, {"x": x1, "v": v1, "f": np.zeros_like(f)}, g["types"], rM, m, frozen, wc.BOX, wc.DT)
        assert ref["v"] <= 1.0 and ref["x"] <= 1.0 and (ref["margin"][~wc.exact_axes()] > wr.MARGIN).all()
        assert list(cnt) == list(ref["flags"].sum(0)) and cnt.sum() > 10
        res[mutate] = max(abs(float(mom[k]) - float(ref["mom"][k])) / (wr.TAU * float(ref["mom_scale"][k])) for k in range(6) if cnt[k])
    print("momentum err / (TAU scale): restated %.3e, mutated %.3e" % (res[None], res["momentum_before_the_kick"]))
    assert res[None] <= 1.0 < res["momentum_before_the_kick"]


def test_kicked_atoms_of_the_oracle_on_the_wall_plane_liquid():
    """the one-step identities the GPU test asserts on the liquid, on the CPU oracle first: v1 = v0 + rM f0 + rM f1, x1 == x0 + (v0 + rM f0) dt (mod L), the
    counter increments decided from (x0, v0, f0), and at most 1 % of the crossing atoms within 1e-9 A of a wall"""
    case = wall_liquid()
    sp = api.Model.from_case(case).query("species").reshape(-1, 10)
    rM, mass, frozen = sp[:, 5].copy(), sp[:, 1].copy(), sp[:, 4] != 0
    types = np.asarray(case["types"])
    o = oracle.Oracle(case)
    o.forces(1)
    pack = lambda s: {"x": np.stack([s["x"], s["y"], s["z"]], 1), "v": np.stack([s["vx"], s["vy"], s["vz"]], 1), "f": np.stack([s["fx"], s["fy"], s["fz"]], 1)}
    s0, c0 = pack(o.state()), np.array(o.stats()["cross"])
    crossed = left_out = 0
    worst = {"v": 0.0, "x": 0.0}
    for _ in range(12):
        o.step(1)
        s1, c1 = pack(o.state()), np.array(o.stats()["cross"])
        r = wr.one_step_ld(s0, s1, types, rM, mass, frozen, case["box"], case["dt"])
        near = r["margin"] < wr.MARGIN
        crossed += int(r["flags"].sum())
        left_out += int(near.any(1).sum())
        if not near.any():
            assert list(c1 - c0) == list(r["flags"].sum(0))
        worst = {k: max(worst[k], r[k]) for k in worst}
        s0, c0 = s1, c1
    print("oracle on the liquid: v %.3e  x %.3e  crossings %d  left out %d" % (worst["v"], worst["x"], crossed, left_out))
    assert worst["v"] <= 1.0 and worst["x"] <= 1.0 and crossed > 0 and left_out <= 0.01 * crossed
