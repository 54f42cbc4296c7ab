"""One-byte pair-list entries (PairLists::entryBytes == 1: k_pair_list<..., EB = 1>, the narrow read-out of k_build_lists, ListStore::narrow_fits).

Where every cell keeps at most 255 candidates - one GPU, one wave per cell, the four-group tile - a list entry is a record number in a byte and a 1 KiB
chunk holds 16 iterations instead of 8.  The same entries are visited in the same order with the same arithmetic, so an engine with one-byte entries and
one held to 16 bits (DBG_WIDE_ENTRIES) must agree bit for bit: x, y, z, vx, vy, vz, fx, fy, fz, every entry of stats() and the per-species crossing
counters, after the same calls.  Both engines of a pair run with use_graph = 0 and per-kernel timing on; 'narrow_lists' counts the k_pair_list launches
that walked one-byte entries (no time of its own).

An engine goes narrow on two roads, and the patterns below take both: the first lists of its life are recorded behind a call (prepare_next_call) and
recorded again in the narrow format at once; or a step recorded them (DBG_FIXED_INTERVAL: the interval is known from the first step) and the look that
reads their report makes the NEXT rebuild record narrow ones.  Neither changes which steps rebuild.

What the numpy model (tests/list_model.py) says about the systems, asserted by the CPU test at the end: the FCC boxes keep at most 228 candidates per
cell and 45 % of their cells walk more than 16 iterations (a second chunk), the radiative box 140, the populations of tests/list_cases.py (cells of
1 ... 65 atoms: one, two and three slices ... 32 slices, lists of up to 123 iterations = 8 chunks) 127.
"""
import contextlib
import os

import numpy as np
import pytest

import list_cases as lc
import list_model as lm
import pair_cases as pc
from aztotmd_amd import api, inputs
from aztotmd_amd.api import DebugBit
from util import on_the_walls, wall_liquid

gpu = pytest.mark.gpu

WIDE = DebugBit.DBG_WIDE_ENTRIES
FOLD = DebugBit.DBG_FOLD_DRIFT | DebugBit.DBG_NO_FUSE_NEXT | DebugBit.DBG_LARGE_KICK_PATH       # the epilogue of the 1 M-atom runs (KICK_DRIFT)
FIXED = DebugBit.DBG_FIXED_INTERVAL
K = 4                                   # sort_every: a rebuild every fourth step at the most, so a few dozen steps hold many


@contextlib.contextmanager
def environment(extra):
    old = {k: os.environ.get(k) for k in extra}
    os.environ.update(extra)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def system(name):
    if name == "lj":                    # 8^3 FCC cells of 5.735 A at 85 K, one species: the one-species kernel
        return wall_liquid()
    if name == "two_species":           # the same box, two charged species, LJ + Fennell: the table-driven kernel
        return on_the_walls(inputs.lj_case((8, 8, 8), seed=75, vel_T=85.0, charges=(0.2, -0.2), elec="fenn"))
    if name == "radiative":             # the thermostat case of tests/test_gpu_fold_drift.py: k_pair_list<..., TSTAT>
        return inputs.lj_case((7, 7, 7), a=5.4, seed=82, rc=6.5, cell_list=6.9, T=200.0, tstat="radi", vel_T=150.0, radii=[(2.73, 4.731, 0.2)])
    raise KeyError(name)


def pair(case, debug=0, env=None, **kw):
    """(narrow, wide): the same engine twice, the second one with DBG_WIDE_ENTRIES"""
    kw.setdefault("use_graph", 0)
    with environment(env or {}):
        a = api.Engine(api.Model.from_case(case), debug=debug, **kw)
        b = api.Engine(api.Model.from_case(case), debug=debug | WIDE, **kw)
    for e in (a, b):
        e.set_profile(1)
    return a, b


def assert_same(a, b, what):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), (what, k, int((sa[k] != sb[k]).sum()))
    sta, stb = a.stats(), b.stats()
    assert sorted(sta) == sorted(stb)
    for k in sta:
        assert np.array_equal(np.asarray(sta[k]), np.asarray(stb[k]), equal_nan=True), (what, k, sta[k], stb[k])
    assert np.array_equal(a.species_crossings(), b.species_crossings()), what
    return sta


def calls_of(e, names=("pair_list", "narrow_lists", "build_lists", "pair_cleanup")):
    t = e.kernel_times()
    return {k: (t[k]["calls"] if k in t else 0) for k in names}


def run_pattern(a, b, pattern):
    both = (a, b)
    if pattern == "one_call":
        for e in both:
            e.step(60)
        return 60
    if pattern == "single_steps":       # every rebuild step is the last step of its call, and every call's last step books energies
        for _ in range(30):
            for e in both:
                e.step(1)
        return 30
    if pattern == "end_on_rebuild":     # DBG_FIXED_INTERVAL, sort_every = 4: steps 1, 5, 9, ... rebuild - each of these calls ends on one
        total = 0
        for n in (5, 4, 8, 4, 12):
            for e in both:
                e.step(n)
            total += n
            assert_same(a, b, (pattern, total))
        return total
    if pattern == "stats_between":      # the energies the last step of a call books, looked at after every call
        total = 0
        for n in (7, 33, 2, 18):
            for e in both:
                e.step(n)
            total += n
            assert_same(a, b, (pattern, total))
        return total
    raise KeyError(pattern)


PATTERNS = ["one_call", "single_steps", "end_on_rebuild", "stats_between"]
SYSTEMS = [("lj", 0), ("two_species", 0), ("lj", FOLD), ("two_species", FOLD), ("radiative", 0)]


@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name,debug", SYSTEMS, ids=["lj", "two_species", "lj_fold", "two_species_fold", "radiative"])
def test_narrow_and_wide_agree_bit_for_bit(name, debug, pattern):
    case = system(name)
    fixed = pattern == "end_on_rebuild"
    a, b = pair(case, debug=debug | (FIXED if fixed else 0), sort_every=K)
    total = run_pattern(a, b, pattern)
    st = assert_same(a, b, (name, pattern, "end"))
    assert st["step"] == total and st["sort_violations"] == 0 and st["pair_lists"] == 1 and st["cells_without_list"] == 0, st
    assert st["rebuilds"] >= total // 8, st                      # (several rebuilds fall inside)
    if fixed:
        assert st["sort_interval"] == K and st["rebuilds"] == 1 + (total - 1) // K, st
    assert calls_of(b)["narrow_lists"] == 0, calls_of(b)
    assert calls_of(a)["narrow_lists"] > 0, calls_of(a)
    # from here on every launch of the list kernel walks one-byte entries: plain steps and rebuild steps alike
    for e in (a, b):
        e.reset_kernel_times()
        e.step(2 * K + 1)
    ka, kb = calls_of(a), calls_of(b)
    assert ka["pair_list"] == 2 * K + 1 and ka["narrow_lists"] == ka["pair_list"] and ka["build_lists"] >= 2, ka
    assert kb["pair_list"] == 2 * K + 1 and kb["narrow_lists"] == 0 and kb["build_lists"] == ka["build_lists"], kb
    assert_same(a, b, (name, pattern, "after"))
    for e in (a, b):
        e.close()


@gpu
def test_lists_of_several_chunks():
    """tests/list_cases.py populations(): cells of 1 ... 65 atoms - 32 slices down to one per atom - whose lists run to 123 iterations, eight chunks of
    one-byte entries (the 65-atom cells keep no list in either engine: one wave serves 64 atoms).  Bit for bit against 16-bit entries, step by step."""
    c = lc.populations(1)
    kw = dict(pair_variant=2, skin=c["skin"], sort_every=c["K"], debug=FIXED, env=c["env"], **c["engine"])
    a, b = pair(c["case"], **kw)
    for step in range(1, c["steps"] + 9):
        for e in (a, b):
            e.step(1)
        st = assert_same(a, b, ("populations", step))
        assert st["pair_lists"] == 1 and st["sort_interval"] == c["K"] and st["sort_violations"] == 0, st
    ka, kb = calls_of(a), calls_of(b)
    # the step that recorded the first lists and the plain steps up to the next rebuild walked 16-bit entries; every one since, one-byte entries
    assert kb["narrow_lists"] == 0 and ka["pair_list"] == kb["pair_list"] == c["steps"] + 8, (ka, kb)
    assert ka["narrow_lists"] == ka["pair_list"] - c["K"], ka
    assert ka["pair_cleanup"] == kb["pair_cleanup"] > 0, (ka, kb)
    for e in (a, b):
        e.close()


def squeezed():
    """The smallest system that outgrows a byte in mid-run: 7 x 7 x 7 cells of 7.5 A (the geometry of tests/list_cases.py: rc 7, skin 0.4), 4 096 atoms of
    one Lennard-Jones species at rest on a jittered cubic lattice of 3.28 A - 120 to 238 kept candidates per cell, up to 257 staged - with eps = 1e-5 eV, so that nothing
    moves noticeably in a few steps whatever the distances.  `dense`: the same atoms with those within 16 A of the box centre drawn towards it by a factor
    0.78: twice the density there, from beyond the reach of the centre cell's atoms to inside it; the densest cell then stages 381 candidates, which the
    staging area sized on the lattice (384) still holds - so it is the record number, not the staging area, that the cell outgrows.  Numbers from the numpy model (asserted by the CPU test below): most kept candidates per cell 238 before, 299 after."""
    rng = np.random.Generator(np.random.PCG64(29))
    n, L = 16, 7 * lc.CELL
    a = L / n
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = np.round(np.mod((grid + 0.5) * a + rng.uniform(-0.25, 0.25, size=grid.shape), L), 6)
    N = len(pos)
    case = {"box": [L, L, L], "dt": lc.DT, "nsteps": 0, "species": [(lc.MASS, 0.0)], "names": ["A"], "vdw": [(0, 0, 1, lc.RC, [1e-5, lc.SIGMA])],
            "types": np.zeros(N, dtype=np.int32), "x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(),
            "vx": np.zeros(N), "vy": np.zeros(N), "vz": np.zeros(N), "elec_type": 0, "rReal": 0.0, "alpha": 0.0, "T": 0.0, "tstat_type": 0, "nEq": 0,
            "freqEq": 1, "use_clist": 1, "cell_list": lc.CELL, "center_box": 0, "init_forces": 1, "radii": None, "seed": 12345}
    d = pos - 0.5 * L
    r = np.sqrt((d * d).sum(1))
    dense = pos.copy()
    m = r < 16.0
    dense[m] = 0.5 * L + 0.78 * d[m]
    return dict(case=case, geom=lm.geometry([L, L, L], lc.RC, lc.CELL, lc.SKIN), pos=pos, dense=np.round(dense, 6), vdw={(0, 0): (1e-5, lc.SIGMA, lc.RC)})


@gpu
def test_a_cell_that_outgrows_a_byte_takes_the_engine_back_to_wide_entries():
    """`squeezed`: the engine records its first lists on the lattice (at most 238 kept candidates: one-byte entries, a tile of 256 records); then the caller
    sets the squeezed positions (set_state: the next step rebuilds).  The narrow builder records the cells that keep more than 255 candidates without a
    list (the clean-up launch serves them: exact), the look behind that call reads the report and takes the engine back to 16-bit entries for good - a
    larger tile, every cell listed.  Forces against the longdouble enumeration of tests/list_model.py at the engine's own positions, to the tolerance of
    tests/test_gpu_pair_lists.py, on every step; not bit for bit against a wide run: the clean-up launch sums in another order."""
    s = squeezed()
    g = s["geom"]
    e = api.Engine(api.Model.from_case(s["case"]), pair_variant=2, skin=lc.SKIN, sort_every=K, use_graph=0, profile=1)
    types = s["case"]["types"]

    def check(step):
        st, x = e.stats(), e.state()
        pos = np.stack([x["x"], x["y"], x["z"]], 1)
        F = np.stack([x["fx"], x["fy"], x["fz"]], 1)
        ref = lm.lj_forces(pos, types, g["box"], s["vdw"], g["r_max"])
        err = np.sqrt(((F - ref["F"]) ** 2).sum(1))
        tol = pc.TAU * ref["scale"]
        bad = np.flatnonzero(~(err <= tol))
        print("step %s: worst err / tol %.3g, cells without a list %d" % (step, float((err[tol > 0] / tol[tol > 0]).max()), st["cells_without_list"]))
        assert bad.size == 0, (step, bad[:6], err[bad[:6]], tol[bad[:6]])
        return st

    e.step(10)
    e.reset_kernel_times()
    e.step(6)
    k = calls_of(e)
    assert k["narrow_lists"] == k["pair_list"] == 6, k           # narrow, on the lattice
    st = check("lattice")
    assert st["pair_lists"] == 1 and st["cells_without_list"] == 0, st
    e.set_state(x=s["dense"][:, 0].copy(), y=s["dense"][:, 1].copy(), z=s["dense"][:, 2].copy())
    e.step(1)                                                     # rebuilds in the narrow format; the look behind the call goes wide
    check("squeezed, first step")
    for step in range(2, 2 * K + 3):
        e.reset_kernel_times()
        e.step(1)
        k = calls_of(e)
        st = check(step)
        assert k["pair_list"] == 1 and k["narrow_lists"] == 0, (step, k)          # wide from the look on ...
        assert st["pair_lists"] == 1 and st["cells_without_list"] == 0, (step, st)         # ... and nobody without a list
    e.reset_kernel_times()
    e.step(40)                                                    # ... for good: looks that find every cell listed do not flip it back
    k = calls_of(e)
    assert k["pair_list"] == 40 and k["narrow_lists"] == 0, k
    st = check("end")
    assert st["cells_without_list"] == 0 and st["pair_lists"] == 1, st
    e.close()


@gpu
def test_a_system_that_never_qualifies():
    """tests/list_cases.py wide_stencil: ~460 kept candidates per cell, two waves per cell (k_pair_list<..., MULTI>): never one-byte entries, and
    DBG_WIDE_ENTRIES changes nothing"""
    case = dict(lc.liquid("wide_stencil")["case"])
    a, b = pair(case, split=2)
    for n in (8, 17, 1, 22):
        for e in (a, b):
            e.step(n)
    st = assert_same(a, b, "wide_stencil")
    assert st["pair_lists"] == 1 and st["step"] == 48, st
    ka, kb = calls_of(a), calls_of(b)
    assert ka["narrow_lists"] == 0 and ka == kb and ka["pair_list"] > 0, (ka, kb)
    for e in (a, b):
        e.close()


def kept_and_iterations(pos, g):
    """per non-empty cell: candidates kept (hit by some atom of the cell; the larger of the two filter roundings) and list iterations"""
    kept, iters = [], []
    for rec in lm.Builder(pos, g).build().values():
        kept.append(max(int(rec["hits"][f].any(0).sum()) for f in (False, True)))
        n = len(rec["atoms"])
        if n <= 64:
            iters.append(int(np.ceil(max(int(rec["hits"][f].sum(1).max()) for f in (False, True)) / min(32, 64 // n))))
    return np.array(kept), np.array(iters)


def test_the_model_says_which_systems_fit_a_byte():
    """CPU: what the docstrings above say about the systems, from the numpy builder"""
    for name, rc, cell in (("lj", 8.5, 0.0), ("two_species", 8.5, 0.0), ("radiative", 6.5, 6.9)):
        c = system(name)
        kept, iters = kept_and_iterations(np.stack([c["x"], c["y"], c["z"]], 1), lm.geometry(c["box"], rc, cell, 0.0))
        assert kept.max() <= 255, (name, kept.max())
        if name != "radiative":
            assert (iters > 16).mean() > 0.3 and (iters <= 16).mean() > 0.3, (name, iters)      # both kinds of cell: with and without a second chunk
    c = lc.populations(1)
    for step in (1, 1 + c["K"], 1 + 2 * c["K"]):
        kept, iters = kept_and_iterations(c["positions"](step), c["geom"])
        assert kept.max() <= 255 and iters.max() > 7 * 16, (step, kept.max(), iters.max())
    s = squeezed()
    before, _ = kept_and_iterations(s["pos"], s["geom"])
    after, _ = kept_and_iterations(s["dense"], s["geom"])
    staged = [max(rec["n_cand"] for rec in lm.Builder(p, s["geom"]).build().values()) for p in (s["pos"], s["dense"])]
    print("squeezed: most kept candidates %d before, %d after; most staged %d before, %d after" % (before.max(), after.max(), staged[0], staged[1]))
    assert before.max() <= 255 and after.max() >= 270, (before.max(), after.max())
    # (ListStore::stage_records_for: the staging area sized on the lattice holds the squeezed cells)
    assert staged[1] <= ((staged[0] + staged[0] // 16 + 4 + 127) & ~127), staged
