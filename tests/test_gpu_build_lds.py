"""The list builder's LDS layout (k_build_lists, BuildLds in pair_list.hip.h): every group's matrix filter runs first and parks its hit masks, then every
group pops its hits into the bytes the tile held; DBG_HITS_BESIDE_TILE keeps the earlier layout - one group in flight, the hit array beside the tile.

The two layouts write the same candidates, headers and list chunks, so an engine of each must agree bit for bit after the same calls: x, y, z, vx, vy,
vz, fx, fy, fz, every entry of stats() and the per-species crossing counters - with one-byte and with 16-bit entries (DBG_WIDE_ENTRIES).  60 steps with
a rebuild every fourth step at the most, on:

lj            the 8^3-cell FCC box of 2 048 atoms at 85 K, the smallest that re-sorts lazily: cells of 4 atoms, one group;
populations   tests/list_cases.py: cells of 1 ... 65 atoms, so one, two, three and four groups per wave, with one and with four waves per cell;
wide_stencil  the 7 x 7 x 7 stencil at 85 K with one and with two waves per cell: a staging area of 768 candidates, whose entries wait in LDS with the hit array
              beside the tile (more than 512) and in registers with the new layout (up to 768); the first lists of an engine's life, which serve up to the second
              rebuild, are recorded with the staging area at the arrays' capacity, 1 024 candidates: entries in LDS in both layouts;
crowded       cells of ~23 atoms at 85 K: two groups everywhere;
sparse        the isolated pairs of tests/list_cases.py with lone atoms between them: empty cells, and cells whose atoms reach nobody (a list with T = 0).

The mask buffer holds the groups of the largest cell the engine has recorded.  `squeezed_slab` outgrows it in mid-run: the lattice of `squeezed`
(tests/test_gpu_narrow_lists.py) has cells of at most 27 atoms - two groups -; with the slab around x = L / 2 drawn together four cells hold 36.  Those cells keep no list for one recording (the
clean-up launch serves them), the look grows the buffer, and every cell is listed again; forces against the longdouble enumeration of tests/list_model.py
on every step.

Two waves per cell (split = 2) and the kinetic energy: the staging kernel then splits a cell over two workgroups, and the one that arrives last books the
cell's kinetic energy in its own partial-sum slot - two identical engines can differ in the last bit of engKin after a step that this kernel served (seen
on this suite's systems after an engine's first step, and where cells without a list go through the clean-up launch; nothing the builder touches).  So the
two-wave systems here are compared after calls whose last step walked lists with every cell listed: the first call is 8 steps long.

No CPU test of the layout itself: it exists only inside the kernel.  What the numpy model says about the systems (atoms per cell) is asserted on the CPU.
"""
import numpy as np
import pytest

import list_cases as lc
import list_model as lm
import pair_cases as pc
from aztotmd_amd import api, inputs
from aztotmd_amd.api import DebugBit
from test_gpu_narrow_lists import assert_same, calls_of, environment, squeezed
from util import wall_liquid

gpu = pytest.mark.gpu

BESIDE = DebugBit.DBG_HITS_BESIDE_TILE
WIDE = DebugBit.DBG_WIDE_ENTRIES
FIXED = DebugBit.DBG_FIXED_INTERVAL
K = 4
STEPS = 60


def sparse():
    """shell_pairs of tests/list_cases.py (18 x 18 x 15 cells, 162 two-atom groups: most cells are empty) plus 40 atoms at rest in the middle of cells
    that have nobody within 12 A: more than the list radius of 7.4 A plus what the pairs travel in 60 steps"""
    c = lc.shell_pairs()
    case = dict(c["case"])
    box = np.array(case["box"])
    pos = np.stack([case["x"], case["y"], case["z"]], 1)
    rng = np.random.Generator(np.random.PCG64(17))
    lone = []
    for cell in rng.permutation(18 * 18 * 15):
        p = (np.array([cell // (18 * 15), (cell // 15) % 18, cell % 15]) + 0.5) * lc.CELL
        d = np.concatenate([pos, np.array(lone).reshape(-1, 3)]) - p
        d -= box * np.round(d / box)
        if np.sqrt((d * d).sum(1)).min() > 12.0:
            lone.append(p)
        if len(lone) == 40:
            break
    lone = np.array(lone)
    n = len(lone)
    for k, col in zip(("x", "y", "z"), lone.T):
        case[k] = np.concatenate([case[k], col])
    for k in ("vx", "vy", "vz"):
        case[k] = np.concatenate([case[k], np.zeros(n)])
    case["types"] = np.concatenate([case["types"], np.zeros(n, dtype=np.int32)])
    return dict(case=case, n_lone=n, kw=dict(pair_variant=2, skin=c["skin"], sort_every=c["K"], debug=FIXED), env={})


def system(name):
    if name == "lj":
        return dict(case=wall_liquid(), kw=dict(sort_every=K), env={})
    if name in ("populations_w1", "populations_w4"):
        c = lc.populations(int(name[-1]))
        return dict(case=c["case"], kw=dict(pair_variant=2, skin=c["skin"], sort_every=c["K"], debug=FIXED, **c["engine"]), env=c["env"])
    if name in ("wide_stencil_w1", "wide_stencil_w2"):      # tests/list_cases.py liquid("wide_stencil") at 85 K
        case = inputs.lj_case((10, 10, 10), a=2.5, jitter=0.05, seed=62, rc=6.12, cell_list=2.75, vel_T=85.0)
        case["vdw"] = [(0, 0, 1, 6.12, [0.002, 1.9])]
        return dict(case=case, kw=dict(sort_every=K, split=int(name[-1])), env={})
    if name == "crowded":                                   # ... liquid("crowded") at 85 K
        return dict(case=inputs.lj_case((9, 9, 9), a=6.0, seed=63, rc=6.0, cell_list=10.5, vel_T=85.0), kw=dict(sort_every=K), env={})
    if name == "sparse":
        return sparse()
    raise KeyError(name)


SYSTEMS = ["lj", "populations_w1", "populations_w4", "wide_stencil_w1", "wide_stencil_w2", "crowded", "sparse"]


@gpu
@pytest.mark.parametrize("wide", [0, WIDE], ids=["narrow", "wide"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_both_layouts_agree_bit_for_bit(name, wide):
    s = system(name)
    kw = dict(s["kw"])
    debug = kw.pop("debug", 0) | wide
    kw.setdefault("use_graph", 0)
    kw.setdefault("profile", 1)
    with environment(s["env"]):
        a = api.Engine(api.Model.from_case(s["case"]), debug=debug, **kw)
        b = api.Engine(api.Model.from_case(s["case"]), debug=debug | BESIDE, **kw)
    total = 0
    for n in (8, 20, 32):
        for e in (a, b):
            e.step(n)
        total += n
        print(name, total, calls_of(a), "cells without a list", a.stats()["cells_without_list"], b.stats()["cells_without_list"])
        st = assert_same(a, b, (name, total))
    assert total == STEPS and st["step"] == STEPS and st["pair_lists"] == 1, st
    assert st["rebuilds"] >= 4, st                               # (several rebuilds fall inside)
    ka, kb = calls_of(a), calls_of(b)
    assert ka == kb and ka["build_lists"] >= 4 and ka["pair_list"] > 0, (ka, kb)
    if wide or "stencil" in name:
        assert ka["narrow_lists"] == 0, ka
    for e in (a, b):
        e.close()


def atoms_per_cell(pos, g):
    return np.array([len(rec["atoms"]) for rec in lm.Builder(pos, g).build().values()])


def squeezed_slab():
    """`squeezed` of tests/test_gpu_narrow_lists.py with another second state: the atoms within 16 A of the plane x = L / 2 drawn towards it by a factor 0.7
    along x only - four lattice planes per cell there instead of three at the most, 36 atoms in a cell instead of 27, at 1.4 times the density: 357
    candidates staged at the most, which the staging area sized on the lattice (384) holds, and 327 kept, which the tile sized on the lattice does not
    (numbers from the numpy model; the atoms per cell are asserted by the CPU test below)"""
    s = squeezed()
    L = s["case"]["box"][0]
    dense = s["pos"].copy()
    d = dense[:, 0] - 0.5 * L
    m = np.abs(d) < 16.0
    dense[m, 0] = 0.5 * L + 0.7 * d[m]
    s["dense"] = np.round(dense, 6)
    return s


@gpu
@pytest.mark.parametrize("wide", [0, WIDE], ids=["narrow", "wide"])
def test_a_cell_with_more_groups_than_the_mask_buffer_holds(wide):
    """`squeezed_slab`: first lists on the lattice (cells of at most 27 atoms: the buffer is sized for two groups), then the caller sets the squeezed positions
    (set_state: the next step rebuilds).  The cells of more than 32 atoms are recorded without a list - the clean-up launch serves them: exact -, the look
    behind that call grows the buffer, and from the next rebuild on every cell is listed.  Forces against the longdouble enumeration at the engine's own
    positions, to the tolerance of tests/test_gpu_pair_lists.py, on every step."""
    s = squeezed_slab()
    g = s["geom"]
    over = int((atoms_per_cell(s["dense"], g) > 32).sum())
    e = api.Engine(api.Model.from_case(s["case"]), pair_variant=2, skin=lc.SKIN, sort_every=K, use_graph=0, profile=1, debug=wide)
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

    e.step(16)
    st = check("lattice")
    assert st["pair_lists"] == 1 and st["cells_without_list"] == 0, st
    e.set_state(x=s["dense"][:, 0].copy(), y=s["dense"][:, 1].copy(), z=s["dense"][:, 2].copy())
    e.step(1)                                                     # rebuilds with the buffer sized on the lattice
    st = check("squeezed, first step")
    for step in range(2, 3 * K + 3):
        e.step(1)
        st = check(step)
    assert st["pair_lists"] == 1 and st["cells_without_list"] == 0, st        # the buffer has grown: nobody without a list
    e.step(40)
    st = check("end")
    assert st["pair_lists"] == 1 and st["cells_without_list"] == 0 and over > 0, (st, over)
    e.close()


def test_the_model_says_how_many_groups_the_cells_hold():
    """CPU: what the docstrings above say about the systems' cells, from the numpy builder"""
    s = squeezed_slab()
    before, after = atoms_per_cell(s["pos"], s["geom"]), atoms_per_cell(s["dense"], s["geom"])
    print("squeezed_slab: most atoms per cell %d before, %d after" % (before.max(), after.max()))
    assert 16 < before.max() <= 31 and 32 < after.max() <= 64, (before.max(), after.max())
    c = lc.populations(1)
    n = atoms_per_cell(c["positions"](1), c["geom"])
    assert {1, 2, 3, 4} <= set(((n[n <= 64] + 15) // 16).tolist()) and n.max() == 65, sorted(set(n.tolist()))
    sp = sparse()
    assert sp["n_lone"] == 40
