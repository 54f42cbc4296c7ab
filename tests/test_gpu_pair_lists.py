"""The pair-list builder (k_build_lists) through the forces of the steps that trust its lists (k_pair_list), atom by atom against an exact enumeration.

A pair the builder lost in the shell between rMax and the list radius rMax + 2 slack is invisible while nothing moves.  Here chosen pairs sit in
that shell at a rebuild and approach afterwards, each atom moving less than slack (tests/list_cases.py): once such a pair is inside rMax, a lost
pair is a whole pair term missing from two atoms.  Every step of at least two intervals is compared with the longdouble enumeration of all pairs
within their cut-off at the positions state() returns (tests/list_model.py lj_forces):
    |F_gpu - F_ref| <= TAU sum_j S_F,ij r_ij         per atom (TAU: pair_cases.py, S_F: the condition scale of pair_reference.py),
filler atoms (no potential) feel exactly nothing, a shell pair's atoms feel exactly nothing while the pair is outside rMax and exactly the pair
term from the first step inside.  The engine runs with pair_variant 2, DBG_FIXED_INTERVAL and sort_every = K, one step per call; the kernel timers and
the statistics say which steps rebuilt, that plain steps walked the lists (pair_list, never pair_tile), and where the clean-up launch served cells
without a list.  Pairs that start deeper than 95 % of the shell cannot reach rMax without a displacement violation (an atom may move slack at the
most): they are harmless by construction and not what this test can see.

tests/test_list_model.py (CPU) holds the cases, the restated builder and the fp64 oracle to the same numbers first.
"""
import contextlib
import os

import numpy as np
import pytest

import list_cases as lc
import list_model as lm
import pair_cases as pc
from aztotmd_amd import api
from aztotmd_amd.api import DebugBit

pytestmark = pytest.mark.gpu


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


def make_engine(c, every_step=False):
    kw = dict(pair_variant=2, profile=1, skin=c["skin"], **c["engine"])
    if every_step:
        kw.update(sort_every=1)
    else:
        kw.update(sort_every=c["K"], debug=DebugBit.DBG_FIXED_INTERVAL)
    with environment(c["env"]):
        return api.Engine(api.Model.from_case(c["case"]), **kw)


def describe(c, step, atom, pos, ref, at_rebuild, g):
    """(case, step, atom id, cell, partner id, distance at the last rebuild, distance now) for the atom's partners inside the cut-off"""
    cell = int(lm.cell_index(lm.cell_coords(pos[atom:atom + 1], g), g)[0])
    out = []
    for a, b in ((ref["i"], ref["j"]), (ref["j"], ref["i"])):
        for k in np.flatnonzero(a == atom)[:4]:
            p = int(b[k])
            d0 = lm.min_image(at_rebuild[atom] - at_rebuild[p], g["box"])
            out.append((c["name"], step, int(atom), cell, p, float(np.sqrt((d0 * d0).sum())), float(np.sqrt(ref["r2"][k]))))
    return out or [(c["name"], step, int(atom), cell, None, None, None)]


def run_case(c, every_step=False):
    """one step per call; returns the worst err / (TAU sum S_F r) seen"""
    g, K = c["geom"], c["K"]
    lists = g["lazy"] and not every_step
    e = make_engine(c, every_step)
    types = c["case"]["types"]
    P = c["pairs"]
    worst, rebuilds, at_rebuild, rebuilt_at = 0.0, e.stats()["rebuilds"], None, []
    inside_before = None
    for step in range(1, c["steps"] + 1):
        e.reset_kernel_times()
        e.step(1)
        ran = {k for k, v in e.kernel_times().items() if v["calls"] > 0}
        st, s = e.stats(), e.state()
        pos = np.stack([s["x"], s["y"], s["z"]], 1)
        F = np.stack([s["fx"], s["fy"], s["fz"]], 1)
        # ---- what the engine says about itself
        assert st["step"] == step and st["sort_violations"] == 0, (c["name"], step, st)
        assert st["n_cells"] == g["n_cells"] and abs(st["skin"] - (g["skin"] if lists else 0.0)) <= 1e-12, (c["name"], st["n_cells"], st["skin"], g["skin"])
        rebuilt = st["rebuilds"] > rebuilds
        rebuilds = st["rebuilds"]
        if rebuilt:
            at_rebuild = pos
            rebuilt_at.append(step)
        if lists:
            assert st["pair_lists"] == 1 and st["sort_interval"] == K, (c["name"], step, st)
            assert rebuilt == ((step - 1) % K == 0), (c["name"], step, rebuilt_at)
            assert ("build_lists" in ran) == rebuilt, (c["name"], step, ran)
            assert "pair_list" in ran and "pair_tile" not in ran, (c["name"], step, ran)
            if c["unlisted"]:
                assert st["cells_without_list"] == int((lm.populations(at_rebuild, g) > 64 * c.get("waves", 1)).sum()) > 0, (c["name"], step, st)
                assert "pair_cleanup" in ran, (c["name"], step, ran)
            else:
                assert st["cells_without_list"] == 0, (c["name"], step, st)
                # (an engine's first look is spent with the clean-up launch in place; from then on nothing asks for it)
                assert step <= 2 or "pair_cleanup" not in ran, (c["name"], step, ran)
        else:
            assert st["pair_lists"] == 0 and rebuilt and "pair_tile" in ran and "pair_list" not in ran, (c["name"], step, st, ran)
        # ---- forces, atom by atom
        ref = lm.lj_forces(pos, types, g["box"], c["vdw"], g["r_max"])
        assert ref["near"] == 0, (c["name"], step)
        err = np.sqrt(((F - ref["F"]) ** 2).sum(1))
        tol = pc.TAU * ref["scale"]
        bad = np.flatnonzero(~(err <= tol))
        assert bad.size == 0, [describe(c, step, a, pos, ref, at_rebuild, g) + [float(err[a]), float(tol[a])] for a in bad[:6]]
        has = ref["scale"] > 0
        if has.any():
            worst = max(worst, float((err[has] / tol[has]).max()))
        assert (F[types != 0] == 0.0).all(), (c["name"], step)
        if P is not None:
            d = lm.min_image(pos[P["i"]].astype(np.longdouble) - pos[P["j"]].astype(np.longdouble), g["box"])
            inside = (d * d).sum(1) <= np.longdouble(g["r_max"]) ** 2
            for a in (P["i"], P["j"]):
                out = np.flatnonzero(~inside & (F[a] != 0.0).any(1))
                assert out.size == 0, (c["name"], step, a[out][:6])
                lost = np.flatnonzero(inside & (F[a] == 0.0).all(1))
                assert lost.size == 0, [describe(c, step, x, pos, ref, at_rebuild, g) for x in a[lost][:6]]
            if lists and rebuilt:                  # in exact arithmetic on the engine's own states: in the shell at its rebuild ...
                grp = rebuilt_at.index(step)
                m = P["group"] == grp
                r = np.sqrt((d * d).sum(1))
                assert grp > 1 or ((r[m] > g["r_max"]) & (r[m] <= g["r_list"])).all(), (c["name"], step, grp)
                assert grp > 1 or (((r[m] - g["r_max"]) / (2 * g["slack"]) >= 0.9).sum() >= 6)
            if lists and step % K == 0:            # ... and inside rMax on the interval's last plain step
                assert inside[P["group"] == step // K - 1].all(), (c["name"], step)
            if inside_before is not None:
                assert (inside | ~inside_before).all()        # (nobody leaves again: the pairs only approach)
            inside_before = inside
    print("%s%s: %d steps, rebuilt at %s, worst err / (TAU sum S_F r) = %.3g" % (c["name"], " (every step)" if every_step else "", c["steps"], rebuilt_at, worst))
    return worst


def test_shell_pairs_across_the_skin():
    run_case(lc.shell_pairs())


def test_shell_pairs_with_the_cells_rebuilt_every_step():
    """the same system served by the staging kernel on every step: a failure above belongs to the lists, not to the case"""
    run_case(lc.shell_pairs(), every_step=True)


@pytest.mark.parametrize("waves", [1, 4])
def test_cell_populations_at_the_builders_block_edges(waves):
    """populations 1 ... 65 of the tested atom's cell (groups of 16 atoms, 64 atoms per wave); one wave per cell: the 65-atom cells keep no list and the
    clean-up launch serves them to the same tolerance; four waves per cell share a cell of up to 256 atoms"""
    run_case(lc.populations(waves))


@pytest.mark.parametrize("kind", lc.LIQUIDS)
def test_liquids_atom_by_atom(kind):
    """many pairs cross rMax inwards and outwards inside every interval; 'three_cells': fewer than five cells on an axis - no lists, the staging kernel
    serves every step (asserted), held to the same enumeration"""
    run_case(lc.liquid(kind))
