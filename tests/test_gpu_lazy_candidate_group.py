"""The fourth candidate group of k_pair_list, asked for only where it holds a candidate (kLazyLast, csrc/pair_list.hip.h).

A wave of the one-wave, four-group kernels loads the entries of its fourth group of 64 candidates - and their coordinates - only if the list header says
T > 192; otherwise records 193 and up of its tile stay unwritten, which is sound as long as no list entry of such a cell names them.  The 2 048-atom box
of tests/test_gpu_fold_kick.py with a skin of 0.4 A keeps 162 to 249 candidates per cell (the numpy builder of tests/list_model.py, asserted here): waves
that ask for the group and waves that do not, in one launch.  Forces against the longdouble enumeration of all pairs within the cut-off at the engine's own
positions, to the tolerance of tests/test_gpu_pair_lists.py (|F_gpu - F_ref| <= TAU sum S_F r per atom): a lost candidate is a whole pair term missing.
On the first step, where both stand on the same positions, also against an engine that keeps no lists (DBG_NO_LISTS: every cell staged), to twice that
tolerance - each of the two is within it of the exact forces.  With one-byte and with 16-bit list entries (both kernels gather four groups).
"""
import numpy as np
import pytest

import list_cases as lc
import list_model as lm
import pair_cases as pc
from aztotmd_amd import api
from aztotmd_amd.api import DebugBit
from util import wall_liquid

pytestmark = pytest.mark.gpu

FIXED = DebugBit.DBG_FIXED_INTERVAL


@pytest.mark.parametrize("wide", [0, DebugBit.DBG_WIDE_ENTRIES], ids=["narrow", "wide"])
def test_a_skipped_fourth_group_loses_no_pair(wide):
    case = wall_liquid()
    _, _, _, rc, (eps, sigma) = case["vdw"][0]
    g = lm.geometry(case["box"], rc, case["cell_list"], lc.SKIN)
    pos0 = np.stack([case["x"], case["y"], case["z"]], 1)
    kept = np.array([int(rec["hits"][True].any(0).sum()) for rec in lm.Builder(pos0, g).build().values()])
    print("kept candidates per cell: %d .. %d, %d cells above 192, %d at or below" % (kept.min(), kept.max(), (kept > 192).sum(), (kept <= 192).sum()))
    assert (kept > 192).sum() >= 10 and (kept <= 192).sum() >= 10 and kept.max() <= 255, kept
    kw = dict(pair_variant=2, profile=1, skin=lc.SKIN, sort_every=4, use_graph=0)
    e = api.Engine(api.Model.from_case(case), debug=FIXED | wide, **kw)
    r = api.Engine(api.Model.from_case(case), debug=FIXED | wide | DebugBit.DBG_NO_LISTS, **kw)
    types = np.asarray(case["types"])
    for step in (1, 18, 19, 20):
        if step == 18:
            for x in (e, r):
                x.step(16)          # the first look: the capacities follow what the builder reported, one-byte entries from the next rebuild on
        e.reset_kernel_times()
        for x in (e, r):
            x.step(1)
        ran = {k for k, v in e.kernel_times().items() if v["calls"] > 0}
        assert "pair_list" in ran and "pair_tile" not in ran and e.stats()["cells_without_list"] == 0, (step, ran)
        if step > 1:
            assert "pair_cleanup" not in ran and ("narrow_lists" in ran) == (not wide), (step, ran)        # (one-byte entries: the four-group kernel for certain)
        s, sr = e.state(), r.state()
        same = all(np.array_equal(s[k], sr[k]) for k in ("x", "y", "z"))       # (the two add a force's terms in different orders: from the second step on the positions differ in their last bits)
        assert same or step > 1, step
        p = np.stack([s["x"], s["y"], s["z"]], 1)
        F, Fr = np.stack([s["fx"], s["fy"], s["fz"]], 1), np.stack([sr["fx"], sr["fy"], sr["fz"]], 1)
        ref = lm.lj_forces(p, types, g["box"], {(0, 0): (eps, sigma, rc)}, g["r_max"])
        tol = pc.TAU * ref["scale"]
        err, diff = np.sqrt(((F - ref["F"]) ** 2).sum(1)), np.sqrt(((F - Fr) ** 2).sum(1))
        print("step %d: worst err / tol %.3g, worst difference from the engine without lists / tol %.3g" % (step, float((err / tol).max()), float((diff / tol).max())))
        assert (err <= tol).all(), (step, np.flatnonzero(~(err <= tol))[:6])
        if same:
            assert (diff <= 2.0 * tol).all(), (step, np.flatnonzero(~(diff <= 2.0 * tol))[:6])
    for x in (e, r):
        x.close()
