"""Every pair-force kernel body, pair by pair, and the bond and angle kernel, atom by atom, against the high-precision reference
(tests/pair_reference.py, committed as tests/golden/pair_functions.npz together with the coordinates of the systems; this file needs numpy only).

The systems are isolated pairs (tests/pair_cases.py): each atom's force is ONE pair term, so every pair is held to |F_gpu - F_ref| <= tau S_F r
(S_F: condition scale of f = -(1/r) dU/dr), every pair that f^2 > 1e10 drops has exactly zero force and is counted, Newton's third law holds bit for
bit, and the VdW and Coulomb energies match the sums of the per-pair energies within tau sum(S_E) each.  Each case goes through every kernel path
that serves it, and the test asserts from the kernel timers that the path really ran:
  atom     pair_variant=1                                  (k_pair_atom, generic pair_visit)
  tile     pair_variant=2, aztot_forces                   (k_pair_tile, pair_body<MODE, VDW>)
  list     pair_variant=2 after step(k), lists in force   (k_pair_list, pair_body<MODE, VDW, MASKED>)
  generic  DBG_GENERIC_PAIR                                (k_pair_tile with the generic pair_visit; not for one-species LJ, whose PM_ONE_LJ kernel
                                                           the bit does not switch off, so there it would repeat the tile path)
  keepcut  DBG_KEEP_VDW_CUT_TEST where VDW_LJ_NOCUT applies (Lennard-Jones with the per-pair cut-off test kept)
  short    DBG_SHORT_LISTS + DBG_ALWAYS_CLEANUP            (cases with filler atoms: k_pair_list + k_pair_tile<CLEANUP> for the cells whose list
                                                           overflowed; DBG_ALWAYS_CLEANUP: the clean-up launch runs on every list step)
The kernel timers name the launch, not the specialisation inside it: which MODE / VDW body runs follows from the case (pair_cases.py) and the
debug bits above.
"""
import os

import numpy as np
import pytest

import pair_cases as pc
from aztotmd_amd import api
from aztotmd_amd.api import DebugBit

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_functions.npz")
_REF = None


def fixture():
    global _REF
    if _REF is None:
        _REF = dict(np.load(FIXTURE))
    return _REF


def reference(name):
    R = fixture()
    sel = R["case"] == list(R["names"]).index(name)
    return {k: R[k][sel] for k in R if k[0] != "b" and k not in ("names", "case")}


def system(name):
    """the case's engine input, built around the coordinates the fixture stores"""
    ref = reference(name)
    xyz = np.empty((2 * len(ref["f"]), 3))
    xyz[0::2] = np.stack([ref["xi"], ref["yi"], ref["zi"]], 1)
    xyz[1::2] = np.stack([ref["xj"], ref["yj"], ref["zj"]], 1)
    case, pairs = pc.build(name, xyz=xyz)
    for k in ("dx", "dy", "dz"):
        assert np.array_equal(ref[k], pairs[k]), (name, k)
    return case, pairs, ref


def paths(name):
    s = pc.spec(name)
    p = ["atom", "tile", "list"]
    if not (len(s["species"]) == 1 and s["vdw"][0][2] == 1 and s["elec"] == 0):
        p.append("generic")
    if s["keepcut"]:
        p.append("keepcut")
    if s["filler"]:
        p.append("short")
    return p


def run_path(case, path):
    """(engine, state, stats, kernel names) of the evaluation whose forces state() returns; stats()["pairs_dropped"] counts that evaluation's drops"""
    kw = dict(pair_variant=1 if path == "atom" else 2, profile=1)
    kw["debug"] = {"generic": DebugBit.DBG_GENERIC_PAIR, "keepcut": DebugBit.DBG_KEEP_VDW_CUT_TEST, "short": DebugBit.DBG_SHORT_LISTS | DebugBit.DBG_ALWAYS_CLEANUP}.get(path, 0)
    if path in ("list", "short"):             # frozen atoms give the adaptive interval nothing to measure: re-sort every 32 steps (DBG_FIXED_INTERVAL)
        kw.update(sort_every=32)
        kw["debug"] |= DebugBit.DBG_FIXED_INTERVAL
    e = api.Engine(api.Model.from_case(case), **kw)
    if path in ("list", "short"):
        e.step(12)
    e.reset_kernel_times()
    before = e.stats()["pairs_dropped"]                  # (a running count, like the oracle's nDropped: every evaluation adds its drops)
    if path in ("list", "short"):
        e.step(1)
    else:
        e.forces()
    kt = e.kernel_times()
    st = e.stats()
    st["pairs_dropped"] -= before
    return e, e.state(), st, {k for k, v in kt.items() if v["calls"] > 0}


EXPECT = {"atom": {"pair_atom"}, "tile": {"pair_tile"}, "generic": {"pair_tile"}, "keepcut": {"pair_tile"}, "list": {"pair_list"},
          "short": {"pair_list", "pair_cleanup"}}


def expected(name, ref, radius, pairs):
    """reference f per pair (before the drop rule), S_F, VdW energy and its scale; surk: the radius-free parts combined with the engine's radii"""
    f, sf = ref["f"].copy(), ref["sf"].copy()
    uv, sev = ref["uv"].copy(), ref["sev"].copy()
    s = pc.spec(name)
    if any(v[2] == 7 for v in s["vdw"]):
        p = s["vdw"][0][4]
        a, b = radius[pairs["i"]], radius[pairs["j"]]
        c1 = (a * b) ** 3
        c2 = a * b / (p[2] * a + p[3] * b)
        f = c1 * ref["fa"] - c2 * ref["fb"]
        sf = c1 * np.abs(ref["fa"]) + c2 * np.abs(ref["fb"])
        uv = c1 * ref["ua"] - c2 * ref["ub"]
        sev = c1 * np.abs(ref["ua"]) + c2 * np.abs(ref["ub"])
    return f, sf, uv, sev


@pytest.mark.parametrize("name", pc.CASES)
def test_pair_functions_against_high_precision(name):
    case, pairs, ref = system(name)
    s = pc.spec(name)
    i, j = pairs["i"], pairs["j"]
    r = np.sqrt(pc.r2_fp64(pairs))
    d = np.stack([pairs["dx"], pairs["dy"], pairs["dz"]], 1)
    asym = any(v[2] == 7 and v[4][2] != v[4][3] for v in s["vdw"])     # surk with ka != kb is asymmetric in the radii: no Newton check
    L = case["box"][0]
    log = []
    for path in paths(name):
        e, st, stats, ran = run_path(case, path)
        log.append("%s: %s" % (path, ",".join(sorted(k for k in ran if k.startswith("pair_")))))
        assert EXPECT[path] <= ran, (name, path, ran)
        if path in ("tile", "generic", "keepcut"):
            assert "pair_list" not in ran and "pair_atom" not in ran, (name, path, ran)
        if path == "list":
            assert stats["pair_lists"] == 1 and "pair_tile" not in ran, (name, stats["pair_lists"], ran)
        if path == "short":
            assert 0 < stats["cells_without_list"], (name, stats)
        # the staging kernels work on coordinates relative to the cell centre: with cells of edge case["cell_list"] (a half-integer) every centre is
        # dyadic and x - centre is exact, so both visits of a pair form exactly negated d (otherwise they round differently and Newton's law holds only
        # to rounding).  The grid the engine chose must be that one.
        assert stats["n_cells"] == round(L / case["cell_list"]) ** 3, (name, path, stats["n_cells"])
        if case.get("radii"):                                   # radius-dependent potential without the radiative thermostat: the engine's own radii
            assert ((st["radius"] >= 0.577) & (st["radius"] <= 0.5771)).all(), (name, path)
        f, sf, uv, sev = expected(name, ref, st["radius"], pairs)
        assert np.isfinite(f).all() and np.isfinite(sf).all()
        dropped = f * f > 1e10
        F = np.stack([st["fx"], st["fy"], st["fz"]], 1)
        Fi, Fj = F[i], F[j]
        want = np.where(dropped[:, None], 0.0, f[:, None] * d)
        tol = pc.TAU * sf * r
        for who, Fa, sign in (("i", Fi, 1.0), ("j", Fj, -1.0)):     # both atoms of every pair against the reference
            err = np.linalg.norm(Fa - sign * want, axis=1)
            bad = np.flatnonzero(~(err <= tol))
            assert bad.size == 0, (name, path, who, bad[:8], r[bad[:8]], (err / np.maximum(sf * r, 1e-300))[bad[:8]])
        assert (Fi[dropped] == 0.0).all() and (Fj[dropped] == 0.0).all(), (name, path)
        if not asym:
            nb = np.flatnonzero((Fi != -Fj).any(1))
            assert nb.size == 0, (name, path, nb[:8], r[nb[:8]], (np.abs(Fi + Fj).max(1) / np.maximum(np.abs(Fi).max(1), 1e-300))[nb[:8]])
        if s["filler"]:                                         # neutral atoms of a species without a potential feel nothing
            assert (F[2 * len(i):] == 0.0).all(), (name, path)
        assert stats["pairs_dropped"] == int(dropped.sum()), (name, path, stats["pairs_dropped"], int(dropped.sum()))
        ev, ec = uv.sum(), ref["uc"].sum()
        assert abs(stats["engVdW"] - ev) <= pc.TAU * sev.sum(), (name, path, stats["engVdW"], ev, sev.sum())
        assert abs(stats["engCoul"] - ec) <= pc.TAU * ref["sec"].sum(), (name, path, stats["engCoul"], ec, ref["sec"].sum())
    print("%s: %s" % (name, "; ".join(log)))


@pytest.mark.parametrize("name", [n for n in pc.CASES if n not in ("surk1", "elin_einv")])
def test_drop_rule_on_both_sides_in_every_family(name):
    """Every family (elin / einv never reach f^2 = 1e10 above 0.05 A) has pairs just inside and just outside the drop rule, and the tile kernel
    drops exactly the inside ones - including the case where the Coulomb part sets ljDropR2 (lnjs_fenn_coul_drop)."""
    case, pairs, ref = system(name)
    f = ref["f"]
    inside, outside = pairs["drop_target"] == 1, pairs["drop_target"] == -1
    assert inside.any() and outside.any()
    assert (f[inside] ** 2 > 1e10).all() and (f[outside] ** 2 < 1e10).all()
    e, st, stats, ran = run_path(case, "tile")
    F = np.stack([st["fx"], st["fy"], st["fz"]], 1)
    assert (F[pairs["i"][inside]] == 0.0).all() and (np.abs(F[pairs["i"][outside]]).max(1) > 0.0).all()
    assert stats["pairs_dropped"] == int((f * f > 1e10).sum()) >= int(inside.sum())


@pytest.mark.parametrize("name", pc.BONDED_CASES)
def test_bonded_molecules_against_high_precision(name):
    """The bond and angle kernel, atom by atom: all five bond types from 0.7 to 1.5 r0, hcos angles from 2 deg to exactly 180 deg (no force there),
    every atom within tau S_F of the reference and engBond / engAngle within tau S_E."""
    R = fixture()
    k = list(R["bnames"]).index(name)
    sel = R["bcase"] == k
    xyz = np.stack([R["bx"][sel], R["by"][sel], R["bz"][sel]], 1)
    case, mols = pc.build_bonded(name, xyz=xyz)
    want = np.stack([R["bfx"][sel], R["bfy"][sel], R["bfz"][sel]], 1)
    for variant in (1, 2):
        e = api.Engine(api.Model.from_case(case), pair_variant=variant, profile=1)
        e.reset_kernel_times()
        e.forces()
        ran = {kk for kk, v in e.kernel_times().items() if v["calls"] > 0}
        assert "bonded" in ran, (name, ran)
        st, stats = e.state(), e.stats()
        F = np.stack([st["fx"], st["fy"], st["fz"]], 1)
        err = np.linalg.norm(F - want, axis=1)
        bad = np.flatnonzero(~(err <= pc.TAU * R["bsf"][sel]))
        assert bad.size == 0, (name, variant, bad[:8], (err / R["bsf"][sel])[bad[:8]])
        eb, ea = stats["engBond"], stats["engAngle"]
        got, other = (eb, ea) if name == "bonds" else (ea, eb)
        assert abs(got - R["beng"][k]) <= pc.TAU * R["bse"][k], (name, variant, got, R["beng"][k])
        assert other == 0.0 and stats["engVdW"] == 0.0
