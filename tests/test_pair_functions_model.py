"""CPU side of the pair-function tests (tests/test_gpu_pair_functions.py): the high-precision reference (tests/pair_reference.py) and its
committed fixture, checked against themselves, against mpmath's numerical derivative, against the fp64 oracle, and against the erfcx fit that
ships in csrc/kernels.hip.h."""
import os
import re

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

import pair_cases as pc           # noqa: E402
import pair_reference as pr       # noqa: E402
from oracle import oracle         # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pair_functions.npz")
KERNELS = os.path.join(os.path.dirname(HERE), "aztotmd_amd", "csrc", "kernels.hip.h")


def test_fixture_is_reproducible():
    """pair_reference.make_fixture regenerates tests/golden/pair_functions.npz bit for bit (cases, separations and reference values)."""
    got = pr.make_fixture()
    ref = np.load(FIXTURE)
    assert list(ref["names"]) == list(got["names"])
    assert list(ref["bnames"]) == list(got["bnames"])
    for k in pr.FIXTURE_KEYS + pr.BONDED_KEYS + ("beng", "bse"):
        assert ref[k].dtype == got[k].dtype and np.array_equal(ref[k], got[k]), k


VDW_CASES = [("lnjs", [0.01006, 3.3952]), ("buck", [1822.0, 0.3, 63.0]), ("p746", [3000.0, 1.0, 20.0]), ("bmhs", [0.25, 3.1, 3.3, 60.0, 80.0]),
             ("elin", [900.0, 0.4, 0.002]), ("einv", [900.0, 0.4, 0.5]), ("surk", [75.0, 8.0, 1.0, 1.3])]


@pytest.mark.parametrize("kind,p", VDW_CASES)
def test_vdw_force_is_the_derivative(kind, p):
    for r in (0.9, 2.0, 3.1, 4.7, 6.9):
        f, U, sf, se = pr.vdw(kind, p, r, 0.577, 0.5771)
        fn = pr.numeric_f(lambda x: pr.vdw(kind, p, x, 0.577, 0.5771)[1], r)
        assert abs(f - fn) <= mp.mpf("1e-30") * sf, (kind, r)
        assert abs(U) <= se and abs(f) <= sf


@pytest.mark.parametrize("elec", [1, 2, 3])
def test_coulomb_force_is_the_derivative(elec):
    for r in (0.3, 1.0, 3.3, 6.99, 7.0):
        f, U, sf, se = pr.coul(elec, 0.4, -0.3, r, 7.0, 0.45, pi=mp.pi)
        fn = pr.numeric_f(lambda x: pr.coul(elec, 0.4, -0.3, x, 7.0, 0.45, pi=mp.pi)[1], r)
        assert abs(f - fn) <= mp.mpf("1e-30") * sf, (elec, r)
    # the engine's constants carry the reference's truncated pi: 2 alpha / sqrt(pi) differs from the true derivative by ~3e-14 relative
    f, _, sf, _ = pr.coul(3, 0.4, -0.3, 2.0, 7.0, 0.45)
    assert abs(f - pr.coul(3, 0.4, -0.3, 2.0, 7.0, 0.45, pi=mp.pi)[0] * pr.fcoul_scale() / pr.fcoul_scale(mp.pi)) < 1e-12 * sf


BOND_CASES = [(1, [30.0, 1.0]), (2, [4.0, 2.0, 1.0, 0.5]), (3, [4.0, 2.0, 1.0, 0.5, 0.002]), (4, [2.0e4, 0.1, 1.513]),
              (5, [2.0e4, 0.1, 1.1467, 0.2, 0.05])]


@pytest.mark.parametrize("kind,p", BOND_CASES)
def test_bond_force_is_the_derivative(kind, p):
    for r in (0.7, 0.95, 1.0, 1.2, 1.6):
        f, U, sf, se = pr.bond(kind, p, r)
        fn = pr.numeric_f(lambda x: pr.bond(kind, p, x)[1], r)
        assert abs(f - fn) <= mp.mpf("1e-30") * sf, (kind, r)
        fo, uo = oracle.bond_pair(kind, p, r * r)
        assert abs(fo - float(f)) <= 1e-13 * float(sf) and abs(uo - float(U)) <= 1e-13 * float(se), (kind, r)


@pytest.mark.parametrize("deg", [2.0, 60.0, 109.5, 179.0, 180.0])
def test_angle_forces_are_the_gradient(deg):
    th = mp.radians(deg)
    u = [mp.mpf("1.02"), mp.mpf("0.03"), mp.mpf("-0.01")]
    nu = mp.sqrt(sum(a * a for a in u))
    e1 = [a / nu for a in u]
    w = [mp.mpf(0), mp.mpf(1), mp.mpf(0)]
    dot = sum(a * b for a, b in zip(w, e1))
    w = [b - dot * a for a, b in zip(e1, w)]
    nw = mp.sqrt(sum(a * a for a in w))
    v = [mp.mpf("0.97") * (mp.cos(th) * a + mp.sin(th) * b / nw) for a, b in zip(e1, w)]
    Fc, F1, F2, U, S, SE = pr.angle(3.0, -0.33, u, v)
    for k in range(3):
        def U1(x, k=k):
            uu = list(u); uu[k] = x
            return pr.angle(3.0, -0.33, uu, v)[3]
        assert abs(F1[k] + mp.diff(U1, u[k])) <= mp.mpf("1e-30") * S[1]
        assert abs(Fc[k] + F1[k] + F2[k]) <= mp.mpf("1e-40") * S[0]


def _oracle_pair_forces(name):
    """f of every pair of case `name` from the oracle's own pair functions (fp64 libm: orc_vdw_pair, orc_coul_pair), at the fp64 r^2"""
    s = pc.spec(name)
    case, pairs = pc.build(name)
    r2 = pc.r2_fp64(pairs)
    rM = pc.r_max(s)
    pots = pc.pot_table(s)
    f = np.zeros(len(r2))
    u = np.zeros(len(r2))
    for k in range(len(r2)):
        a, b = int(pairs["ti"][k]), int(pairs["tj"][k])
        if not r2[k] <= rM * rM:
            continue
        pt = pots.get((a, b))
        if pt is not None and pt[0] != 7 and r2[k] <= pt[1] * pt[1]:
            fv, ev = oracle.vdw_pair(pt[0], pt[1], pt[2], r2[k])
            f[k] += fv; u[k] += ev
        qa, qb = s["species"][a][1], s["species"][b][1]
        if s["elec"] and abs(qa) > 1e-10 and abs(qb) > 1e-10:
            fc, ec = oracle.coul_pair(s["elec"], s["rReal"], s["alpha"], qa, qb, r2[k])
            f[k] += fc; u[k] += ec
    return f, u


@pytest.mark.parametrize("name", [n for n in pc.CASES if n != "surk1"])
def test_oracle_meets_tau(name):
    """The bound the GPU is held to is reachable by plain fp64 arithmetic of the reference's formulas: the oracle (libm) meets it on every pair."""
    ref = np.load(FIXTURE)
    sel = ref["case"] == list(ref["names"]).index(name)
    f, u = _oracle_pair_forces(name)
    err = np.abs(f - ref["f"][sel])
    bad = err > pc.TAU * ref["sf"][sel]
    assert not bad.any(), (name, np.flatnonzero(bad), (err / np.maximum(ref["sf"][sel], 1e-300)).max())
    se = ref["sev"][sel] + ref["sec"][sel]
    uerr = np.abs(u - ref["uv"][sel] - ref["uc"][sel])
    assert (uerr <= pc.TAU * se).all(), (name, (uerr / np.maximum(se, 1e-300)).max())


@pytest.mark.parametrize("name", [n for n in pc.CASES if n != "surk1"])
def test_oracle_drops_what_the_reference_drops(name):
    """The whole system through the oracle (pair_inter, integrators.cpp:139-185): its nDropped counts the pairs with f_ref^2 > 1e10 - the
    number the GPU test holds stats()["pairs_dropped"] to - and those pairs' atoms keep exactly zero force."""
    ref = np.load(FIXTURE)
    sel = ref["case"] == list(ref["names"]).index(name)
    case, pairs = pc.build(name)
    o = oracle.Oracle(case)
    o.forces(0)
    f = ref["f"][sel]
    dropped = f * f > 1e10
    assert o.stats()["nDropped"] == dropped.sum(), (name, o.stats()["nDropped"], dropped.sum())
    st = o.state()
    for k in ("fx", "fy", "fz"):
        assert (st[k][pairs["i"][dropped]] == 0.0).all() and (st[k][pairs["j"][dropped]] == 0.0).all()


@pytest.mark.parametrize("name", pc.BONDED_CASES)
def test_oracle_meets_tau_on_bonded_molecules(name):
    """bonds.cpp / angles.cpp as the oracle restates them meet the bound the GPU test holds the bonded kernel to: every atom, and the energy."""
    ref = np.load(FIXTURE)
    sel = ref["bcase"] == list(ref["bnames"]).index(name)
    case, mols = pc.build_bonded(name)
    o = oracle.Oracle(case)
    o.forces(0)
    st = o.state()
    F = np.stack([st["fx"], st["fy"], st["fz"]], 1)
    want = np.stack([ref["bfx"][sel], ref["bfy"][sel], ref["bfz"][sel]], 1)
    err = np.linalg.norm(F - want, axis=1)
    assert (err <= pc.TAU * ref["bsf"][sel]).all(), (name, (err / ref["bsf"][sel]).max())
    e = o.stats()["engBond" if name == "bonds" else "engAngle"]
    k = list(ref["bnames"]).index(name)
    assert abs(e - ref["beng"][k]) <= pc.TAU * ref["bse"][k]
    if name == "angles":                                        # 180 deg: cos th == -1 exactly, the force vanishes
        assert np.count_nonzero(case["angles"]) and np.abs(want[-3:]).max() == 0.0


def test_cases_cover_their_edges():
    """What the sweep claims to place is there: drop pairs on both sides of f^2 = 1e10 and clear of it by more than the reference's error,
    exact cut-off ties, the alpha rReal edges, bmhs inside sigma, buck at r / rho of several hundred."""
    ref = np.load(FIXTURE)
    names = list(ref["names"])
    for name in pc.CASES:
        s = pc.spec(name)
        case, pairs = pc.build(name)
        sel = ref["case"] == names.index(name)
        f = ref["f"][sel]
        for side in (+1, -1):
            m = pairs["drop_target"] == side
            if name not in ("surk1", "elin_einv"):                  # (elin / einv never reach f^2 = 1e10 above 0.05 A; surk: radii from the engine)
                assert m.sum() >= 1, (name, side)                   # every family sits on both sides of the drop rule
            if m.any():
                ratio = f[m] ** 2 / 1e10
                assert ((ratio > 1 + 1e-7) if side > 0 else (ratio < 1 - 1e-7)).all(), (name, side, ratio)
        r2 = pc.r2_fp64(pairs)
        for (a, b, rc), k0 in zip(s["ties"], range(0, 3 * len(s["ties"]), 3)):
            tie, lo, hi = r2[k0], r2[k0 + 1], r2[k0 + 2]
            assert pairs["tie"][k0:k0 + 3].tolist() == [2, -1, 1]
            assert tie == rc * rc and lo < rc * rc < hi, (name, tie, lo, hi)
            assert np.count_nonzero([pairs["dx"][k0], pairs["dy"][k0], pairs["dz"][k0]]) == 1
        assert (pairs["dx"][pairs["tie"] == 0] != 0).all() and (pairs["dz"][pairs["tie"] == 0] != 0).all()
    assert 4.0 == 8.0 * pc.spec("fenn_ar400")["alpha"] and 8.0 * pc.spec("ewald_ar420")["alpha"] > 4.0
    _, p = pc.build("bmhs")
    assert (np.sqrt(pc.r2_fp64(p)) < 3.0).sum() >= 3
    _, p = pc.build("buck_hard")
    assert np.sqrt(pc.r2_fp64(p)).max() / 0.02 > 300
    # pairs straddle the walls
    case, p = pc.build("lnjs")
    L = case["box"][0]
    assert (np.abs(case["x"][p["i"]] - case["x"][p["j"]]) > 0.5 * L).any()


def test_erfcx_fit_within_its_claim():
    """The degree-15 erfcx fit of csrc/kernels.hip.h (kCoulCoef[0..15], read from the file that ships, as the fp64 values the device holds),
    evaluated in mpmath, stays within the 7.2e-14 relative error its comment claims on [0, 4]: a scan on a 1e-3 grid, then every local maximum of
    the scan refined by golden-section search."""
    src = open(KERNELS).read()
    body = src[src.index("kCoulCoef[32] = {"):]
    coef = [mp.mpf(float(v)) for v in re.findall(r"[-+]?\d\.\d+e[-+]\d+", body)[:16]]

    def err(x):
        t = 3 / (1 + x / 2) - 2
        return abs(mp.polyval(coef, t) / (mp.exp(x * x) * mp.erfc(x)) - 1)

    xs = [mp.mpf(k) / 1000 for k in range(4001)]
    es = [err(x) for x in xs]
    worst = max(es)
    g = (mp.sqrt(5) - 1) / 2
    for k in range(len(xs)):
        if es[k] >= max(es[max(k - 1, 0)], es[min(k + 1, len(xs) - 1)]) and es[k] > worst / 4:
            a, b = xs[max(k - 1, 0)], xs[min(k + 1, len(xs) - 1)]
            for _ in range(40):
                c, d = b - g * (b - a), a + g * (b - a)
                if err(c) > err(d):
                    b = d
                else:
                    a = c
            worst = max(worst, err((a + b) / 2))
    assert worst <= 7.2e-14, float(worst)
