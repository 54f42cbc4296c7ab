"""The pressure-tensor contract (include/aztot.h) pinned on the CPU, independently of any kernel: the thermodynamic identity tr W = -3 V dU/dV, the
known answer of a perfect FCC crystal, the fp64 restatement of the kernel's rule against the high-precision enumeration (and mutations of it that
must break a bound), the summation tree, the struct layout and the parser."""
import ctypes

import numpy as np
import pytest

import stress_model as sm
import tcf_model
from aztotmd_amd import api, inputs

LD = np.longdouble


def lj_liquid(seed=5, frozen=None):
    case = inputs.lj_case((3, 3, 3), a=5.4, seed=seed, rc=6.5, cell_list=6.5, vel_T=120.0)
    if frozen is not None:
        case = dict(case, species=case["species"] * 2, names=["Ar", "Fz"], frozen=[0, 1], types=(np.arange(len(case["x"])) % 3 == 0).astype(np.int32),
                    vdw=[(a, b, 1, 6.5, [inputs.AR_EPS, inputs.AR_SIGMA]) for a, b in ((0, 0), (0, 1), (1, 1))])
    return case


def fennell_liquid():
    return inputs.lj_case((3, 3, 3), a=5.4, seed=6, rc=6.5, cell_list=6.5, vel_T=120.0, charges=(0.3, -0.3), elec="fenn", r_real=6.5, alpha=0.4)


def wall_pair():
    case = inputs.lj_case((3, 3, 3), a=5.4, seed=7, rc=6.5, cell_list=6.5)
    L = case["box"][0]
    keep = np.array([0, 1])
    case = dict(case, types=case["types"][keep], **{k: np.asarray(case[k])[keep].copy() for k in ("x", "y", "z", "vx", "vy", "vz")})
    case["x"][:] = [0.3, L - 3.5]
    case["y"][:] = [L - 0.25, 0.5]
    case["z"][:] = [4.0, 5.5]
    return case


def energy_mp(S, scale, pi):
    """total pair energy in mpmath with box and coordinates scaled by `scale` (the pair set of the unscaled system)"""
    import mpmath as mp
    import pair_reference as pr
    i, j, d64, r2 = sm.fp64_pairs(S)
    U = mp.mpf(0)
    for a, b, rr in zip(i, j, r2):
        d = []
        for k in range(3):
            L = mp.mpf(float(S["box"][k])) * scale
            v = (mp.mpf(float(S["pos"][a, k])) - mp.mpf(float(S["pos"][b, k]))) * scale
            v = v - L if v > L / 2 else (v + L if v < -L / 2 else v)
            d.append(v)
        r = mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
        ta, tb = int(S["types"][a]), int(S["types"][b])
        qa, qb = S["species"][ta][1], S["species"][tb][1]
        if S["elec"] and qa and qb:
            U += pr.coul(S["elec"], qa, qb, r, S["rReal"], S["alpha"], pi=pi)[1]
        pt = S["pots"].get((ta, tb))
        if pt is not None and rr <= pt[1] * pt[1]:
            U += pr.vdw(pt[0], pt[2], r)[1]
    return U


@pytest.mark.parametrize("make", [lj_liquid, fennell_liquid, wall_pair])
def test_trace_of_the_virial_is_minus_3V_dUdV(make):
    """tr W = sum over pairs of f r^2 = -sum r dU/dr = -3 V dU/dV under a uniform scaling of box and coordinates; central difference in mpmath with
    pi = mp.pi, so that f is exactly the derivative.  h = 1e-15 at 50 digits: the quotient is good to ~1e-30 relative, the comparison is limited by the
    longdouble the reference returns (2^-63 per term)."""
    import mpmath as mp
    S = sm.system_from_case(make())
    q = 2.0 ** 20                       # coordinates and box on a dyadic grid: every r_i - r_j and every shift by L is exact, d is the same in both sums
    S["pos"], S["box"] = np.round(S["pos"] * q) / q, np.round(S["box"] * q) / q
    assert sm.near_cutoff(S) == 0
    ref = sm.stress_reference(S, "mp", pi=mp.pi)
    assert ref["pairs"] > 0
    h = mp.mpf("1e-15")
    # V = V0 s^3: dU/dV = dU/ds / (3 V0 s^2) at s = 1
    dUds = (energy_mp(S, 1 + h, mp.pi) - energy_mp(S, 1 - h, mp.pi)) / (2 * h)
    trW = ref["W"][0] + ref["W"][1] + ref["W"][2]
    scale = ref["W_scale"][0] + ref["W_scale"][1] + ref["W_scale"][2]
    assert abs(trW + LD(mp.nstr(dUds, 25))) <= LD(1e-16) * scale, (trW, dUds, scale)


def test_fcc_crystal_known_answer():
    """a = 5.75 (dyadic) on 5^3 cells, LJ rc = 8.5: shells of 12, 6, 24 and 12 neighbours at a / sqrt 2, a, a sqrt 1.5, a sqrt 2"""
    import list_model as lm
    a = 5.75
    case = inputs.lj_case((5, 5, 5), a=a, jitter=0.0, seed=1, rc=8.5, cell_list=8.5)
    S = sm.system_from_case(case)
    N = len(S["pos"])
    assert N == 500
    ref = sm.stress_reference(S, "ld")
    assert ref["pairs"] == N * (12 + 6 + 24 + 12) // 2 and ref["pairs_dropped"] == 0
    want = LD(0)
    for n, r2 in ((12, a * a / 2), (6, a * a), (24, 1.5 * a * a), (12, 2 * a * a)):
        f, sf = lm.lj_term(inputs.AR_EPS, inputs.AR_SIGMA, LD(r2))
        want += n * f * LD(r2)
    want *= LD(N) / 6
    for c in range(3):
        assert abs(ref["W"][c] - want) <= LD(sm.TAU) * ref["W_scale"][c], (c, ref["W"][c], want)
    for c in range(3, 6):
        assert abs(ref["W"][c]) <= LD(sm.TAU) * ref["W_scale"][c]
    got = sm.fp64_stress(S)
    ok, ratio = sm.within(got["W"], ref["W"], ref["W_scale"])
    assert ok, ratio
    # every atom of the perfect crystal carries the same virial
    ok, ratio = sm.within(got["w"], np.broadcast_to(ref["W"] / N, (N, 6)), ref["w_scale"])
    assert ok, ratio


def mutation_system():
    """an LJ liquid with a frozen species, a wall-straddling pair, and one pair at r2 == rMax^2 exactly (axis-aligned, dyadic coordinates)"""
    case = lj_liquid(frozen=True)
    L = case["box"][0]
    for k in ("x", "y", "z", "vx", "vy", "vz"):
        case[k] = np.asarray(case[k]).copy()
    S = sm.system_from_case(case)
    return case, S


def fp64_against_reference(S, ref, mutate=None):
    got = sm.fp64_stress(S, mutate)
    res = [sm.within(got["w"], ref["w"], ref["w_scale"])[0], sm.within(got["W"], ref["W"], ref["W_scale"])[0],
           sm.within(got["K"], ref["K"], ref["K_scale"])[0], sm.within(got["eng_vdw"], ref["eng_vdw"], ref["eng_vdw_scale"])[0],
           got["pairs"] == ref["pairs"], got["pairs_dropped"] == ref["pairs_dropped"]]
    return all(res)


def tie_system():
    """two atoms, axis-aligned on dyadic coordinates, r2 == rMax^2 exactly, across the periodic wall"""
    case = wall_pair()
    L = case["box"][0]
    case["x"][:] = [1.25, L - 5.25]
    case["y"][:] = [2.0, 2.0]
    case["z"][:] = [3.0, 3.0]
    return sm.system_from_case(case)


def test_fp64_restatement_within_every_bound_and_mutations_break_one():
    case, S = mutation_system()
    assert sm.near_cutoff(S) == 0
    ref = sm.stress_reference(S, "ld")
    assert (S["types"] == 1).any() and np.abs(S["vel"][S["types"] == 1]).max() > 0      # frozen atoms with velocities: the kinetic rule is live
    i, j, d, r2 = sm.fp64_pairs(S)
    raw = S["pos"][i] - S["pos"][j]
    assert (np.abs(raw) > 0.5 * S["box"]).any()                                          # pairs straddle the walls
    assert fp64_against_reference(S, ref)
    for m in ("no_half", "no_min_image", "xy_as_xx", "sign", "frozen_in_K", "mass_amu"):
        assert not fp64_against_reference(S, ref, m), m
    T = tie_system()
    if (T["box"][0] / 2) < 6.5:
        pytest.fail("box too small for the tie pair")
    i, j, d, r2 = sm.fp64_pairs(T)
    assert len(i) == 1 and r2[0] == 6.5 * 6.5 and abs(T["pos"][0, 0] - T["pos"][1, 0]) > T["box"][0] / 2
    rt = sm.stress_reference(T, "ld")
    assert rt["pairs"] == 1 and fp64_against_reference(T, rt)
    assert not fp64_against_reference(T, rt, "exclusive_cut")
    assert not fp64_against_reference(T, rt, "no_min_image")


def test_mp_and_longdouble_references_agree():
    S = sm.system_from_case(wall_pair())
    a, b = sm.stress_reference(S, "mp"), sm.stress_reference(S, "ld")
    assert a["pairs"] == b["pairs"] == 1
    assert sm.within(b["w"], a["w"], a["w_scale"], tau=1e-17)[0]
    assert sm.within(b["eng_vdw"], a["eng_vdw"], a["eng_vdw_scale"], tau=1e-17)[0]


def test_struct_layout():
    assert ctypes.sizeof(api._Stress) == 208
    assert api._Stress.pressure_iso.offset == 24 + 3 * 48 and api._Stress.pairs.offset == 192


def test_parser_reads_the_stress_directive(tmp_path):
    case = inputs.config("F1")
    d = str(tmp_path / "with")
    inputs.write_input_files(dict(case, stress=5), d)
    assert api.Model.from_dir(d).query("stress")[0] == 5
    d = str(tmp_path / "without")
    inputs.write_input_files(case, d)
    assert api.Model.from_dir(d).query("stress")[0] == 0
    d = str(tmp_path / "negative")
    inputs.write_input_files(dict(case, stress=-3), d)
    with pytest.raises(api.AztotError) as e:
        api.Model.from_dir(d)
    assert "ERROR[415]" in str(e.value) and e.value.code == -2        # AZTOT_ERR_INPUT


def test_m_scale_matches_the_library():
    assert api.Model.from_case(inputs.config("F1")).query("m_scale")[0] == sm.M_SCALE


@pytest.mark.parametrize("n", [1, 255, 256, 257, 769, 70000])
def test_totals_rule_is_the_tcf_tree(n):
    """the totals of fp64_stress are tcf_model.tree_sum column by column; the tree itself against a plain restatement of the three steps"""
    rng = np.random.Generator(np.random.PCG64(n))
    t = rng.normal(size=(n, 6)) * 10.0 ** rng.integers(-3, 4, size=(n, 6))
    for c in range(6):
        col = t[:, c]
        chunks = max(1, -(-n // 256))
        a = np.zeros(chunks * 256)
        a[:n] = col
        sums = []
        for k in range(chunks):
            runs = []
            for r in range(4):
                v = a[256 * k + 64 * r:256 * k + 64 * r + 64].copy()
                h = 32
                while h:
                    v = v[:h] + v[h:2 * h]
                    h //= 2
                runs.append(v[0])
            sums.append((runs[0] + runs[2]) + (runs[1] + runs[3]))
        pad = 1
        while pad < chunks:
            pad *= 2
        p = np.zeros(pad)
        p[:chunks] = sums
        h = pad // 2
        while h:
            p = p[:h] + p[h:2 * h]
            h //= 2
        assert tcf_model.tree_sum(col) == p[0]
