"""Restatement of the pressure-tensor sampler's contract (include/aztot.h, 'pressure tensor') for the tests: tests/test_stress_model.py on the CPU and
tests/test_gpu_stress.py on the GPU.

A SYSTEM is what a sample reads, as a dict: box (3,), pos (N, 3) wrapped, vel (N, 3), types (N,), radius (N,) or None, species [(mass_amu, charge,
frozen)], pots {(a, b): (type, rc, params)} in both orders, elec (0 none, 1 direct, 3 Fennell), rReal, alpha, rmax.

stress_reference  every pair inside rMax, each term in high precision: mpmath (tests/pair_reference.py, any potential) or numpy.longdouble
                  (Lennard-Jones only, tests/list_model.lj_term), with the condition scales the bounds are stated in;
fp64_stress       the rule as the kernel states it, every operation one fp64 operation, totals by tcf_model.tree_sum; `mutate` breaks one rule.

The separation d of a pair is the contract's: the fp64 difference r_i - r_j, shifted by L where |d| > L / 2; the references evaluate every term at
exactly that d.  The pair SET is decided in fp64 by the rule of the contract (minimum image, (dx*dx + dy*dy) + dz*dz <= rMax^2, r2 <= rc * rc per pair): the liquid cases
assert through `near` that no pair lies within 1e-9 (relative) of a cut-off, so the set is never in doubt."""
import numpy as np

import tcf_model

LD = np.longdouble
COMP = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # xx yy zz xy xz yz
M_SCALE = 1.6605402E-27 / (1.60217733E-19 * 1.0E-12 * 1.0E-12 / 1.0E-10 / 1.0E-10)      # units::m_scale (csrc/model.h): amu -> internal mass, same operations
PRESSURE_FACTOR = 1.58e6                                        # units::pressure_factor
PI = 3.14159265359                                              # units::pi
FCOUL = 0.25 / PI / 8.854187817E-12 * 1.60217657E-19 ** 2 / 1e-20 / (1.60217733E-19 / 1e-10)
TAU = 1e-13                                                     # pair_cases.TAU


def system_from_case(case, state=None):
    """the sampled state of a case (inputs.lj_case / pair_cases.build layout); state: Engine.state() of a run of it"""
    box = np.array(case["box"], dtype=np.float64)
    src = state if state is not None else case
    pos = np.stack([np.asarray(src[k], dtype=np.float64) for k in "xyz"], 1)
    pos = np.mod(pos, box)
    pos[pos >= box] = 0.0
    vel = np.stack([np.asarray(src[k], dtype=np.float64) for k in ("vx", "vy", "vz")], 1)
    frozen = case.get("frozen") or [0] * len(case["species"])
    pots = {}
    for a, b, ty, rc, p in case["vdw"]:
        pots[(a, b)] = pots[(b, a)] = (ty, float(rc), list(p))
    elec = int(case.get("elec_type", 0))
    rmax = float(case["rReal"]) if elec else max([v[3] for v in case["vdw"]] + [0.0])
    radius = None
    if any(v[2] == 7 for v in case["vdw"]):
        radius = np.asarray(state["radius"], dtype=np.float64)
    return dict(box=box, pos=pos, vel=vel, types=np.asarray(case["types"]), radius=radius,
                species=[(m, q, int(f)) for (m, q), f in zip(case["species"], frozen)], pots=pots, elec=elec, rReal=float(case.get("rReal", 0.0)),
                alpha=float(case.get("alpha", 0.0)), rmax=rmax)


def fp64_pairs(S, include_ties=True, min_image=True):
    """(i, j, d (n, 3), r2) of the unordered pairs i < j inside rMax by the fp64 rule of the contract; d = r_i - r_j"""
    pos, box = S["pos"], S["box"]
    N = len(pos)
    if N < 2 or S["rmax"] <= 0.0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros((0, 3)), np.zeros(0)
    if N <= 3000:
        i, j = np.triu_indices(N, 1)
    else:
        from scipy.spatial import cKDTree
        ij = cKDTree(pos, boxsize=box).query_pairs(S["rmax"] * (1.0 + 1e-6) + 1e-6, output_type="ndarray")
        i, j = ij[:, 0], ij[:, 1]
    d = pos[i] - pos[j]
    if min_image:
        half = 0.5 * box
        d = np.where(d > half, d - box, np.where(d < -half, d + box, d))
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r2max = S["rmax"] * S["rmax"]
    keep = (r2 <= r2max) if include_ties else (r2 < r2max)
    o = np.lexsort((j[keep], i[keep]))
    return i[keep][o], j[keep][o], d[keep][o], r2[keep][o]


def near_cutoff(S, rel=1e-9):
    """pairs within `rel` (relative, in r^2) of rMax^2 or of their own cut-off: such a pair could be decided either way"""
    pos, box = S["pos"], S["box"]
    T = dict(S, rmax=S["rmax"] * 1.01)
    i, j, d, r2 = fp64_pairs(T)
    n = int((np.abs(r2 / (S["rmax"] * S["rmax"]) - 1.0) < rel).sum())
    ti, tj = S["types"][i], S["types"][j]
    for (a, b), (ty, rc, p) in S["pots"].items():
        m = (ti == a) & (tj == b)
        n += int((np.abs(r2[m] / (rc * rc) - 1.0) < rel).sum())
    return n


def _terms_mp(S, i, j, d64, r2, pi=None):
    """per pair, mpmath: f, S_F, uv, sev, uc, sec as float-convertible mpf lists"""
    import mpmath as mp
    import pair_reference as pr
    pi = pr.MODEL_PI if pi is None else pi
    out = []
    for a, b, dd, rr in zip(i, j, d64, r2):
        ta, tb = int(S["types"][a]), int(S["types"][b])
        d = [mp.mpf(float(v)) for v in dd]          # the contract's separation: the fp64 difference, shifted by L (its rounding is part of the definition)
        r = mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
        f = sf = uv = sev = uc = sec = mp.mpf(0)
        qa, qb = S["species"][ta][1], S["species"][tb][1]
        if S["elec"] and qa != 0.0 and qb != 0.0:
            f, uc, sf, sec = pr.coul(S["elec"], qa, qb, r, S["rReal"], S["alpha"], pi=pi)
        pt = S["pots"].get((ta, tb))
        if pt is not None and rr <= pt[1] * pt[1]:
            ra, rb = (S["radius"][a], S["radius"][b]) if S["radius"] is not None else (0.0, 0.0)
            fv, uv, sfv, sev = pr.vdw(pt[0], pt[2], r, ra, rb)
            f, sf = f + fv, sf + sfv
        out.append((f, sf, uv, sev, uc, sec, d))
    return out


def stress_reference(S, prec="mp", pi=None):
    """dict(w (N, 6), w_scale (N, 6), W, W_scale, K, K_scale (6,), eng_vdw, eng_vdw_scale, eng_coul, eng_coul_scale, pairs, pairs_dropped, i, j)
    prec 'mp': mpmath terms (any potential);  'ld': numpy.longdouble, Lennard-Jones without electrostatics only"""
    N = len(S["pos"])
    i, j, d64, r2 = fp64_pairs(S)
    w, ws = np.zeros((N, 6), dtype=LD), np.zeros((N, 6), dtype=LD)
    ev = sev = ec = sec = LD(0)
    dropped = 0
    if prec == "ld":
        import list_model as lm
        assert S["elec"] == 0 and all(v[0] == 1 or (v[0] == 7 and v[2][2] == v[2][3]) for v in S["pots"].values())
        d = d64.astype(LD)              # the contract's separation: the fp64 difference, shifted by L (its rounding is part of the definition)
        rr = (d * d).sum(1)
        f, sf, u, su = (np.zeros(len(i), dtype=LD) for _ in range(4))
        ti, tj = S["types"][i], S["types"][j]
        for (a, b), (ty, rc, p) in S["pots"].items():
            m = (ti == a) & (tj == b) & (r2 <= rc * rc)
            if ty == 7:         # surk (pair_reference.vdw kind 7) with the sampled radii; ka == kb: the term is the same from both ends
                ra, rb, r = S["radius"][i[m]].astype(LD), S["radius"][j[m]].astype(LD), np.sqrt(rr[m])
                t1, t2 = LD(p[0]) * (ra * rb) ** 3, LD(p[1]) * ra * rb / (LD(p[2]) * ra + LD(p[3]) * rb)
                f[m], sf[m] = 7 * t1 / r ** 9 - 6 * t2 / r ** 8, 7 * abs(t1) / r ** 9 + 6 * abs(t2) / r ** 8
                u[m], su[m] = t1 / r ** 7 - t2 / r ** 6, abs(t1) / r ** 7 + abs(t2) / r ** 6
                continue
            f[m], sf[m] = lm.lj_term(p[0], p[1], rr[m])
            s6 = (LD(p[1]) * LD(p[1]) / rr[m]) ** 3
            u[m], su[m] = LD(4.0) * LD(p[0]) * (s6 * s6 - s6), LD(4.0) * LD(p[0]) * (s6 * s6 + s6)
        drop = f * f > LD(1e10)
        dropped = int(drop.sum())
        ev, sev = u.sum(), su.sum()
        for c, (a, b) in enumerate(COMP):
            t = np.where(drop, LD(0), LD(0.5) * f * d[:, a] * d[:, b])
            s = np.where(drop, LD(0), LD(0.5) * sf * abs(d[:, a]) * abs(d[:, b]))
            for idx in (i, j):
                np.add.at(w[:, c], idx, t)
                np.add.at(ws[:, c], idx, s)
    else:
        import mpmath as mp
        wm = [[mp.mpf(0)] * 6 for _ in range(N)]
        wsm = [[mp.mpf(0)] * 6 for _ in range(N)]
        evm = sevm = ecm = secm = mp.mpf(0)
        for a, b, (f, sf, uv, sv, uc, sc, d) in zip(i, j, _terms_mp(S, i, j, d64, r2, pi)):
            evm += uv; sevm += sv; ecm += uc; secm += sc
            if f * f > 1e10:
                dropped += 1
                continue
            for c, (p, q) in enumerate(COMP):
                t, s = f * d[p] * d[q] / 2, sf * abs(d[p]) * abs(d[q]) / 2
                for k in (a, b):
                    wm[k][c] += t
                    wsm[k][c] += s
        w = np.array([[LD(mp.nstr(v, 25)) for v in row] for row in wm], dtype=LD).reshape(N, 6)
        ws = np.array([[LD(mp.nstr(v, 25)) for v in row] for row in wsm], dtype=LD).reshape(N, 6)
        ev, sev, ec, sec = (LD(mp.nstr(v, 25)) for v in (evm, sevm, ecm, secm))
    mass = np.array([0.0 if fr else m for m, q, fr in S["species"]])[S["types"]].astype(LD) * LD(M_SCALE)
    V = S["vel"].astype(LD)
    K = np.array([(mass * V[:, a] * V[:, b]).sum() for a, b in COMP], dtype=LD)
    Ks = np.array([(mass * abs(V[:, a]) * abs(V[:, b])).sum() for a, b in COMP], dtype=LD)
    return dict(w=w, w_scale=ws, W=w.sum(0), W_scale=ws.sum(0), K=K, K_scale=Ks, eng_vdw=ev, eng_vdw_scale=sev, eng_coul=ec, eng_coul_scale=sec,
                pairs=len(i), pairs_dropped=dropped, i=i, j=j)


def _lj_f64(eps, sigma, r2):
    """fer_lj (vdw.cpp:16-26) in fp64: (f, U) with the host's folded constants 4 eps, sigma^2, 24 eps"""
    r2i = 1.0 / r2
    sr2 = sigma * sigma * r2i
    sr6 = sr2 * sr2 * sr2
    return 24.0 * eps * r2i * sr6 * (2.0 * sr6 - 1.0), 4.0 * eps * sr6 * (sr6 - 1.0)


def fp64_stress(S, mutate=None):
    """the sampler's rule in fp64 numpy (Lennard-Jones, no electrostatics): dict(w (N, 6), W, K (6,), eng_vdw, pairs, pairs_dropped).
    mutate: 'no_half', 'no_min_image', 'xy_as_xx', 'sign', 'frozen_in_K', 'mass_amu', 'exclusive_cut'"""
    assert S["elec"] == 0 and all(v[0] == 1 for v in S["pots"].values())
    N = len(S["pos"])
    i, j, d, r2 = fp64_pairs(S, include_ties=mutate != "exclusive_cut", min_image=mutate != "no_min_image")
    f, u = np.zeros(len(i)), np.zeros(len(i))
    ti, tj = S["types"][i], S["types"][j]
    for (a, b), (ty, rc, p) in S["pots"].items():
        m = (ti == a) & (tj == b) & (r2 <= rc * rc)
        f[m], u[m] = _lj_f64(p[0], p[1], r2[m])
    drop = f * f > 1e10
    f = np.where(drop, 0.0, -f if mutate == "sign" else f)
    h = f if mutate == "no_half" else 0.5 * f
    w = np.zeros((N, 6))
    for c, (a, b) in enumerate(COMP):
        if mutate == "xy_as_xx" and c == 3:
            a, b = 0, 0
        t = (h * d[:, a]) * d[:, b]
        np.add.at(w[:, c], i, t)
        np.add.at(w[:, c], j, t)
    e = np.zeros(N)
    np.add.at(e, i, 0.5 * u)
    np.add.at(e, j, 0.5 * u)
    mass = np.array([m if (mutate == "frozen_in_K" or not fr) else 0.0 for m, q, fr in S["species"]])[S["types"]]
    if mutate != "mass_amu":
        mass = mass * M_SCALE
    V = S["vel"]
    K = np.array([tcf_model.tree_sum((mass * V[:, a]) * V[:, b]) for a, b in COMP])
    return dict(w=w, W=np.array([tcf_model.tree_sum(w[:, c]) for c in range(6)]), K=K, eng_vdw=tcf_model.tree_sum(e), pairs=len(i), pairs_dropped=int(drop.sum()))


def pressure(K, W, box):
    """P[ab] in atm and its isotropic part, the contract's formula in fp64"""
    V = float(box[0]) * float(box[1]) * float(box[2])
    P = (np.asarray(K, dtype=np.float64) + np.asarray(W, dtype=np.float64)) / V * PRESSURE_FACTOR
    return P, (P[0] + P[1] + P[2]) / 3.0


def within(got, ref, scale, tau=TAU):
    """(ok, worst err / (tau scale)): |got - ref| <= tau scale, component by component (a zero scale demands equality)"""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    bound = LD(tau) * np.asarray(scale, dtype=LD)
    ok = bool((err <= bound).all())
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return ok, float(np.max(ratio)) if np.size(ratio) else 0.0


def check_sample(S, ref, per_atom, tot, tau=TAU):
    """every bound of the issue for one sample: per_atom (N, 6), tot = Engine.stress().  Returns the worst ratios (w, W, K, eng)"""
    ok_w, r_w = within(per_atom, ref["w"], ref["w_scale"], tau)
    ok_W, r_W = within(tot["virial"], ref["W"], ref["W_scale"], tau)
    ok_K, r_K = within(tot["kinetic"], ref["K"], ref["K_scale"], tau)
    ok_v, r_v = within(tot["eng_vdw"], ref["eng_vdw"], ref["eng_vdw_scale"], tau)
    ok_c, r_c = within(tot["eng_coul"], ref["eng_coul"], ref["eng_coul_scale"], tau)
    print("stress ratios err / (tau scale): per-atom %.3g  W %.3g  K %.3g  eVdW %.3g  eCoul %.3g" % (r_w, r_W, r_K, r_v, r_c))
    assert ok_w, ("per-atom virial", r_w)
    assert ok_W, ("total virial", r_W)
    assert ok_K, ("kinetic", r_K)
    assert ok_v and ok_c, ("pair energies", r_v, r_c)
    assert tot["pairs"] == ref["pairs"] and tot["pairs_dropped"] == ref["pairs_dropped"], (tot["pairs"], ref["pairs"], tot["pairs_dropped"], ref["pairs_dropped"])
    P, iso = pressure(tot["kinetic"], tot["virial"], S["box"])
    assert np.array_equal(P, tot["pressure"]) and iso == tot["pressure_iso"]
    return r_w, r_W, r_K, max(r_v, r_c)
