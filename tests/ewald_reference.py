"""High-precision restatement of the truncated reciprocal-space Ewald sum the four kernels of csrc/ewald.hip.h compute, from the USER-level numbers
of a case (box, alpha, ewald_k, charges, coordinates), plus the systems the tests run it on (tests/test_ewald_model.py, tests/test_gpu_ewald.py).

The operation (csrc/sys_init.cpp finish_model, csrc/ewald.hip.h), with pi the model's truncated value 3.14159265359 (csrc/model.h units::pi):
  k = 2 pi (l / a, m / b, n / c) over the half space l >= 0 (m >= 0 when l == 0, n >= 1 when l == m == 0), |l| < kx, |m| < ky, |n| < kz,
      kept iff k^2 < rkcut^2 - decided in fp64 exactly as finish_model decides it (kvectors below; a k-vector ON the sphere is in or out by its
      last bit, so the rule is part of the operation, not of the precision)
  akk = exp(-k^2 / 4 alpha^2) / k^2
  S(k) = sum_j q_j exp(i k r_j)                        E = scale sum_k akk |S(k)|^2
  F_i = scale2 sum_k akk Im(conj(S(k)) q_i exp(i k r_i)) k            scale = 4 pi Fcoul_scale / (a b c), scale2 = 2 scale
Every phase is evaluated directly, cos / sin((l x / a + m y / b + n z / c) 2 pi): no per-axis tables, no recurrence, no conjugation tricks - a
route that shares nothing with the kernels' but the formula.  With the truncated pi the phase is NOT periodic in x / a: 2 pi_model l x / a is the
number the kernels' recurrence raises exp(i 2 pi_model x / a) to, so it is taken as it stands, without any reduction.

Condition scales (sums of the absolute values of the terms, as in tests/pair_reference.py): a kernel is held to |F_gpu,i - F_i| <= TAU S_F,i and
|E_gpu - E| <= TAU S_E with TAU = pair_cases.TAU,
  S_F,i = scale2 |q_i| sum_k akk |S(k)| (|kx| + |ky| + |kz|)          S_E = scale sum_k akk |S(k)| sum_j |q_j|

Two engines, one interface (reciprocal(case, engine)): "mp" - mpmath at 50 digits, for up to a few hundred atoms times k-vectors (it feeds the
committed fixture tests/golden/ewald_reciprocal.npz); "ld" - numpy.longdouble (x87 extended, eps 1.08e-19), vectorised, for the cases too large to
store, evaluated at test time.  Both return longdouble arrays, so that they can be compared with each other below fp64's resolution.
restate_fp64 is the kernels' own route (per-axis harmonics by the recurrence, conjugation for negative m / n, the work-item and group tables of
Engine::upload_ewald, the summation tree of S(k)) in numpy fp64: the CPU test shows that it stays within the bounds, and that the bounds catch its mutations.

mpmath is imported only where the "mp" engine runs: the GPU test needs numpy alone.
"""
import math
import os

import numpy as np

import pair_cases as pc

LD = np.longdouble
PI_STR = "3.14159265359"                                      # csrc/model.h units::pi
SI = {"r": "1.0E-10", "E": "1.60217733E-19", "q": "1.60217657E-19", "e0": "8.854187817E-12"}     # csrc/model.h namespace units
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ewald_reciprocal.npz")


def require_longdouble():
    """The "ld" engine is a reference only where long double is wider than double; where it is not, the tests that need it FAIL (no skip)."""
    eps = float(np.finfo(LD).eps)
    assert eps < 2e-19, "numpy.longdouble has eps %.3g here: no extended precision, the longdouble Ewald reference cannot be trusted" % eps


# ---- the k-vector list: finish_model's loop and cut-off rule, operation by operation, in fp64 -----------------------------------------------
def kvectors(box, alpha, ewald_k):
    """dict(lmn int32 (nK, 3), rk fp64 (nK, 3), akk fp64 (nK,), rkcut2, mr4a2) in the order finish_model lists them (l, then m, then n)."""
    la, lb, lc = (float(v) for v in box)
    kx, ky, kz = (int(v) for v in ewald_k)
    twopi = 2.0 * pc.PI
    ra, rb, rc = 1.0 / la, 1.0 / lb, 1.0 / lc
    mr4a2 = -0.25 / alpha / alpha
    axb3, bxc1, cxa2 = la * lb, lb * lc, la * lc
    vol = la * lb * lc
    det = la * bxc1
    rdet, rv = 1.0 / det, 1.0 / vol
    iax, iby, icz = rdet * bxc1, rdet * cxa2, rdet * axb3
    iaxb3, ibxc1, icxa2 = iax * iby, iby * icz, iax * icz
    ip1, ip2, ip3 = rv / math.sqrt(ibxc1 * ibxc1), rv / math.sqrt(icxa2 * icxa2), rv / math.sqrt(iaxb3 * iaxb3)
    rkcut = kx * ip1
    if rkcut > ky * ip2:
        rkcut = ky * ip2
    if rkcut > kz * ip3:
        rkcut = kz * ip3
    rkcut *= twopi * 1.05
    rkcut2 = rkcut * rkcut
    l, m, n = np.meshgrid(np.arange(kx), np.arange(1 - ky, ky), np.arange(1 - kz, kz), indexing="ij")
    l, m, n = l.ravel(), m.ravel(), n.ravel()
    half = (l > 0) | (m > 0) | ((m == 0) & (n >= 1))
    l, m, n = l[half], m[half], n[half]
    rkx, rky, rkz = l * twopi * ra, m * twopi * rb, n * twopi * rc          # (int * twopi) * ra, as the loop forms them
    rk2 = rkx * rkx + rky * rky + rkz * rkz
    keep = rk2 < rkcut2
    l, m, n, rkx, rky, rkz, rk2 = (v[keep] for v in (l, m, n, rkx, rky, rkz, rk2))
    akk = np.array([math.exp(v * mr4a2) / v for v in rk2.tolist()], dtype=np.float64).reshape(-1)
    return {"lmn": np.stack([l, m, n], 1).astype(np.int32).reshape(-1, 3), "rk": np.stack([rkx, rky, rkz], 1).reshape(-1, 3), "akk": akk,
            "rkcut2": rkcut2, "mr4a2": mr4a2}


def charges(case):
    return np.array([q for _, q in case["species"]], dtype=np.float64)[np.asarray(case["types"])]


# ---- engine "ld": numpy.longdouble ----------------------------------------------------------------------------------------------------------
def _ld_consts(case):
    pi = LD(PI_STR)
    r, E, q, e0 = (LD(SI[k]) for k in ("r", "E", "q", "e0"))
    fcoul = (LD("0.25") / pi / e0 * q * q / r / r) / (E / r)
    a, b, c = (LD(float(v)) for v in case["box"])
    scale = 4 * pi * fcoul / (a * b * c)
    return pi, fcoul, (a, b, c), scale


def _reciprocal_ld(case, kv, chunk=1 << 21):
    require_longdouble()
    pi, _, (a, b, c), scale = _ld_consts(case)
    twopi = 2 * pi
    q = charges(case).astype(LD)
    N = len(q)
    u, v, w = np.asarray(case["x"], dtype=LD) / a, np.asarray(case["y"], dtype=LD) / b, np.asarray(case["z"], dtype=LD) / c
    lmn = kv["lmn"].astype(LD)
    kvec = lmn * (twopi / np.array([a, b, c], dtype=LD))
    k2 = (kvec * kvec).sum(1)
    al = LD(float(case["alpha"]))
    akk = np.exp(-k2 / (4 * al * al)) / k2
    nK = len(k2)
    S = np.zeros((nK, 2), dtype=LD)
    F = np.zeros((N, 3), dtype=LD)
    step = max(1, chunk // max(N, 1))
    for k0 in range(0, nK, step):
        sl = slice(k0, min(nK, k0 + step))
        arg = (lmn[sl, 0:1] * u[None, :] + lmn[sl, 1:2] * v[None, :] + lmn[sl, 2:3] * w[None, :]) * twopi
        co, si = np.cos(arg), np.sin(arg)
        sc, ss = (co * q).sum(1), (si * q).sum(1)
        S[sl, 0], S[sl, 1] = sc, ss
        x = (si * sc[:, None] - co * ss[:, None]) * akk[sl, None]            # akk Im(conj(S) e^{ikr}), per (k, atom)
        for d in range(3):
            F[:, d] += (x * kvec[sl, d:d + 1]).sum(0)
    F *= (2 * scale) * q[:, None]
    absS = np.sqrt(S[:, 0] ** 2 + S[:, 1] ** 2)
    E = scale * (akk * (S[:, 0] ** 2 + S[:, 1] ** 2)).sum()
    SF = (2 * scale) * np.abs(q) * (akk * absS * np.abs(kvec).sum(1)).sum()
    SE = scale * (akk * absS).sum() * np.abs(q).sum()
    return {"lmn": kv["lmn"], "S": S, "E": E, "F": F, "SF": SF, "SE": SE, "scale": scale}


# ---- engine "mp": mpmath, 50 digits ---------------------------------------------------------------------------------------------------------
def _to_ld(v):
    """mpf -> longdouble through a (hi, lo) pair of doubles: exact to about 1e-32 relative, far below longdouble's own eps"""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def _reciprocal_mp(case, kv):
    import mpmath as mp
    import pair_reference as pr                                # sets 50 digits; fcoul_scale() with the model's pi
    assert mp.mp.dps >= 50
    M = lambda t: mp.mpf(float(t))
    pi = mp.mpf(PI_STR)
    twopi = 2 * pi
    a, b, c = (M(t) for t in case["box"])
    scale = 4 * pi * pr.fcoul_scale(pi) / (a * b * c)
    q = [M(t) for t in charges(case)]
    N = len(q)
    u, v, w = [M(t) / a for t in case["x"]], [M(t) / b for t in case["y"]], [M(t) / c for t in case["z"]]
    al = M(case["alpha"])
    F = [[mp.mpf(0)] * 3 for _ in range(N)]
    S, E, sumF, sumE = [], mp.mpf(0), mp.mpf(0), mp.mpf(0)
    live = [i for i in range(N) if q[i] != 0]
    for l, m, n in kv["lmn"].tolist():
        kvec = (l * twopi / a, m * twopi / b, n * twopi / c)
        k2 = kvec[0] ** 2 + kvec[1] ** 2 + kvec[2] ** 2
        akk = mp.exp(-k2 / (4 * al * al)) / k2
        cs = {i: mp.cos_sin((l * u[i] + m * v[i] + n * w[i]) * twopi) for i in live}
        sc = mp.fsum(q[i] * cs[i][0] for i in live)
        ss = mp.fsum(q[i] * cs[i][1] for i in live)
        S.append((sc, ss))
        for i in live:
            x = akk * (cs[i][1] * sc - cs[i][0] * ss)
            F[i] = [F[i][d] + x * kvec[d] for d in range(3)]
        absS = mp.sqrt(sc * sc + ss * ss)
        E += akk * (sc * sc + ss * ss)
        sumF += akk * absS * (abs(kvec[0]) + abs(kvec[1]) + abs(kvec[2]))
        sumE += akk * absS
    qabs = mp.fsum(abs(t) for t in q)
    out = {"lmn": kv["lmn"], "S": np.array([[_to_ld(t) for t in row] for row in S], dtype=LD).reshape(-1, 2),
           "E": _to_ld(scale * E), "F": np.array([[_to_ld(2 * scale * q[i] * F[i][d]) for d in range(3)] for i in range(N)], dtype=LD).reshape(N, 3),
           "SF": np.array([_to_ld(2 * scale * abs(q[i]) * sumF) for i in range(N)], dtype=LD), "SE": _to_ld(scale * sumE * qabs),
           "scale": _to_ld(scale)}
    return out


def reciprocal(case, engine="ld", kv=None):
    """S(k) (nK, 2), E, F (N, 3), S_F (N,), S_E of `case`, as longdouble; engine "mp" (mpmath, 50 digits) or "ld" (numpy.longdouble)."""
    kv = kv or kvectors(case["box"], case["alpha"], case["ewald_k"])
    return _reciprocal_mp(case, kv) if engine == "mp" else _reciprocal_ld(case, kv)


# ---- the kernels' own route in numpy fp64 (what the bounds are shown to pass, and to catch) --------------------------------------------------
MUTATIONS = ("atom_missing_from_S", "minus_n_takes_plus_n", "sign_of_m_ignored", "T_shifted_in_one_group")


def _harmonics(arg, n, pref):
    """ew_harmonics: out[h] = pref * exp(i arg)^h by repeated complex multiplication; (c, s) arrays of shape (n, N)"""
    e1c, e1s = np.cos(arg), np.sin(arg)
    cc, cs_ = np.ones_like(arg), np.zeros_like(arg)
    C, S = np.empty((n, len(arg))), np.empty((n, len(arg)))
    for h in range(n):
        C[h], S[h] = pref * cc, pref * cs_
        if h == 0:
            cc, cs_ = e1c, e1s
        else:
            cc, cs_ = cc * e1c - cs_ * e1s, cs_ * e1c + e1s * cc
    return C, S


def _seq(a):
    """left-to-right sum (numpy's add.reduce is pairwise; cumsum is sequential)"""
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


TILE, MAX_BLOCKS, RED_GROUPS = 64, 1024, 16                   # kEwTile, the cap of nBlocksA (Engine::upload_ewald), kEwRedGroups


def _tree(a):
    """The summation tree of S(k) (csrc/ewald.hip.h): tiles of 64 atoms summed left to right; block b of nB = min(1024, ceil(N / 64)) adds the
    tiles b, b + nB, ... in that order; k_ewald_reduce's group g adds the rows g, g + 16, ...; the 16 group sums are added in group order."""
    nT = max(1, -(-len(a) // TILE))
    nB = min(MAX_BLOCKS, nT)
    rounds = -(-nT // nB)
    t = np.zeros(rounds * nB * TILE)
    t[:len(a)] = a
    tiles = np.cumsum(t.reshape(rounds * nB, TILE), axis=1)[:, -1]
    rows = np.cumsum(tiles.reshape(rounds, nB), axis=0)[-1]
    r = np.zeros(-(-nB // RED_GROUPS) * RED_GROUPS)
    r[:nB] = rows
    groups = np.cumsum(r.reshape(-1, RED_GROUPS), axis=0)[-1]
    return float(np.cumsum(groups)[-1])


def restate_fp64(case, kv=None, mutate=None, sequential=False):
    """{"F", "E", "S"} by the kernels' arithmetic in fp64.  mutate: None or one of MUTATIONS - faults of the kind the kernels could have.
    sequential: S(k) summed atom after atom, as the serial code does, instead of in the kernels' tree (with 70 000 atoms the partial sums
    of a plain loop wander far above |S(k)|, and its error with them: 5e-14 S_F against 4e-15 S_F for the tree)."""
    ssum = _seq if sequential else _tree
    assert mutate is None or mutate in MUTATIONS
    kv = kv or kvectors(case["box"], case["alpha"], case["ewald_k"])
    lmn, akk = kv["lmn"], kv["akk"]
    kx, ky, kz = (int(t) for t in case["ewald_k"])
    L = [float(t) for t in case["box"]]
    invL = [1.0 / t for t in L]
    twopi = 2.0 * pc.PI
    scale = 2 * twopi * (1.0 / (L[0] * L[1] * L[2])) * pc.FCOUL
    scale2 = 2 * scale
    q = charges(case)
    N = len(q)
    XC, XS = _harmonics(twopi * np.asarray(case["x"], dtype=np.float64) * invL[0], kx, q)
    YC, YS = _harmonics(twopi * np.asarray(case["y"], dtype=np.float64) * invL[1], ky, 1.0)
    ZC, ZS = _harmonics(twopi * np.asarray(case["z"], dtype=np.float64) * invL[2], kz, 1.0)
    nK = len(akk)
    index = {tuple(r): k for k, r in enumerate(lmn.tolist())}
    keepS = np.ones(N, dtype=bool)
    if mutate == "atom_missing_from_S":
        keepS[np.flatnonzero(q != 0.0)[-1]] = False              # the last charged atom: the partial last tile's last real lane
    S = np.zeros((nK, 2))
    for k, (l, m, n) in enumerate(lmn.tolist()):
        sm = -1.0 if (m < 0 and mutate != "sign_of_m_ignored") else 1.0
        emc, ems = YC[abs(m)], YS[abs(m)] * sm
        lmc, lms = XC[l] * emc - XS[l] * ems, XS[l] * emc + ems * XC[l]
        enc, ens = ZC[abs(n)], ZS[abs(n)]
        cc, ss, sc, cs_ = lmc * enc, lms * ens, lms * enc, lmc * ens
        if n >= 0:
            S[k] = ssum(np.where(keepS, cc - ss, 0.0)), ssum(np.where(keepS, sc + cs_, 0.0))
        else:
            S[k] = ssum(np.where(keepS, cc + ss, 0.0)), ssum(np.where(keepS, sc - cs_, 0.0))
    if mutate == "minus_n_takes_plus_n":
        k = next(k for k, (l, m, n) in enumerate(lmn.tolist()) if n < 0 and (l, m, -n) in index)
        l, m, n = lmn[k].tolist()
        S[k] = S[index[(l, m, -n)]]
    E = scale * _seq(akk * (S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]))
    T = (akk * scale2)[:, None] * S
    # groups of k_ewald_force: runs of consecutive n with the same (l, m); T is addressed as Tg[n] with Tg = T + kStart - nLo
    starts = [k for k in range(nK) if k == 0 or lmn[k, 0] != lmn[k - 1, 0] or lmn[k, 1] != lmn[k - 1, 1] or lmn[k - 1, 2] + 1 != lmn[k, 2]]
    shifted = starts[len(starts) // 2] if mutate == "T_shifted_in_one_group" else -1
    fx, fy, fz = np.zeros(N), np.zeros(N), np.zeros(N)
    for gi, k0 in enumerate(starts):
        k1 = starts[gi + 1] if gi + 1 < len(starts) else nK
        l, m = int(lmn[k0, 0]), int(lmn[k0, 1])
        emc, ems = YC[abs(m)], (YS[abs(m)] if (m >= 0 or mutate == "sign_of_m_ignored") else -YS[abs(m)])
        lmc, lms = XC[l] * emc - XS[l] * ems, XS[l] * emc + ems * XC[l]
        sx, sz = np.zeros(N), np.zeros(N)
        for k in range(k0, k1):
            n = int(lmn[k, 2])
            enc, ens = ZC[abs(n)], (ZS[abs(n)] if n >= 0 else -ZS[abs(n)])
            ckc, cks = lmc * enc - lms * ens, lms * enc + ens * lmc
            kt = min(k + 1, nK - 1) if k0 == shifted else k
            x = cks * T[kt, 0] - ckc * T[kt, 1]
            sx += x
            sz += n * x
        fx += (l * (twopi * invL[0])) * sx
        fy += (m * (twopi * invL[1])) * sx
        fz += sz
    fz *= twopi * invL[2]
    return {"F": np.stack([fx, fy, fz], 1), "E": E, "S": S}


def worst_ratios(F, E, ref):
    """(max_i |F_i - F_ref,i| / S_F,i, |E - E_ref| / S_E) against a reciprocal() result; an atom with S_F = 0 (a neutral one) must have F = 0"""
    dF = np.asarray(F, dtype=LD) - ref["F"]
    err = np.sqrt((dF * dF).sum(1))
    SF = ref["SF"]
    assert (err[SF == 0] == 0).all(), "a neutral atom carries a reciprocal force"
    rF = float((err[SF > 0] / SF[SF > 0]).max()) if (SF > 0).any() else 0.0
    return rF, float(abs(LD(E) - ref["E"]) / ref["SE"])


# ---- the isolated systems --------------------------------------------------------------------------------------------------------------------
# Charged species WITHOUT any VdW entry on a jittered lattice whose spacing exceeds rReal by more than twice the jitter: no pair lies inside
# the real-space cut-off, the pair kernels add exactly nothing, and the force the engine returns is the reciprocal part alone.  Species 0 is
# neutral (so the charged species are not first in the table) and is interleaved with the two charged ones; the lattice planes of index 0 sit
# ON the periodic walls (their atoms wrap), and in the cases with `walls` six atoms of those planes have a coordinate of exactly 0 or of the
# last double below L.  alpha follows the k-space cut-off, exp(-k_cut^2 / 4 alpha^2) ~ e^-6, so that the outermost harmonics still carry
# about 1e-3 of the sum - far above TAU - instead of vanishing against the first shell.
RREAL, JITTER = 2.0, 0.4
SPECIES = [(20.18, 0.0), (22.99, 0.7), (35.45, -1.1)]
TYPE_PATTERN = (1, 2, 0, 2, 1, 1, 0, 2)
#            atoms  ewald_k       lattice spacing     walls  stored (mpmath fixture) or evaluated at test time in longdouble
ISOLATED = {
    "n1":     (1,     (4, 4, 4),    (3.0, 3.0, 3.0),    False, True),
    "n2":     (2,     (4, 4, 4),    (3.0, 3.0, 3.0),    False, True),
    "n63":    (63,    (4, 4, 4),    (3.0, 3.0, 3.0),    False, True),
    "n64":    (64,    (4, 4, 4),    (3.0, 3.0, 3.0),    False, True),
    "n65":    (65,    (4, 4, 4),    (3.0, 3.0, 3.0),    True,  True),
    "n500":   (500,   (4, 4, 4),    (3.0, 3.0, 3.0),    True,  True),
    "n70000": (70000, (4, 4, 4),    (3.0, 3.0, 3.0),    True,  False),
    "k114":   (100,   (1, 1, 4),    (3.0, 3.0, 9.0),    False, True),      # c = 3 a: n = 1, 2, 3 all lie inside the cut-off 1.05 * 2 pi / a
    "k411":   (100,   (4, 1, 1),    (9.0, 3.0, 3.0),    False, True),
    "k151":   (100,   (1, 5, 1),    (3.0, 12.0, 3.0),   False, True),
    "k479":   (100,   (4, 7, 9),    (3.0, 4.4, 5.8),    True,  True),
    "k19":    (100,   (19, 19, 19), (3.0, 3.0, 3.0),    False, True),
    "k48":    (100,   (48, 48, 48), (3.0, 3.0, 3.0),    False, False),     # kEwaldKMax: 144 harmonics, 156 KiB of LDS in k_ewald_force
}
STORED = [k for k, v in ISOLATED.items() if v[4]]
LIVE = [k for k, v in ISOLATED.items() if not v[4]]


def isolated_case(name, xyz=None):
    """Engine / oracle input of isolated system `name`.  xyz: the coordinates the fixture stores (the placement's random stream then plays no
    part); without it they are generated (generator of the fixture, and the cases evaluated at test time)."""
    N, ek, sp, walls, _ = ISOLATED[name]
    g = max(6, int(math.ceil(N ** (1.0 / 3.0) - 1e-9)))
    sp = np.array(sp)
    box = g * sp
    kcut = 1.05 * 2.0 * pc.PI * min(k / b for k, b in zip(ek, box))
    alpha = round(kcut / 4.9, 4)
    if xyz is None:
        rng = np.random.Generator(np.random.PCG64(7000 + N + 97 * sum(ek)))
        sites = rng.permutation(g ** 3)[:N]
        sites = np.sort(sites) if N > 1000 else sites            # (large case: keep neighbours in the list near each other, as a liquid's file would)
        idx = np.stack([sites // (g * g), (sites // g) % g, sites % g], 1)
        X = idx * sp + rng.uniform(-JITTER, JITTER, size=(N, 3))
        if walls:                                                # atoms of the wall planes: coordinate exactly 0 / the last double below L
            for ax in range(3):
                on = np.flatnonzero(idx[:, ax] == 0)
                assert len(on) >= 2
                X[on[0], ax] = 0.0
                X[on[1], ax] = -1e-300                           # wraps to nextafter(L, 0) below
        X = np.where(X < 0, X + box, X)
        X = np.minimum(X, np.nextafter(box, 0.0))
    else:
        X = np.array(xyz, dtype=np.float64)
        assert X.shape == (N, 3)
    types = np.array([TYPE_PATTERN[i % len(TYPE_PATTERN)] for i in range(N)], dtype=np.int32)
    return {"box": [float(v) for v in box], "dt": 0.001, "nsteps": 0, "species": list(SPECIES), "names": ["Ne", "Na", "Cl"], "vdw": [],
            "types": types, "x": X[:, 0].copy(), "y": X[:, 1].copy(), "z": X[:, 2].copy(), "vx": np.zeros(N), "vy": np.zeros(N), "vz": np.zeros(N),
            "elec_type": 2, "rReal": RREAL, "alpha": alpha, "ewald_k": tuple(ek), "T": 0.0, "tstat_type": 0, "nEq": 0, "freqEq": 1, "use_clist": 1,
            "cell_list": 6.0, "center_box": 0, "init_forces": 1, "seed": 12345}


def min_image_distance(case, block=2048):
    """smallest minimum-image distance between two atoms (the placement rule: it exceeds rReal); cell-binned, so 70 000 atoms are cheap"""
    X = np.stack([case["x"], case["y"], case["z"]], 1)
    box = np.array(case["box"])
    N = len(X)
    if N < 2:
        return math.inf
    nc = np.maximum(1, np.floor(box / (RREAL + 2 * JITTER + 0.2)).astype(int))
    if N <= 3000 or (nc < 3).any():
        best = math.inf
        for i0 in range(0, N, block):
            d = X[i0:i0 + block, None, :] - X[None, :, :]
            d -= box * np.round(d / box)
            r2 = (d * d).sum(-1)
            r2[np.arange(len(r2)), np.arange(i0, i0 + len(r2))] = math.inf
            best = min(best, float(r2.min()))
        return math.sqrt(best)
    # every pair closer than the cell edge lies in the same or in adjacent cells: compare each cell's atoms with the 27 shifted copies
    ci = np.minimum((X / box * nc).astype(int), nc - 1)
    key = (ci[:, 0] * nc[1] + ci[:, 1]) * nc[2] + ci[:, 2]
    order = np.argsort(key, kind="stable")
    start = np.searchsorted(key[order], np.arange(nc.prod() + 1))
    best = math.inf
    occ = np.diff(start).max()
    slots = np.full((nc.prod(), occ), -1)
    for s in range(occ):
        has = start[:-1] + s < start[1:]
        slots[has, s] = order[start[:-1][has] + s]
    grid = slots.reshape(nc[0], nc[1], nc[2], occ)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                other = np.roll(grid, (dx, dy, dz), axis=(0, 1, 2))
                for s in range(occ):
                    for t in range(occ):
                        a, b = grid[..., s].ravel(), other[..., t].ravel()
                        ok = (a >= 0) & (b >= 0) & (a != b)
                        d = X[a[ok]] - X[b[ok]]
                        d -= box * np.round(d / box)
                        if len(d):
                            best = min(best, float((d * d).sum(1).min()))
    return math.sqrt(best)


def rocksalt_case(n=8, r0=2.82, q=1.0):
    """The rock-salt lattice of test_oracle_golden.test_ewald_madelung_constant: 512 ions, energy -M k q^2 / r0 per ion pair"""
    g = np.arange(n)
    ii, jj, kk = np.meshgrid(g, g, g, indexing="ij")
    pos = np.stack([ii.ravel(), jj.ravel(), kk.ravel()], axis=1).astype(float) * r0 + 0.1
    types = ((ii + jj + kk).ravel() % 2).astype(np.int32)
    N = len(types)
    L = n * r0
    return {"box": [L, L, L], "dt": 0.001, "species": [(22.99, q), (35.45, -q)], "vdw": [], "types": types,
            "x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": np.zeros(N), "vy": np.zeros(N), "vz": np.zeros(N),
            "elec_type": 2, "rReal": 11.0, "alpha": 0.3, "ewald_k": (10, 10, 10), "use_clist": 0}


def dense_case():
    """test_gpu_parity.ewald_case: 500 ions (+-0.4 e, Lennard-Jones), 'elec pme 6.5 0.45 6 6 6'"""
    from aztotmd_amd import inputs
    c = inputs.lj_case((5, 5, 5), a=5.26, seed=11, rc=6.5, cell_list=6.5, charges=(0.4, -0.4), elec="fenn", r_real=6.5, alpha=0.45, vel_T=80.0)
    c.update(elec_type=2, ewald_k=(6, 6, 6))
    return c


# ---- the dense system: reciprocal part + every real-space and Lennard-Jones pair term, all in mpmath ----------------------------------------
def dense_reference(case):
    """Per atom: total force and its scale S_F,i + sum_pairs S_F r; the four energies with their scales."""
    import mpmath as mp
    import pair_reference as pr
    M = lambda t: mp.mpf(float(t))
    rec = reciprocal(case, "mp")
    N = len(case["types"])
    box = [M(t) for t in case["box"]]
    X = [[M(case[k][i]) for k in ("x", "y", "z")] for i in range(N)]
    Xf = np.stack([case["x"], case["y"], case["z"]], 1)
    bf = np.array(case["box"])
    q = charges(case)
    pots = {}
    for a, b, ty, rc, p in case["vdw"]:
        pots[(a, b)] = pots[(b, a)] = (ty, rc, p)
    r2Max = case["rReal"] * case["rReal"]
    F = [[mp.mpf(0)] * 3 for _ in range(N)]
    SF = [mp.mpf(0)] * N
    ev = ec = sev = sec = mp.mpf(0)
    npairs = 0
    for i in range(N - 1):
        d = Xf[i] - Xf[i + 1:]
        d -= bf * np.round(d / bf)
        r2 = (d * d).sum(1)
        for j in (np.flatnonzero(r2 <= r2Max * (1 + 1e-9)) + i + 1).tolist():
            dm = [X[i][k] - X[j][k] for k in range(3)]
            dm = [t - box[k] if t > box[k] / 2 else (t + box[k] if t < -box[k] / 2 else t) for k, t in enumerate(dm)]
            rr = dm[0] ** 2 + dm[1] ** 2 + dm[2] ** 2
            assert abs(float(rr) - r2Max) > 1e-9 * r2Max, "a pair on the cut-off: its membership would hang on the engine's rounding"
            if float(rr) > r2Max:
                continue
            r = mp.sqrt(rr)
            f = sf = mp.mpf(0)
            pt = pots.get((int(case["types"][i]), int(case["types"][j])))
            if pt is not None:
                assert abs(float(rr) - pt[1] ** 2) > 1e-9 * pt[1] ** 2
                if float(rr) <= pt[1] ** 2:
                    df, u, dsf, se = pr.vdw(pt[0], pt[2], r)
                    f, sf, ev, sev = f + df, sf + dsf, ev + u, sev + se
            if abs(q[i]) > 1e-10 and abs(q[j]) > 1e-10:
                df, u, dsf, se = pr.coul(2, q[i], q[j], r, case["rReal"], case["alpha"])
                f, sf, ec, sec = f + df, sf + dsf, ec + u, sec + se
            assert float(f * f) < 1e9                              # far from the drop rule f^2 > 1e10
            for k in range(3):
                F[i][k] += f * dm[k]
                F[j][k] -= f * dm[k]
            SF[i] += sf * r
            SF[j] += sf * r
            npairs += 1
    # ewald_const (finish_model): Fcoul_scale (-alpha / sqrt(pi) sum q^2 - pi / 2 (sum q)^2 / alpha^2 / V), model pi
    pi, al = mp.mpf(PI_STR), M(case["alpha"])
    sq, sqq = mp.fsum(M(t) for t in q), mp.fsum(M(t) ** 2 for t in q)
    t1 = pr.fcoul_scale(pi) * al / mp.sqrt(pi) * sqq
    t2 = pr.fcoul_scale(pi) * pi / 2 * sq * sq / al / al / (box[0] * box[1] * box[2])
    Ft = np.array([[float(F[i][k]) for k in range(3)] for i in range(N)]) + rec["F"].astype(np.float64)
    return {"F": Ft, "SF": np.array([float(t) for t in SF]) + rec["SF"].astype(np.float64), "npairs": npairs,
            "engCoul": float(ec), "engCoul_scale": float(sec), "engVdW": float(ev), "engVdW_scale": float(sev),
            "engCoulRec": float(rec["E"]), "engCoulRec_scale": float(rec["SE"]), "engCoulConst": float(-t1 - t2), "engCoulConst_scale": float(t1 + t2)}


# ---- tests/golden/ewald_reciprocal.npz -------------------------------------------------------------------------------------------------------
def stored_reference(name):
    """One stored isolated system in the fixture's layout: x, y, z, fx, fy, fz, sf per atom; e, se; box, alpha, ewald_k as the builder gave them"""
    case = isolated_case(name)
    ref = reciprocal(case, "mp")
    F = ref["F"].astype(np.float64)
    return {"x": case["x"], "y": case["y"], "z": case["z"], "fx": F[:, 0].copy(), "fy": F[:, 1].copy(), "fz": F[:, 2].copy(),
            "sf": ref["SF"].astype(np.float64), "e": np.float64(ref["E"]), "se": np.float64(ref["SE"]), "box": np.array(case["box"]),
            "alpha": np.float64(case["alpha"]), "ewald_k": np.array(case["ewald_k"], dtype=np.int32), "nk": np.int32(len(ref["lmn"]))}


def make_fixture(path=None, names=None, dense=True):
    arrays = {}
    for name in (names if names is not None else STORED):
        for k, v in stored_reference(name).items():
            arrays["%s__%s" % (name, k)] = v
    if dense:
        case = dense_case()
        ref = dense_reference(case)
        for k in ("x", "y", "z"):
            arrays["dense__" + k] = np.asarray(case[k])
        for k, v in ref.items():
            arrays["dense__" + k] = np.asarray(v)
    if path:
        np.savez_compressed(path, **arrays)
    return arrays


_FIX = None


def fixture(name):
    """{field: value} of one system of the committed fixture ("dense" or a name of STORED)"""
    global _FIX
    if _FIX is None:
        _FIX = dict(np.load(FIXTURE))
    pre = name + "__"
    return {k[len(pre):]: v for k, v in _FIX.items() if k.startswith(pre)}


def fixture_case(name):
    """(case, reference) of a stored isolated system, built around the coordinates the fixture holds; the reference in reciprocal()'s layout"""
    R = fixture(name)
    case = isolated_case(name, xyz=np.stack([R["x"], R["y"], R["z"]], 1))
    assert np.array_equal(R["box"], case["box"]) and float(R["alpha"]) == case["alpha"] and tuple(R["ewald_k"]) == tuple(case["ewald_k"]), name
    ref = {"F": np.stack([R["fx"], R["fy"], R["fz"]], 1).astype(LD), "SF": R["sf"].astype(LD), "E": LD(float(R["e"])), "SE": LD(float(R["se"])),
           "nk": int(R["nk"])}
    return case, ref
