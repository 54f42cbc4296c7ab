"""High-precision (mpmath, 50 digits) restatement of every pair, bond and angle term the engine computes, from the USER-level parameters of
a case (field.txt / control.txt numbers), so that the constants the host folds (lj.p3 / p4, 1 / rho, el_scale2, Fcoul_scale) are tested too.

Every function returns (f, U, S_F, S_E): f = -(1/r) dU/dr, the energy U, and the condition scales of both: the sum of the absolute values of
the terms of the formula, plus |y| |A e^y| for every term A e^y (exp amplifies the rounding of its argument; erfc(x) = e^{-x^2} erfcx(x) counts
as one).  A kernel is held to |f_gpu - f| <= tau S_F: honest cancellations (the Lennard-Jones force zero, the Fennell shift at rReal) pass,
a wrong digit does not.

`pi` is a parameter: the engine uses the reference's truncated value (csrc/model.h units::pi) in Fcoul_scale and in 2 alpha / sqrt(pi); the
derivative checks pass mpmath's pi, for which f is exactly -(1/r) dU/dr.
"""
import mpmath as mp

mp.mp.dps = 50
MODEL_PI = mp.mpf("3.14159265359")                     # csrc/model.h units::pi


def fcoul_scale(pi=MODEL_PI):
    """units::Fcoul_scale (csrc/model.h): 0.25 / pi / e0 q^2 / r^2, over F_SI = E_SI / r_SI."""
    r_SI, E_SI, q_SI, e0_SI = mp.mpf("1e-10"), mp.mpf("1.60217733e-19"), mp.mpf("1.60217657e-19"), mp.mpf("8.854187817e-12")
    return (mp.mpf("0.25") / pi / e0_SI * q_SI * q_SI / r_SI / r_SI) / (E_SI / r_SI)


def _m(v):
    return mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v


def vdw(kind, p, r, radi=0.0, radj=0.0):
    """VdW term of type `kind` (inputs.VDW_TYPES ids or names) with the user-level parameters p of field.txt."""
    kind = {"lnjs": 1, "buck": 2, "p746": 3, "bmhs": 4, "elin": 5, "einv": 6, "surk": 7}.get(kind, kind)
    r = _m(r)
    p = [_m(v) for v in p] + [mp.mpf(0)] * (5 - len(p))
    A = abs
    if kind == 1:                      # 4 eps ((s/r)^12 - (s/r)^6)
        eps, sg = p[0], p[1]
        s6 = (sg / r) ** 6
        s12 = s6 * s6
        U = 4 * eps * (s12 - s6)
        f = 24 * eps / r ** 2 * (2 * s12 - s6)
        return f, U, 24 * A(eps) / r ** 2 * (2 * s12 + s6), 4 * A(eps) * (s12 + s6)
    if kind in (2, 5, 6):              # A exp(-r/rho) + {-C/r^6, C r, -C/r}
        a, rho, c = p[0], p[1], p[2]
        ex = a * mp.exp(-r / rho)
        y = r / rho
        fe = ex / (rho * r)
        if kind == 2:
            U, f, fc, ec = ex - c / r ** 6, fe - 6 * c / r ** 8, 6 * A(c) / r ** 8, A(c) / r ** 6
        elif kind == 5:
            U, f, fc, ec = ex + c * r, fe - c / r, A(c) / r, A(c) * r
        else:
            U, f, fc, ec = ex - c / r, fe - c / r ** 3, A(c) / r ** 3, A(c) / r
        return f, U, A(fe) * (1 + y) + fc, A(ex) * (1 + y) + ec
    if kind == 3:                      # p0/r^7 - p1/r^4 - p2/r^6
        U = p[0] / r ** 7 - p[1] / r ** 4 - p[2] / r ** 6
        f = 7 * p[0] / r ** 9 - 4 * p[1] / r ** 6 - 6 * p[2] / r ** 8
        return f, U, 7 * A(p[0]) / r ** 9 + 4 * A(p[1]) / r ** 6 + 6 * A(p[2]) / r ** 8, A(p[0]) / r ** 7 + A(p[1]) / r ** 4 + A(p[2]) / r ** 6
    if kind == 4:                      # A exp(B (sigma - r)) - C/r^6 - D/r^8
        a, b, sg, c, d = p
        y = b * (sg - r)
        ex = a * mp.exp(y)
        U = ex - c / r ** 6 - d / r ** 8
        f = b * ex / r - 6 * c / r ** 8 - 8 * d / r ** 10
        amp = A(b * r) + A(b * sg)                     # the kernel forms B (sigma - r): both products round
        return (f, U, A(b * ex / r) * (1 + amp) + 6 * A(c) / r ** 8 + 8 * A(d) / r ** 10,
                A(ex) * (1 + amp) + A(c) / r ** 6 + A(d) / r ** 8)
    if kind == 7:                      # surk: a b r^-6 (C1 a^2 b^2 / r - C2 / (ka a + kb b)), a, b = radii of atom i, j
        c1, c2, ka, kb = p[0], p[1], p[2], p[3]
        a, b = _m(radi), _m(radj)
        t1 = c1 * (a * b) ** 3
        t2 = c2 * a * b / (ka * a + kb * b)
        U = t1 / r ** 7 - t2 / r ** 6
        f = 7 * t1 / r ** 9 - 6 * t2 / r ** 8
        return f, U, 7 * A(t1) / r ** 9 + 6 * A(t2) / r ** 8, A(t1) / r ** 7 + A(t2) / r ** 6
    raise ValueError(kind)


def coul(elec, qi, qj, r, rReal=0.0, alpha=0.0, pi=MODEL_PI):
    """Real-space electrostatics of one pair: elec 1 direct, 3 Fennell/DSF, 2 real-space Ewald term (control.txt 'elec')."""
    r, rc, al = _m(r), _m(rReal), _m(alpha)
    kqq = _m(qi) * _m(qj) * fcoul_scale(pi)
    k = abs(kqq)
    if elec == 1:
        return kqq / r ** 3, kqq / r, k / r ** 3, k / r
    daipi2 = 2 * al / mp.sqrt(pi)
    y = (al * r) ** 2
    ex = mp.exp(-y)
    erfc = mp.erfc(al * r)
    if elec == 3:
        es = mp.erfc(al * rc) / rc
        es2 = mp.erfc(al * rc) / rc ** 2 + daipi2 * mp.exp(-(al * rc) ** 2) / rc
        U = kqq * (erfc / r - es + es2 * (r - rc))
        f = kqq / r * (erfc / r ** 2 + daipi2 * ex / r - es2)
        SF = k * (erfc / r ** 3 * (1 + y) + daipi2 * ex / r ** 2 * (1 + y) + es2 / r)
        SE = k * (erfc / r * (1 + y) + es + es2 * (r + rc))
        return f, U, SF, SE
    if elec == 2:
        U = kqq * erfc / r
        f = kqq / r ** 3 * (erfc + daipi2 * r * ex)
        return f, U, k / r ** 3 * (erfc + daipi2 * r * ex) * (1 + y), k * erfc / r * (1 + y)
    raise ValueError(elec)


def bond(kind, p, r):
    """Bond term (bonds.cpp bond_iter; user-level parameters of field.txt 'bonds'): 1 harm (k r0), 2 mors (D a r0 C), 3 pdn (D a r0 C E),
    4 buck (A ro C), 5 e612 (A ro C D F)."""
    r = _m(r)
    p = [_m(v) for v in p] + [mp.mpf(0)] * (5 - len(p))
    A = abs
    if kind == 1:
        k, r0 = p[0], p[1]
        return -k * (r - r0) / r, k * (r - r0) ** 2 / 2, A(k) * (r + A(r0)) / r, A(k) * (r + A(r0)) ** 2 / 2
    if kind in (2, 3):
        D, a, r0, C, E = p
        y = -a * (r - r0)
        x = mp.exp(y)
        amp = A(a * r) + A(a * r0)
        U = D * (1 - x) ** 2 - C - E / r ** 12
        f = -2 * D * a * x * (1 - x) / r - 12 * E / r ** 14
        SF = 2 * A(D * a * x) / r * ((1 + x) + 2 * x * amp) + 12 * A(E) / r ** 14
        SE = A(D) * ((1 + x) ** 2 + 2 * x * (1 + x) * amp) + A(C) + A(E) / r ** 12
        return f, U, SF, SE
    if kind in (4, 5):
        a, ro, C, Dd, F = p
        ex = a * mp.exp(-r / ro)
        y = r / ro
        U = ex - C / r ** 6 - Dd / r ** 8 - F / r ** 12
        f = ex / (r * ro) - 6 * C / r ** 8 - 8 * Dd / r ** 10 - 12 * F / r ** 14
        return (f, U, A(ex / (r * ro)) * (1 + y) + 6 * A(C) / r ** 8 + 8 * A(Dd) / r ** 10 + 12 * A(F) / r ** 14,
                A(ex) * (1 + y) + A(C) / r ** 6 + A(Dd) / r ** 8 + A(F) / r ** 12)
    raise ValueError(kind)


def angle(k, cos0, u, v):
    """hcos angle U = k/2 (cos th - cos0)^2 between u = x_l1 - x_c and v = x_l2 - x_c (angles.cpp angle_iter).
    Returns (F_c, F_l1, F_l2, U, S_F per atom (3,), S_E)."""
    k, c0 = _m(k), _m(cos0)
    u = [_m(a) for a in u]
    v = [_m(a) for a in v]
    ru = mp.sqrt(sum(a * a for a in u))
    rv = mp.sqrt(sum(a * a for a in v))
    c = sum(a * b for a, b in zip(u, v)) / (ru * rv)
    dc = c - c0
    gu = [b / (ru * rv) - c * a / ru ** 2 for a, b in zip(u, v)]     # d cos / d u
    gv = [a / (ru * rv) - c * b / rv ** 2 for a, b in zip(u, v)]
    F1 = [-k * dc * g for g in gu]
    F2 = [-k * dc * g for g in gv]
    Fc = [-(a + b) for a, b in zip(F1, F2)]
    s = abs(k) * (abs(c) + abs(c0))                   # the rounding of cos th is absolute: scaled by k and the gradient's terms
    S1, S2 = s * 2 / ru, s * 2 / rv
    return Fc, F1, F2, k * dc * dc / 2, (S1 + S2, S1, S2), abs(k) * (abs(c) + abs(c0)) ** 2 / 2


def numeric_f(U_of_r, r):
    """-(1/r) dU/dr by mpmath's numerical differentiation (the CPU test's check of the analytic forces)."""
    r = _m(r)
    return -mp.diff(U_of_r, r) / r


# ---- reference values of the isolated-pair cases (tests/pair_cases.py) -> tests/golden/pair_functions.npz ----------------------------------
# per pair: the case, the atoms' coordinates (the GPU test builds its systems from them), d, f, the energies and their condition scales
FIXTURE_KEYS = ("case", "xi", "yi", "zi", "xj", "yj", "zj", "dx", "dy", "dz", "f", "uv", "uc", "sf", "sev", "sec", "fa", "fb", "ua", "ub")
# per atom of the bonded cases: the case, coordinates, reference force and its scale; per bonded case: energy and its scale
BONDED_KEYS = ("bcase", "bx", "by", "bz", "bfx", "bfy", "bfz", "bsf")


def case_reference(name):
    """Per pair of case `name`: f (total, before the drop rule), uv / uc (VdW / Coulomb energy), sf / sev / sec (condition scales).  The inclusion
    predicates are the reference's, in fp64 on the exact d: VdW iff r^2 <= rc*rc (and r^2 <= rMax^2), Coulomb iff both species are charged and
    r^2 <= rReal^2.  surk: f = (ab)^3 fa - ab / (ka a + kb b) fb, U = (ab)^3 ua - ab / (ka a + kb b) ub with the radii a, b the engine holds."""
    import numpy as np
    import pair_cases as pc
    s = pc.spec(name)
    case, pairs = pc.build(name)
    r2 = pc.r2_fp64(pairs)
    rM = pc.r_max(s)
    r2Max = rM * rM
    pots = pc.pot_table(s)
    keys = ("f", "uv", "uc", "sf", "sev", "sec", "fa", "fb", "ua", "ub")
    out = {k: [] for k in keys}
    for k in range(len(r2)):
        a, b = int(pairs["ti"][k]), int(pairs["tj"][k])
        r = mp.sqrt(_m(pairs["dx"][k]) ** 2 + _m(pairs["dy"][k]) ** 2 + _m(pairs["dz"][k]) ** 2)
        f = uv = uc = sf = sev = sec = fa = fb = ua = ub = mp.mpf(0)
        if r2[k] <= r2Max:
            pt = pots.get((a, b))
            if pt is not None and r2[k] <= pt[1] * pt[1]:
                ty, rc, p = pt
                if ty == 7:
                    fa, ua = 7 * _m(p[0]) / r ** 9, _m(p[0]) / r ** 7
                    fb, ub = 6 * _m(p[1]) / r ** 8, _m(p[1]) / r ** 6
                else:
                    df, uv, dsf, sev = vdw(ty, p, r)
                    f, sf = f + df, sf + dsf
            qa, qb = s["species"][a][1], s["species"][b][1]
            if s["elec"] and abs(qa) > 1e-10 and abs(qb) > 1e-10:
                df, uc, dsf, sec = coul(s["elec"], qa, qb, r, s["rReal"], s["alpha"])
                f, sf = f + df, sf + dsf
        for key, v in zip(keys, (f, uv, uc, sf, sev, sec, fa, fb, ua, ub)):
            out[key].append(float(v))
    res = {k: np.array(v) for k, v in out.items()}
    X = np.stack([case["x"], case["y"], case["z"]], 1)
    res.update(dx=pairs["dx"], dy=pairs["dy"], dz=pairs["dz"], xi=X[pairs["i"], 0], yi=X[pairs["i"], 1], zi=X[pairs["i"], 2],
               xj=X[pairs["j"], 0], yj=X[pairs["j"], 1], zj=X[pairs["j"], 2])
    return res


def bonded_reference(name):
    """Per atom of bonded case `name`: reference force (3,), its scale (|F_gpu - F| <= tau scale), and the case's energy with its scale."""
    import numpy as np
    import pair_cases as pc
    case, mols = pc.build_bonded(name)
    X = [[_m(v) for v in row] for row in np.stack([case["x"], case["y"], case["z"]], 1)]
    N = len(X)
    F = [[mp.mpf(0)] * 3 for _ in range(N)]
    S = [mp.mpf(0)] * N
    E = SE = mp.mpf(0)
    for a, b, t in case["bonds"]:
        bt = pc.BOND_TYPES[t - 1]
        d = [X[a][k] - X[b][k] for k in range(3)]
        r = mp.sqrt(sum(v * v for v in d))
        f, U, sf, se = bond(bt[2], bt[3], r)
        for k in range(3):
            F[a][k] += f * d[k]
            F[b][k] -= f * d[k]
        S[a] += sf * r; S[b] += sf * r
        E += U; SE += se
    for c, l1, l2, t in case["angles"]:
        k_, c0 = pc.ANGLE_TYPE[2]
        u = [X[l1][k] - X[c][k] for k in range(3)]
        v = [X[l2][k] - X[c][k] for k in range(3)]
        Fc, F1, F2, U, Sa, se = angle(k_, c0, u, v)
        for k in range(3):
            F[c][k] += Fc[k]; F[l1][k] += F1[k]; F[l2][k] += F2[k]
        S[c] += Sa[0]; S[l1] += Sa[1]; S[l2] += Sa[2]
        E += U; SE += se
    return (np.array([[float(v) for v in row] for row in F]), np.array([float(v) for v in S]), float(E), float(SE),
            np.stack([case["x"], case["y"], case["z"]], 1))


def make_fixture(path=None):
    """Reference values of every case of pair_cases.CASES (concatenated, 'case' = index into 'names') and of pair_cases.BONDED_CASES."""
    import numpy as np
    import pair_cases as pc
    cols = {k: [] for k in FIXTURE_KEYS}
    for ci, name in enumerate(pc.CASES):
        ref = case_reference(name)
        n = len(ref["f"])
        cols["case"].append(np.full(n, ci, dtype=np.int16))
        for k in FIXTURE_KEYS[1:]:
            cols[k].append(ref[k])
    arrays = {k: np.concatenate(v) for k, v in cols.items()}
    arrays["names"] = np.array(pc.CASES)
    b = {k: [] for k in BONDED_KEYS}
    beng, bse = [], []
    for ci, name in enumerate(pc.BONDED_CASES):
        F, S, E, SE, X = bonded_reference(name)
        b["bcase"].append(np.full(len(S), ci, dtype=np.int16))
        for k, col in zip(("bx", "by", "bz"), X.T):
            b[k].append(col)
        for k, col in zip(("bfx", "bfy", "bfz"), F.T):
            b[k].append(col)
        b["bsf"].append(S)
        beng.append(E); bse.append(SE)
    arrays.update({k: np.concatenate(v) for k, v in b.items()})
    arrays.update(bnames=np.array(pc.BONDED_CASES), beng=np.array(beng), bse=np.array(bse))
    if path:
        np.savez_compressed(path, **arrays)
    return arrays
