"""The bond-orientational order contract of include/aztot.h (aztot_boo_*) restated: Steinhardt q_lm, q_l and the neighbour-averaged q-bar_l.

  bonds(pos, types, box, R, central_mask, ligand_mask)    the neighbours of every atom: the separation rule of adf_model.py (u = r_j - r_i, one shift by L where
                                                          |d| > L / 2, r2 = (ux*ux + uy*uy) + uz*uz in fp64), j != i, 0 < r2 < R * R, ligand species
  exact_qlm(B, l)                                         q_lm of every atom at 60 digits (216-bit fixed point on Python integers, vectorised through numpy
                                                          object arrays): the fp64 bond vectors u of the rule are the data, everything behind them is exact
  route_qlm(B, l)                                         the route of the kernel in plain fp64: one sqrt and one division per bond, (x + i y)^m by complex
                                                          multiplication, T_l^m = P_l^m / sin^m by the three-term recurrence, the normalisation once per atom
  invariant(qlm, l), averaged(B, qlm)                     q_l from q_lm, and q-bar_lm = (q_lm(i) + sum over the central neighbours) / (1 + |C(i)|), in fp64
  bin_of(q, n_bins), totals(...)                          min(n_bins - 1, (int) fl(q n_bins)); histograms, sums through tcf_model.species_sums, entered

The device may contract the harmonic arithmetic and deals the bonds to lanes, so q_lm is held to a tolerance, not to the bit:

  ROUTE_WORST    the worst |route_qlm - exact_qlm| per component over the cases of tests/test_gpu_boo.py, measured on the CPU by boo_cases.measure()
  QLM_TOL        4 * ROUTE_WORST: the bound of the device (the margin of four is for another summation order and contraction)
  Q_TOL          sqrt(8 pi) * QLM_TOL for q_l and q-bar_l: q_l = sqrt(4 pi / (2l + 1)) * ||v||, v the 2l + 1 values q_lm of m = -l ... l; a norm moves by at
                 most the norm of the change, every complex component is off by at most sqrt 2 * QLM_TOL, so |dq| <= sqrt(4 pi / (2l + 1)) *
                 sqrt((2l + 1) * 2) * QLM_TOL.  An average of q_lm is a convex combination: it is off by no more than its terms.

`mutate` switches one rule off at a time: the tests use it to show that the model notices."""
import functools
import math

import numpy as np

import tcf_model

ROUTE_WORST = 3.248e-15     # measured (3.2475e-15): `python tests/boo_cases.py` over the cases of test_gpu_boo.py, worst component (12 alone, 9 neighbours)
QLM_TOL = 4.0 * ROUTE_WORST
Q_TOL = math.sqrt(8.0 * math.pi) * QLM_TOL
KNOWN_TOL = 5e-7            # the known answers are quoted to six decimals

FRAC = 216
ONE = 1 << FRAC


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bonds
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Bonds:
    """flat arrays over all bonds, ordered by the central atom (owner) then by the partner's index: owner, partner, u[B, 3], r2[B]; n[N] (-1: not central)"""

    def __init__(self, N, owner, partner, u, r2, n, central):
        self.N, self.owner, self.partner, self.u, self.r2, self.n, self.central = N, owner, partner, u, r2, n, central
        self.start = np.searchsorted(owner, np.arange(N + 1))


def bonds(pos, types, box, R, central_mask, ligand_mask, atoms=None, mutate=None):
    """`atoms`: only these are treated as central candidates (the others get n = -1): for large systems.  mutate: 'inclusive', 'self', 'no_image'"""
    L = np.asarray(box, dtype=np.float64)
    half = L * 0.5
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    types = np.asarray(types)
    N = len(pos)
    is_c = ((central_mask >> types) & 1).astype(bool) if N else np.zeros(0, dtype=bool)
    is_l = ((ligand_mask >> types) & 1).astype(bool) if N else np.zeros(0, dtype=bool)
    n = np.full(N, -1, dtype=np.int64)
    own, par, us, r2s = [], [], [], []
    idx = np.arange(N)
    for i in (range(N) if atoms is None else atoms):
        if not is_c[i]:
            continue
        u = []
        for k in range(3):
            d = pos[:, k] - pos[i, k]
            if mutate != "no_image":
                d = np.where(d > half[k], d - L[k], np.where(d < -half[k], d + L[k], d))
            u.append(d)
        r2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
        hit = is_l & ((r2 <= R * R) if mutate == "inclusive" else (r2 < R * R))
        hit &= (r2 > 0.0) & (idx != i)
        j = np.flatnonzero(hit)
        n[i] = len(j) + (1 if mutate == "self" and is_l[i] else 0)     # (the atom itself has no direction: the mutation counts it and adds nothing)
        own.append(np.full(len(j), i, dtype=np.int64))
        par.append(j)
        us.append(np.stack([u[0][j], u[1][j], u[2][j]], axis=1))
        r2s.append(r2[j])
    cat = (lambda a, shape, dt: np.concatenate(a) if a else np.zeros(shape, dtype=dt))
    return Bonds(N, cat(own, 0, np.int64), cat(par, 0, np.int64), cat(us, (0, 3), np.float64), cat(r2s, 0, np.float64), n, is_c)


def shell(vectors):
    """one central atom (index 0) with the given bond vectors, no box"""
    v = np.asarray(vectors, dtype=np.float64).reshape(-1, 3)
    r2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    k = len(v)
    n = np.full(k + 1, -1, dtype=np.int64)
    n[0] = k
    central = np.zeros(k + 1, dtype=bool)
    central[0] = True
    return Bonds(k + 1, np.zeros(k, dtype=np.int64), np.arange(1, k + 1), v, r2, n, central)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 60-digit values: fixed point on Python integers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def fx(a):
    """float64 array -> fixed point (exact for every double of magnitude >= 2^-163; the positions here are far above that)"""
    out = np.empty(np.shape(a), dtype=object)
    flat = out.reshape(-1)
    for k, v in enumerate(np.asarray(a, dtype=np.float64).reshape(-1)):
        p, q = float(v).as_integer_ratio()
        flat[k] = (p << FRAC) // q
    return out


def to_float(a):
    return np.array([v / ONE for v in np.asarray(a, dtype=object).reshape(-1)], dtype=np.float64).reshape(np.shape(a))


def _mul(a, b):
    return (a * b) // ONE


@functools.lru_cache(maxsize=None)
def norm_fixed(l, m, mutate=None):
    """N_lm = sqrt((2l + 1) / (4 pi) (l - m)! / (l + m)!) in fixed point, from mpmath at 80 digits"""
    import mpmath
    with mpmath.workdps(80):
        ratio = mpmath.factorial(l - m) / mpmath.factorial(l + m)
        if mutate == "inverted_factorial":
            ratio = 1 / ratio
        return int(mpmath.floor(mpmath.sqrt((2 * l + 1) / (4 * mpmath.pi) * ratio) * ONE))


@functools.lru_cache(maxsize=None)
def scale_fixed(l):
    import mpmath
    with mpmath.workdps(80):
        return int(mpmath.floor(4 * mpmath.pi / (2 * l + 1) * ONE))


def _double_factorial_signed(m):
    v = 1
    for k in range(1, m + 1):
        v *= -(2 * k - 1)
    return v


def exact_bond_terms(B, l):
    """(re, im)[bond, m]: T_l^m(z) (x + i y)^m of every bond in fixed point, (x, y, z) the exact unit vector of the fp64 bond vector u"""
    nb = len(B.r2)
    re, im = np.empty((nb, l + 1), dtype=object), np.empty((nb, l + 1), dtype=object)
    if nb == 0:
        return re, im
    u = fx(B.u)
    r2 = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]                   # scaled by ONE^2, exact
    r = np.array([math.isqrt(int(v)) for v in r2], dtype=object)                      # scaled by ONE
    x, y, z = [(u[:, k] * ONE) // r for k in range(3)]
    cr, ci = np.full(nb, ONE, dtype=object), np.full(nb, 0, dtype=object)
    for m in range(l + 1):
        p0 = np.full(nb, _double_factorial_signed(m) * ONE, dtype=object)
        p1 = p0
        if m < l:
            p1 = (2 * m + 1) * _mul(z, p0)
        for k in range(m + 2, l + 1):
            p0, p1 = p1, ((2 * k - 1) * _mul(z, p1) - (k + m - 1) * p0) // (k - m)
        re[:, m], im[:, m] = _mul(p1, cr), _mul(p1, ci)
        cr, ci = _mul(cr, x) - _mul(ci, y), _mul(cr, y) + _mul(ci, x)
    return re, im


def _segment_sums(a, start):
    """exact sums of the rows [start[i], start[i + 1]) of an integer object array"""
    c = np.concatenate([np.zeros((1,) + a.shape[1:], dtype=object), np.cumsum(a, axis=0, dtype=object)]) if len(a) else np.zeros((1,) + a.shape[1:], dtype=object)
    return c[start[1:]] - c[start[:-1]]


def exact_qlm(B, l, mutate=None):
    """(re, im)[atom, m] in fixed point; zeros where n <= 0"""
    tre, tim = exact_bond_terms(B, l)
    sre, sim = _segment_sums(tre, B.start), _segment_sums(tim, B.start)
    n = np.array([int(max(v, 1)) for v in B.n], dtype=object)
    for m in range(l + 1):
        N = norm_fixed(l, m, mutate)
        sre[:, m] = (sre[:, m] * N) // (ONE * n)
        sim[:, m] = (sim[:, m] * N) // (ONE * n)
    return sre, sim


def exact_invariant(re, im, l, mutate=None):
    """q_l[atom] in fixed point from fixed-point q_lm"""
    w = 1 if mutate == "no_factor2" else 2
    s = re[:, 0] * re[:, 0] + im[:, 0] * im[:, 0]
    for m in range(1, l + 1):
        s = s + w * (re[:, m] * re[:, m] + im[:, m] * im[:, m])                       # scaled by ONE^2
    c = scale_fixed(l)
    return np.array([math.isqrt(int(v) * c // ONE) for v in s], dtype=object)


def exact_averaged(B, re, im, mutate=None):
    """q-bar_lm in fixed point: (q_lm(i) + sum over the central partners) / (1 + |C(i)|)"""
    keep = B.central[B.partner] if len(B.partner) else np.zeros(0, dtype=bool)
    start = np.searchsorted(B.owner[keep], np.arange(B.N + 1))
    cnt = np.array([int(v) for v in np.diff(start)], dtype=object)
    div = np.array([max(int(v), 1) for v in cnt], dtype=object) if mutate == "div_by_C" else cnt + 1
    out = []
    for a in (re, im):
        s = _segment_sums(a[B.partner[keep]], start) if keep.any() else np.zeros(a.shape, dtype=object) * 0
        out.append((a + s) // div[:, None])
    central = B.central[:, None]
    return np.where(central, out[0], 0), np.where(central, out[1], 0)


def exact_q(B, l, mutate=None):
    """(q_l, q-bar_l)[atom] as floats (correctly rounded from the 60-digit values)"""
    re, im = exact_qlm(B, l, mutate)
    are, aim = exact_averaged(B, re, im, mutate)
    return to_float(exact_invariant(re, im, l, mutate)), to_float(exact_invariant(are, aim, l, mutate))


def qlm_error(got, exact):
    """the largest |component of got - exact| over a complex array got[atom, m >= l + 1] and the fixed-point pair exact[atom, l + 1]"""
    re, im = exact
    if re.size == 0:
        return 0.0
    k = re.shape[1]
    d = np.maximum(np.abs(fx(np.real(got[:, :k])) - re), np.abs(fx(np.imag(got[:, :k])) - im))
    return float(int(d.max()) / ONE)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the route in plain fp64
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def norm_table(l):
    """the host table of the library: N_lm rounded to double, and 4 pi / (2l + 1)"""
    import mpmath
    with mpmath.workdps(50):
        N = [float(mpmath.sqrt((2 * l + 1) / (4 * mpmath.pi) * mpmath.factorial(l - m) / mpmath.factorial(l + m))) for m in range(l + 1)]
        return np.array(N), float(4 * mpmath.pi / (2 * l + 1))


def route_qlm(B, l):
    """complex q_lm[atom, l + 1]: every fp64 operation of the kernel as one numpy operation, the bonds of an atom added in their order"""
    N = B.N
    out = np.zeros((N, l + 1), dtype=np.complex128)
    if len(B.r2) == 0:
        return out
    inv = 1.0 / np.sqrt(B.r2)
    x, y, z = B.u[:, 0] * inv, B.u[:, 1] * inv, B.u[:, 2] * inv
    norm, _ = norm_table(l)
    cr, ci = np.ones(len(inv)), np.zeros(len(inv))
    dn = np.maximum(B.n, 1).astype(np.float64)
    for m in range(l + 1):
        p0 = np.full(len(inv), float(_double_factorial_signed(m)))
        p1 = p0
        if m < l:
            p1 = float(2 * m + 1) * z * p0
        for k in range(m + 2, l + 1):
            p0, p1 = p1, (float(2 * k - 1) * z * p1 - float(k + m - 1) * p0) * (1.0 / float(k - m))
        sre = np.bincount(B.owner, weights=p1 * cr, minlength=N)
        sim = np.bincount(B.owner, weights=p1 * ci, minlength=N)
        out[:, m] = (sre * norm[m] / dn) + 1j * (sim * norm[m] / dn)
        cr, ci = cr * x - ci * y, cr * y + ci * x
    out[B.n <= 0] = 0.0
    return out


def invariant(qlm, l):
    """q_l[atom] from complex q_lm[atom, >= l + 1] in fp64: sqrt(4 pi / (2l + 1) * (|q_l0|^2 + 2 sum_{m > 0} |q_lm|^2)), m ascending"""
    _, scale = norm_table(l)
    re, im = np.real(qlm), np.imag(qlm)
    s0 = re[:, 0] * re[:, 0] + im[:, 0] * im[:, 0]
    sm = np.zeros(len(qlm))
    for m in range(1, l + 1):
        sm = sm + (re[:, m] * re[:, m] + im[:, m] * im[:, m])
    return np.sqrt(scale * (s0 + 2.0 * sm))


def averaged(B, qlm):
    """q-bar_lm[atom] in fp64 from complex q_lm[atom, k]: the central partners of an atom added in their order, then (own + sum) / (1 + |C|)"""
    keep = B.central[B.partner] if len(B.partner) else np.zeros(0, dtype=bool)
    own, par = B.owner[keep], B.partner[keep]
    cnt = np.bincount(own, minlength=B.N).astype(np.float64)
    out = np.zeros(qlm.shape, dtype=np.complex128)
    for m in range(qlm.shape[1]):
        sre = np.bincount(own, weights=np.real(qlm[par, m]), minlength=B.N)
        sim = np.bincount(own, weights=np.imag(qlm[par, m]), minlength=B.N)
        out[:, m] = (np.real(qlm[:, m]) + sre) / (1.0 + cnt) + 1j * ((np.imag(qlm[:, m]) + sim) / (1.0 + cnt))
    out[~B.central] = 0.0
    return out


def per_atom(B, qlm_by_order, orders):
    """q[atom, order, kind] from the q_lm of every order (complex [atom, order, 13], as aztot_boo_qlm hands them out)"""
    q = np.zeros((B.N, len(orders), 2))
    for o, l in enumerate(orders):
        own = np.where(B.central[:, None], qlm_by_order[:, o, :l + 1], 0.0)
        q[:, o, 0] = invariant(own, l)
        q[:, o, 1] = invariant(averaged(B, own), l)
    return q


def bin_of(q, n_bins):
    return np.minimum(n_bins - 1, (np.asarray(q, dtype=np.float64) * float(n_bins)).astype(np.int64))


def totals(n, q, types, n_species, n_bins):
    """(hist[2, orders, species, bins], sums[2, orders, species], entered[species]) of one sample from its per-atom values n[atom], q[atom, order, kind]"""
    n, types = np.asarray(n), np.asarray(types)
    n_orders = q.shape[1]
    hist = np.zeros((2, n_orders, n_species, n_bins), dtype=np.int64)
    sums = np.zeros((2, n_orders, n_species))
    inn = n > 0
    entered = np.array([int((inn & (types == s)).sum()) for s in range(n_species)], dtype=np.int64)
    for kind in range(2):
        for o in range(n_orders):
            v = q[:, o, kind]
            b = bin_of(v, n_bins)
            for s in range(n_species):
                hist[kind, o, s] = np.bincount(b[inn & (types == s)], minlength=n_bins)
            sums[kind, o] = tcf_model.species_sums(np.where(inn, v, 0.0), types, n_species)
    return hist, sums, entered


def values(hist, sums, entered):
    """centre[bins], density (count / (column total * width), width = 1 / n_bins), mean = sum / entered"""
    n_bins = hist.shape[-1]
    tot = hist.sum(axis=-1, keepdims=True).astype(np.float64)
    width = 1.0 / float(n_bins)
    with np.errstate(divide="ignore", invalid="ignore"):
        dens = np.where(tot > 0, hist.astype(np.float64) / (tot * width), 0.0)
        mean = np.where(entered > 0, sums / entered.astype(np.float64), 0.0)
    return (np.arange(n_bins) + 0.5) / float(n_bins), dens, mean


# ---------------------------------------------------------------------------------------------------------------------------------------------
# known shells
# ---------------------------------------------------------------------------------------------------------------------------------------------
def fcc_shell():
    return [(a, b, 0) for a in (1, -1) for b in (1, -1)] + [(a, 0, b) for a in (1, -1) for b in (1, -1)] + [(0, a, b) for a in (1, -1) for b in (1, -1)]


def hcp_shell():
    """ideal c / a: six in the plane, three above, three below (the lower triangle is the upper one mirrored in the plane)"""
    s3, h = math.sqrt(3.0), math.sqrt(2.0 / 3.0)
    plane = [(math.cos(k * math.pi / 3), math.sin(k * math.pi / 3), 0.0) for k in range(6)]
    tri = [(0.5, s3 / 6, h), (-0.5, s3 / 6, h), (0.0, -s3 / 3, h)]
    return plane + tri + [(a, b, -c) for a, b, c in tri]


def bcc_shell():
    return [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)] + [(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2)]


def sc_shell():
    return [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def icosahedron_shell():
    g = (1.0 + math.sqrt(5.0)) / 2.0
    return [(0, a, b * g) for a in (1, -1) for b in (1, -1)] + [(a, b * g, 0) for a in (1, -1) for b in (1, -1)] + [(b * g, 0, a) for a in (1, -1) for b in (1, -1)]


KNOWN = {   # q4, q6, q8, q10, q12
    "fcc": (fcc_shell, (0.190941, 0.574524, 0.403915, 0.012857, 0.600083)),
    "hcp": (hcp_shell, (0.097222, 0.484762, 0.316992, 0.010169, 0.564979)),
    "bcc": (bcc_shell, (0.036370, 0.510688, 0.429322, 0.195191, 0.404799)),
    "sc": (sc_shell, (0.763763, 0.353553, 0.718070, 0.411425, 0.695503)),
    "icosahedron": (icosahedron_shell, (0.0, 0.663325, 0.0, 0.362951, 0.585423)),
}
KNOWN_ORDERS = (4, 6, 8, 10, 12)


def shell_q(vectors, l, mutate=None):
    B = shell(vectors)
    re, im = exact_qlm(B, l, mutate)
    return float(to_float(exact_invariant(re, im, l, mutate))[0])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the measurement behind ROUTE_WORST
# ---------------------------------------------------------------------------------------------------------------------------------------------
def route_error(B, orders):
    """the worst |route_qlm - exact_qlm| per component over the central atoms of B"""
    worst = 0.0
    for l in orders:
        worst = max(worst, qlm_error(route_qlm(B, l), exact_qlm(B, l)))
    return worst
