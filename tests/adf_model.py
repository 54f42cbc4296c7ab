"""The bond-angle distribution contract of include/aztot.h (aztot_adf_*) restated in numpy, and a 50-digit angle for single triplets.

  edges(n_bins)                          the table T_b = c_b |c_b|, c_b = cos(pi b / n_bins), with T_0 = 1, T_n = -1 and T_(n/2) = 0 forced
  bin_of(s, p, T)                        #{ b in [1, n_bins - 1] : s <= fl(T_b p) }, found from an estimate corrected by the exact comparisons
  bin_of_plain(s, p, T)                  the same count taken literally
  host_adf(pos, types, box, cols, T)     counts[bin, col] and the neighbours per atom (-1: not a central atom)
  exact_angle(u, v)                      the angle between two fp64 vectors in degrees, mpmath at 50 digits

Every fp64 operation of the rule is one numpy operation on float64 arrays (no fused multiply-add, no reassociation), so the device, which evaluates the
same correctly rounded operations in the same order, must reproduce every count exactly.  `mutate` switches one rule off at a time: the tests use it
to show that the model notices."""
import numpy as np

MAX_NEIGHBOURS = 256


def cos_edges(n_bins):
    """c_b = cos(pi b / n_bins) rounded to double, as the library makes it: the sine of the complementary angle in the middle half, the cosine of the angle
    counted from the nearer end elsewhere, in extended precision (cos(pi b / n) in plain double loses its relative accuracy towards 90 degrees)"""
    b = np.arange(n_bins + 1)
    k = n_bins - 2 * b
    if np.finfo(np.longdouble).nmant >= 63:
        ld = np.longdouble
        pi, n = ld("3.141592653589793238462643383279502884"), ld(n_bins)
        mid = np.sin(pi * k.astype(ld) / (ld(2) * n))
        lo = np.cos(pi * b.astype(ld) / n)
        hi = -np.cos(pi * (n_bins - b).astype(ld) / n)
        return np.where(2 * np.abs(k) <= n_bins, mid, np.where(k > 0, lo, hi)).astype(np.float64)
    import mpmath                                   # no extended precision on this host: the correctly rounded values
    with mpmath.workdps(50):
        return np.array([float(mpmath.cos(mpmath.pi * int(x) / n_bins)) for x in b])


def edges(n_bins):
    c = cos_edges(n_bins)
    T = c * np.abs(c)
    T[0], T[n_bins] = 1.0, -1.0
    if n_bins % 2 == 0:
        T[n_bins // 2] = 0.0
    return T


def bin_of_plain(s, p, T, strict=False):
    s, p = np.atleast_1d(np.asarray(s, dtype=np.float64)), np.atleast_1d(np.asarray(p, dtype=np.float64))
    inner = T[1:-1]
    prod = inner[None, :] * p[:, None]
    return ((s[:, None] < prod) if strict else (s[:, None] <= prod)).sum(axis=1).astype(np.int64)


def bin_of(s, p, T, strict=False):
    """the predicate is true on a prefix of b = 1 .. n - 1 (T decreases, a rounded product is monotone): walk from an estimate to the end of the prefix"""
    s, p = np.atleast_1d(np.asarray(s, dtype=np.float64)), np.atleast_1d(np.asarray(p, dtype=np.float64))
    n = len(T) - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(p > 0, s / p, 0.0)
    b = np.clip(np.searchsorted(-T, -q, side="right") - 1, 0, n - 1).astype(np.int64)

    def holds(k):       # the predicate at b = k, for 1 <= k <= n - 1
        prod = T[np.clip(k, 0, n)] * p
        return (s < prod) if strict else (s <= prod)
    while True:
        up = (b + 1 <= n - 1) & holds(b + 1)
        down = ~up & (b >= 1) & ~holds(b)
        if not up.any() and not down.any():
            return b
        b = b + up.astype(np.int64) - down.astype(np.int64)


def normalise(cols):
    """(c, a, b, R_a, R_b) with a <= b, the radii swapped with the species"""
    return [(c, a, b, ra, rb) if a <= b else (c, b, a, rb, ra) for c, a, b, ra, rb in cols]


def host_adf(pos, types, box, cols, T, mutate=None):
    """counts[n_bins, n_cols] (int64) and neighbours[N] (-1 where the atom's species is central to no column).
    mutate: None or one of 'twice', 'inclusive', 'no_image', 'strict_bin', 'ra_both', 'coincident'"""
    L = np.asarray(box, dtype=np.float64)
    half = L * 0.5
    pos = np.asarray(pos, dtype=np.float64)
    types = np.asarray(types)
    N, n_bins = len(pos), len(T) - 1
    cols = normalise(cols)
    counts = np.zeros((n_bins, len(cols)), dtype=np.int64)
    neigh = np.full(N, -1, dtype=np.int64)
    nspec = int(max([types.max() if N else 0] + [max(c[:3]) for c in cols])) + 1
    mine = [[k for k, c in enumerate(cols) if c[0] == g] for g in range(nspec)]
    idx = np.arange(N)
    for i in range(N):
        live = mine[types[i]]
        if not live:
            continue
        u = []
        for k in range(3):
            d = pos[:, k] - pos[i, k]
            if mutate != "no_image":
                d = np.where(d > half[k], d - L[k], np.where(d < -half[k], d + L[k], d))
            u.append(d)
        r2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
        other = idx != i
        if mutate != "coincident":
            other &= r2 > 0.0

        def inside(R):
            return other & ((r2 <= R * R) if mutate == "inclusive" else (r2 < R * R))
        rmax = max(max(cols[k][3], cols[k][4]) for k in live)
        ligands = sorted({cols[k][1] for k in live} | {cols[k][2] for k in live})
        neigh[i] = int((inside(rmax) & np.isin(types, ligands)).sum())
        for k in live:
            _, a, b, ra, rb = cols[k]
            if mutate == "ra_both":
                rb = ra
            A = np.flatnonzero(inside(ra) & (types == a))
            B = np.flatnonzero(inside(rb) & (types == b))
            if a == b:
                jj, kk = np.triu_indices(len(A), 1)
                if mutate == "twice":
                    jj, kk = np.concatenate([jj, kk]), np.concatenate([kk, jj])
                j, k2 = A[jj], A[kk]
            else:
                j, k2 = np.repeat(A, len(B)), np.tile(B, len(A))
            if not len(j):
                continue
            dot = (u[0][j] * u[0][k2] + u[1][j] * u[1][k2]) + u[2][j] * u[2][k2]
            s = dot * np.abs(dot)
            p = r2[j] * r2[k2]
            counts[:, k] += np.bincount(bin_of(s, p, T, strict=mutate == "strict_bin"), minlength=n_bins)
    return counts, neigh


def exact_angle(u, v):
    """degrees, from the exact values of the six doubles"""
    import mpmath
    with mpmath.workdps(50):
        uu = [mpmath.mpf(float(x)) for x in u]
        vv = [mpmath.mpf(float(x)) for x in v]
        dot = sum(a * b for a, b in zip(uu, vv))
        c = dot / mpmath.sqrt(sum(a * a for a in uu) * sum(b * b for b in vv))
        c = max(mpmath.mpf(-1), min(mpmath.mpf(1), c))
        return mpmath.acos(c) * 180 / mpmath.pi


def rule_bin(u, v, T):
    """the bin of one triplet by the rule, from the displacement vectors"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    dot = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    r2u = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
    r2v = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    return int(bin_of(dot * abs(dot), r2u * r2v, T)[0])


def values(counts):
    """theta[n_bins], p[n_bins, n_cols]: count / (column total * width), 0 where the column is empty"""
    n_bins = counts.shape[0]
    width = 180.0 / n_bins
    tot = counts.sum(axis=0).astype(np.float64)
    p = np.zeros(counts.shape)
    nz = tot > 0
    p[:, nz] = counts[:, nz].astype(np.float64) / (tot[nz] * width)
    return (np.arange(n_bins) + 0.5) * width, p
