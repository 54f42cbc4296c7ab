"""The contract of the static structure factors (aztot_sk_*, include/aztot.h) restated in numpy, for tests/test_sk_model.py (CPU) and tests/test_gpu_sk.py.

  vector_set        the k-vector set: half space, kk and the bin rule in correctly rounded fp64 operations, lexicographic order, thinning - it reproduces
                    aztot_sk_vectors exactly
  pair_index        the RDF's pair index;  accumulate: the rule of one sample;  values: aztot_sk_values from the sums, operation by operation
  amplitudes        rho_s(k) = sum_{j of s} exp(2 pi i (l x / Lx + m y / Ly + n z / Lz)) with the true pi, every phase evaluated directly (no per-axis table,
                    no recurrence, no conjugation): engine "mp" - mpmath at 50 digits - for up to some ten thousand (atom, vector) pairs, engine "ld" -
                    numpy.longdouble (x87 extended, eps 1.08e-19), vectorised - for the larger cases.  Both return longdouble arrays
  restate_fp64      the kernels' own route in fp64: exp(2 pi i x / L) once per atom and axis, higher harmonics by repeated complex multiplication, negative
                    m / n by conjugation, the row sums (tiles of 64 ids dealt to min(256, tiles) rows, one atom at a time) and the fold by halving.  The CPU
                    test shows that it stays inside the bound the GPU is held to, and that the bound catches its mutations
The bound: |rho_gpu - rho| <= TAU n_s per component, TAU = pair_cases.TAU.  mpmath is imported only where the "mp" engine runs."""
import numpy as np

import pair_cases as pc
from tcf_model import fold

LD = np.longdouble
TAU = pc.TAU
TWO_PI = 6.283185307179586                  # the correctly rounded double of 2 pi (== 2.0 * numpy.pi)
MAX_HARMONIC, MAX_BINS = 48, 4096           # AZTOT_SK_MAX_HARMONIC, AZTOT_SK_MAX_BINS
ID_TILE, ROWS = 64, 256
MUTATIONS = ("full_space", "no_conjugation_for_negative_m", "harmonics_shifted_by_one", "transposed_pair_index", "normalised_by_N", "bins_from_kk")


def require_longdouble():
    assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended type on this machine: the longdouble reference cannot be trusted"


# ---- the vector set --------------------------------------------------------------------------------------------------------------------------
def n_bins_of(kmax, dk):
    return int(kmax * (1.0 / dk))


def vector_set(box, kmax, dk, max_per_bin=0, mutate=None):
    """{"lmn" int32 (n_k, 3), "bin" int32 (n_k,), "n_bins", "n_in_bin" int32 (n_bins,), "unthinned" (count per bin before thinning)}; ValueError where the set-up refuses"""
    assert mutate in (None, "full_space", "bins_from_kk")
    kmax, dk = float(kmax), float(dk)
    if not (kmax > 0.0 and dk > 0.0) or max_per_bin < 0:
        raise ValueError("kmax, dk must be positive, max_per_bin not negative")
    idk = 1.0 / dk
    n_bins = int(kmax * idk)
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError("n_bins outside [1, %d]" % MAX_BINS)
    kmax2 = kmax * kmax
    sq = []
    for a in range(3):
        g = TWO_PI / float(box[a])
        k = np.arange(MAX_HARMONIC + 2, dtype=np.float64) * g
        sq.append(k * k)
        if sq[a][MAX_HARMONIC + 1] <= kmax2:
            raise ValueError("harmonic %d on axis %s" % (MAX_HARMONIC + 1, "xyz"[a]))
    H = [int(np.flatnonzero(s[:MAX_HARMONIC + 1] <= kmax2).max()) for s in sq]
    l, m, n = np.meshgrid(np.arange(-H[0] if mutate == "full_space" else 0, H[0] + 1), np.arange(-H[1], H[1] + 1), np.arange(-H[2], H[2] + 1), indexing="ij")
    l, m, n = l.ravel(), m.ravel(), n.ravel()                       # (ascending lexicographic order of (l, m, n))
    half = (l > 0) | ((l == 0) & (m > 0)) | ((l == 0) & (m == 0) & (n > 0))
    if mutate == "full_space":
        half = (l != 0) | (m != 0) | (n != 0)
    l, m, n = l[half], m[half], n[half]
    kk = (sq[0][np.abs(l)] + sq[1][np.abs(m)]) + sq[2][np.abs(n)]
    b = ((kk if mutate == "bins_from_kk" else np.sqrt(kk)) * idk).astype(np.int64)
    keep = (kk <= kmax2) & (b < n_bins)
    l, m, n, b = l[keep], m[keep], n[keep], b[keep]
    count = np.bincount(b, minlength=n_bins).astype(np.int64)
    # j: the number of a vector inside its bin, in set order
    order = np.argsort(b, kind="stable")
    j = np.empty(len(b), dtype=np.int64)
    j[order] = np.arange(len(b)) - np.concatenate([[0], np.cumsum(count)])[b[order]]
    c = count[b]
    M = int(max_per_bin)
    kept = np.ones(len(b), dtype=bool) if M == 0 else (c <= M) | ((j + 1) * M // np.maximum(c, 1) > j * M // np.maximum(c, 1))
    l, m, n, b = l[kept], m[kept], n[kept], b[kept]
    if len(b) == 0:
        raise ValueError("empty set")
    return {"lmn": np.stack([l, m, n], 1).astype(np.int32), "bin": b.astype(np.int32), "n_bins": n_bins,
            "n_in_bin": np.bincount(b, minlength=n_bins).astype(np.int32), "unthinned": count}


def brute_force_set(box, kmax, dk, H):
    """The unthinned set by another route: every integer triple of the cube [-H, H]^3 but 0, kk from the triple's own products, ONE of each +-k pair chosen
    as the member that sorts behind its negative, sorted.  (lmn, bin)"""
    idk = 1.0 / float(dk)
    n_bins = int(float(kmax) * idk)
    g = [TWO_PI / float(L) for L in box]
    out = []
    r = range(-H, H + 1)
    for l in r:
        for m in r:
            for n in r:
                t = (l, m, n)
                if t <= (-l, -m, -n):                                  # 0 and the lower member of each pair
                    continue
                kx, ky, kz = l * g[0], m * g[1], n * g[2]
                kk = (kx * kx + ky * ky) + kz * kz
                if kk <= float(kmax) * float(kmax):
                    b = int(np.sqrt(kk) * idk)
                    if b < n_bins:
                        out.append((l, m, n, b))
    out.sort()
    a = np.array(out, dtype=np.int32).reshape(-1, 4)
    return a[:, :3], a[:, 3]


# ---- pairs, accumulation, values ---------------------------------------------------------------------------------------------------------------
def pair_index(a, b, nspec, mutate=None):
    mn, mx = (min(a, b), max(a, b)) if mutate != "transposed_pair_index" else (max(a, b), min(a, b))
    return mn * (nspec - 1) + mn * (1 - mn) // 2 + mx


def pairs(nspec):
    return [(a, b) for a in range(nspec) for b in range(a, nspec)]


def accumulate(acc, rho, mutate=None):
    """acc[k][pair] + fl(fl(re_a re_b) + fl(im_a im_b)) for a sample with amplitudes rho[k][species][re, im]"""
    nspec = rho.shape[1]
    out = acc.copy()
    for a, b in pairs(nspec):
        t = rho[:, a, 0] * rho[:, b, 0] + rho[:, a, 1] * rho[:, b, 1]
        p = pair_index(a, b, nspec, mutate)
        out[:, p] = out[:, p] + t
    return out


def _add_in_order(n_bins, bins, v):
    """out[b] = the v of bin b added one after the other in set order, from 0.0 (ufunc.at is unbuffered and sequential)"""
    out = np.zeros((n_bins,) + v.shape[1:])
    np.add.at(out, bins, v)
    return out


def values(acc, samples, bins, n_bins, numbers, dk, mutate=None):
    """(k, n_in_bin, S_total[bin], S_pair[bin][pair]) as aztot_sk_values forms them from the sums; numbers: atoms per species"""
    nspec = len(numbers)
    N = float(sum(numbers))
    P = pairs(nspec)
    assert acc.shape[1] == len(P) and [pair_index(a, b, nspec) for a, b in P] == list(range(len(P)))
    root = np.array([np.sqrt(float(numbers[a]) * float(numbers[b])) for a, b in P])
    weight = np.array([1.0 if a == b else 2.0 for a, b in P]) * root
    d = float(samples) * (np.full(len(P), N) if mutate == "normalised_by_N" else root)
    sab = np.zeros_like(acc)
    np.divide(acc, d[None, :], out=sab, where=(d != 0.0)[None, :])
    tot = np.zeros(len(acc))
    for p in range(len(P)):
        tot = tot + weight[p] * sab[:, p]
    sv = tot / N if N > 0 else np.zeros(len(acc))
    cnt = np.bincount(bins, minlength=n_bins).astype(np.int32)
    s_pair, s_tot = _add_in_order(n_bins, bins, sab), _add_in_order(n_bins, bins, sv)
    has = cnt > 0
    s_pair[has] = s_pair[has] / cnt[has, None].astype(np.float64)
    s_tot[has] = s_tot[has] / cnt[has].astype(np.float64)
    return (np.arange(n_bins) + 0.5) * float(dk), cnt, s_tot, s_pair


# ---- the references ----------------------------------------------------------------------------------------------------------------------------
def amplitudes_ld(pos, types, box, lmn, nspec, chunk=1 << 21):
    """rho[k][species][re, im] in numpy.longdouble: the phase in turns is reduced to its fraction before it meets pi (exactly periodic)"""
    require_longdouble()
    pos, types = np.asarray(pos), np.asarray(types)
    u = [np.asarray(pos[:, a], dtype=LD) / LD(float(box[a])) for a in range(3)]
    twopi = 2 * LD("3.14159265358979323846264338327950288")
    nK, N = len(lmn), len(types)
    out = np.zeros((nK, nspec, 2), dtype=LD)
    sel = [types == s for s in range(nspec)]
    step = max(1, chunk // max(N, 1))
    L = lmn.astype(LD)
    for k0 in range(0, nK, step):
        sl = slice(k0, min(nK, k0 + step))
        turns = L[sl, 0:1] * u[0][None, :] + L[sl, 1:2] * u[1][None, :] + L[sl, 2:3] * u[2][None, :]
        arg = (turns - np.rint(turns)) * twopi
        co, si = np.cos(arg), np.sin(arg)
        for s in range(nspec):
            out[sl, s, 0], out[sl, s, 1] = co[:, sel[s]].sum(1), si[:, sel[s]].sum(1)
    return out


def _to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def amplitudes_mp(pos, types, box, lmn, nspec):
    """the same at 50 digits (mpmath); longdouble array"""
    import mpmath as mp
    with mp.workdps(50):
        M = lambda t: mp.mpf(float(t))
        Lx, Ly, Lz = (M(t) for t in box)
        u = [(M(p[0]) / Lx, M(p[1]) / Ly, M(p[2]) / Lz) for p in np.asarray(pos)]
        twopi = 2 * mp.pi
        out = np.zeros((len(lmn), nspec, 2), dtype=LD)
        for k, (l, m, n) in enumerate(np.asarray(lmn).tolist()):
            re, im = [mp.mpf(0)] * nspec, [mp.mpf(0)] * nspec
            for j, s in enumerate(np.asarray(types).tolist()):
                c, sn = mp.cos_sin((l * u[j][0] + m * u[j][1] + n * u[j][2]) * twopi)
                re[s] += c
                im[s] += sn
            for s in range(nspec):
                out[k, s, 0], out[k, s, 1] = _to_ld(re[s]), _to_ld(im[s])
    return out


def amplitudes(pos, types, box, lmn, nspec, engine="ld"):
    return amplitudes_mp(pos, types, box, lmn, nspec) if engine == "mp" else amplitudes_ld(pos, types, box, lmn, nspec)


def numbers_of(types, nspec):
    return np.bincount(np.asarray(types), minlength=nspec)[:nspec]


def worst_ratio(rho, ref, numbers):
    """max over vectors, species and components of |rho - ref| / n_s; a species without atoms must be exactly 0"""
    err = np.abs(np.asarray(rho, dtype=LD) - ref)
    n = np.asarray(numbers, dtype=np.float64)
    assert (np.asarray(rho)[:, n == 0] == 0.0).all(), "a species without atoms has an amplitude"
    return float((err[:, n > 0] / n[n > 0][None, :, None]).max()) if (n > 0).any() else 0.0


# ---- the kernels' route in fp64 ----------------------------------------------------------------------------------------------------------------
def _phase(c, L):
    """exp(2 pi i c / L): u = fl(c / L) reduced to (-1/2, 1/2] exactly, and the small turn that the division lost"""
    u = c / L
    r = c - u * L                               # (the kernel takes it exactly, in an fma; it only has to be small here)
    v = u - np.rint(u)
    arg = TWO_PI * v + TWO_PI * (r / L)
    return np.cos(arg), np.sin(arg)


def _harmonics(c, L, n, shift=0):
    """(C, S)[h] = exp(2 pi i c / L)^(h + shift), h = 0 ... n - 1, by repeated complex multiplication"""
    e1c, e1s = _phase(c, L)
    cc, cs = np.ones_like(c), np.zeros_like(c)
    for _ in range(shift):
        cc, cs = cc * e1c - cs * e1s, cs * e1c + cc * e1s
    C, S = np.empty((n, len(c))), np.empty((n, len(c)))
    for h in range(n):
        C[h], S[h] = cc, cs
        cc, cs = cc * e1c - cs * e1s, cs * e1c + cc * e1s
    return C, S


def row_sums(terms):
    """terms[..., N] in id order -> [..., 256]: the nB = min(256, ceil(N / 64)) row sums (row r: tiles r, r + nB, ... one atom at a time from 0.0), zero-padded"""
    N = terms.shape[-1]
    nT = max(1, -(-N // ID_TILE))
    nB = min(ROWS, nT)
    rounds = -(-nT // nB)
    t = np.zeros(terms.shape[:-1] + (rounds * nB * ID_TILE,))
    t[..., :N] = terms
    t = t.reshape(terms.shape[:-1] + (rounds, nB, ID_TILE))
    t = np.moveaxis(t, -3, -2).reshape(terms.shape[:-1] + (nB, rounds * ID_TILE))
    rows = np.cumsum(t, axis=-1)[..., -1]                       # (cumsum is sequential; add.reduce would be pairwise)
    out = np.zeros(terms.shape[:-1] + (ROWS,))
    out[..., :nB] = rows
    return out


def restate_fp64(pos, types, box, lmn, nspec, mutate=None):
    """rho[k][species][re, im] by the kernels' arithmetic in fp64"""
    assert mutate in (None, "no_conjugation_for_negative_m", "harmonics_shifted_by_one")
    pos, types, lmn = np.asarray(pos, dtype=np.float64), np.asarray(types), np.asarray(lmn)
    h = np.abs(lmn).max(0) + 1
    XC, XS = _harmonics(pos[:, 0].copy(), float(box[0]), int(h[0]))
    YC, YS = _harmonics(pos[:, 1].copy(), float(box[1]), int(h[1]), 1 if mutate == "harmonics_shifted_by_one" else 0)
    ZC, ZS = _harmonics(pos[:, 2].copy(), float(box[2]), int(h[2]))
    out = np.zeros((len(lmn), nspec, 2))
    sel = [types == s for s in range(nspec)]
    for k, (l, m, n) in enumerate(lmn.tolist()):
        sm = -1.0 if (m < 0 and mutate != "no_conjugation_for_negative_m") else 1.0
        sn = -1.0 if n < 0 else 1.0
        emc, ems = YC[abs(m)], YS[abs(m)] * sm
        enc, ens = ZC[abs(n)], ZS[abs(n)] * sn
        lmc, lms = XC[l] * emc - XS[l] * ems, XS[l] * emc + XC[l] * ems
        ckc, cks = lmc * enc - lms * ens, lms * enc + lmc * ens
        for s in range(nspec):
            out[k, s, 0] = fold(row_sums(np.where(sel[s], ckc, 0.0)))
            out[k, s, 1] = fold(row_sums(np.where(sel[s], cks, 0.0)))
    return out
