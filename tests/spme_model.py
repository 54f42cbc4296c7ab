"""numpy restatement of the smooth particle-mesh Ewald contract ('elec spme', csrc/spme.hip.h, DESIGN.md "Smooth particle-mesh Ewald"), in two
routes, plus the systems tests/test_spme_model.py and tests/test_gpu_spme.py run it on.

The contract (Essmann et al. 1995 with the model's constants; orthorhombic box, mesh K, even spline order p):
  u = K x / L per axis, f = floor(u), w = u - f; theta(j) = M_p(w + j), j = 0 .. p - 1, lands on mesh index (f - j) mod K;
  theta'(j) = M_{p-1}(w + j) - M_{p-1}(w + j - 1)
  Q(g) = sum_i q_i theta_x theta_y theta_z                (kernels: 2^-40 sum_i llrint(((q theta_x) theta_y) theta_z 2^40), 64-bit integers)
  G(m) = exp(-k^2 / 4 alpha^2) / k^2 b_x b_y b_z, k = 2 pi_model m' / L, m' the signed index, b(m) = 1 / |sum_{k=0}^{p-2} M_p(k+1) e^{2 pi i m k / K}|^2, G(0) = 0
  E = 1/2 scale sum_m G |FQ|^2, FQ the forward DFT of Q, scale = 4 pi_model Fcoul_scale / V
  phi = scale * unnormalised inverse DFT of G FQ (real part); F_i,a = -q_i (K_a / L_a) sum_g phi(g) theta'_a theta_b theta_c
(the phases of the DFT and of b are exact: the full pi; only k carries the model's truncated pi, as the plain sum's k-vectors do)

Routes, one interface (spme(case, route)):
  "ld"    numpy.longdouble throughout, Q exact (not quantised), DFTs by a radix-2 recursion in long double with exactly reduced phases: the reference
  "fp64"  the kernels' route: fp64 weights by the kernels' recurrence, own-rounded products, the integer mesh, numpy.fft, fp64 gather
Condition scales (sums of absolute values, as tests/ewald_reference.py):
  Phi = scale sum_m |G FQ|  (a bound of |phi(g)|);  S_F,i = |q_i| sum_a (K_a / L_a) sum_g Phi |theta'_a theta_b theta_c|
  S_E = 1/2 scale sum_m G |FQ| sum_g |Q(g)|           (every |FQ(m)| is a sum of mesh charges: bounded by sum |Q|)
MUTATIONS are faults the kernels could have; tests/test_spme_model.py shows that the bounds catch each of them.
"""
import numpy as np

import ewald_reference as er
import pair_cases as pc

LD = np.longdouble
CLD = np.clongdouble
FIX = 2.0 ** 40
MUTATIONS = ("moduli_dropped", "sign_of_dtheta", "weight_index_off_by_one", "g0_kept", "unsigned_m_above_nyquist", "f_equal_K_not_wrapped",
             "axes_swapped_in_mesh")


# Measured by tests/test_spme_model.py (which fails when a measurement exceeds its record): the fp64 route against the long-double route of the
# same SPME, worst over the convergence table's five settings and the nine isolated systems.  Both exceed pair_cases.TAU = 1e-13 - the fp64 route
# carries the mesh's quantum of 2^-40 e, the long-double route does not -, so the GPU test holds the kernels to four times the records.
ROUTE_F, ROUTE_E = 2.11e-12, 2.65e-12          # max_i |F_i - F_ld,i| / S_F,i (32^3 / p = 8) and |E - E_ld| / S_E (one ion, 8^3 / p = 4)
BOUND_F, BOUND_E = 4 * ROUTE_F, 4 * ROUTE_E
# relative rms force error of the long-double route against the converged plain Ewald sum, 512 jittered rock-salt ions, L = 22.56, alpha = 0.3
DISCRETISATION = {(32, 4): 4.26e-4, (32, 6): 5.57e-6, (64, 6): 7.95e-8, (32, 8): 1.21e-7, (64, 8): 3.36e-10}
# the model's total Coulomb energy of the perfect rock-salt lattice (real-space term to rReal = 11 + mesh + constant) against -M k q^2 / r0 per ion pair,
# relative; the real-space cut-off, not the mesh, sets it
MADELUNG = {(32, 6): 2.56e-6, (64, 8): 2.56e-6}
# ... and of the 500-ion dense_case() at alpha = 0.45 against alpha = 0.40, rReal = 6.5 and mesh 32^3 / p = 8 fixed: relative difference of the totals
TWO_ALPHA = 6.59e-5


def pi_exact():
    return LD(4) * np.arctan(LD(1))


def bspline(w, p, dtype):
    """theta (p, N), dtheta (p, N): M_p(w + j) and M_{p-1}(w + j) - M_{p-1}(w + j - 1) by the recurrence
    M_n(u) = (u M_{n-1}(u) + (n - u) M_{n-1}(u - 1)) / (n - 1) from M_2(u) = 1 - |u - 1|, in place from the top index down (spme_weights)"""
    w = np.asarray(w, dtype=dtype)
    th = np.zeros((p,) + w.shape, dtype=dtype)
    th[0], th[1] = w, dtype(1) - w
    dth = None
    for n in range(3, p + 1):
        if n == p:
            dth = th.copy()
            dth[1:] = th[1:] - th[:-1]
        div = dtype(1) / dtype(n - 1)
        for j in range(n - 1, 0, -1):
            th[j] = div * ((w + dtype(j)) * th[j] + (dtype(n - j) - w) * th[j - 1])
        th[0] = div * (w * th[0])
    return th, dth


def _phase(num, K):
    """exp(2 pi i num / K) in long double, the phase reduced exactly"""
    a = (2 * pi_exact()) * (np.asarray(num) % K).astype(LD) / LD(K)
    return np.cos(a) + 1j * np.sin(a)


def influence(box, alpha, mesh, order, mutate=None):
    """G (Kx, Ky, Kz) in long double"""
    pi_model = LD(pc.PI)                                                      # units::pi is a double: the value the host code widens
    M = bspline(np.zeros(1, dtype=LD), order, LD)[0][:, 0]                    # M_p(j), j = 0 .. p - 1
    b, kk = [], []
    for a in range(3):
        K = int(mesh[a])
        m = np.arange(K)
        s = np.zeros(K, dtype=CLD)
        for k in range(order - 1):
            s = s + M[k + 1] * _phase(m * k, K)
        mod = (s.real * s.real + s.imag * s.imag).astype(LD)
        b.append(np.ones(K, dtype=LD) if mutate == "moduli_dropped" else LD(1) / mod)
        ms = m if mutate == "unsigned_m_above_nyquist" else np.where(m <= K // 2, m, m - K)
        kk.append(LD(2) * pi_model * ms.astype(LD) / LD(float(box[a])))
    k2 = kk[0][:, None, None] ** 2 + kk[1][None, :, None] ** 2 + kk[2][None, None, :] ** 2
    r4a2 = LD(1) / (LD(4) * LD(float(alpha)) * LD(float(alpha)))
    k2[0, 0, 0] = LD(1)
    G = np.exp(-k2 * r4a2) / k2 * b[0][:, None, None] * b[1][None, :, None] * b[2][None, None, :]
    G[0, 0, 0] = G[1, 0, 0] if mutate == "g0_kept" else LD(0)
    return G


def _fft_ld(x, sign):
    """unnormalised DFT along the last axis (a power of two), exp(sign 2 pi i m g / K), long double"""
    n = x.shape[-1]
    if n == 1:
        return x
    e, o = _fft_ld(x[..., ::2], sign), _fft_ld(x[..., 1::2], sign)
    t = _phase(sign * np.arange(n // 2), n) * o
    return np.concatenate([e + t, e - t], axis=-1)


def dft3_ld(a, sign):
    a = np.asarray(a, dtype=CLD)
    for ax in range(3):
        a = np.moveaxis(_fft_ld(np.moveaxis(a, ax, -1), sign), -1, ax)
    return a


def placement(case, mesh, order, dtype, mutate=None):
    """per axis: mesh indices (N, p) and the weights theta, dtheta (N, p); `lost` marks contributions a fault would drop"""
    idx, th, dth, lost = [], [], [], []
    for a, key in enumerate(("x", "y", "z")):
        K = int(mesh[a])
        x = np.asarray(case[key], dtype=np.float64)
        if dtype is LD:
            u = LD(K) * x.astype(LD) / LD(float(case["box"][a]))
        else:
            u = (float(K) * x) / float(case["box"][a])
        f = np.floor(u)
        t, d = bspline(u - f, order, dtype)
        j = np.arange(order)
        raw = f.astype(np.int64)[:, None] - j[None, :] + (1 if mutate == "weight_index_off_by_one" and a == 0 else 0)
        if mutate == "f_equal_K_not_wrapped":
            raw = np.where(raw < 0, raw + K, raw)
            lost.append(raw >= K)
        else:
            lost.append(np.zeros_like(raw, dtype=bool))
        idx.append(raw % K)
        th.append(t.T.copy())
        dth.append(-d.T.copy() if mutate == "sign_of_dtheta" else d.T.copy())
    return idx, th, dth, lost


def spme(case, route="ld", mutate=None, G=None):
    """{"Q", "Qint" (fp64 route), "count", "FQ", "phi", "G", "E", "F", "SF", "SE", "scale"} of `case` (keys box, alpha, spme_mesh, spme_order,
    species, types, x, y, z)"""
    assert mutate is None or mutate in MUTATIONS
    if route == "ld":
        er.require_longdouble()
    dtype = LD if route == "ld" else np.float64
    mesh, order = tuple(int(v) for v in case["spme_mesh"]), int(case["spme_order"])
    q = er.charges(case)
    N = len(q)
    _, _, (a, b, c), scale = er._ld_consts(case)
    box = (a, b, c)
    if G is None:
        G = influence(case["box"], case["alpha"], mesh, order, mutate)
    idx, th, dth, lost = placement(case, mesh, order, dtype, mutate)
    ix, iy, iz = idx[0][:, :, None, None], idx[1][:, None, :, None], idx[2][:, None, None, :]
    keep = ~(lost[0][:, :, None, None] | lost[1][:, None, :, None] | lost[2][:, None, None, :]) & (q != 0.0)[:, None, None, None]
    qd = q.astype(dtype)
    contrib = ((qd[:, None, None, None] * th[0][:, :, None, None]) * th[1][:, None, :, None]) * th[2][:, None, None, :]
    shape = np.broadcast_shapes(ix.shape, iy.shape, iz.shape)
    IX, IY, IZ = (np.broadcast_to(v, shape)[keep] for v in (ix, iy, iz))
    if mutate == "axes_swapped_in_mesh" and mesh[0] == mesh[1]:
        IX, IY = IY, IX
    count = np.zeros(mesh, dtype=np.int64)
    np.add.at(count, (IX, IY, IZ), 1)
    out = {"count": count, "G": G, "scale": scale}
    if route == "ld":
        Q = np.zeros(mesh, dtype=LD)
        np.add.at(Q, (IX, IY, IZ), contrib[keep])
        FQ = dft3_ld(Q, -1)
        conv = G * FQ
        phi = (scale * dft3_ld(conv, +1)).real
        E = LD(0.5) * scale * (G * (FQ.real ** 2 + FQ.imag ** 2)).sum()
    else:
        Qint = np.zeros(mesh, dtype=np.int64)
        np.add.at(Qint, (IX, IY, IZ), np.rint(contrib[keep] * FIX).astype(np.int64))
        Q = Qint.astype(np.float64) * (1.0 / FIX)
        G64, s64 = G.astype(np.float64), float(scale)
        FQ = np.fft.fftn(Q)
        conv = G64 * FQ
        phi = np.fft.ifftn(conv * (G64 * 0 + s64)).real * float(np.prod(mesh))
        E = 0.5 * s64 * float((G64 * (FQ.real * FQ.real + FQ.imag * FQ.imag)).sum())
        out["Qint"] = Qint
    ph = phi[ix, iy, iz]                                                       # (N, p, p, p)
    KoL = [dtype(mesh[k]) / dtype(float(case["box"][k])) if route != "ld" else LD(mesh[k]) / box[k] for k in range(3)]
    X, Y, Z, dX, dY, dZ = th[0], th[1], th[2], dth[0], dth[1], dth[2]
    F = np.zeros((N, 3), dtype=dtype)
    F[:, 0] = -qd * KoL[0] * np.einsum("nijk,ni,nj,nk->n", ph, dX, Y, Z)
    F[:, 1] = -qd * KoL[1] * np.einsum("nijk,ni,nj,nk->n", ph, X, dY, Z)
    F[:, 2] = -qd * KoL[2] * np.einsum("nijk,ni,nj,nk->n", ph, X, Y, dZ)
    absGF = np.abs(G * FQ) if route == "ld" else np.abs(G.astype(np.float64) * FQ)
    Phi = scale * LD(absGF.sum())
    aX, aY, aZ, adX, adY, adZ = (np.abs(v).astype(LD) for v in (X, Y, Z, dX, dY, dZ))
    sums = [v.sum(1) for v in (aX, aY, aZ, adX, adY, adZ)]
    geo = (LD(mesh[0]) / box[0]) * sums[3] * sums[1] * sums[2] + (LD(mesh[1]) / box[1]) * sums[0] * sums[4] * sums[2] + (LD(mesh[2]) / box[2]) * sums[0] * sums[1] * sums[5]
    out.update(Q=Q, FQ=FQ, phi=phi, E=E, F=F, SF=np.abs(q).astype(LD) * Phi * geo,
               SE=LD(0.5) * scale * LD((np.abs(G.astype(np.float64)) * np.abs(FQ)).sum()) * LD(np.abs(Q).sum()))
    return out


def worst_ratios(F, E, ref):
    """(max_i |F_i - F_ref,i| / S_F,i, |E - E_ref| / S_E) against an spme() result; a neutral atom must carry no force"""
    return er.worst_ratios(F, E, ref)


def rel_rms(F, Fref):
    d = np.asarray(F, dtype=LD) - np.asarray(Fref, dtype=LD)
    return float(np.sqrt((d * d).sum() / (np.asarray(Fref, dtype=LD) ** 2).sum()))


# ---- the systems ------------------------------------------------------------------------------------------------------------------------------
def as_spme(case, mesh, order, **over):
    c = dict(case)
    c.update(elec_type=4, spme_mesh=tuple(int(v) for v in mesh), spme_order=int(order))
    c.update(over)
    return c


def jittered_rocksalt(jitter=0.3, seed=5):
    """512 ions, L = 22.56, alpha = 0.3: the box the convergence table is measured on.  rReal = 1 lies inside the nearest-neighbour distance
    2.82 - 2 sqrt(3) jitter, so an engine's forces() is the reciprocal part alone."""
    c = er.rocksalt_case()
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in ("x", "y", "z"):
        c[k] = c[k] + rng.uniform(-jitter, jitter, size=len(c[k]))
    c.update(rReal=1.0, names=["Na", "Cl"], use_clist=1, cell_list=5.0, T=0.0, tstat_type=0, nEq=0, freqEq=1, init_forces=1, seed=12345, nsteps=0)
    return c


CONVERGED_K = (14, 14, 14)        # |l| <= 13: exp(-k_cut^2 / 4 alpha^2) = 6e-21 for L = 22.56, alpha = 0.3 (k_cut = 1.05 * 14 * 2 pi / L)
TABLE = [((32, 32, 32), 4), ((32, 32, 32), 6), ((64, 64, 64), 6), ((32, 32, 32), 8), ((64, 64, 64), 8)]


def converged_plain_sum(case):
    """the plain Ewald sum of tests/ewald_reference.py, converged: reciprocal() result in long double"""
    kv = er.kvectors(case["box"], case["alpha"], CONVERGED_K)
    full = er._reciprocal_ld(case, kv)
    kcut2 = kv["rkcut2"]
    assert np.exp(-kcut2 / (4 * case["alpha"] ** 2)) < 1e-16
    return full


#           atoms  cells (lattice sites per axis)  spacing            mesh            order  walls
ISOLATED = {
    "one":    (1,    (1, 1, 1),                      (8.0, 8.0, 8.0),   (8, 8, 8),      4,     False),     # every support wraps
    "two":    (2,    (2, 4, 8),                      (5.0, 5.0, 5.0),   (8, 16, 32),    6,     False),     # box 10 x 20 x 40: axis mix-ups
    "n65a":   (65,   (6, 6, 6),                      (3.0, 3.0, 3.0),   (16, 16, 16),   4,     True),
    "n65b":   (65,   (6, 6, 6),                      (3.0, 3.0, 3.0),   (32, 32, 32),   6,     True),
    "n769a":  (769,  (10, 10, 10),                   (3.0, 3.0, 3.0),   (16, 16, 16),   4,     True),
    "n769b":  (769,  (10, 10, 10),                   (3.0, 3.0, 3.0),   (32, 32, 32),   6,     True),
    "n4097":  (4097, (17, 17, 17),                   (3.0, 3.0, 3.0),   (32, 32, 32),   8,     True),      # more than one workgroup everywhere
    "longx":  (7,    (8, 3, 3),                      (6.0, 3.0, 3.0),   (256, 8, 8),    8,     False),     # the longest line, contiguous
    "longz":  (7,    (3, 3, 8),                      (3.0, 3.0, 6.0),   (8, 8, 256),    8,     False),     # ... and strided
}


RREAL = 1.0         # the atom moved onto a mesh point leaves its site by up to half a mesh spacing (0.94 A) per axis: 3 - 0.4 - 0.94 > 1


def isolated_case(name):
    """Charged species without any VdW entry on a jittered lattice whose spacing exceeds rReal by more than twice the jitter (the placement of
    ewald_reference.isolated_case): forces() is the reciprocal part alone.  `walls`: per axis one atom exactly on 0 and one on nextafter(L, 0);
    and one atom exactly on a mesh point."""
    N, g, sp, mesh, order, walls = ISOLATED[name]
    g, sp = np.array(g), np.array(sp)
    box = g * sp
    rng = np.random.Generator(np.random.PCG64(9000 + N + 31 * sum(mesh) + order))
    sites = rng.permutation(int(g.prod()))[:N]
    idx = np.stack([sites // (g[1] * g[2]), (sites // g[2]) % g[1], sites % g[2]], 1)
    X = idx * sp + rng.uniform(-er.JITTER, er.JITTER, size=(N, 3))
    if N == 1:
        X[0] = (0.3, 7.9, 4.1)
    if walls:
        for ax in range(3):
            on = np.flatnonzero(idx[:, ax] == 0)
            assert len(on) >= 2
            X[on[0], ax] = 0.0
            X[on[1], ax] = -1e-300                                              # wraps to nextafter(L, 0) below
        h = box / np.array(mesh)
        i = N // 2
        X[i] = np.round(X[i] / h) * h                                           # on a mesh point (within the jitter of its site)
    X = np.where(X < 0, X + box, X)
    X = np.minimum(X, np.nextafter(box, 0.0))
    types = np.array([er.TYPE_PATTERN[i % len(er.TYPE_PATTERN)] for i in range(N)], dtype=np.int32)
    alpha = round(float(pc.PI * min(k / b for k, b in zip(mesh, box)) / 4.9), 4)
    return {"box": [float(v) for v in box], "dt": 0.001, "nsteps": 0, "species": list(er.SPECIES), "names": ["Ne", "Na", "Cl"], "vdw": [],
            "types": types, "x": X[:, 0].copy(), "y": X[:, 1].copy(), "z": X[:, 2].copy(), "vx": np.zeros(N), "vy": np.zeros(N), "vz": np.zeros(N),
            "elec_type": 4, "rReal": RREAL, "alpha": alpha, "spme_mesh": tuple(mesh), "spme_order": order, "T": 0.0, "tstat_type": 0, "nEq": 0,
            "freqEq": 1, "use_clist": 1, "cell_list": 2.5, "center_box": 0, "init_forces": 1, "seed": 12345}


def coulomb_total_model(case, route="ld"):
    """real-space erfc term (pairs within rReal, minimum image) + the mesh part + ewald_const, as finish_model and the pair kernels form them;
    the real-space and constant parts in long double"""
    import math
    rec = spme(case, route)
    q = er.charges(case)
    X = np.stack([case["x"], case["y"], case["z"]], 1)
    box = np.array(case["box"], dtype=np.float64)
    al, rc2 = float(case["alpha"]), float(case["rReal"]) ** 2
    erfc = np.frompyfunc(math.erfc, 1, 1)
    real = 0.0
    for i in range(len(q) - 1):
        d = X[i] - X[i + 1:]
        d -= box * np.round(d / box)
        r2 = (d * d).sum(1)
        sel = (r2 <= rc2) & (q[i + 1:] != 0.0)
        r = np.sqrt(r2[sel])
        real += float((q[i] * q[i + 1:][sel] * erfc(al * r).astype(np.float64) / r).sum())
    pi = float(er.PI_STR)
    const = pc.FCOUL * (-al / math.sqrt(pi) * float((q * q).sum()) - 0.5 * pi * float(q.sum()) ** 2 / al / al / float(box.prod()))
    return {"real": pc.FCOUL * real, "rec": float(rec["E"]), "const": const, "total": pc.FCOUL * real + float(rec["E"]) + const}
