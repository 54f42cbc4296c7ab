"""Systems of ISOLATED pairs for the pair-function tests (tests/test_gpu_pair_functions.py, tests/test_pair_functions_model.py).

Each case puts M pairs on a cubic grid of sites whose spacing exceeds 2 rMax + 1, so every atom has exactly one partner inside rMax and its force
is one pair term f(r) d, comparable pair by pair.  Pairs have random orientations (dx, dy, dz all non-zero); the sites of the first grid plane
along x and y sit on the periodic walls, so those pairs straddle them.  Coordinates are multiples of 2^-32: every difference and every image
shift is exact in fp64.  The cells are half a site spacing wide (an integer edge, `cell_list`), so the cell centres the staging kernels subtract
(k_pair_tile / k_pair_list work on x - centre) are dyadic as well: x - centre is exact, d is the same whichever kernel forms it, and the two visits
of a pair see exactly negated d.  (With a non-dyadic cell edge x - centre can round, differently for the two atoms' cells, and Newton's third law
then holds only to rounding.)  Every species is frozen: step(n) keeps the positions bit-exact, so the list
kernel sees the same pairs as the tile kernel.

Per species pair the separations are log-spaced from just outside the radius where f^2 reaches 1e10 up to the cut-off, dense in the last 0.5 A
before every cut-off, plus two pairs at f^2 = 1e10 (1 -+ 1e-6) (the drop rule of integrators.cpp:170) and the case's own edge points.
Cut-off ties: axis-aligned pairs on dyadic coordinates with r^2 == rc^2 exactly and the nearest representable separations on either side.
Cases with `filler` also carry a lattice of neutral atoms of a species without any potential: they add exactly nothing to any force, make the
cells dense enough for the pair lists to overflow under DBG_SHORT_LISTS (so cells go through the clean-up launch), and are the neutral species
among charged ones / the species pair without a potential.

No mpmath here: the GPU test imports this module to rebuild the systems whose reference values tests/golden/pair_functions.npz holds.
"""
import math
import zlib

import numpy as np

Q = 2.0 ** -32                         # coordinate quantum
TAU = 1e-13                            # |f_gpu - f_ref| <= TAU S_F (pair_reference.py); the CPU test holds the fp64 oracle to it first
PI = 3.14159265359                     # csrc/model.h units::pi
FCOUL = 0.25 / PI / 8.854187817E-12 * 1.60217657E-19 ** 2 / 1e-20 / (1.60217733E-19 / 1e-10)   # units::Fcoul_scale (placement only)

LJ = (0.01006, 3.3952)


def _pairs(n):
    return [(a, b) for a in range(n) for b in range(a, n)]


def _spec(name):
    """User-level description of case `name`: species [(mass, q)], vdw [(a, b, type, rc, params)], electrostatics, extra options."""
    s = dict(species=None, vdw=None, elec=0, rReal=0.0, alpha=0.0, filler=False, edges={}, ties=[], radii=None, keepcut=False, seed=zlib.crc32(name.encode()) % 1000)
    fam, _, rest = name.partition("_")
    P2 = {"lnjs": lambda a, b, rc: (a, b, 1, rc, [LJ[0] * (1 + 0.3 * a), LJ[1] * (1 - 0.05 * b)]),
          "buck": lambda a, b, rc: (a, b, 2, rc, [1822.0 - 300 * b, 0.3 - 0.01 * a, 63.0 - 20 * b]),
          "p746": lambda a, b, rc: (a, b, 3, rc, [3000.0, 1.0, 20.0 + 5 * b]),
          "bmhs": lambda a, b, rc: (a, b, 4, rc, [0.25, 3.1, 3.3 - 0.1 * b, 60.0 - 10 * a, 80.0])}
    if fam in P2 and rest in ("", "dir", "fenn", "ewald"):
        # two charged species (+ filler when charged): one pair with a shorter cut-off (per-pair test live, ties on it)
        s["species"] = [(39.9, 0.4), (20.2, -0.4)] if rest else [(39.9, 0.0), (20.2, 0.0)]
        s["vdw"] = [P2[fam](0, 0, 7.0), P2[fam](0, 1, 6.5), P2[fam](1, 1, 7.0)]
        s["ties"] = [(0, 1, 6.5)]
        if rest:
            s.update(elec={"dir": 1, "ewald": 2, "fenn": 3}[rest], rReal=7.0, alpha=0.0 if rest == "dir" else 0.4, filler=True)
            s["ties"].append((0, 0, 7.0))
        if fam == "bmhs":
            s["edges"] = {(0, 0): [1.5, 2.0, 2.5, 3.0]}                       # r < sigma: exp_nonpos with a positive argument
        if fam == "buck":
            s["edges"] = {(0, 0): [6.0, 6.9]}
    elif name == "lnjs_fenn_vdw6":     # every pair LJ, cut-offs >= rReal: VDW_LJ_NOCUT (cut-off test compiled out), and DBG_KEEP_VDW_CUT_TEST keeps it
        s.update(species=[(39.9, 0.3), (20.2, -0.3)], vdw=[(a, b, 1, 7.5, [LJ[0], LJ[1]]) for a, b in _pairs(2)], elec=3, rReal=7.5, alpha=0.35, keepcut=True)
        s["ties"] = [(0, 0, 7.5)]
    elif name == "lnjs_fenn_4sp":      # the last uniform case
        q = [0.3, -0.3, 0.5, -0.2]
        s.update(species=[(40.0, v) for v in q], vdw=[(a, b, 1, 7.0 - 0.25 * ((a + b) % 2), [LJ[0] * (1 + 0.1 * a), LJ[1] * (1 - 0.03 * b)]) for a, b in _pairs(4)],
                 elec=3, rReal=7.0, alpha=0.4)
    elif name in ("buck_fenn_4sp", "p746_dir_4sp", "bmhs_ewald_4sp"):   # the other families at 4 species, one electrostatics each
        q = [0.3, -0.3, 0.5, -0.2]
        s.update(species=[(40.0, v) for v in q], vdw=[P2[fam](a % 2, b % 2, 7.0 - 0.25 * ((a + b) % 2))[2:] for a, b in _pairs(4)],
                 elec={"dir": 1, "ewald": 2, "fenn": 3}[rest[:-4]], rReal=7.0, alpha=0.0 if "dir" in rest else 0.4)
        s["vdw"] = [(a, b) + v for (a, b), v in zip(_pairs(4), s["vdw"])]
    elif name == "lnjs_fenn_5sp":      # one species more: generic kernel
        q = [0.3, -0.3, 0.5, -0.2, 0.0]
        s.update(species=[(40.0, v) for v in q], vdw=[(a, b, 1, 7.0, [LJ[0] * (1 + 0.1 * a), LJ[1] * (1 - 0.03 * b)]) for a, b in _pairs(5)],
                 elec=3, rReal=7.0, alpha=0.4)
    elif name == "mixed_fenn":         # VDW 5: families mixed per species pair, and one species pair without a potential
        s.update(species=[(39.9, 0.3), (20.2, -0.3), (30.0, 0.2)],
                 vdw=[P2["lnjs"](0, 0, 7.0), P2["buck"](0, 1, 7.0), P2["bmhs"](1, 1, 6.5), P2["p746"](0, 2, 7.0), P2["lnjs"](2, 2, 7.0)],
                 elec=3, rReal=7.0, alpha=0.4, filler=True)
        s["ties"] = [(1, 1, 6.5)]
    elif name == "elin_einv":          # generic only
        s.update(species=[(39.9, 0.0), (20.2, 0.0)],
                 vdw=[(0, 0, 5, 7.0, [900.0, 0.4, 0.002]), (0, 1, 6, 7.0, [900.0, 0.4, 0.5]), (1, 1, 5, 6.5, [700.0, 0.35, 0.003])])
        s["ties"] = [(1, 1, 6.5)]
        s["edges"] = {(0, 0): [0.5, 0.8], (0, 1): [0.5, 0.8]}                 # r / rho up to ~ 20 .. 2 .. 17
    elif name == "buck_hard":          # Buckingham with r / rho up to several hundred
        s.update(species=[(39.9, 0.0)], vdw=[(0, 0, 2, 7.0, [1.0e6, 0.02, 5.0])])
        s["edges"] = {(0, 0): [3.0, 5.0, 6.0, 6.99]}
    elif name == "lj1":                # MODE 1: one species, LJ, no charges
        s.update(species=[(39.9, 0.0)], vdw=[(0, 0, 1, 6.5, list(LJ))])
        s["ties"] = [(0, 0, 6.5)]
    elif name == "surk1":              # PM_ONE_SURK (and the generic body under DBG_GENERIC_PAIR): radii from the engine's state
        s.update(species=[(39.9, 0.0)], vdw=[(0, 0, 7, 6.0, [75.0, 8.0, 1.0, 1.0])], radii=[(2.73, 4.731, 0.2)])
        s["ties"] = [(0, 0, 6.0)]
    elif name.startswith(("fenn_ar", "ewald_ar")):     # alpha rReal = 3.99, 4.0 (fit, inclusive), 4.2 (libm erfc, generic fallback)
        ar = {"399": 3.99, "400": 4.0, "420": 4.2}[name[-3:]]
        s.update(species=[(39.9, 0.5), (20.2, -0.5)], vdw=[(0, 0, 1, 8.0, list(LJ)), (1, 1, 1, 8.0, list(LJ))], elec=3 if name[0] == "f" else 2,
                 rReal=8.0, alpha=ar / 8.0)
    elif name in ("lnjs_fenn_rbelow", "lnjs_fenn_rabove"):   # rReal below / above the largest VdW cut-off
        rr = 6.0 if name.endswith("below") else 8.0
        s.update(species=[(39.9, 0.3), (20.2, -0.3)], vdw=[(0, 0, 1, 7.0, list(LJ)), (0, 1, 1, 7.0, list(LJ)), (1, 1, 1, 5.0, list(LJ))],
                 elec=3, rReal=rr, alpha=0.4)
    elif name == "lnjs_fenn_coul_drop":   # strong charges, weak short LJ: the Coulomb part sets ljDropR2
        s.update(species=[(39.9, 8.0), (20.2, -8.0)], vdw=[(a, b, 1, 7.0, [1e-3, 0.2]) for a, b in _pairs(2)], elec=3, rReal=7.0, alpha=0.4)
    else:
        raise KeyError(name)
    if s["filler"]:
        s["species"] = s["species"] + [(40.0, 0.0)]
    return s


CASES = ["lnjs", "buck", "p746", "bmhs", "lnjs_dir", "buck_dir", "p746_dir", "bmhs_dir", "lnjs_fenn", "buck_fenn", "p746_fenn", "bmhs_fenn",
         "lnjs_ewald", "buck_ewald", "p746_ewald", "bmhs_ewald", "lnjs_fenn_vdw6", "lnjs_fenn_4sp", "buck_fenn_4sp", "p746_dir_4sp", "bmhs_ewald_4sp", "lnjs_fenn_5sp", "mixed_fenn", "elin_einv",
         "buck_hard", "lj1", "surk1", "fenn_ar399", "fenn_ar400", "fenn_ar420", "ewald_ar400", "ewald_ar420", "lnjs_fenn_rbelow",
         "lnjs_fenn_rabove", "lnjs_fenn_coul_drop"]


def spec(name):
    return _spec(name)


def r_max(s):
    return s["rReal"] if s["elec"] else max(v[3] for v in s["vdw"])


def pot_table(s):
    """{(a, b): (type, rc, params)} for both orders of every species pair with a potential"""
    t = {}
    for a, b, ty, rc, p in s["vdw"]:
        t[(a, b)] = t[(b, a)] = (ty, rc, p)
    return t


def _f_float(s, a, b, r, radius=None):
    """pair force f(r) = -(1/r) dU/dr in plain float (only to place pairs; the reference values come from pair_reference.py)"""
    f = 0.0
    pt = pot_table(s).get((a, b))
    if pt is not None and r <= pt[1]:
        ty, rc, p = pt
        if ty == 1:
            s6 = (p[1] / r) ** 6
            f += 24 * p[0] / r ** 2 * (2 * s6 * s6 - s6)
        elif ty in (2, 5, 6):
            ex = p[0] * np.exp(-r / p[1]) / (p[1] * r)
            f += ex + {2: -6 * p[2] / r ** 8, 5: -p[2] / r, 6: -p[2] / r ** 3}[ty]
        elif ty == 3:
            f += 7 * p[0] / r ** 9 - 4 * p[1] / r ** 6 - 6 * p[2] / r ** 8
        elif ty == 4:
            f += p[1] * p[0] * np.exp(p[1] * (p[2] - r)) / r - 6 * p[3] / r ** 8 - 8 * p[4] / r ** 10
        elif ty == 7:
            ra = radius or 0.577
            f += 7 * p[0] * ra ** 6 / r ** 9 - 6 * p[1] * ra * ra / (p[2] * ra + p[3] * ra) / r ** 8
    qa, qb = s["species"][a][1], s["species"][b][1]
    if s["elec"] and qa and qb and r <= s["rReal"]:
        kqq, al, rc = qa * qb * FCOUL, s["alpha"], s["rReal"]
        if s["elec"] == 1:
            f += kqq / r ** 3
        else:
            d2 = 2 * al / math.sqrt(PI)
            if s["elec"] == 3:
                es2 = math.erfc(al * rc) / rc ** 2 + d2 * math.exp(-(al * rc) ** 2) / rc
                f += kqq / r * (math.erfc(al * r) / r ** 2 + d2 * math.exp(-(al * r) ** 2) / r - es2)
            else:
                f += kqq / r ** 3 * (math.erfc(al * r) + d2 * r * math.exp(-(al * r) ** 2))
    return f


def _drop_bracket(s, a, b):
    """(r_in, r_out): f^2 > 1e10 at r_in, <= 1e10 at r_out, scanning down from rMax; None if the pair never gets there above 0.05 A"""
    r = r_max(s)
    prev = r
    while r > 0.05:
        if _f_float(s, a, b, r) ** 2 > 1e10:
            return r, prev
        prev = r
        r *= 0.97
    return None


def separations(s, a, b):
    """requested r values for species pair (a, b)"""
    rM = r_max(s)
    pt = pot_table(s).get((a, b))
    rc = min(pt[1], rM) if pt is not None else rM
    br = _drop_bracket(s, a, b) if (pt is None or pt[0] != 7) else None      # (surk: the radii come from the engine, no pair is placed on the edge)
    lo = br[1] * 1.02 if br else 0.6 * rc
    rs = list(np.geomspace(lo, rc, 10)[:-1]) + list(np.linspace(rc - 0.5, rc, 5, endpoint=False)[1:])
    if pt is not None and rc < rM:
        rs += list(np.linspace(rM - 0.5, rM, 4, endpoint=False)[1:])      # beyond the per-pair cut-off: Coulomb only / nothing
    rs += list(s["edges"].get((min(a, b), max(a, b)), []))
    return rs, br


def _rng(s):
    return np.random.Generator(np.random.PCG64(20261016 + s["seed"]))


def build(name, xyz=None):
    """(case, pairs): the engine / oracle input dict and per-pair arrays i, j, ti, tj, dx, dy, dz (d = x_i - x_j, minimum image, exact),
    tie (0 / -1 inside / +1 outside / 2 exactly on the cut-off), drop_target (+1 / -1 for pairs placed at f^2 = 1e10 (1 +- 1e-6), else 0).
    xyz: the pair atoms' coordinates (2 M x 3) as the fixture stores them; the placement then only decides the species and flags, so the systems
    the GPU test builds do not depend on how this numpy rounds geomspace, its random stream or libm's exp / erfc."""
    s = spec(name)
    rng = _rng(s)
    nsp = len(s["species"]) - (1 if s["filler"] else 0)
    want = []                                                  # (ti, tj, r, drop_target, drop_bracket)
    for a in range(nsp):
        for b in range(a, nsp):
            if s["elec"] == 0 and (a, b) not in pot_table(s):
                continue
            rs, br = separations(s, a, b)
            want += [(a, b, float(r), 0, None) for r in rs]
            if br:
                want += [(a, b, 0.0, +1, br), (a, b, 0.0, -1, br)]
    ntie = 3 * len(s["ties"])
    M = len(want) + ntie
    n = max(3, int(np.ceil(M ** (1 / 3))))
    rM = r_max(s)
    sp = 2.0 * np.ceil(rM + 2.0)                                # site spacing: an even integer >= 2 rMax + 4 (cells of sp / 2, below)
    L = n * sp
    sites = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3) * sp
    sites[:, 2] += 0.5 * sp                                     # planes i = 0 / j = 0 sit on the x / y walls
    order = rng.permutation(len(sites))
    sites = sites[order]
    # ties first, on sites away from the walls: axis-aligned along a rotating axis, x_j = x_i + rc (exact), then one representable step in / out
    X, T, I, J, TI, TJ, TIE, DROP, R = [], [], [], [], [], [], [], [], []
    inner = [k for k in range(len(sites)) if sites[k, 0] > 0 and sites[k, 1] > 0]
    used = set()
    k_t = 0
    for (a, b, rc) in s["ties"]:
        for side in (2, -1, +1):
            k = inner[k_t]; used.add(k); k_t += 1
            ax = k_t % 3
            xi = sites[k] - 0.5 * rc * np.eye(3)[ax]
            xi = np.round(xi * 4) / 4                            # dyadic, 0.25 steps
            xj = xi.copy()
            xj[ax] = xi[ax] + rc
            if side != 2:
                xj[ax] = np.nextafter(xj[ax], -np.inf if side < 0 else np.inf)
            X += [xi, xj]; T += [a, b]
            R.append(None); TIE.append(side); DROP.append(0)
    rest = [k for k in range(len(sites)) if k not in used]
    for m, (a, b, r, dt_, br) in enumerate(want):
        c = sites[rest[m]]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if dt_:
            r = drop_radius(s, a, b, dt_, br)
        xi, xj = c + 0.5 * r * u, c - 0.5 * r * u
        X += [xi, xj]; T += [a, b]
        R.append(r); TIE.append(0); DROP.append(dt_)
    X = np.array(X)
    nt = 2 * len(TIE) - 2 * len(want)                           # the tie atoms keep their exact dyadic / nextafter coordinates
    X[nt:] = np.round(X[nt:] / Q) * Q
    X = np.mod(X, L)
    X[X >= L] = 0.0
    if xyz is not None:
        assert xyz.shape == X.shape
        X = np.array(xyz, dtype=np.float64)
    types = np.array(T, dtype=np.int32)
    npair = len(T) // 2
    if s["filler"]:                                            # neutral atoms, no potential, >= 1.2 A from every pair atom
        g = np.arange(0.0, L, 3.0)
        F = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 1.0
        d = F[:, None, :] - X[None, :, :]
        d -= L * np.round(d / L)
        keep = (d ** 2).sum(-1).min(1) > 1.44
        F = F[keep]
        X = np.concatenate([X, F])
        types = np.concatenate([types, np.full(len(F), nsp, dtype=np.int32)])
    N = len(types)
    case = {"box": [L, L, L], "dt": 0.001, "nsteps": 0, "species": s["species"], "names": ["S%d" % k for k in range(len(s["species"]))],
            "vdw": s["vdw"], "types": types, "x": X[:, 0].copy(), "y": X[:, 1].copy(), "z": X[:, 2].copy(),
            "vx": np.zeros(N), "vy": np.zeros(N), "vz": np.zeros(N), "elec_type": s["elec"], "rReal": s["rReal"], "alpha": s["alpha"],
            "T": 0.0, "tstat_type": 0, "nEq": 0, "freqEq": 1, "use_clist": 1, "cell_list": 0.5 * sp, "center_box": 0, "init_forces": 1,
            "radii": s["radii"], "seed": 12345, "frozen": [1] * len(s["species"])}
    if s["elec"] == 2:
        case["ewald_k"] = (1, 1, 1)                              # no k-vector survives: the real-space term is the whole pair force
    i = np.arange(npair) * 2
    j = i + 1
    d = X[i] - X[j]
    d -= L * (d > 0.5 * L)
    d += L * (d < -0.5 * L)
    pairs = {"i": i, "j": j, "ti": types[i], "tj": types[j], "dx": d[:, 0].copy(), "dy": d[:, 1].copy(), "dz": d[:, 2].copy(),
             "tie": np.array(TIE), "drop_target": np.array(DROP)}
    return case, pairs


def drop_radius(s, a, b, side, br):
    """r where f^2 = 1e10 (1 + side 1e-6) inside the bracket (float bisection on the placement force; the reference decides afterwards)"""
    target = 1e10 * (1 + side * 1e-6)
    lo, hi = br                                                 # f^2(lo) > 1e10 >= f^2(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _f_float(s, a, b, mid) ** 2 > target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def r2_fp64(pairs):
    """r^2 as the kernels form it for axis-aligned and general pairs alike (fp64, left to right)"""
    return pairs["dx"] * pairs["dx"] + pairs["dy"] * pairs["dy"] + pairs["dz"] * pairs["dz"]


# ---- isolated bonded molecules ---------------------------------------------------------------------------------------------------------------
# Species C (0) and L (1), no charges; the only pair potential is C-C with a 2.5 A cut-off, and the molecules sit 8 A apart, so bonds and angles are
# the whole force.  'bonds': one C-L bond per molecule, all five bond types from 0.7 r0 (compressed) to 1.5 r0 (stretched), every second one listed
# ligand-first.  'angles': L-C-L with an hcos angle and no bonds, from 2 deg to exactly 180 deg (axis-aligned, so cos th == -1 in fp64).
BONDED_CASES = ["bonds", "angles"]
BOND_TYPES = [(0, 1, 1, [30.0, 1.0]), (0, 1, 2, [4.0, 2.0, 1.0, 0.5]), (0, 1, 3, [4.0, 2.0, 1.0, 0.5, 0.002]), (1, 0, 4, [2.0e4, 0.1, 1.513]),
              (0, 1, 5, [2.0e4, 0.1, 1.1467, 0.2, 0.05])]
BOND_STRETCH = [0.7, 0.85, 0.95, 1.0, 1.05, 1.2, 1.5]
ANGLE_TYPE = (0, 1, [3.0, -0.33])
ANGLE_DEG = [2.0, 10.0, 45.0, 90.0, 109.5, 150.0, 179.0, 180.0]


def build_bonded(name, xyz=None):
    """(case, mols): the engine / oracle input and, per molecule, its atoms (c, l) or (c, l1, l2) and its type id (1-based)"""
    rng = np.random.Generator(np.random.PCG64(20261017 + zlib.crc32(name.encode()) % 1000))
    if name == "bonds":
        mols = [(t, f) for t in range(1, 6) for f in BOND_STRETCH]
    else:
        mols = [(1, d) for d in ANGLE_DEG]
    n = max(3, int(np.ceil(len(mols) ** (1 / 3))))
    sp = 8.0
    L = n * sp
    sites = (np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3) + 0.5) * sp
    X, T, bonds, angles = [], [], [], []
    for m, (t, v) in enumerate(mols):
        c = sites[m]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if name == "bonds":
            r = v                                                   # every bond type has its minimum at r0 = 1.0 (inputs.molecular_case)
            k0 = len(X)
            X += [c + 0.5 * r * u, c - 0.5 * r * u]; T += [0, 1]
            bonds.append((k0 + 1, k0, t) if m % 2 else (k0, k0 + 1, t))
        else:
            th = np.radians(v)
            if v == 180.0:
                e1, e2 = np.array([1.0, 0.0, 0.0]), np.array([-1.0, 0.0, 0.0])
            else:
                w = rng.normal(size=3)
                w -= (w @ u) * u
                w /= np.linalg.norm(w)
                e1, e2 = u, np.cos(th) * u + np.sin(th) * w
            k0 = len(X)
            X += [c, c + 1.0 * e1, c + 0.97 * e2]; T += [0, 1, 1]
            angles.append((k0, k0 + 1, k0 + 2, t))
    X = np.round(np.array(X) / Q) * Q
    if xyz is not None:
        assert xyz.shape == X.shape
        X = np.array(xyz, dtype=np.float64)
    N = len(T)
    case = {"box": [L, L, L], "dt": 0.0005, "nsteps": 0, "species": [(15.999, 0.0), (1.008, 0.0)], "names": ["C", "L"],
            "vdw": [(0, 0, 1, 2.5, list(LJ))], "types": np.array(T, dtype=np.int32), "x": X[:, 0].copy(), "y": X[:, 1].copy(), "z": X[:, 2].copy(),
            "vx": np.zeros(N), "vy": np.zeros(N), "vz": np.zeros(N), "elec_type": 0, "rReal": 0.0, "alpha": 0.0, "T": 0.0, "tstat_type": 0,
            "nEq": 0, "freqEq": 1, "use_clist": 1, "cell_list": 4.0, "center_box": 0, "init_forces": 1, "radii": None, "seed": 12345,
            "frozen": [1, 1], "bond_types": BOND_TYPES if name == "bonds" else [], "angle_types": [ANGLE_TYPE] if name == "angles" else [],
            "bonds": np.array(bonds, dtype=np.int32).reshape(-1, 3), "angles": np.array(angles, dtype=np.int32).reshape(-1, 4)}
    return case, mols
