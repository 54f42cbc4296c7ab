"""Replicated boxes that hold a loopback slab rank to the one-GPU engine (tests/test_slab_cases_model.py on the CPU, tests/test_gpu_slab_loopback.py on
the GPU): numpy only.

A loopback rank (LoopbackExchanger, csrc/exchange.h) sends its halo and its migrants to itself, one slab width along x away: "the physics is that of a
system made of N copies of this slab".  So the truth for rank r of n is a box that IS n exact translates of one period along x, run by the ordinary
one-GPU engine - which is held to the oracle and to high-precision references everywhere else.  With options.loopback_ranks = 2 (slab={"loopback": True,
"replicated": True}) the transport also moves ids from copy to copy (copy index -+ 1 on the way), so the rank holds the very ids rank r of a real n-rank run of the
box would hold: owned sets, bond and angle partners across a seam and md_to_host can be compared id by id.

  period    5 x 5 x 5 FCC cells of a = 5.75 A ('lj', 'fennell', 'hot': 500 atoms) or 8 x 8 x 8 triatomic molecules 3.59375 A apart ('mol': 1 536 atoms) in
            p = 28.75 A.  p and every coordinate are multiples of 2^-20 A, so x + k p is exact in fp64 for every copy of every box used here and copy k is
            an exact translate of copy 0 (asserted by the CPU test with np.array_equal).
  ids       replicate(): copy k of atom j has id k n0 + j, bonds and angles are copied with the id offset; the boxes the tests run (box_case()) use the
            interleaved numbering j n + k that options.loopback_ranks = 2 asks for.  Molecules are kept whole before they are copied (a ligand
            may start beyond p), so that a molecule across a seam is bonded to the atoms next to it and not to their images a period away; replicate()
            wraps the copies into [0, n p).
  grid      cell_size = (p / 3) (1 - 1e-9), passed explicitly: Engine::choose_cells takes floor(L / size), and the relative margin - far above the rounding
            of n p / size, far below anything that could add a layer - gives exactly 3 n layers along x (3 per rank: two boundary layers and an interior one
            for the overlapped exchange, hw = 1 at rc 8.5 and 7.5) and 3 cells along y and z, the fewest that keep the tiled pair kernels and the pair lists.
  seams     the lattice is shifted so that a lattice plane lies 0.01 A inside every slab boundary, the periodic wall included.  Its 50 atoms are spread
            by 0.015 to 0.04 A about that position, each to the side it is moving away from: at 85 K (1.3 A / ps per axis, 0.0013 A per step) most of
            the 25 that move either way cross the boundary within 60 steps.  The central atoms of a plane of molecules ('mol') lie within 0.1 A of the
            boundary, their ligands an Angstrom to either side.  No atom starts within 1e-6 A of a boundary.

Deliberately not here:
  * the radiative thermostat.  Its draws and its photon index are keyed by atom id, so the copies of a replicated box decorrelate at the first photon: the
    box stops being periodic in p and no loopback rank can follow it.
  * the Ewald sum, the Nose-Hoover thermostat and equilibration rescaling.  They need sums over all ranks, and LoopbackExchanger::allreduce_sum and
    allreduce_device are empty: a loopback rank would use the structure factor or the kinetic energy of its own slab alone.
  For those a loopback rank's timing means something, its physics does not (include/aztot.h, options.loopback_ranks).
"""
import math

import numpy as np

from aztotmd_amd import inputs

A = 5.75                                  # dyadic lattice constant
NC = 5                                    # FCC cells per period and axis
P = A * NC                                # 28.75 A: the period, and the slab width
K = 3                                     # cell layers per period (and per rank)
CELL_SIZE = (P / K) * (1.0 - 1e-9)
Q = 2.0 ** 20                             # coordinates are multiples of 1 / Q
SEAM_INSIDE = 0.01                        # mean distance of the seam plane from the boundary, on its upper side
SEAM_SPREAD_MIN, SEAM_SPREAD = 0.015, 0.04
MOL_GRID = 8                              # molecules per period and axis: spacing P / 8 = 3.59375 A, dyadic
STATE_KEYS = ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz")
INTERLEAVED = True                        # numbering of box_case()
_CACHE = {}


def _quantise(a):
    return np.round(np.asarray(a, dtype=np.float64) * Q) / Q


def _fcc(seed, vel_T, **kw):
    """lj_case on the dyadic lattice with the seam plane in place and everything rounded to 2^-20 A"""
    c = inputs.lj_case((NC, NC, NC), a=A, seed=seed, vel_T=vel_T, **kw)
    assert c["box"] == [P, P, P]
    rng = np.random.default_rng(seed + 1000)
    x = np.asarray(c["x"], dtype=np.float64)
    # lj_case puts lattice plane i at 0.25 + i a / 2 (+- 0.15 of jitter): plane 0 becomes the seam plane, the others are moved along with it
    plane0 = x < 0.25 + 0.2
    assert plane0.sum() == 2 * NC * NC
    x = x - 0.25 + SEAM_INSIDE
    # the plane has 50 atoms and half of them move either way: an atom starts on the side it is leaving, 0.015 to 0.04 A from the plane's mean position
    # (0.005 to 0.03 A below the boundary, or 0.025 to 0.05 A above it), so that most of the 25 cross within 60 steps of 0.0013 A
    toward = np.sign(np.asarray(c["vx"])[plane0])
    toward[toward == 0.0] = 1.0
    x[plane0] = SEAM_INSIDE - toward * rng.uniform(SEAM_SPREAD_MIN, SEAM_SPREAD, size=int(plane0.sum()))
    c["x"] = _quantise(np.mod(x, P))
    for k in ("y", "z"):
        c[k] = _quantise(c[k])
    for k in ("x", "y", "z"):
        assert c[k].min() >= 0.0 and c[k].max() < P
    return c


def period(name):
    """the one-period case of a system (not meant to be run by itself: 'mol' holds whole molecules, some of whose atoms lie beyond p)"""
    if name in _CACHE:
        return _CACHE[name]
    if name == "lj":              # one species, Lennard-Jones, rc 8.5: the one-species list kernel
        c = _fcc(seed=411, vel_T=85.0)
    elif name == "fennell":       # two charged species, LJ + Fennell: the table-driven kernel
        c = _fcc(seed=412, vel_T=85.0, charges=(0.2, -0.2), elec="fenn")
    elif name == "hot":           # 'lj' at 4 000 K: outruns a sort interval held at 32 steps
        c = _fcc(seed=413, vel_T=4000.0)
    elif name == "mol":           # bent triatomics with bonds and angles, LJ + Fennell between the central atoms; some straddle the seams
        c = inputs.molecular_case((MOL_GRID,) * 3, a=P / MOL_GRID, seed=414, charges=(-0.2, 0.1), elec="fenn", vel_T=300.0)
        assert c["box"] == [P, P, P]
        # whole molecules along x: the ligands next to their central atom (molecular_case wrapped them into the box one by one)
        cen = np.repeat(np.arange(0, len(c["types"]), 3), 3)
        v = np.asarray(c["x"], dtype=np.float64)
        v = v - P * np.round((v - v[cen]) / P)
        # the central atoms of the first site plane sit 1.8 A above the boundary, with ligands 1 A long: move everything so that they lie around it
        # (+- 0.1 A), some molecules on either side and many across
        v = v - (0.5 * P / MOL_GRID) + SEAM_INSIDE
        c["x"] = _quantise(v - P * np.floor(v[cen] / P))  # molecule by molecule, by where the central atom lies
        for k in ("y", "z"):
            v = _quantise(c[k])
            v[v >= P] = 0.0
            c[k] = v
    else:
        raise KeyError(name)
    c["cell_list"] = CELL_SIZE
    _CACHE[name] = c
    return c


def copy_ids(n, n0, k, interleaved=False):
    """ids of copy k of the atoms 0 ... n0 - 1 of the period: k n0 + j, or j n + k in the interleaved numbering"""
    j = np.arange(n0)
    return j * n + k if interleaved else k * n0 + j


def replicate(case, n, interleaved=False):
    """n copies of `case` along x: copy k of atom j gets id k n0 + j and is translated by k p (p = case["box"][0]), wrapped into [0, n p) - exact for
    coordinates that are multiples of 2^-20 A; velocities, types and radii are copied, bonds and angles are copied with the id offset; box[0] = n p.
    interleaved: id j n + k instead (bonds and angles follow) - the numbering options.loopback_ranks = 2 asks for, see box_case()"""
    n0 = len(case["types"])
    p = float(case["box"][0])
    out = dict(case)
    out["box"] = [n * p, float(case["box"][1]), float(case["box"][2])]
    ids = [copy_ids(n, n0, k, interleaved) for k in range(n)]

    def spread(per_copy, dtype):
        a = np.empty(n * n0, dtype=dtype)
        for k in range(n):
            a[ids[k]] = per_copy(k)
        return a

    x0 = np.asarray(case["x"], dtype=np.float64)
    out["x"] = spread(lambda k: np.mod(x0 + k * p, n * p), np.float64)
    assert out["x"].min() >= 0.0 and out["x"].max() < n * p
    for key in ("y", "z", "vx", "vy", "vz"):
        out[key] = spread(lambda k, v=np.asarray(case[key], dtype=np.float64): v, np.float64)
    out["types"] = spread(lambda k: np.asarray(case["types"], dtype=np.int32), np.int32)
    for key, cols in (("bonds", 2), ("angles", 3)):
        if case.get(key) is not None and len(case[key]):
            rows = np.asarray(case[key], dtype=np.int32)
            parts = []
            for k in range(n):
                r = rows.copy()
                r[:, :cols] = ids[k][rows[:, :cols]]      # (the last column is the type)
                parts.append(r)
            out[key] = np.concatenate(parts)
    return out


def box_case(name, n):
    """the replicated box of system `name` for n ranks, in the interleaved numbering (INTERLEAVED below): the replicated loopback turns copy k of an atom
    into copy k -+ 1 on the way, and only with the copy index in the low digits does that keep the order of the ids inside a cell - which a plain step's
    coordinate exchange relies on (ghosts and their sources are sorted alike)"""
    key = (name, n)
    if key not in _CACHE:
        _CACHE[key] = replicate(period(name), n, interleaved=INTERLEAVED)
    return _CACHE[key]


def expected_grid(case, n, cell_size=CELL_SIZE):
    """Engine::choose_cells for a slab engine of n ranks with an explicit cell_size: (cells per axis, half-width of the stencil along x, slab width).
    floor(L / size) cells; along x a count that does not divide by n is rounded down to one that does if that lengthens the cells by 8 % at most."""
    rmax = max([v[3] for v in case["vdw"]] + [case.get("rReal") or 0.0])
    dims = []
    for k, L in enumerate(case["box"]):
        m = max(1, min(1024, int(math.floor(L / cell_size))))
        if k == 0 and n > 1 and m % n != 0:
            even = m - m % n
            if even >= 2 * n and m / even <= 1.08:
                m = even
        dims.append(m)
    csz = case["box"][0] / dims[0]
    hw = max(int(math.ceil(rmax / csz - 1e-12)), 1)
    lo = [dims[0] * r // n for r in range(n + 1)]
    widths = {(lo[r + 1] - lo[r]) * csz for r in range(n)}
    assert len(widths) == 1, widths
    return tuple(dims), hw, widths.pop()


def boundaries(n, L):
    """lower boundaries of the n slabs (the first is the periodic wall)"""
    return np.array([r * (L / n) for r in range(n)])


def owner(x, n, L):
    """rank whose [xlo, xhi) holds x (x in [0, L))"""
    x = np.asarray(x, dtype=np.float64)
    r = np.floor(x * (n / L)).astype(np.int64)
    w = L / n
    r = np.where(x < r * w, r - 1, r)                     # (floor of a rounded product, put right against the boundaries themselves)
    r = np.where(x >= (r + 1) * w, r + 1, r)
    return np.mod(r, n)


def seam_distance(x, n, L):
    """distance of every x from the nearest slab boundary, the periodic wall included"""
    w = L / n
    d = np.mod(np.asarray(x, dtype=np.float64), w)
    return np.minimum(d, w - d)


def slab_changes(x_first, x_last, n, L):
    """[(atoms that changed slab in the positive direction, in the negative direction)] per boundary (the one nearest to where the atom ended: no atom
    moves half a slab in a test) between two sets of positions"""
    changed = owner(x_first, n, L) != owner(x_last, n, L)
    d = position_diff(x_last, x_first, L)
    b = np.mod(np.round(np.asarray(x_last, dtype=np.float64) * (n / L)).astype(np.int64), n)
    return [(int((changed & (b == k) & (d > 0)).sum()), int((changed & (b == k) & (d < 0)).sum())) for k in range(n)]


def position_diff(a, b, L):
    """a - b, taken to the nearest periodic image"""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return d - L * np.round(d / L)


def rel_diff(a, b, L=None):
    """util.rel_err's measure, max |a - b| / max |b|; for coordinates (L given) the difference is taken to the nearest image"""
    d = position_diff(a, b, L) if L else np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.abs(d).max() / (np.abs(np.asarray(b, dtype=np.float64)).max() + 1e-300))


def divergence(state, n, p, box=None, interleaved=False):
    """{key: largest relative difference between copy k and copy 0} of a full-box state (atoms in id order, copy k = copy_ids(n, n0, k, interleaved)): how
    far the roundings of a one-GPU run have taken its own copies apart.  x is taken minus k p (to the nearest image of the box n p)."""
    out = {}
    for key in STATE_KEYS:
        if key not in state:
            continue
        v = np.asarray(state[key], dtype=np.float64)
        n0 = len(v) // n
        worst = 0.0
        for k in range(1, n):
            a, b = v[copy_ids(n, n0, k, interleaved)], v[copy_ids(n, n0, 0, interleaved)]
            if key == "x":
                worst = max(worst, rel_diff(a - k * p, b, n * p))
            elif key in ("y", "z"):
                worst = max(worst, rel_diff(a, b, box[{"y": 1, "z": 2}[key]] if box else None))
            else:
                worst = max(worst, rel_diff(a, b))
        out[key] = worst
    return out


def stray_bond_case(n=3):
    """box_case('lj', n) with ONE harmonic bond between an atom of the middle layer of slab 0 and its copy in slab 1 (a period away: less than half the box
    for n >= 3): two or more cell layers from every atom slab 0 owns, so never among its ghosts (hw = 1).  k is small and r0 the distance itself: the bond
    exerts no force to speak of."""
    c = dict(box_case("lj", n))
    x = np.asarray(c["x"])
    csz = c["box"][0] / (n * K)
    n0 = len(x) // n
    own, nxt = copy_ids(n, n0, 0, INTERLEAVED), copy_ids(n, n0, 1, INTERLEAVED)
    m = int(np.argmin(np.abs(x[own] - 1.5 * csz)))               # an atom in the middle of slab 0's middle layer
    j, partner = int(own[m]), int(nxt[m])
    c["bond_types"] = [(0, 0, 1, [0.01, P])]
    c["bonds"] = np.array([(j, partner, 1)], dtype=np.int32)
    return c, j, partner
