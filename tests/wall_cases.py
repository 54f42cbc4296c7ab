"""A force-free gas with designed wall atoms (tests/test_walls_model.py on the CPU, tests/test_gpu_walls.py on the GPU): numpy only.

The first half of a step - half-kick, drift, periodic wrap, wall-crossing counters with wall momenta - is written out five times in csrc/ (k_integrate1_bin
<STEP_RESORT> and <STEP_PLAIN>, integrate_plain2_body as k_integrate_plain2 and k_drift_plain2, the second half of k_boundary_radi, next_step_atom /
next_step_finish behind k_pair_list and the clean-up launch of k_pair_tile).  A thermal run lets a handful of atoms cross a wall per step, wherever they
happen to sit.  Here every crossing is placed on purpose.

  box       three different lengths, asserted by check_box(): L_x = 37.3 with int((2 L) * (1 / L)) == 1, L_y = 64 dyadic, L_z = 52.98 with L * (1 / L) < 1
  lattice   11 x 19 x 16 sites of spacing L / n (3.39, 3.37, 3.31 A) whose plane 0 lies ON the wall of every axis; an atom of plane 0 sits just inside the
            lower wall or just inside the upper one - the same periodic site.  Interior coordinates are jittered by +- 0.15 A, so no two atoms ever
            come closer than 3.0 A: LJ with the 2.5 A cut-off of pair_cases gives forces of exactly 0 and v stays constant (min_distance(); asserted on
            every step by the CPU test).  Three species: two mobile ones of different mass and a frozen one that is given velocities all the same.
  dt        2^-9.  Designed atoms have dyadic velocities, so v dt and every partial sum of the drift are exact in fp64 - the same with or without an FMA.
  ids       a random permutation of the sites: the sorted order (cell index (cx ncy + cy) ncz + cz, ids ascending inside a cell) is not the id order
  classes   per (atom, axis) of plane 0, each on both walls where it exists, in both mobile species; s is the step of the event
              cross    crosses outward by a generic amount at step s; half a step length (>= 3e-4 A) from the wall before and after
              stay     comes within 5e-7 A of the wall at step 12 and never crosses
              land0    lands exactly on 0.0 at step s (no crossing), is beyond it one step later
              landL    lands exactly on L at step s: the every-step rule reports 0.0 and never counts it, the image rule counts it at s + 1
              startL   starts at exactly L, moves inward (never counted) or outward (counted at step 1) - under the every-step rule; a lazy engine's initial
                       force call sets it to 0.0, from where the inward one crosses the LOWER wall at step 1 and the outward one none
              ulp      lower wall: x = 2^-20 before the last step, dx = -(2^-20 + 2^-60): lands on -2^-60 at step 12, counted once, L - 2^-60 rounds to L and
                       is reported as 0.0.  Upper wall: lands on nextafter(L, +inf) at step s, counted once, reported as ulp(L)
              corner   plane 0 of two or of three axes: crosses two or three walls in the same step
              frozen   frozen species, 1e-3 A from the wall, velocity pointing outward: never moves, never counted
              block    the 200 atoms that fill the first cells of the sorted order (plane 0 of x, lower side, y-planes 0..12) and ALL cross the lower x wall at
                       step 3: a wave whose 64 lanes all cross the same wall, threads whose two atoms both cross it
              jump     (variant "jump", every-step schedule only) +-1.5 L and 2.5 L per step along a row of the lattice that holds no other atom, and one
                       atom per axis that starts at 0.0 and moves nextafter(2 L, 0) per step
            The last atom of the sorted order is the corner atom just inside the three upper walls: with N odd it is the unpaired atom of the two-atoms-per-
            thread kernels, in the last, partly filled workgroup, and it crosses three walls at step 4.
layout_counts() counts, from the reference's flags and the sorted order of a grid, the thread / wave / workgroup layouts the kernels distinguish.
"""
import math

import numpy as np

import pair_cases as pc

TAU = pc.TAU
BOX = (37.3, 64.0, 52.98)
GRID = (11, 19, 16)
DT = 2.0 ** -9
RC = 2.5
NSTEPS = 12
SPECIES = [(39.9, 0.0), (20.2, 0.0), (63.5, 0.0)]                 # (mass in amu, charge); species 2 is frozen
FROZEN = [0, 0, 1]
RADII = [(2.73, 4.731, 0.2), (2.1, 3.9, 0.05), (2.4, 4.2, 0.1)]   # radiative variant only
M_SCALE = 1.6605402E-27 / (1.60217733E-19 * 1.0E-12 * 1.0E-12 / 1.0E-10 / 1.0E-10)      # csrc/model.h units::m_scale
JITTER = 0.15
D0 = 2.0 ** -11                                                   # |v dt| of the dyadic classes: v = 2^-2
CROSS_STEPS = (3, 4, 7, 9, 1, 12, 2, 6)
BLOCK_STEP, LAST_ATOM_STEP = 3, 4
BLOCK_PLANES = range(0, 13)                                       # y-planes of the block
CELL_COARSE, CELL_FINE = 0.0, 1.9                                 # Engine(cell_size=): 0 -> the engine's own cells; 1.9 -> more than 16384 cells
# (cells, lazy schedule?) -> grid; asserted against stats()["n_cells"] on the GPU and against grid_dims() on the CPU
N_CELLS = {(CELL_COARSE, True): (14, 24, 19), (CELL_COARSE, False): (14, 25, 21), (CELL_FINE, True): (19, 33, 27), (CELL_FINE, False): (19, 33, 27)}
JUMP_ROWS = {0: [(14, 3), (15, 6), (16, 9), (17, 12)], 1: [(2, 2), (4, 5), (6, 8), (8, 11)], 2: [(3, 4), (5, 8), (7, 12), (9, 18)]}   # the two other indices
JUMP_KINDS = ("+1.5L", "-1.5L", "+2.5L", "2L-")
EXACT_CLASSES = ("land0", "landL", "startL", "ulp", "frozen", "rest")
_CACHE = {}


def check_box():
    """the three rounding properties the box is chosen for, evaluated, not taken on trust"""
    lx, ly, lz = BOX
    assert int((2.0 * lx) * (1.0 / lx)) == 1                      # (2 L) * (1 / L) is twice L * (1 / L), exactly: the two properties go together
    assert math.frexp(ly)[0] == 0.5 and ly * (1.0 / ly) == 1.0
    assert lz * (1.0 / lz) < 1.0
    for L in BOX:                                                 # the upper neighbour of L never truncates to image 0
        assert int(np.nextafter(L, np.inf) * (1.0 / L)) == 1
    return {L: int(np.nextafter(2.0 * L, 0.0) * (1.0 / L)) for L in BOX}


def grid_dims(cell_size, lazy=True):
    """Engine::choose_cells for this system: floor(L / size) cells per axis; size = cell_size if given, else the case's cell_list = rc, which an engine on
    the lazy schedule widens to rc + skin (skin = max(0.15, 0.036 rc))"""
    size = cell_size if cell_size > 0 else (RC + max(0.15, 0.036 * RC) if lazy else RC)
    return tuple(int(math.floor(L / size)) for L in BOX)


def masses():
    return np.array([m * M_SCALE for m, _ in SPECIES])


def _quantise(a):
    return np.round(np.asarray(a) * 2.0 ** 20) / 2.0 ** 20


def _wall_axis(cls, side, s, rng, L):
    """(x0, v) along one axis for a plane-0 atom: side 0 = just inside the lower wall, 1 = just inside the upper wall"""
    W, sg = (0.0, 1.0) if side == 0 else (L, -1.0)                # sg: the inward direction
    if cls in ("cross", "corner", "block"):
        d = float(rng.uniform(0.6e-3, 1.4e-3))
        return W + sg * ((s - 0.5) * d), -sg * d / DT
    if cls == "stay":
        d = float(rng.uniform(0.6e-3, 1.4e-3))
        return W + sg * (NSTEPS * d + 5e-7), -sg * d / DT
    if cls == "land0":
        assert side == 0
        return s * D0, -D0 / DT
    if cls == "landL":
        assert side == 1
        return L - s * D0, D0 / DT
    if cls == "startL":                                           # s: 0 inward, 1 outward
        assert side == 1
        return L, (D0 if s else -D0) / DT
    if cls == "ulp":
        if side == 0:
            assert s == NSTEPS                                    # (one step later the every-step rule, having rounded L - 2^-60 to L -> 0.0, would count it again)
            d = 2.0 ** -20 + 2.0 ** -60
            return s * 2.0 ** -20 + (s - 1) * 2.0 ** -60, -d / DT
        u = float(np.nextafter(L, np.inf) - L)
        d = 2.0 ** -20 + u
        return L - 2.0 ** -20 - (s - 1) * d, d / DT
    if cls == "frozen":
        return W + sg * 1e-3, -sg * 0.7
    raise KeyError(cls)


def _face_plan():
    """[(class, side, s, species)] dealt to the atoms of one face in turn"""
    plan = []
    for sp in (0, 1):
        for k, s in enumerate(CROSS_STEPS):
            plan += [("cross", 0, s, sp), ("cross", 1, s, sp)]
            if k == 3:
                plan += [("stay", 0, 0, sp), ("stay", 1, 0, sp), ("land0", 0, 3, sp), ("land0", 0, NSTEPS, sp), ("landL", 1, 3, sp), ("landL", 1, 8, sp),
                         ("landL", 1, NSTEPS, sp), ("startL", 1, 0, sp), ("startL", 1, 1, sp), ("ulp", 0, NSTEPS, sp), ("ulp", 1, 4, sp), ("ulp", 1, NSTEPS, sp)]
        plan += [("frozen", sp, 0, 2)]
    return plan


def build():
    """the gas: a dict with x, v (N, 3), types, and per (atom, axis) the class name, the side and the event step; cached and read-only"""
    if "gas" in _CACHE:
        return _CACHE["gas"]
    check_box()
    rng = np.random.Generator(np.random.PCG64(20240917))
    a = [L / n for L, n in zip(BOX, GRID)]
    removed, jumpers = set(), {}
    for ax, rows in JUMP_ROWS.items():
        others = [k for k in range(3) if k != ax]
        for kind, (p, q) in zip(JUMP_KINDS, rows):
            for i in range(GRID[ax]):
                site = [0, 0, 0]
                site[ax], site[others[0]], site[others[1]] = i, p, q
                removed.add(tuple(site))
            site[ax] = 0 if kind == "2L-" else 5
            jumpers[tuple(site)] = (ax, kind)
            removed.discard(tuple(site))
    sites = [(i, j, k) for i in range(GRID[0]) for j in range(GRID[1]) for k in range(GRID[2]) if (i, j, k) not in removed]
    if len(sites) % 2 == 0:
        sites.remove((5, 5, 5))
    N = len(sites)
    ids = rng.permutation(N)                                      # id of the atom on sites[k]
    x, v = np.zeros((N, 3)), np.zeros((N, 3))
    types = np.zeros(N, dtype=np.int32)
    cls = np.full((N, 3), "", dtype="U8")
    side, when = np.full((N, 3), -1, dtype=np.int32), np.zeros((N, 3), dtype=np.int32)
    jump = np.full(N, "", dtype="U8")
    jump_axis = np.full(N, -1, dtype=np.int32)
    plan = _face_plan()
    dealt = [0, 0, 0]
    n_int = 0
    for k, site in enumerate(sites):
        i = ids[k]
        zero = [ax for ax in range(3) if site[ax] == 0]
        sp = None
        if site in jumpers:
            ax, kind = jumpers[site]
            jump[i], jump_axis[i] = kind, ax
            zero = []                                             # at rest unless the variant "jump" moves it; the 2L- atom sits at exactly 0.0 on its axis
        ev = None
        if len(zero) >= 2:
            ev = ("corner", (3, 4, 7, 9, 1, 12)[(site[0] + site[1] + site[2]) % 6])
            if site[0] == 0 and site[1] in BLOCK_PLANES:
                ev = ("corner", BLOCK_STEP)
            if site == (0, 0, 0):
                ev = ("corner", LAST_ATOM_STEP)
        for ax in range(3):
            if ax in zero:
                if ev is not None:
                    sd = 1 if site == (0, 0, 0) else int((site[(ax + 1) % 3] + site[(ax + 2) % 3] + ax) % 2)
                    if ax == 0 and site[1] in BLOCK_PLANES and site != (0, 0, 0):
                        sd = 0
                    c, s = ev
                elif ax == 0 and site[1] in BLOCK_PLANES:
                    c, sd, s = "block", 0, BLOCK_STEP
                else:
                    c, sd, s, sp = plan[dealt[ax] % len(plan)]
                    dealt[ax] += 1
                x[i, ax], v[i, ax] = _wall_axis(c, sd, s, rng, BOX[ax])
                cls[i, ax], side[i, ax], when[i, ax] = c, sd, s
            elif site in jumpers and jumpers[site][0] == ax:
                x[i, ax] = 0.0 if jumpers[site][1] == "2L-" else _quantise(site[ax] * a[ax] + 0.37)
                cls[i, ax] = "rest"
            else:
                x[i, ax] = _quantise(site[ax] * a[ax] + rng.uniform(-JITTER, JITTER))
                v[i, ax] = float(rng.uniform(-0.3, 0.3))
                cls[i, ax] = "free"
        if sp is None:
            if zero or site in jumpers:
                sp = int(k % 2)
            else:
                sp = 2 if n_int % 7 == 3 else n_int % 2
                n_int += 1
        types[i] = sp
        if sp == 2:                                               # frozen atoms keep their velocities and never move: every axis is exact
            for ax in range(3):
                if cls[i, ax] == "free":
                    cls[i, ax] = "frozen"
    gas = {"N": N, "x": x, "v": v, "types": types, "cls": cls, "side": side, "when": when, "jump": jump, "jump_axis": jump_axis, "site_of_id": np.array(sites)[np.argsort(ids)]}
    for val in gas.values():
        if isinstance(val, np.ndarray):
            val.setflags(write=False)
    _CACHE["gas"] = gas
    return gas


def velocities(variant="plain"):
    """(N, 3): the designed velocities; variant "jump" adds the per-step displacements of the jump atoms (generic ones, away from every tie of the image
    index, and nextafter(2 L, 0) from 0.0)"""
    g = build()
    v = g["v"].copy()
    if variant == "jump":
        for i in np.flatnonzero(g["jump"] != ""):
            ax, L = int(g["jump_axis"][i]), BOX[int(g["jump_axis"][i])]
            d = {"+1.5L": 1.5 * L + 0.0123, "-1.5L": -1.5 * L - 0.0171, "+2.5L": 2.5 * L + 0.0089, "2L-": float(np.nextafter(2.0 * L, 0.0))}[str(g["jump"][i])]
            v[i, ax] = d / DT
            assert v[i, ax] * DT == d
    return v


def case(variant="plain"):
    """the case dict of api.Model.from_case / oracle.Oracle; variant "plain", "jump" or "radiative" (tstat_type 2: only to reach k_boundary_radi)"""
    g = build()
    v = velocities(variant)
    lj = [pc.LJ[0], pc.LJ[1]]
    c = {"box": list(BOX), "dt": DT, "nsteps": 0, "species": list(SPECIES), "names": ["A", "B", "F"], "frozen": list(FROZEN),
         "vdw": [(a, b, 1, RC, lj) for a in range(3) for b in range(a, 3)], "types": g["types"].copy(),
         "x": g["x"][:, 0].copy(), "y": g["x"][:, 1].copy(), "z": g["x"][:, 2].copy(), "vx": v[:, 0].copy(), "vy": v[:, 1].copy(), "vz": v[:, 2].copy(),
         "elec_type": 0, "rReal": 0.0, "alpha": 0.0, "T": 298.0, "tstat_type": 0, "nEq": 0, "freqEq": 1, "use_clist": 1, "cell_list": RC,
         "center_box": 0, "init_forces": 1, "seed": 12345}
    if variant == "radiative":
        c.update(tstat_type=2, radii=list(RADII))
    return c


def exact_axes(variant="plain"):
    """(N, 3) bool: the chain of this coordinate is exact in fp64 (dyadic velocity, or the atom never moves)"""
    g = build()
    ex = np.isin(g["cls"], EXACT_CLASSES)
    if variant == "jump":
        ex &= ~((g["jump"] != "")[:, None] & (np.arange(3)[None, :] == g["jump_axis"][:, None]))
    return ex


def pinned_axes():
    """(N, 3) bool: the coordinate that moves nextafter(2 L, 0) per step in the variant "jump" - one ulp from a multiple of L by design, so its image index is
    whatever (int)(x * (1 / L)) makes of it: counted like any crossing, compared modulo L, and pinned bit for bit to the oracle"""
    g = build()
    return (g["jump"] == "2L-")[:, None] & (np.arange(3)[None, :] == g["jump_axis"][:, None])


def min_distance(pos):
    """smallest minimum-image distance between two atoms of `pos` (N, 3)"""
    pos = np.asarray(pos, dtype=np.float64)
    box = np.array(BOX)
    best = np.inf
    for a in range(0, len(pos), 400):
        d = pos[a:a + 400, None, :] - pos[None, :, :]
        d -= box * np.round(d / box)
        r2 = (d * d).sum(-1)
        r2[np.arange(len(r2)), np.arange(a, a + len(r2))] = np.inf
        best = min(best, float(r2.min()))
    return math.sqrt(best)


# ---- where an atom sits in a launch ------------------------------------------------------------------------------------------------------------------
def sorted_order(pos, dims):
    """ids in the order of the sorted arrays for wrapped positions `pos`: cell index (cx ncy + cy) ncz + cz as cell_coord computes it, ids ascending inside a cell"""
    pos = np.asarray(pos, dtype=np.float64)
    c = [np.mod(np.floor(pos[:, k] * (dims[k] / BOX[k])).astype(np.int64), dims[k]) for k in range(3)]
    cell = (c[0] * dims[1] + c[1]) * dims[2] + c[2]
    return np.lexsort((np.arange(len(pos)), cell)), cell


LAYOUTS = ("workgroup_only_crossing_in_last_wave", "wave_all_64_lanes_cross_one_wall", "workgroup_both_directions_of_an_axis", "pair_both_cross_same_wall",
           "pair_cross_different_walls", "unpaired_last_atom_crosses", "crossing_in_last_partial_workgroup", "pair_kernel_wave_all_64_lanes")


def layout_counts(steps, dims, rebuild_steps):
    """{layout: how often it occurs} over the steps of a reference run (wall_reference.run: each step holds "flags" (N, 6) and "wrapped" (N, 3)).  The order
    of the arrays during step s is the sort of the last rebuild before s (step 0: the initial sort); rebuild_steps: set of step numbers, or None for every step.
    Counted for the one-atom-per-thread kernels (256 atoms a workgroup, 64 a wave) and for the two-atoms-per-thread body (512 and 128)."""
    out = dict.fromkeys(LAYOUTS, 0)
    N = len(steps[0]["wrapped"])
    order, _ = sorted_order(steps[0]["wrapped"], dims)
    for s in range(1, len(steps)):
        fl = steps[s]["flags"][order]                             # (N, 6) in launch order
        anyc = fl.any(1)
        for b in range(0, N, 256):                                # one atom per thread
            blk = fl[b:b + 256]
            waves = [blk[w:w + 64] for w in range(0, len(blk), 64)]
            has = [w_.any() for w_ in waves]
            if len(waves) == 4 and has[3] and not any(has[:3]):
                out["workgroup_only_crossing_in_last_wave"] += 1
            for w_ in waves:
                if len(w_) == 64 and w_.all(0).any():
                    out["wave_all_64_lanes_cross_one_wall"] += 1
            if any(blk[:, 2 * ax].any() and blk[:, 2 * ax + 1].any() for ax in range(3)):
                out["workgroup_both_directions_of_an_axis"] += 1
            if len(blk) < 256 and blk.any():
                out["crossing_in_last_partial_workgroup"] += 1
        for p in range(0, N - 1, 2):                              # two atoms per thread
            a, b = fl[p], fl[p + 1]
            if (a & b).any():
                out["pair_both_cross_same_wall"] += 1
            if a.any() and b.any() and (a != b).any():
                out["pair_cross_different_walls"] += 1
        if N % 2 == 1 and anyc[N - 1]:
            out["unpaired_last_atom_crosses"] += 1
        for w in range(0, N, 128):
            lanes = fl[w:w + 128]
            if len(lanes) == 128 and (lanes[0::2] | lanes[1::2]).all(0).any():
                out["pair_kernel_wave_all_64_lanes"] += 1
        if rebuild_steps is None or s in rebuild_steps:
            order, _ = sorted_order(steps[s]["wrapped"], dims)
    return out


def populated_wall_layers(pos, dims):
    """per axis: (atoms in the first cell layer, atoms in the last one)"""
    pos = np.asarray(pos, dtype=np.float64)
    out = []
    for k in range(3):
        c = np.mod(np.floor(pos[:, k] * (dims[k] / BOX[k])).astype(np.int64), dims[k])
        out.append((int((c == 0).sum()), int((c == dims[k] - 1).sum())))
    return out


def class_counts():
    """{(class, axis, side, species): atoms} of the designed coordinates"""
    g = build()
    out = {}
    for i, ax in zip(*np.nonzero(g["side"] >= 0)):
        key = (str(g["cls"][i, ax]), int(ax), int(g["side"][i, ax]), int(g["types"][i]))
        out[key] = out.get(key, 0) + 1
    return out
