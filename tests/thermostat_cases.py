"""The designed atoms of the radiative-thermostat tests (tests/test_thermostat_model.py on the CPU, tests/test_gpu_thermostat_atoms.py on the GPU): numpy only.

post_tstat_atom (csrc/kernels.hip.h) has branches a thermal lattice takes by luck or never: the second and third branch of angled_vector (v_x == 0,
v_x == v_y == 0), its ill-conditioned directions, U <= radThr (no emission), ermc / v0 >= 1 (the emission stops the atom), the mxEng clamp of the
radius, a second species, the wrap of the photon index.  Here they are reached on purpose:

  geometry  the force-free gas of test_gpu_parity.test_radiative_thermostat_fused_into_the_pair_kernel[gas]: 3000 atoms on jittered sites of a 15^3 grid in
            a box of 480, rc = 4, cells of 80 - no pair within the cut-off, forces exactly 0, the lazy re-sort engages.  Two species interleaved by id with
            different masses and different (radA, radB, mxEng).
  RNG       mix64 / rng_draw of csrc/rng.h restated in Python integers (and in numpy uint64 for whole arrays); the 3072 preset unit vectors regenerated
            from the formula of unit_vectors (csrc/sys_init.cpp) with libm's sin / cos.  An atom at rest that absorbs a photon moves exactly along its
            table entry, so the atoms whose absorption draw of step 1 hits a special entry are left at rest.
  SEED      found by search_seed(): the first seed from 12345 on for which every table class below has at least two of the 3000 ids at step 1.
  classes   at rest, absorption draw of step 1 on an entry with
              x0      x == 0, y != 0                      second branch of angled_vector
              z       (0, 0, +-1)                         third branch
              tiny    0 < |x| < 1e-9, y + z not small     first branch, v2 = (-(y + z) / x, 1, 1) of length ~1e10: well-conditioned after all
              cancel  (~1e-13, -+0.7071, +-0.7071)        first branch, y + z cancels: the ill-conditioned directions of the kernel's comment
            (the table holds 62 + 2 + 240 + 8 such entries: 64 with x == 0.0, 248 with 0 < |x| < 1e-9, of which 8 cancel)
            moving    speeds over three decades (1e-3 .. 1), general directions, every 8th with one component exactly 0
            dark      U so negative that U + photon <= radThr: no emission, the radius from a negative energy
            stop      U large and v tiny: ermc / v0 >= 1, the emission is aimed at -v
            clamp     U after the emission above the species' mxEng; below: just under it (between the two species' mxEng for species 1)
            wrap      the ids N - 1, N - 2, ... for which id + step >= N during the steps run: the photon index wraps (at step 1 that is id N - 1 alone, so
                      the count is taken over the steps of a run)
assign() gives every atom its (v, U); count_classes() and the assertions of check_design() are conditions on the INPUTS, evaluated on the reference's
own branch flags (tests/thermostat_reference.py), on the CPU.
"""
import math

import numpy as np

import pair_cases as pc

TAU = pc.TAU
N, L, RC, CELL, GRID = 3000, 480.0, 4.0, 80.0, 15
DT, TEMP = 0.001, 298.0
SPECIES = [(39.9, 0.0), (20.2, 0.0)]                              # (mass in amu, charge)
RADII = [(2.73, 4.731, 0.2), (2.1, 3.9, 0.05)]                    # (radA, radB, mxEng)
M_SCALE = 1.6605402E-27 / (1.60217733E-19 * 1.0E-12 * 1.0E-12 / 1.0E-10 / 1.0E-10)      # csrc/model.h units::m_scale, the same operations in the same order
KB = 1.3806488E-23 / (1.0 * 1.60217733E-19)                      # units::kB
REV_LIGHT, RAD_FRAC, RAD_THR, NUM_PI = 3.33567e-5, 0.9, 1e-4, 3.14159
N_UVECT = 3072
SEED = 12345                                                      # search_seed(); asserted by tests/test_thermostat_model.py
MIN_PER_CLASS = 2
TIE_MARGIN = 1e-6
M64 = (1 << 64) - 1


# ---- csrc/rng.h ------------------------------------------------------------------------------------------------------------------------------
def mix64(z):
    z &= M64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def rng_draw(seed, step, atom_id, draw):
    z = mix64(seed + 0x9E3779B97F4A7C15 * (step + 1))
    z = mix64(z ^ ((0xD1B54A32D192ED03 * (atom_id + 1)) & M64))
    z = mix64(z ^ ((0x8CB92BA72F3D8DD7 * (draw + 1)) & M64))
    return z >> 32


def _mix64_np(z):
    z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(seed, step, ids, draw):
    """rng_draw for an array of ids (uint64 arithmetic wraps as in C); int64 array of 32-bit draws"""
    ids = np.asarray(ids, dtype=np.uint64)
    z0 = np.uint64(mix64(seed + 0x9E3779B97F4A7C15 * (step + 1)))
    with np.errstate(over="ignore"):
        z = _mix64_np(z0 ^ (np.uint64(0xD1B54A32D192ED03) * (ids + np.uint64(1))))
        z = _mix64_np(z ^ np.uint64((0x8CB92BA72F3D8DD7 * (draw + 1)) & M64))
    return (z >> np.uint64(32)).astype(np.int64)


# ---- the preset unit vectors (unit_vectors, csrc/sys_init.cpp) -----------------------------------------------------------------------------------
_UV = None


def unit_table():
    """(3072, 3) fp64: 32 phi x 16 theta, each with its negative, in three axis permutations - libm's sin / cos on the same arguments"""
    global _UV
    if _UV is None:
        n_th, n_phi, twopi = 16, 32, 2.0 * pc.PI
        out = np.empty((N_UVECT, 3))
        k = 0
        for perm in range(3):
            for i in range(n_phi):
                phi = float(i) / n_phi * twopi
                for j in range(n_th):
                    theta = float(j) / n_th * pc.PI
                    st, ct, sp, cp = math.sin(theta), math.cos(theta), math.sin(phi), math.cos(phi)
                    a, b, c = cp * ct, sp * ct, st
                    X, Y, Z = ((a, b, c), (a, c, b), (c, b, a))[perm]
                    out[k] = (X, Y, Z)
                    out[k + 1] = (-X, -Y, -Z)
                    k += 2
        _UV = out
        _UV.setflags(write=False)
    return _UV


TABLE_CLASSES = ("x0", "z", "tiny", "cancel")


def table_classes():
    """{class: boolean mask over the 3072 entries}; the four classes are disjoint"""
    u = unit_table()
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    small = (x != 0.0) & (np.abs(x) < 1e-9)
    cancel = small & (np.abs(y + z) < 1e-9) & (np.abs(y) > 0.5)
    return {"x0": (x == 0.0) & (y != 0.0), "z": (x == 0.0) & (y == 0.0), "tiny": small & ~cancel, "cancel": cancel}


def absorption_class(seed, step=1):
    """class name of the table entry each id's absorption draw of `step` hits ('' for an ordinary entry)"""
    rnd = draws(seed, step, np.arange(N), 1) % N_UVECT
    out = np.full(N, "", dtype="U6")
    for name, mask in table_classes().items():
        out[mask[rnd]] = name
    return out


def search_seed(first=12345, tries=200):
    for seed in range(first, first + tries):
        c = absorption_class(seed)
        if all(int((c == k).sum()) >= MIN_PER_CLASS for k in TABLE_CLASSES):
            return seed
    raise AssertionError("no seed in [%d, %d) gives every table class %d atoms" % (first, first + tries, MIN_PER_CLASS))


# ---- the system ------------------------------------------------------------------------------------------------------------------------------------
def masses():
    """per-species mass in the engine's units (Model.query("species")[:, 1])"""
    return np.array([m * M_SCALE for m, _ in SPECIES])


def t_kin():
    """finish_model: tKin = 0.5 T kB degFree, degFree = 3 N - 1 with a thermostat (csrc/sys_init.cpp)"""
    return 0.5 * TEMP * KB * (3 * N - 1)


def positions():
    rng = np.random.Generator(np.random.PCG64(77))
    site = rng.permutation(GRID ** 3)[:N]
    pos = np.stack([site // (GRID * GRID), (site // GRID) % GRID, site % GRID], axis=1) * (L / GRID) + L / (2 * GRID) + rng.uniform(-10.0, 10.0, size=(N, 3))
    return np.round(np.mod(pos, L), 6)


def assign(photons, seed=SEED):
    """(v (N, 3), U (N,), intended class per atom) - see the module text.  `photons`: the model's photon table for `seed` (Model.query("photons", seed))."""
    photons = np.asarray(photons, dtype=np.float64)
    assert photons.shape == (N,)
    ids = np.arange(N)
    types = ids % 2
    m = masses()[types]
    mx = np.array([r[2] for r in RADII])[types]
    pe = photons[(ids + 1) % N]                                   # the photon of step 1
    rest = absorption_class(seed)
    rng = np.random.Generator(np.random.PCG64(4242))
    d = rng.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    frac = rng.uniform(size=N)
    v, U = np.zeros((N, 3)), np.zeros(N)
    cls = np.where(rest != "", rest, "").astype("U8")
    free = np.flatnonzero(rest == "")
    for j, i in enumerate(free):
        k = j % 8
        if k <= 3:
            cls[i] = "moving"
            v[i] = 10.0 ** (-3.0 + 3.0 * frac[i]) * d[i]
            if k == 3 and (j // 8) % 2 == 0:
                v[i, (j // 16) % 3] = 0.0                          # one component exactly 0
        elif k == 4:
            cls[i] = "dark"
            U[i] = -(pe[i] + (1e-3 if (j // 8) % 2 else 1.0))
            v[i] = 10.0 ** (-2.0 + 2.0 * frac[i]) * d[i]
        elif k == 5:
            cls[i] = "stop"
            U[i] = 0.1 * (1.0 + frac[i])
            v[i] = 1e-5 * d[i]
        else:
            cls[i] = "clamp" if k == 6 else "below"
            U[i] = 10.0 * mx[i] * (1.25 if k == 6 else 0.95) - pe[i]
            v[i] = 0.5 * (1.0 + frac[i]) * d[i]
    return v, U, cls


def gas_case(photons=None, seed=SEED, n_eq=0, freq_eq=1):
    """the case dict (aztotmd_amd.api.Model.from_case / oracle.Oracle); with `photons` the designed velocities, else a gas at rest.  The designed U goes in
    through Engine.set_state / Oracle.set_thermo."""
    pos = positions()
    v = assign(photons, seed)[0] if photons is not None else np.zeros((N, 3))
    lj = [pc.LJ[0], pc.LJ[1]]
    return {"box": [L, L, L], "dt": DT, "nsteps": 0, "species": list(SPECIES), "names": ["A", "B"],
            "vdw": [(0, 0, 1, RC, lj), (0, 1, 1, RC, lj), (1, 1, 1, RC, lj)], "types": (np.arange(N) % 2).astype(np.int32),
            "x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": v[:, 0].copy(), "vy": v[:, 1].copy(), "vz": v[:, 2].copy(),
            "elec_type": 0, "rReal": 0.0, "alpha": 0.0, "T": TEMP, "tstat_type": 2, "nEq": n_eq, "freqEq": freq_eq, "use_clist": 1, "cell_list": CELL,
            "center_box": 0, "init_forces": 1, "radii": list(RADII), "seed": seed}


def min_image_distance(pos):
    """smallest minimum-image distance between two of the atoms"""
    best = np.inf
    for a in range(0, N, 500):
        d = pos[a:a + 500, None, :] - pos[None, :, :]
        d -= L * np.round(d / L)
        r2 = (d * d).sum(-1)
        r2[np.arange(len(r2)), np.arange(a, a + len(r2))] = np.inf
        best = min(best, float(r2.min()))
    return math.sqrt(best)


# ---- conditions on the inputs ----------------------------------------------------------------------------------------------------------------------
def count_classes(cls, first, wraps):
    """{class: atoms} from the reference's own flags of step 1 (`first`: a step result of thermostat_reference) and the intended classes; `wraps`: number
    of ids whose photon index wraps during the run"""
    emit, stop, clamp = first["emit"], first["stop"], first["clamp"]
    mx = np.array([r[2] for r in RADII])[np.arange(N) % 2]
    U = first["U"].astype(np.float64)
    out = {k: int(((cls == k) & emit & ~stop).sum()) for k in TABLE_CLASSES}
    moving = (cls == "moving") & emit & ~stop
    out["moving"] = int(moving.sum())
    out["moving_component_0"] = int((moving & (first["v_in"] == 0).any(1)).sum())
    out["dark"] = int((~emit).sum())
    out["dark_negative_radius_energy"] = int((~emit & (U < 0)).sum())
    out["stop"] = int((emit & stop).sum())
    for s in (0, 1):
        out["clamp_species_%d" % s] = int((clamp & (np.arange(N) % 2 == s)).sum())
        out["below_species_%d" % s] = int((~clamp & emit & (U > 0.9 * mx) & (np.arange(N) % 2 == s)).sum())
    out["between_the_species_mxEng"] = int((emit & (np.arange(N) % 2 == 1) & (U > RADII[1][2]) & (U < RADII[0][2])).sum())
    out["wrap"] = int(wraps)
    return out


def check_design(cls, first, wraps):
    counts = count_classes(cls, first, wraps)
    short = {k: v for k, v in counts.items() if v < MIN_PER_CLASS}
    assert not short, ("classes with fewer than %d atoms" % MIN_PER_CLASS, short, counts)
    v0 = np.linalg.norm(first["v_in"], axis=1)
    sp = v0[cls == "moving"]
    assert sp.min() < 2e-3 and sp.max() > 0.5, (sp.min(), sp.max())             # three decades
    return counts


def check_no_ties(step_result, tag=""):
    """|U_mid - radThr| and |ermc / v0 - 1| at least TIE_MARGIN relative, so that fp64 and the reference take the same branches"""
    a, b = float(step_result["tie_thr"].min()), float(step_result["tie_stop"].min())
    assert a >= TIE_MARGIN and b >= TIE_MARGIN, (tag, a, b)
    return a, b
