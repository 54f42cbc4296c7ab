"""Systems for the tests of the pair-list builder (tests/test_list_model.py on the CPU, tests/test_gpu_pair_lists.py on the GPU).  numpy only,
deterministic.

The builder is tested through forces: a pair the rebuild lost from the shell between rMax and the list radius rMax + 2 slack shows as a whole
missing pair term once the pair has come inside rMax.  So the cases put chosen pairs INTO that shell at a rebuild and let them approach:

shell_pairs   isolated two-atom groups of one Lennard-Jones species (the one-species kernel, list entries are byte offsets).  Each atom has exactly
              one partner inside the list radius.  27 cell offsets (same cell + the 26 neighbours) x 3 random directions, start depths 10 %, 50 %
              and 92 % of the shell, each in two groups: group g sits at its depth at rebuild g (step 1 + g K) and is inside rMax before rebuild
              g + 1.  The atoms of a pair fly head-on at each other, 0.95 slack per interval each: no displacement violation.  Sites with lattice
              index 0 straddle the periodic walls, so every image code occurs on every axis.  A pair deeper than ~95 % of the shell cannot reach
              rMax without a violation (each atom may move slack at the most): such pairs are harmless by construction and out of reach here.
populations   the same pairs (neighbour offsets only) with filler atoms of two species WITHOUT any potential - one frozen, one moving - setting
              the population of the tested atom's cell to 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65 and that of the partner's cell; ids
              chosen so that the tested atom is first / last of a group of 16 / last of its cell and the partner first or last of its cell's run.
              (Three species: the table-driven kernel, list entries are record numbers.)
liquids       jittered lattices with Maxwell velocities at 300 K: cells of about rc + skin on an anisotropic 5 x 6 x 7 grid, cells of rc / 2.2
              (7 x 7 x 7 stencil), crowded cells of ~23 atoms; and the first of them with one axis at three cells, where the engine keeps no lists
              at all (fewer than five cells on an axis leave the stencil no room to widen): the staging kernel serves every step.

Every builder returns dict(name, case, geom, K, skin, steps, engine (keyword arguments), env, positions(step), pairs, ...).
"""
import numpy as np

import list_model as lm
from aztotmd_amd import inputs

K_SHELL = 8                    # sort_every of the shell cases: 7 plain steps per interval
TRAVEL = 0.95                  # of slack, per atom and interval
DEPTHS = (0.1, 0.5, 0.92)      # start depth in the shell, fraction of 2 slack
RC = 7.0
CELL = 7.5
SKIN = 0.4
EPS, SIGMA, MASS = 0.001, 3.3952, 39.9
DT = 0.001
POPULATIONS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)
SHELL_SEED, POP_SEED = 3, 5    # pinned: the coverage test (test_list_model.py) names what they must give


def _direction(rng, o):
    """unit vector from atom i to its partner: along the cell offset o on the axes where o != 0, small enough elsewhere for both to share the layer"""
    while True:
        if o == (0, 0, 0):
            u = rng.uniform(0.4, 0.7, 3) * rng.choice([-1.0, 1.0], 3)
        else:
            u = np.array([ok * rng.uniform(0.35, 1.0) if ok else rng.uniform(-0.6, 0.6) for ok in o])
        u /= np.linalg.norm(u)
        if all((abs(uk) >= 0.3) if ok else (abs(uk) <= 0.72) for uk, ok in zip(u, o)):
            return u


def _midpoint(rng, g, site, o):
    """where the pair's midpoint sits: on the cell boundary 3 m csz on the axes the pair crosses (m = 0: the periodic wall), in the middle of cell 3 m elsewhere"""
    return np.array([(3 * m + (0.0 if ok else 0.5)) * c + rng.uniform(-0.2, 0.2) for m, c, ok in zip(site, g["csz"], o)])


def _shell_system(name, g, specs, rng, fillers=None, travel=TRAVEL):
    """specs: [(site (3,), offset, depth, group)].  Atoms i, j of pair n fly at each other along u; d(s) = rMax + depth 2 slack - 2 w (s - s_group)."""
    slack = g["slack"]
    w = travel * slack / (K_SHELL - 1)
    X, V, T = [], [], []
    pairs = dict(i=[], j=[], group=[], depth=[], offset=[], site=[], d0=[], u=[])
    cells = []
    for site, o, depth, group in specs:
        u = _direction(rng, o)
        mid = _midpoint(rng, g, site, o)
        d0 = g["r_max"] + depth * 2.0 * slack + 2.0 * w * (1 + group * K_SHELL)      # separation at step 0
        xi, xj = mid - 0.5 * d0 * u, mid + 0.5 * d0 * u
        block = [(xi, u * w / DT, 0), (xj, -u * w / DT, 0)]
        if fillers is not None:
            block = fillers(rng, g, site, o, block)
        k0 = len(X)
        for x, v, t in block:
            X.append(x); V.append(v); T.append(t)
        ids = [k0 + k for k, b in enumerate(block) if b[2] == 0]
        pairs["i"].append(ids[0]); pairs["j"].append(ids[1])
        for k, v in (("group", group), ("depth", depth), ("offset", o), ("site", site), ("d0", d0), ("u", u)):
            pairs[k].append(v)
    X, V, T = np.array(X), np.array(V), np.array(T, dtype=np.int32)
    pairs = {k: np.array(v) for k, v in pairs.items()}
    box = np.array(g["box"])
    nsp = int(T.max()) + 1
    x0 = np.mod(X, box)
    case = {"box": list(g["box"]), "dt": DT, "nsteps": 0, "species": [(MASS, 0.0)] * nsp, "names": ["A", "F", "M"][:nsp],
            "frozen": [0, 1, 0][:nsp], "vdw": [(0, 0, 1, RC, [EPS, SIGMA])], "types": T,
            "x": x0[:, 0].copy(), "y": x0[:, 1].copy(), "z": x0[:, 2].copy(), "vx": V[:, 0].copy(), "vy": V[:, 1].copy(), "vz": V[:, 2].copy(),
            "elec_type": 0, "rReal": 0.0, "alpha": 0.0, "T": 0.0, "tstat_type": 0, "nEq": 0, "freqEq": 1, "use_clist": 1, "cell_list": CELL,
            "center_box": 0, "init_forces": 1, "radii": None, "seed": 12345}

    def positions(step):
        """ballistic positions at the end of step `step` (0: the input), wrapped"""
        return np.mod(X + step * DT * V, box)

    return dict(name=name, case=case, geom=g, K=K_SHELL, skin=SKIN, steps=2 * K_SHELL + 1, positions=positions, pairs=pairs, w=w, velocity=V,
                vdw={(0, 0): (EPS, SIGMA, RC)}, engine={}, env={}, unlisted=False)


def _sites(shape, rng):
    s = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    return s[rng.permutation(len(s))]


_CACHE = {}


def shell_pairs():
    if "shell" not in _CACHE:
        rng = np.random.Generator(np.random.PCG64(SHELL_SEED))
        shape = (6, 6, 5)
        g = lm.geometry([3 * n * CELL for n in shape], RC, CELL, SKIN)
        sites = _sites(shape, rng)
        specs, k = [], 0
        for group in (0, 1):
            for o in [(0, 0, 0)] + lm.OFFSETS26:
                for depth in DEPTHS:
                    specs.append((tuple(sites[k]), o, depth, group))
                    k += 1
        _CACHE["shell"] = _shell_system("shell_pairs", g, specs, rng)
    return _CACHE["shell"]


def edge_pairs():
    """CPU only (test_list_model.py, sharpness of the bounding box): pairs that start 3e-7 A inside the list radius, alone in their cells (the box of the
    cell's atoms is a point), and travel 0.9999999 slack each - they end 2.5e-7 A inside rMax.  No room for the engine's own rounding: not run on the GPU."""
    if "edge" not in _CACHE:
        rng = np.random.Generator(np.random.PCG64(11))
        shape = (4, 4, 4)
        g = lm.geometry([3 * n * CELL for n in shape], RC, CELL, SKIN)
        sites = _sites(shape, rng)
        depth = 1.0 - 3e-7 / (2.0 * g["slack"])
        specs = [(tuple(sites[k]), o, depth, k % 2) for k, o in enumerate([(0, 0, 0)] + lm.OFFSETS26 + lm.OFFSETS26)]
        _CACHE["edge"] = _shell_system("edge_pairs", g, specs, rng, travel=0.9999999)
    return _CACHE["edge"]


def populations(waves=1):
    """waves: 1 or 4 waves per cell (Engine(split=...)); with four a cell keeps its list up to 256 atoms, so only waves = 1 leaves the 65-atom cells without one"""
    if "pop" not in _CACHE:
        rng = np.random.Generator(np.random.PCG64(POP_SEED))
        shape = (4, 4, 3)
        g = lm.geometry([3 * n * CELL for n in shape], RC, CELL, SKIN)
        sites = _sites(shape, rng)
        specs, plan = [], {}
        for n, (p, var) in enumerate((p, var) for p in POPULATIONS for var in range(3)):
            site = tuple(sites[n])
            q = (1, 16 * ((p + 17) // 16) - p, min(64, 128 - p) if p >= 63 else 33)[var]
            plan[site] = dict(p=p, q=q, first=(0, min(15, p - 1), p - 1)[var], partner_last=var != 1, species=1 + n % 2)
            specs.append((site, lm.OFFSETS26[n % 26], DEPTHS[n % 3], n % 2))

        def fillers(rng, g, site, o, block):
            pl = plan[site]
            csz = np.array(g["csz"])
            w = TRAVEL * g["slack"] / (K_SHELL - 1)

            def fill(n, cell):
                out = []
                for _ in range(n):
                    x = (cell + rng.uniform(0.6 / csz, 1.0 - 0.6 / csz)) * csz
                    v = np.zeros(3)
                    if pl["species"] == 2:                      # the moving filler: at most 0.9 of the tested atoms' travel, so nobody leaves slack or cell
                        v = rng.normal(size=3)
                        v *= rng.uniform(0.2, 0.9) * w / DT / np.linalg.norm(v)
                    out.append((x, v, pl["species"]))
                return out
            base = np.array([3 * m for m in site])
            ca = base + np.array([-1 if ok > 0 else 0 for ok in o])        # cell of atom i (below the boundary when the offset points up)
            cb = ca + np.array(o)
            fa, fb = fill(pl["p"] - 1, ca), fill(pl["q"] - 1, cb)
            a = fa[:pl["first"]] + [block[0]] + fa[pl["first"]:]
            b = fb + [block[1]] if pl["partner_last"] else [block[1]] + fb
            return a + b
        c = _shell_system("populations", g, specs, rng, fillers)
        c["plan"] = plan
        c["env"] = {"AZTOT_ITER_CAP": "160"}                  # the capacities come from the MEAN density, which says nothing about these few crowded cells
        _CACHE["pop"] = c
    c = dict(_CACHE["pop"])
    c["name"] = "populations_w%d" % waves
    c["engine"] = dict(split=waves)
    c["unlisted"] = waves == 1
    c["waves"] = waves
    return c


LIQUIDS = ("skin_cells", "wide_stencil", "crowded", "three_cells")


def liquid(kind):
    if kind not in _CACHE:
        if kind in ("skin_cells", "three_cells"):
            case = inputs.lj_case((7, 8, 9) if kind == "skin_cells" else (4, 8, 9), a=5.4, seed=61, rc=6.5, cell_list=6.9, vel_T=300.0)
        elif kind == "wide_stencil":
            # (the cut-off sits on the lattice's twelfth shell, a sqrt(6): the jitter and the motion carry pairs across it all the time)
            case = inputs.lj_case((10, 10, 10), a=2.5, jitter=0.05, seed=62, rc=6.12, cell_list=2.75, vel_T=300.0)
            case["vdw"] = [(0, 0, 1, 6.12, [0.002, 1.9])]
        else:
            case = inputs.lj_case((9, 9, 9), a=6.0, seed=63, rc=6.0, cell_list=10.5, vel_T=300.0)        # (the cut-off on the second shell, a)
        _, _, _, rc, (eps, sigma) = case["vdw"][0]
        g = lm.geometry(case["box"], rc, case["cell_list"], 0.0)
        _CACHE[kind] = dict(name=kind, case=case, geom=g, K=8, skin=0.0, steps=17, positions=None, pairs=None, vdw={(0, 0): (eps, sigma, rc)},
                            engine={}, env={}, unlisted=False)
    return _CACHE[kind]


def all_cases():
    return [shell_pairs(), populations(1), populations(4)] + [liquid(k) for k in LIQUIDS]
