"""What the pair-list builder KEEPS of a cell's staged candidates (k_build_lists, csrc/pair_list.hip.h), restated on top of tests/list_model.py, and
the dilute system of the tile-pruning tests (tests/test_tile_pruning_model.py on the CPU, tests/test_gpu_tile_pruning.py on the GPU).  numpy only,
deterministic.

The builder stages the candidates inside the dilated bounding box of the cell's atoms (list_model.Builder.candidates), filters them atom by atom
(Builder.filter) and then keeps only those that some atom of the cell hit, in tile order: kept candidate n sits in record n + 1 of k_pair_list's
tile, and every hit entry is mapped to its candidate's new record.  `PrunedBuilder` is that renumbering; its `mutation` "drop_first" /
"drop_last" loses one kept candidate per cell (a count that is off by one at either end).
"""
import numpy as np

import list_cases as lc
import list_model as lm

DROPS = ("drop_first", "drop_last")


class PrunedBuilder(lm.Builder):
    """The lists k_pair_list walks: per cell the kept candidates (tile order preserved) and the hits mapped onto them, for one accumulation order of
    the matrix filter (`fused`).  build() adds, per cell: staged (count), keep (mask over the staged), remap (staged number -> record 1 ... T, 0 =
    dropped)."""

    def __init__(self, pos, g, fused, drop=None):
        assert drop is None or drop in DROPS
        super().__init__(pos, g)
        self.fused, self.drop = fused, drop
        self._pruned = None

    def build(self):
        if self._pruned is None:
            out = {}
            for c, rec in super().build().items():
                hits = rec["hits"][self.fused]
                keep = hits.any(0)
                if self.drop and keep.any():
                    k = np.flatnonzero(keep)
                    keep[k[0] if self.drop == "drop_first" else k[-1]] = False
                remap = np.where(keep, np.cumsum(keep), 0)
                kept_hits = hits[:, keep]
                out[c] = dict(atoms=rec["atoms"], cand=rec["cand"][keep], code=rec["code"][keep], n_cand=int(keep.sum()), hits={self.fused: kept_hits},
                              staged=rec["n_cand"], keep=keep, remap=remap, staged_cand=rec["cand"], staged_hits=hits)
            self._pruned = out
        return self._pruned


# ---- the dilute box ------------------------------------------------------------------------------------------------------------------------
DILUTE_SEED = 17
DILUTE_ATOMS = 60
LONE_CELL = (2, 2, 2)


def dilute():
    """5 x 5 x 5 cells of 7.5 A with 60 atoms of one Lennard-Jones species (rMax 7, list radius 7.49): most occupied cells hold one atom, whose partners
    all sit in neighbour cells; the atom in the middle of cell (2, 2, 2) stands still with nobody within 9 A - its cell reaches nobody and keeps a
    list with T = 0.  Everybody else drifts 20-80 % of the shell cases' step (nobody leaves his slack in an interval)."""
    if "dilute" not in lc._CACHE:
        rng = np.random.Generator(np.random.PCG64(DILUTE_SEED))
        g = lm.geometry([5 * lc.CELL] * 3, lc.RC, lc.CELL, lc.SKIN)
        box = np.array(g["box"])
        w = lc.TRAVEL * g["slack"] / (lc.K_SHELL - 1)
        lone = (np.array(LONE_CELL) + 0.5) * np.array(g["csz"])
        X, V = [lone], [np.zeros(3)]
        while len(X) < DILUTE_ATOMS:
            x = rng.uniform(0.0, 1.0, 3) * box
            d = lm.min_image(np.array(X) - x, box)
            r = np.sqrt((d * d).sum(1))
            if r[0] < 9.0 or r.min() < 3.8:
                continue
            v = rng.normal(size=3)
            X.append(x); V.append(v * rng.uniform(0.2, 0.8) * w / lc.DT / np.linalg.norm(v))
        X, V = np.array(X), np.array(V)
        case = {"box": list(g["box"]), "dt": lc.DT, "nsteps": 0, "species": [(lc.MASS, 0.0)], "names": ["A"], "frozen": [0],
                "vdw": [(0, 0, 1, lc.RC, [lc.EPS, lc.SIGMA])], "types": np.zeros(len(X), dtype=np.int32),
                "x": X[:, 0].copy(), "y": X[:, 1].copy(), "z": X[:, 2].copy(), "vx": V[:, 0].copy(), "vy": V[:, 1].copy(), "vz": V[:, 2].copy(),
                "elec_type": 0, "rReal": 0.0, "alpha": 0.0, "T": 0.0, "tstat_type": 0, "nEq": 0, "freqEq": 1, "use_clist": 1, "cell_list": lc.CELL,
                "center_box": 0, "init_forces": 1, "radii": None, "seed": 12345}

        def positions(step):
            """ballistic positions at the end of step `step` (the forces are a few 1e-4 of what would show in 17 steps), wrapped"""
            return np.mod(X + step * lc.DT * V, box)

        lc._CACHE["dilute"] = dict(name="dilute", case=case, geom=g, K=lc.K_SHELL, skin=lc.SKIN, steps=2 * lc.K_SHELL + 1, positions=None, pairs=None,
                                   ballistic=positions, velocity=V, vdw={(0, 0): (lc.EPS, lc.SIGMA, lc.RC)}, engine={}, env={}, unlisted=False, lone=0)
    return lc._CACHE["dilute"]
