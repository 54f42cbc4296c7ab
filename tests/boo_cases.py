"""The configurations on which tests/test_gpu_boo.py holds the device's q_lm to the 60-digit model, as data: the GPU tests build engines from them, and
`python tests/boo_cases.py` measures on the CPU the worst error of the fp64 restatement of the route (boo_model.route_qlm) over the very same bonds.  That
figure is boo_model.ROUTE_WORST; four times it is the bound of the device.

A case: name, the engine's case dict, box, R, central_mask, ligand_mask, orders, and `atoms`: None (every atom is compared with the model) or the
indices of a sample of atoms (large systems: the neighbour counts of all atoms are then compared through the coordination-number sampler).

Lanes per atom of k_boo_qlm / k_boo_average (Samplers::boo_setup: the fewest 2^k <= 64 with N * 2^k >= 65536): N <= 2047: 64, 2048 - 4095: 32,
4096 - 8191: 16, 8192 - 16383: 8, 16384 - 32767: 4, 32768 - 65535: 2, from 65536: 1."""
import os
import sys

import numpy as np

if __name__ == "__main__":      # run as a script: the package is one level up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_gpu_cn import GEOMETRIES, random_case

import boo_model as bm

LANE_COUNTS = {2047: 64, 2048: 32, 4096: 16, 8192: 8, 16384: 4, 32768: 2, 65536: 1}


def radius_for(n_atoms, box, neighbours=5.0):
    """the radius inside which a random configuration has about `neighbours` partners, rounded to three decimals"""
    rho = n_atoms / float(np.prod(box))
    return round(float((neighbours / (rho * 4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)), 3)


def _case(name, case, box, R, cm, lm, orders, atoms=None):
    return {"name": name, "case": case, "box": tuple(box), "R": R, "central": cm, "ligand": lm, "orders": tuple(orders), "atoms": atoms}


def geometry_cases():
    """the six geometries of test_gpu_cn.py at 3000 atoms, R for a handful of neighbours; masks equal, overlapping and disjoint"""
    masks = [(3, 3), (1, 6), (1, 3), (5, 3), (2, 1), (3, 3)]
    out = []
    for g, (nspec, box, _, faces) in enumerate(GEOMETRIES):
        out.append(_case("geometry%d" % g, random_case(nspec, 3000, box, seed=900 + g, faces=faces), box, radius_for(3000, box), masks[g][0], masks[g][1], (4, 6)))
    return out


def sparse_cases():
    """the radii of test_gpu_cn.py (one cell per axis, 1 / 2 / 3 cells, R > L / 2, R > L_x) on few atoms: every partner once, through its nearest image;
    an atom has a third of the system as neighbours, so a sample of the atoms goes through the 60-digit model"""
    out = []
    for (g, n), orders in zip([(2, 200), (3, 300), (4, 500), (5, 250)], [(1, 2, 12), (12,), (4, 6), (4, 6)]):
        nspec, box, R, faces = GEOMETRIES[g]
        atoms = np.unique(np.concatenate([np.arange(0, n, max(n // 16, 1)), [n - 1]]))
        out.append(_case("sparse%d" % g, random_case(nspec, n, box, seed=950 + g, faces=faces), box, R, 3, 3, orders, atoms))
    return out


def count_cases():
    out = []
    for n in (1, 2, 63, 64, 65, 257):
        box = (10.0, 11.0, 12.0) if n < 100 else (20.0, 21.0, 22.0)
        out.append(_case("atoms%d" % n, random_case(2, n, box, seed=n), box, 3.0 if n < 100 else 3.5, 3, 3, (4, 6)))
    return out


def lane_cases():
    out = []
    for n in LANE_COUNTS:
        edge = round(float((n / 0.05) ** (1.0 / 3.0)), 1)
        box = (edge, edge + 1.0, edge + 2.0)
        atoms = None if n <= 2048 else np.unique(np.concatenate([np.arange(0, n, n // 48), [n - 1]]))
        out.append(_case("lanes%d" % LANE_COUNTS[n], random_case(2, n, box, seed=1000 + n % 997), box, 3.0, 1, 3, (4, 6), atoms))
    return out


def mask_cases():
    box = (22.0, 23.0, 24.0)
    return [_case("empty_species", random_case(3, 600, box, seed=77, used=2), box, 3.5, 5, 6, (1, 2, 12)),
            _case("order12_alone", random_case(2, 600, box, seed=78), box, 3.5, 3, 3, (12,))]


def all_cases():
    return geometry_cases() + sparse_cases() + count_cases() + lane_cases() + mask_cases()


def positions_of(case):
    return np.stack([case["x"], case["y"], case["z"]], axis=1), np.asarray(case["types"])


def measure():
    """the worst |route_qlm - exact_qlm| per component, case by case (the positions of a case dict are inside the box: the engine hands them out unchanged)"""
    worst = 0.0
    for c in all_cases():
        pos, types = positions_of(c["case"])
        B = bm.bonds(pos, types, c["box"], c["R"], c["central"], c["ligand"], atoms=c["atoms"])
        e = bm.route_error(B, c["orders"])
        live = B.n[B.n >= 0]
        print("%-16s atoms %6d bonds %7d mean neighbours %6.2f orders %-12s route error %.3e" % (c["name"], len(pos), len(B.r2), live.mean() if live.size else 0.0,
                                                                                                 c["orders"], e))
        worst = max(worst, e)
    print("worst", worst)
    return worst


if __name__ == "__main__":
    measure()
