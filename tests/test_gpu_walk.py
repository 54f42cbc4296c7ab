"""The neighbour walk the coordination-number, bond-angle and bond-order samplers share (grid_walk, grid.hip.h): one engine, one configuration, one
radius, all-species masks, three hit rules.

  cn 'species'   R * R >= r2, the atom itself counted (out_cn's rule)
  adf, boo       0 < r2 < R * R, j != i

With no two atoms in one place and no pair exactly at the radius the three differ by the self count alone, so adf_neighbours == boo's n == the row sum
of cn_per_atom('species') - 1 for every atom.  The box gives each private grid (cell edge >= R = 5: floor(L / R) cells per axis) 2 cells on x, 3 on y
and 4 on z: an axis whose two cells are each other's only neighbour beside axes with the full three-cell stencil.  611 atoms take 64 lanes each.

test_configuration_is_generic needs no GPU: it holds the chosen configuration to what the GPU test assumes, with the Python models."""
import numpy as np
import pytest

from aztotmd_amd import api

import boo_model as bm
from test_gpu_cn import host_cn, positions, random_case

BOX = (12.0, 17.0, 23.0)
R = 5.0
N_ATOMS = 611
N_SPEC = 2
ALL = (1 << N_SPEC) - 1
CN_COLS = [(a, b, R) for a in range(N_SPEC) for b in range(N_SPEC)]
ADF_MAX_NEIGHBOURS = 256        # AZTOT_ADF_MAX_NEIGHBOURS of include/aztot.h


def the_case():
    return random_case(N_SPEC, N_ATOMS, BOX, seed=20)


def model_counts(pos, types):
    """(neighbours by the rule of adf and boo, row sums of the species coordination numbers) of the Python models"""
    n = bm.bonds(pos, types, BOX, R, ALL, ALL).n
    cn = np.maximum(host_cn(pos, types, BOX, CN_COLS, "species")[0], 0).sum(axis=1)
    return n, cn


def test_configuration_is_generic():
    c = the_case()
    n, cn = model_counts(np.stack([c["x"], c["y"], c["z"]], axis=1), c["types"])
    assert np.array_equal(cn - 1, n)                    # no coincident atoms, no pair exactly at the radius: only the self count separates the rules
    assert n.min() >= 1 and n.max() <= ADF_MAX_NEIGHBOURS
    assert [int(L // (R * (1.0 + 1e-9))) for L in BOX] == [2, 3, 4]


@pytest.mark.gpu
def test_three_hit_rules_on_one_walk():
    eng = api.Engine(api.Model.from_case(the_case()))
    pos, types = positions(eng)
    n_model, cn_model = model_counts(pos, types)
    assert np.array_equal(cn_model - 1, n_model)        # what the engine holds is the configuration checked above
    print("neighbours per atom: min", int(n_model.min()), "max", int(n_model.max()))

    eng.cn_setup("species", CN_COLS)
    eng.cn_sample("species")
    cn = eng.cn_per_atom("species")
    assert cn.shape == (N_ATOMS, len(CN_COLS)) and ((cn >= 0) == (np.asarray(CN_COLS)[:, 0][None, :] == types[:, None])).all()
    cn_sum = np.maximum(cn, 0).sum(axis=1)

    eng.adf_setup(36, [(c, a, b, R, R) for c in range(N_SPEC) for a in range(N_SPEC) for b in range(a, N_SPEC)])
    eng.adf_sample()
    adf_n = eng.adf_neighbours()

    eng.boo_setup(R, [4], 10, ALL, ALL)
    eng.boo_sample()
    boo_n = eng.boo_per_atom()[0]

    print("mismatches adf / boo", int((adf_n != boo_n).sum()), "cn - 1 / boo", int((cn_sum - 1 != boo_n).sum()), "boo / model", int((boo_n != n_model).sum()))
    assert adf_n.shape == boo_n.shape == (N_ATOMS,)
    assert np.array_equal(adf_n, boo_n)
    assert np.array_equal(cn_sum - 1, adf_n) and np.array_equal(cn_sum - 1, boo_n)
    assert np.array_equal(boo_n, n_model)
