"""The candidates k_build_lists keeps (only those some atom of the cell reaches, renumbered in tile order) through the forces of k_pair_list, with the
cases, the runner and the per-atom bound of tests/test_gpu_pair_lists.py: every step of two intervals against the longdouble enumeration,
|F_gpu - F_ref| <= TAU sum_j S_F r per atom (TAU = 1e-13), atoms without a partner feel exactly nothing, plain steps run pair_list and never
pair_tile, no cell is left without a list.

  dilute        5 x 5 x 5 cells, 60 atoms (tests/tile_cases.py): cells of one atom whose partners all sit in neighbour cells - the atom's own record is
                dropped from its tile -, and one cell whose atom reaches nobody: a list with T = 0, forces exactly zero
  skin_cells    the liquid on 5 x 6 x 7 cells of rc + skin: tiles of up to 256 records, the kernel that gathers four groups up front
  crowded       ~23 atoms per cell.  (Chosen for "more than 256 kept candidates"; it keeps 152 at the most - test_tile_pruning_model.py - so it runs the
                four-group kernel too.  Kept as a case; the next one covers what it was meant to.)
  wide_stencil  the dense liquid with the 7 x 7 x 7 stencil, ONE wave per cell: ~460 kept candidates per cell, up to 635 - the kernel that gathers five
                groups and its dense-system loop
  populations   cells of 1 ... 65 atoms with one and four waves per cell (table-driven kernel: list entries are record numbers)

Each case runs (1) with lists, (2) with the cells rebuilt on every step (the staging kernel: no lists) - both held to the same enumeration -, and
(3) twice more with lists in two fresh engines, whose states must agree bit for bit.  tests/test_tile_pruning_model.py (CPU) holds the restated
builder and these systems to what is claimed here first.
"""
import numpy as np
import pytest

import list_cases as lc
import test_gpu_pair_lists as base
import tile_cases as tc

pytestmark = pytest.mark.gpu


def wide_stencil_one_wave():
    c = dict(lc.liquid("wide_stencil"))
    c.update(name="wide_stencil_w1", engine=dict(split=1))
    return c


CASES = {"dilute": tc.dilute, "skin_cells": lambda: lc.liquid("skin_cells"), "crowded": lambda: lc.liquid("crowded"), "wide_stencil_w1": wide_stencil_one_wave,
         "populations_w1": lambda: lc.populations(1), "populations_w4": lambda: lc.populations(4)}


def final_state(c):
    e = base.make_engine(c)
    for _ in range(c["steps"]):
        e.step(1)
    return e.state(), e.stats()


@pytest.mark.parametrize("name", list(CASES))
def test_forces_over_the_kept_candidates(name):
    c = CASES[name]()
    worst = base.run_case(c)
    assert worst <= 1.0
    if name == "dilute":
        # the lone atom's cell reaches nobody: its list has T = 0 and its force is written as zero (run_case holds every atom without a partner to
        # exactly zero on every step; here once more by name, with the velocity it started with: nothing ever pushed it)
        s, _ = final_state(c)
        k = c["lone"]
        assert s["fx"][k] == 0.0 and s["fy"][k] == 0.0 and s["fz"][k] == 0.0
        assert s["vx"][k] == 0.0 and s["vy"][k] == 0.0 and s["vz"][k] == 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_same_system_with_the_cells_rebuilt_every_step(name):
    """served by the staging kernel, to the same enumeration and tolerance: a failure above belongs to the lists, not to the case"""
    assert base.run_case(CASES[name](), every_step=True) <= 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_two_engines_agree_bit_for_bit(name):
    c = CASES[name]()
    (a, sa), (b, sb) = final_state(c), final_state(c)
    for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz"):
        assert np.array_equal(a[k], b[k]), (name, k, int((a[k] != b[k]).sum()))
    for k in ("engTot", "engVdw", "engKin"):
        if k in sa:
            assert sa[k] == sb[k], (name, k, sa[k], sb[k])
    assert sa["cells_without_list"] == sb["cells_without_list"]
