"""The four reciprocal-space Ewald kernels (csrc/ewald.hip.h: k_ewald_sfac, k_ewald_reduce, k_ewald_energy, k_ewald_force) against the
high-precision reference of tests/ewald_reference.py, atom by atom: |F_gpu,i - F_i| <= TAU S_F,i and |engCoulRec - E| <= TAU S_E with
TAU = pair_cases.TAU and the condition scales stated there.  The 50-digit values and the coordinates they belong to are committed
(tests/golden/ewald_reciprocal.npz); the 70 000-atom system and the (48, 48, 48) harmonics are evaluated at test time in numpy.longdouble.
This file needs numpy only.

Isolated systems: charged species without any VdW entry, no two atoms within rReal - the pair kernels add exactly nothing (engCoul == engVdW
== 0.0), so state()["f*"] is the reciprocal force alone.  They cover what 500 atoms never reach:
  atoms    1, 2, 63, 64, 65, 500 and 70 000 = 1094 tiles on 1024 blocks: blocks 0..69 of k_ewald_sfac run a second round (`mine[...] +=`), the
           last tile is partial (48 atoms), k_ewald_reduce's strided loop runs 64 passes
  k shapes (1,1,4), (4,1,1), (1,5,1): one-entry harmonic tables, the l == m == 0 branch alone; (4,7,9) in an anisotropic box; (19,19,19): more
           than 64 KiB of LDS; (48,48,48) = kEwaldKMax: 144 harmonics, 156 KiB of LDS in k_ewald_force, 264 371 k-vectors
  a neutral species interleaved with the charged ones (its atoms carry exactly no force), the charged species not first in the table, atoms at
  coordinate exactly 0 and at the last double below L of every axis.
Dense system: the 500-ion case of test_gpu_parity, per-atom TOTAL force against reciprocal + real-space + Lennard-Jones terms, all in mpmath.
Known answer: the Madelung constant of rock salt through api.Engine.
Every case prints its worst err / S_F,i and err / S_E before it asserts.
"""
import time

import numpy as np
import pytest

import ewald_reference as er
import pair_cases as pc
from aztotmd_amd import api

pytestmark = pytest.mark.gpu
EWALD_KERNELS = {"ewald_sfac", "ewald_energy", "ewald_force"}


def evaluate(case, variant=2):
    """one force evaluation of `case`: (forces (N, 3), stats, kernel timers of that evaluation)"""
    e = api.Engine(api.Model.from_case(case), pair_variant=variant, profile=1)
    e.reset_kernel_times()
    e.forces()
    kt = e.kernel_times()
    st, stats = e.state(), e.stats()
    e.close()
    return np.stack([st["fx"], st["fy"], st["fz"]], 1), stats, kt


def hold(name, tag, F, stats, kt, ref):
    """the checks every isolated system goes through; returns the two worst ratios"""
    for k in EWALD_KERNELS:
        assert k in kt and kt[k]["calls"] == 1, (name, tag, k, {a: b["calls"] for a, b in kt.items()})
    assert stats["engCoul"] == 0.0 and stats["engVdW"] == 0.0, (name, tag, stats["engCoul"], stats["engVdW"])
    assert np.isfinite(F).all()
    rF, rE = er.worst_ratios(F, stats["engCoulRec"], ref)
    print("%s [%s]: worst err / S_F,i = %.3e   err / S_E = %.3e   (engCoulRec %.15e)" % (name, tag, rF, rE, stats["engCoulRec"]))
    assert rF <= pc.TAU, (name, tag, rF)
    assert rE <= pc.TAU, (name, tag, rE)
    return rF, rE


@pytest.mark.parametrize("name", er.STORED)
def test_isolated_systems_against_high_precision(name):
    """atom counts around the 64-atom tile and the k shapes up to (19, 19, 19): both pair variants, every atom within TAU S_F,i of the 50-digit
    reference, engCoulRec within TAU S_E"""
    case, ref = er.fixture_case(name)
    N = len(case["types"])
    for variant in (1, 2):
        F, stats, kt = evaluate(case, variant)
        hold(name, "pair_variant %d" % variant, F, stats, kt, ref)
        assert (F[er.charges(case) == 0.0] == 0.0).all(), (name, variant)
        if N == 1:                                              # a lone ion: a reciprocal energy, and a force of zero within the tolerance
            assert stats["engCoulRec"] > 0.0 and float(np.abs(ref["F"]).max()) <= 1e-30 * float(ref["SF"][0])
    assert abs(stats["engCoulConst"]) > 0.0


def test_70000_atoms_second_round_and_partial_tile():
    """More atoms than 1024 blocks x 64: the `it > 0` rounds of k_ewald_sfac, a partial last tile, 64 passes of k_ewald_reduce's loop.
    kernel_times() names the launch, not its grid: that the launch had 1024 blocks and a second round follows from N (asserted here) and
    Engine::upload_ewald's nBlocksA = min(1024, ceil(capacity / 64))."""
    er.require_longdouble()
    case = er.isolated_case("n70000")
    N = len(case["types"])
    assert N > 65536 and -(-N // 64) == 1094 and N % 64 == 48
    assert er.min_image_distance(case) > case["rReal"]
    t = time.time()
    ref = er.reciprocal(case, "ld")
    print("n70000: longdouble reference of %d k-vectors in %.1f s" % (len(ref["lmn"]), time.time() - t))
    assert len(ref["lmn"]) == 137
    for variant in (1, 2):
        F, stats, kt = evaluate(case, variant)
        hold("n70000", "pair_variant %d" % variant, F, stats, kt, ref)
        assert (F[er.charges(case) == 0.0] == 0.0).all()


def test_largest_accepted_k_48_48_48():
    """kEwaldKMax harmonics per axis: 156 KiB of dynamic LDS in k_ewald_force, 144 KiB in k_ewald_sfac, 264 371 k-vectors; one evaluation"""
    er.require_longdouble()
    case = er.isolated_case("k48")
    t = time.time()
    ref = er.reciprocal(case, "ld")
    print("k48: longdouble reference of %d k-vectors in %.1f s" % (len(ref["lmn"]), time.time() - t))
    assert len(ref["lmn"]) == 264371 and np.abs(ref["lmn"]).max() == 47
    F, stats, kt = evaluate(case, 2)
    hold("k48", "pair_variant 2", F, stats, kt, ref)


@pytest.mark.parametrize("name", ["n65", "n500", "k479"])
def test_two_engines_are_bitwise_identical(name):
    """The partial sums of S(k) are taken in a fixed order (tile, block row, reduce group: the tree in the header of csrc/ewald.hip.h), so two
    engines on the same input agree bit for bit, in every force and in engCoulRec."""
    case, _ = er.fixture_case(name)
    (Fa, sa, _), (Fb, sb, _) = evaluate(case), evaluate(case)
    assert np.array_equal(Fa, Fb) and sa["engCoulRec"] == sb["engCoulRec"] != 0.0


def test_two_engines_are_bitwise_identical_70000():
    """... also where blocks take a second round and add to their row (`mine[...] +=`)"""
    case = er.isolated_case("n70000")
    (Fa, sa, _), (Fb, sb, _) = evaluate(case), evaluate(case)
    assert np.array_equal(Fa, Fb) and sa["engCoulRec"] == sb["engCoulRec"] != 0.0


@pytest.mark.parametrize("name", ["n65", "n500", "k479"])
def test_permuted_input_order(name):
    """Every atom gets the same force whichever place it has in the input (tile membership changes, so to tolerance, not bitwise): the
    permuted run is held to the permuted reference, and the two runs to each other within 2 TAU S_F,i."""
    case, ref = er.fixture_case(name)
    N = len(case["types"])
    perm = np.random.Generator(np.random.PCG64(11)).permutation(N)
    pcase = dict(case)
    for k in ("types", "x", "y", "z", "vx", "vy", "vz"):
        pcase[k] = np.ascontiguousarray(np.asarray(case[k])[perm])
    pref = {"F": ref["F"][perm], "SF": ref["SF"][perm], "E": ref["E"], "SE": ref["SE"]}
    F, _, _ = evaluate(case)
    Fp, stats, kt = evaluate(pcase)
    hold(name, "permuted", Fp, stats, kt, pref)
    d = np.linalg.norm((Fp - F[perm]).astype(np.longdouble), axis=1)
    assert (d <= 2 * pc.TAU * pref["SF"]).all(), (name, float((d[pref["SF"] > 0] / pref["SF"][pref["SF"] > 0]).max()))


def test_dense_system_total_force_per_atom():
    """The 500-ion system of test_gpu_parity.ewald_case: each atom's TOTAL force within TAU (S_F,i + sum_pairs S_F r) of the all-mpmath reference
    (reciprocal part + real-space Ewald + Lennard-Jones terms, pair by pair), and the four energies each within TAU of its own scale."""
    case = er.dense_case()
    R = er.fixture("dense")
    for k in ("x", "y", "z"):
        assert np.array_equal(R[k], case[k]), "the case generator drifted away from the committed fixture"
    for variant in (1, 2):
        F, stats, kt = evaluate(case, variant)
        assert EWALD_KERNELS <= {k for k, v in kt.items() if v["calls"] > 0}
        err = np.linalg.norm(F - R["F"], axis=1)
        line = ["worst err / S_F,i = %.3e" % float((err / R["SF"]).max())]
        ratios = {}
        for k in ("engCoul", "engVdW", "engCoulRec", "engCoulConst"):
            ratios[k] = abs(stats[k] - float(R[k])) / float(R[k + "_scale"])
            line.append("%s err / scale = %.3e" % (k, ratios[k]))
        print("dense [pair_variant %d]: %s" % (variant, "   ".join(line)))
        bad = np.flatnonzero(~(err <= pc.TAU * R["SF"]))
        assert bad.size == 0, (variant, bad[:8], (err / R["SF"])[bad[:8]])
        for k, v in ratios.items():
            assert v <= pc.TAU, (variant, k, stats[k], float(R[k]), v)
        assert stats["pairs_dropped"] == 0


def test_madelung_constant_through_the_engine():
    """Known answer on the GPU: the Ewald energy of a rock-salt lattice is -M k q^2 / r0 per ion pair, M = 1.7475646 (NaCl); 512 ions,
    real + reciprocal + constant terms, to the tolerance test_oracle_golden.test_ewald_madelung_constant uses for the oracle."""
    case = er.rocksalt_case()
    q, r0, N = 1.0, 2.82, len(case["types"])
    F, stats, kt = evaluate(case)
    assert EWALD_KERNELS <= {k for k, v in kt.items() if v["calls"] > 0}
    e = stats["engCoul"] + stats["engCoulRec"] + stats["engCoulConst"]
    expect = -1.7475645946 * pc.FCOUL * q * q / r0 * (N / 2)
    print("rock salt: E = %.12e, -M k q^2 / r0 N / 2 = %.12e, relative difference %.3e, largest force component %.3e" % (e, expect, abs(e - expect) / abs(expect), np.abs(F).max()))
    assert abs(e - expect) < 2e-5 * abs(expect), (e, expect)
    assert np.abs(F).max() < 1e-4                                # a perfect lattice is force-free
