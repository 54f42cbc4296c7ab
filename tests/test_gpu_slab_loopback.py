"""A loopback slab rank against the one-GPU engine on replicated boxes (tests/slab_cases.py).

Everything that runs device-side on a slab rank - LoopbackExchanger with k_loopback_shift and k_loopback_ranges, the overlapped exchange, the graph replay,
and the device_side() branches of Engine that the RCCL transport takes as well - had only ever been compared with itself.  Here rank r of n, opened with
slab={"rank": r, "nranks": n, "loopback": True, "replicated": True} on a box of n exact translates of one period, must reproduce its share of the run of
the ordinary one-GPU engine on that box: after every call the atoms it owns (ids and all: the replicated loopback moves ids from copy to copy), their
x, v and f, its energies times n, and the crossings of the periodic wall if it holds one.

Ownership.  Atoms change hands when the cells are rebuilt, not when they cross a boundary.  On a rebuild step - the first call, and every step of an
engine that rebuilds every step - the owned ids are exactly those the reference has inside [xlo, xhi).  Between two rebuilds an atom moves by less than
skin / 2 (or the window is run again), so an atom held by the wrong rank must lie within skin / 2 of a boundary, and what a rank still holds of its own
atoms must be what it lacks of its neighbour's copies of them.  x, v and f are compared for every owned atom, wherever it is.

What a rank reports (Engine::get_stats): its LOCAL sums - LoopbackExchanger::allreduce_sum is empty, nothing is divided by nranks.  So energies are compared
as n x rank against the box (every rank holds the same share of an n-fold periodic system), and wall counters with factor 1: the negative-x crossings of
the box are those of rank 0's atoms through x = 0, the positive-x crossings those of rank n - 1's through x = L, and every other rank reports none along x.

Bounds.  A loopback rank differs from the box only by roundings (a ghost is its source -+ w, good to an ulp), which a chaotic system amplifies; how much, the
reference shows itself: its own n copies drift apart by slab_cases.divergence().  A compared quantity may be off by the larger of the project's own bound
(tests/test_gpu_slab.py: 1e-9 relative on the state, 1e-10 on energies) and 4 x the reference's divergence of that quantity at that step - two independent
rounding histories on either side and a factor of two in hand.  An energy is a smooth function of the whole state, so it takes the largest divergence
of any state quantity.  Every case prints divergence, bound and error / bound; no case may need a divergence above 1e-7.

One process, one engine after another (two alive at most), no torchrun.
"""
import functools

import numpy as np
import pytest

import slab_cases as sc
from aztotmd_amd import api
from aztotmd_amd.api import DebugBit

pytestmark = pytest.mark.gpu

KEYS = sc.STATE_KEYS
ENERGIES = ("engVdW", "engCoul", "engKin", "engBond", "engAngle")
CALLS = (1, 19, 20, 20)               # one step (a rebuild step: the full message), then three calls that hold plain steps and rebuilds
STATE_BOUND, ENERGY_BOUND = 1e-9, 1e-10
DIVERGENCE_CAP = 1e-7


def _key(opts):
    return tuple(sorted(opts.items()))


def _snapshot(e):
    s = e.state(KEYS)
    return {k: s[k].copy() for k in KEYS}, e.stats()


@functools.lru_cache(maxsize=None)
def reference(name, n, opts_key):
    """[(state, stats, divergence)] after every call of the one-GPU engine on the replicated box, with the conditions on the reference alone asserted"""
    case = sc.box_case(name, n)
    L = case["box"][0]
    e = api.Engine(api.Model.from_case(case), cell_size=sc.CELL_SIZE, **dict(opts_key))
    assert e.stats()["n_cells"] == 9 * n * sc.K
    out = []
    for calls in CALLS:
        e.step(calls)
        s, st = _snapshot(e)
        # ownership must be unambiguous at every compared step: no atom is left out of the ownership comparison
        assert sc.seam_distance(s["x"], n, L).min() > 1e-6, (name, n, st["step"])
        for k in KEYS:
            s[k].setflags(write=False)
        out.append((s, st, sc.divergence(s, n, sc.P, case["box"], sc.INTERLEAVED)))
    e.close()
    changes = sc.slab_changes(out[0][0]["x"], out[-1][0]["x"], n, L)
    st = out[-1][1]
    print("reference %s x %d %s: slab changes per boundary (+x, -x) %s, wall crossings -x %d +x %d" % (name, n, dict(opts_key), changes, st["negCross"][0], st["posCross"][0]))
    for s, st_, div in out:
        print("  step %3d divergence of the reference's own copies: %s" % (st_["step"], " ".join("%s %.2e" % kv for kv in div.items())))
    assert all(a >= 10 and b >= 10 for a, b in changes), changes
    assert st["negCross"][0] > 0 and st["posCross"][0] > 0, st
    assert max(out[-1][2].values()) <= DIVERGENCE_CAP, out[-1][2]
    return out


@functools.lru_cache(maxsize=None)
def rank_run(name, n, r, opts_key, lazy=True):
    """[(state, stats)] of loopback rank r of n after every call"""
    case = sc.box_case(name, n)
    e = api.Engine(api.Model.from_case(case), cell_size=sc.CELL_SIZE, slab={"rank": r, "nranks": n, "loopback": True, "replicated": True}, **dict(opts_key))
    out = []
    for calls in CALLS:
        e.step(calls)
        out.append(_snapshot(e))
    e.close()
    first, last = out[0][1], out[-1][1]
    print("rank %d of %d %s %s: sort interval %d, rebuilds %d of %d steps, violations %d, pair lists %d" % (r, n, name, dict(opts_key), last["sort_interval"], last["rebuilds"], last["step"], last["sort_violations"], last["pair_lists"]))
    assert last["n_cells"] == 9 * n * sc.K and last["step"] == sum(CALLS)
    if lazy:
        # plain steps went through exchange_ranges, and migrants were re-exchanged after an interval of unwrapped coordinates - at least twice
        assert last["sort_interval"] > 1, last
        assert last["rebuilds"] - first["rebuilds"] >= 2 and last["rebuilds"] < last["step"], (first["rebuilds"], last["rebuilds"])
    return out


def compare(name, n, r, rank_snaps, ref_snaps):
    """the comparison after every call; prints divergence, bound and error / bound per quantity, asserts at the end of each step"""
    box = sc.box_case(name, n)["box"]
    L = box[0]
    worst = 0.0
    for (s, st), (rs, rst, div) in zip(rank_snaps, ref_snaps):
        assert st["step"] == rst["step"]
        own = ~np.isnan(s["x"])
        expected = sc.owner(rs["x"], n, L) == r
        lost, extra = np.flatnonzero(expected & ~own), np.flatnonzero(own & ~expected)
        # Atoms change hands when the cells are rebuilt, not when they cross: exact on a rebuild step (the first call is one; so is every step of an engine
        # that rebuilds every step).  Between two rebuilds an atom moves by less than skin / 2 or the window is run again, so whoever is with the wrong
        # rank lies within skin / 2 of a boundary - and since every copy does the same, what a rank still holds of its own is what it lacks of its neighbour's
        band = 0.0 if (st["step"] == 1 or st["rebuilds"] >= st["step"]) else 0.5 * st["skin"]
        late = np.concatenate([lost, extra])
        assert late.size == 0 or (band > 0.0 and sc.seam_distance(rs["x"][late], n, L).max() < band), (
            "rank %d of %d at step %d (band %.3f): not owned %s, owned and not its own %s" % (r, n, st["step"], band, lost[:8], extra[:8]))
        n0 = len(own) // n
        atom = (lambda ids: ids // n) if sc.INTERLEAVED else (lambda ids: ids % n0)
        assert np.array_equal(np.sort(atom(lost)), np.sort(atom(extra))) and own.sum() == n0, (lost, extra)
        print("rank %d of %d %s step %3d  owned %d, of them beyond a boundary since the last rebuild %d" % (r, n, name, st["step"], own.sum(), extra.size))
        rows = []
        for k in KEYS:
            assert not np.isnan(s[k][own]).any(), k
            per = box["xyz".index(k)] if k in "xyz" else None
            err, bound = sc.rel_diff(s[k][own], rs[k][own], per), max(STATE_BOUND, 4.0 * div[k])
            rows.append((k, div[k], bound, err))
        ebound = max(ENERGY_BOUND, 4.0 * max(div.values()))
        for k in ENERGIES:
            if rst[k] != 0.0:
                rows.append((k, max(div.values()), ebound, abs(n * st[k] - rst[k]) / abs(rst[k])))
            else:
                assert st[k] == 0.0, k
        print("rank %d of %d %s step %3d  " % (r, n, name, st["step"]) + "  ".join("%s div %.1e bound %.1e err/bound %.2e" % (k, d, b, e / b) for k, d, b, e in rows))
        worst = max([worst] + [e / b for _, _, b, e in rows])
        for k, d, b, e in rows:
            assert e <= b, (name, n, r, st["step"], k, e, b)
        # wall counters: local sums (factor 1)
        assert st["negCross"][0] == (rst["negCross"][0] if r == 0 else 0), (r, st["negCross"], rst["negCross"])
        assert st["posCross"][0] == (rst["posCross"][0] if r == n - 1 else 0), (r, st["posCross"], rst["posCross"])
    print("rank %d of %d %s: worst error / bound %.3e" % (r, n, name, worst))
    return worst


def held_to_the_box(name, n, r, lazy=True, **opts):
    k = _key(opts)
    snaps = rank_run(name, n, r, k, lazy)
    compare(name, n, r, snaps, reference(name, n, k))
    return snaps


def assert_bit_identical(a, b, what):
    for (sa, sta), (sb, stb) in zip(a, b):
        for k in KEYS:
            assert np.array_equal(sa[k], sb[k], equal_nan=True), (what, sta["step"], k)
        for k in ("negCross", "posCross"):
            assert sta[k] == stb[k], (what, k)
        for k in ENERGIES:
            assert abs(sta[k] - stb[k]) <= 1e-12 * abs(stb[k]), (what, k)


@pytest.mark.parametrize("n,r", [(2, 0), (2, 1), (4, 0), (4, 2), (4, 3)])
def test_every_rank_of_a_ring(n, r):
    """rank 0 holds the periodic wall at x = 0, the last rank the one at x = L, a middle rank neither"""
    held_to_the_box("lj", n, r)


def test_the_three_ranks_of_a_ring_make_up_the_box():
    """n = 3 in full: after every call the three owned sets partition the ids and their union is the reference state"""
    n = 3
    runs = [held_to_the_box("lj", n, r) for r in range(n)]
    ref = reference("lj", n, _key({}))
    box = sc.box_case("lj", n)["box"]
    for c in range(len(CALLS)):
        owned = np.stack([~np.isnan(runs[r][c][0]["x"]) for r in range(n)])
        assert (owned.sum(0) == 1).all(), "an atom is owned by no rank or by two"
        rs, rst, div = ref[c]
        for k in KEYS:
            merged = np.nansum(np.stack([runs[r][c][0][k] for r in range(n)]), axis=0)
            per = box["xyz".index(k)] if k in "xyz" else None
            assert sc.rel_diff(merged, rs[k], per) <= max(STATE_BOUND, 4.0 * div[k]), (c, k)
        for k in ENERGIES:
            if rst[k] != 0.0:
                assert abs(sum(runs[r][c][1][k] for r in range(n)) - rst[k]) <= max(ENERGY_BOUND, 4.0 * max(div.values())) * abs(rst[k]), (c, k)
        assert sum(runs[r][c][1]["negCross"][0] for r in range(n)) == rst["negCross"][0] and sum(runs[r][c][1]["posCross"][0] for r in range(n)) == rst["posCross"][0]


@pytest.mark.parametrize("split", [0, 2])
def test_the_table_kernel(split):
    """two charged species, LJ + Fennell; with the default launch and with two waves per cell"""
    held_to_the_box("fennell", 2, 0, **({"split": split} if split else {}))


@pytest.mark.parametrize("r", [0, 1])
def test_molecules_across_the_seams(r):
    """bonds and angles whose partners are ghosts (k_bonded<VERIFY>, idxOfId on ghosts), molecules that migrate atom by atom: rank 0 and rank n - 1"""
    snaps = held_to_the_box("mol", 2, r)
    assert snaps[-1][1]["engBond"] != 0.0 and snaps[-1][1]["engAngle"] != 0.0 and snaps[-1][1]["engCoul"] != 0.0


def test_the_per_atom_kernel():
    """pair_variant 1 (one thread per atom, ghosts read like owned atoms) on the same lazy schedule: plain steps between rebuilds here too"""
    held_to_the_box("lj", 2, 0, pair_variant=1)


@pytest.mark.parametrize("bits", [DebugBit.DBG_LARGE_KICK_PATH, DebugBit.DBG_FOLD_KICK, DebugBit.DBG_FOLD_DRIFT], ids=lambda b: b.name)
def test_kick_paths(bits):
    """the deferred half-kick of large systems, and the two folding switches a slab rank must ignore - against the box, not against a twin"""
    held_to_the_box("lj", 2, 0, debug=int(bits))


def test_the_overlapped_exchange():
    """DBG_OVERLAP_HALO: the coordinate exchange on a second stream beside the interior cells, three launches - against the box, and bit for bit
    against the serial order on the same rank.  The overlap runs on plain steps of an engine that is not profiling, walks lists (pair variant 2) and has
    an interior layer (ncxLocal - 4 hw >= 1): asserted here as far as a caller can see it."""
    dims, hw, _ = sc.expected_grid(sc.box_case("lj", 2), 2)
    assert dims[0] // 2 + 2 * hw - 4 * hw >= 1
    over = held_to_the_box("lj", 2, 0, debug=int(DebugBit.DBG_OVERLAP_HALO))
    assert over[-1][1]["pair_lists"] == 1 and over[-1][1]["sort_interval"] > 1 and over[-1][1]["rebuilds"] < over[-1][1]["step"]
    assert_bit_identical(over, held_to_the_box("lj", 2, 0), "overlap against the serial order")


def test_the_replayed_graph():
    """DBG_SLAB_GRAPH (serial order only): against the box, and bit for bit against the rank that launches its kernels one by one.  Cycles are replayed
    only where every step rebuilds the cells (sort_every = 1: a plain step's exchange takes its ranges from the host, and they change with every sort; a
    capture of the lazy schedule used to end the call with 'operation not permitted when stream is capturing').  On the lazy schedule the switch must
    change nothing."""
    graph = held_to_the_box("lj", 2, 0, lazy=False, sort_every=1, debug=int(DebugBit.DBG_SLAB_GRAPH))
    assert graph[-1][1]["rebuilds"] >= sum(CALLS) and graph[-1][1]["sort_interval"] == 1, graph[-1][1]
    assert_bit_identical(graph, held_to_the_box("lj", 2, 0, lazy=False, sort_every=1), "graph replay against eager launches")
    lazy = held_to_the_box("lj", 2, 0, debug=int(DebugBit.DBG_SLAB_GRAPH))
    assert_bit_identical(lazy, held_to_the_box("lj", 2, 0), "the switch on the lazy schedule")


def test_a_violation_repaired_by_running_the_window_again():
    """a sort interval held at 32 steps on atoms at 4 000 K: the look finds the violation, the rank goes back to its snapshot and runs the window again
    with the cells rebuilt every step - and still follows the box"""
    snaps = held_to_the_box("hot", 2, 0, lazy=False, sort_every=32, debug=int(DebugBit.DBG_FIXED_INTERVAL))
    assert snaps[-1][1]["sort_violations"] > 0, snaps[-1][1]


def test_a_bond_that_reaches_past_the_halo_is_an_error():
    """Counts::bondedMissing: the partner of an owned atom lies four cell layers away, hw = 1.  k_bonded skips the term and raises the flag (no device fault);
    the first step's force phase is the first to evaluate bonds (the initial force call computes pair forces only), so the first call ends with an
    AztotError that says so, and the handle refuses to step on."""
    case, j, partner = sc.stray_bond_case()
    e = api.Engine(api.Model.from_case(case), cell_size=sc.CELL_SIZE, slab={"rank": 0, "nranks": 3, "loopback": True, "replicated": True})
    with pytest.raises(api.AztotError) as first:
        e.step(1)
    assert "partner was not resident" in str(first.value), str(first.value)
    with pytest.raises(api.AztotError) as again:
        e.step(1)
    assert "earlier call" in str(again.value) and "partner was not resident" in str(again.value), str(again.value)
    assert e.clock()["step"] >= 0                 # a failed handle still answers a post-mortem read
    e.close()
    # ... and the same box without the bond steps
    e = api.Engine(api.Model.from_case(sc.box_case("lj", 3)), cell_size=sc.CELL_SIZE, slab={"rank": 0, "nranks": 3, "loopback": True, "replicated": True})
    e.step(1)
    e.close()
