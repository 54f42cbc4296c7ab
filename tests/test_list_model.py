"""CPU side of the pair-list tests (tests/test_gpu_pair_lists.py): the numpy restatement of the builder (tests/list_model.py) and the cases
(tests/list_cases.py) checked against themselves - the longdouble Lennard-Jones term against the mpmath reference, the restated filter as a
superset of the exact pairs within the list radius, what the cases cover, three mutations of the builder that must each lose a pair, and
the fp64 oracle held to the force tolerance of the GPU test before the kernel is."""
import numpy as np
import pytest

import list_cases as lc
import list_model as lm
import pair_cases as pc
from oracle import oracle

SHELL_CASES = [lc.shell_pairs, lambda: lc.populations(1)]
IDS = ["shell_pairs", "populations"]


def test_longdouble_lj_term_against_mpmath():
    mp = pytest.importorskip("mpmath")
    import pair_reference as pr
    for eps, sigma in ((lc.EPS, lc.SIGMA), (0.002, 1.9), (0.01006, 3.3952)):
        for r in np.concatenate([np.linspace(0.8 * sigma, 7.5, 40), [lc.RC, 6.0, 6.5, np.nextafter(lc.RC, 0)]]):
            f, sf = lm.lj_term(eps, sigma, np.longdouble(r) * np.longdouble(r))
            fr, _, sfr, _ = pr.vdw(1, [eps, sigma], r)
            # (mpmath reads the longdouble through 26 decimal digits)
            assert abs(mp.mpf(np.format_float_scientific(f, precision=25, unique=False)) - fr) <= mp.mpf("1e-17") * sfr, (eps, sigma, r)
            assert abs(mp.mpf(np.format_float_scientific(sf, precision=25, unique=False)) - sfr) <= mp.mpf("1e-17") * sfr, (eps, sigma, r)


def _rebuild_steps(c):
    return [1 + g * c["K"] for g in (0, 1)]


def _positions_at(c, step):
    if c["positions"] is not None:
        return c["positions"](step)
    o = _oracle_run(c)
    return o[step]


_ORC = {}


def _oracle_run(c):
    """the liquid's trajectory from the fp64 oracle: positions (unwrapped displacements are small: wrapped coordinates do) after every step"""
    if c["name"] not in _ORC:
        o = oracle.Oracle(c["case"])
        o.forces(1)
        out = {0: np.stack([c["case"][k] for k in "xyz"], 1)}
        for s in range(1, c["steps"] + 1):
            o.step(1)
            st = o.state()
            out[s] = np.stack([st[k] for k in "xyz"], 1)
        _ORC[c["name"]] = out
    return _ORC[c["name"]]


CASES = [lc.shell_pairs, lambda: lc.populations(1)] + [(lambda k=k: lc.liquid(k)) for k in lc.LIQUIDS if k != "three_cells"]
CASE_IDS = IDS + [k for k in lc.LIQUIDS if k != "three_cells"]


@pytest.mark.parametrize("make", CASES, ids=CASE_IDS)
def test_restated_filter_keeps_every_pair_within_the_list_radius(make):
    """at both rebuilds of the run, for both accumulation orders of the matrix filter"""
    c = make()
    g = c["geom"]
    assert g["lazy"]
    for step in _rebuild_steps(c):
        pos = _positions_at(c, step)
        i, j, r2 = lm.exact_pairs(pos, g["box"], g["r_list"])
        assert len(i) > 0
        b = lm.Builder(pos, g)
        for fused in (False, True):
            lost = b.lost(i, j, r2, fused)
            assert not lost.any(), (c["name"], step, fused, i[lost][:5], j[lost][:5], np.sqrt(r2[lost][:5].astype(float)))


def test_three_cells_on_an_axis_leave_no_lists():
    g = lc.liquid("three_cells")["geom"]
    assert min(g["nc"]) == 3 and not g["lazy"] and g["slack"] == 0.0


@pytest.mark.parametrize("make", SHELL_CASES, ids=IDS)
def test_shell_pairs_start_outside_and_end_inside(make):
    """Under ballistic motion every pair of group g is in the shell at rebuild g - at its depth, at least one pair per offset at >= 0.9 - and inside rMax
    before rebuild g + 1; nobody travels more than slack in an interval; every tested atom has exactly one partner with a potential within the list
    radius at every step."""
    c = make()
    g, P, K = c["geom"], c["pairs"], c["K"]
    slack, rM = g["slack"], g["r_max"]
    assert abs(slack - 0.245) < 1e-12 and abs(g["r_list"] - 7.49) < 1e-12 and g["nc"] == [int(round(L / lc.CELL)) for L in g["box"]]
    dist = {}
    for s in range(0, c["steps"] + 1):
        x = c["positions"](s)
        d = lm.min_image(x[P["i"]] - x[P["j"]], g["box"])
        dist[s] = np.sqrt((d * d).sum(1))
    for grp in (0, 1):
        m = P["group"] == grp
        s0 = 1 + grp * K
        depth = (dist[s0][m] - rM) / (2 * slack)
        assert np.allclose(depth, P["depth"][m], atol=1e-9)
        assert (dist[s0][m] > rM).all() and (dist[s0][m] <= g["r_list"]).all()
        assert (dist[s0 + K - 1][m] < rM).all()                          # the last plain step of the interval
        first_in = np.array([min(s for s in range(s0, s0 + K) if dist[s][k] <= rM) for k in np.flatnonzero(m)])
        assert len(set(first_in.tolist())) >= 3                          # the pairs come in at different steps of the interval
        for o in set(map(tuple, P["offset"][m])):
            mo = m & (P["offset"] == np.array(o)).all(1)
            if c["name"] == "shell_pairs":                               # three directions per offset, the deepest at >= 90 % of the shell
                assert mo.sum() >= 3 and (P["depth"][mo] >= 0.9).any(), o
        assert (P["depth"][m] >= 0.9).sum() >= 6
    step_len = np.linalg.norm(c["velocity"], axis=1) * lc.DT
    assert (step_len * (K - 1) <= 0.95 * slack * (1 + 1e-12)).all() and (step_len[P["i"]] * (K - 1) >= 0.949 * slack).all()
    tested = c["case"]["types"] == 0
    for s in (0, 1, K, 1 + K, 2 * K, 2 * K + 1):
        x = c["positions"](s)[tested]
        i, j, _ = lm.exact_pairs(x, g["box"], g["r_list"] + 2.5 * slack)
        assert len(i) <= tested.sum() // 2 and np.bincount(np.concatenate([i, j]), minlength=tested.sum()).max() == 1, s


def _image_codes(c, step):
    """per axis the set of image codes the tested pairs need at the rebuild of `step` (both directions of every pair)"""
    g, P = c["geom"], c["pairs"]
    cc = lm.cell_coords(c["positions"](step), g)
    codes = [set(), set(), set()]
    offs = set()
    for a, b in ((P["i"], P["j"]), (P["j"], P["i"])):
        o = cc[b] - cc[a]
        n = np.array(g["nc"])
        img = np.where(o > 1, 0, np.where(o < -1, 2, 1))               # the partner's cell index wrapped: it is reached through the wall
        o = o - n * np.rint(o / n).astype(np.int64)
        for k in range(3):
            codes[k] |= set(img[:, k].tolist())
        offs |= set(map(tuple, o.tolist()))
    return codes, offs


def test_cases_cover_the_builders_edges():
    sp, pop = lc.shell_pairs(), lc.populations(1)
    for step in (1, 1 + sp["K"]):
        codes, offs = _image_codes(sp, step)
        assert all(cs == {0, 1, 2} for cs in codes), codes
        assert offs == set(lm.OFFSETS26) | {(0, 0, 0)}
        _, offs = _image_codes(pop, step)
        assert offs == set(lm.OFFSETS26)
    g = pop["geom"]
    near16, near128 = False, False
    for step in (1, 1 + pop["K"]):
        pos = pop["positions"](step)
        n = lm.populations(pos, g)
        assert set(lc.POPULATIONS) <= set(n.tolist()), sorted(set(n.tolist()))
        assert n.max() == 65 and (n > 64).sum() == 3
        b = lm.Builder(pos, g)
        T = np.array(list(b.candidate_counts().values()))
        assert T.max() <= 300                                            # (the engine's smallest tile holds 320 candidates)
        near16 |= bool((np.minimum(T % 16, 16 - T % 16) <= 1).any())
        near128 |= bool(((T > 64) & (np.minimum(T % 128, 128 - T % 128) <= 1)).any())
        # where the ids put the tested atom and its partner in their cells' runs
        P = pop["pairs"]
        where = {"first16": 0, "last16": 0, "last": 0, "partner_first": 0, "partner_last": 0}
        for i, j in zip(P["i"], P["j"]):
            ra, rb = b.atoms_of(b.cell[i]), b.atoms_of(b.cell[j])
            ka, kb = int(np.flatnonzero(ra == i)[0]), int(np.flatnonzero(rb == j)[0])
            where["first16"] += ka % 16 == 0
            where["last16"] += ka % 16 == 15
            where["last"] += ka == len(ra) - 1 and len(ra) > 1
            where["partner_first"] += kb == 0 and len(rb) > 1
            where["partner_last"] += kb == len(rb) - 1 and len(rb) > 1
        assert all(v >= 5 for v in where.values()), where
    assert near16 and near128
    moving = pop["case"]["types"] == 2
    assert moving.sum() > 100 and (pop["case"]["types"] == 1).sum() > 100
    assert (np.linalg.norm(pop["velocity"][moving], axis=1) > 0).all()
    for kind in lc.LIQUIDS:
        c = lc.liquid(kind)
        assert len(c["case"]["types"]) <= 4000
    assert sorted(lc.liquid("skin_cells")["geom"]["nc"]) == [5, 6, 7]
    assert lc.liquid("wide_stencil")["geom"]["hw"] == [3, 3, 3]
    n = lm.populations(np.stack([lc.liquid("crowded")["case"][k] for k in "xyz"], 1), lc.liquid("crowded")["geom"])
    assert 12 <= n.min() and n.max() <= 45 and n.mean() > 20, (n.min(), n.max(), n.mean())


@pytest.mark.parametrize("kind", [k for k in lc.LIQUIDS if k != "three_cells"])
def test_liquids_stay_inside_their_slack(kind):
    """nobody travels more than slack between two rebuilds (fp64 oracle trajectory), and plenty of pairs cross rMax inwards and outwards in an interval"""
    c = lc.liquid(kind)
    g, K = c["geom"], c["K"]
    tr = _oracle_run(c)
    for s0 in _rebuild_steps(c):
        d = lm.min_image(tr[s0 + K - 1] - tr[s0], g["box"])
        assert np.sqrt((d * d).sum(1)).max() < 0.9 * g["slack"], (kind, np.sqrt((d * d).sum(1)).max(), g["slack"])
        a = lm.exact_pairs(tr[s0], g["box"], g["r_max"], dtype=np.float64)
        b = lm.exact_pairs(tr[s0 + K - 1], g["box"], g["r_max"], dtype=np.float64)
        N = len(tr[0])
        ka, kb = set((a[0] * N + a[1]).tolist()), set((b[0] * N + b[1]).tolist())
        assert len(kb - ka) > 100 and len(ka - kb) > 100, (kind, len(kb - ka), len(ka - kb))


@pytest.mark.parametrize("mutation", lm.MUTATIONS)
def test_every_mutation_of_the_builder_loses_a_pair_that_comes_inside(mutation):
    """Sharpness: each mutation loses, in at least one case, a pair that is inside rMax before the next rebuild - a missing force term on the GPU.  (The
    unmutated builder loses none: test_restated_filter_keeps_every_pair_within_the_list_radius.)"""
    caught = []
    for c in (lc.shell_pairs(), lc.populations(1), lc.edge_pairs()):
        g, K = c["geom"], c["K"]
        for s0 in _rebuild_steps(c):
            pos = c["positions"](s0)
            i, j, r2 = lm.exact_pairs(pos, g["box"], g["r_list"])
            end = c["positions"](s0 + K - 1)
            d = lm.min_image(end[i] - end[j], g["box"]).astype(np.longdouble)
            comes_in = (d * d).sum(1) <= np.longdouble(g["r_max"]) ** 2
            b = lm.Builder(pos, g, mutation)
            for fused in (False, True):
                n = int((b.lost(i, j, r2, fused) & comes_in).sum())
                if n:
                    caught.append((c["name"], s0, fused, n))
    assert caught, mutation
    print(mutation, caught)


ORACLE_CASES = [lc.shell_pairs, lambda: lc.populations(1)] + [(lambda k=k: lc.liquid(k)) for k in lc.LIQUIDS]


@pytest.mark.parametrize("make", ORACLE_CASES, ids=IDS + list(lc.LIQUIDS))
def test_oracle_meets_the_force_tolerance_and_no_pair_can_hide(make):
    """The fp64 oracle's forces at the positions of three steps of the run against the longdouble enumeration: |F - F_ref| <= TAU sum_j S_F r per atom,
    before the kernel is held to it.  And the condition on the inputs: the smallest single pair term of every atom is at least 1000 times its
    tolerance, so one lost pair can never hide inside it."""
    c = make()
    g = c["geom"]
    worst = 0.0
    for step in (c["K"], 2 * c["K"], c["steps"]):
        pos = _positions_at(c, step)
        ref = lm.lj_forces(pos, c["case"]["types"], g["box"], c["vdw"], g["r_max"])
        assert ref["near"] == 0
        has = np.isfinite(ref["smallest"].astype(np.float64))
        assert has.any() and (ref["smallest"][has] >= 1000 * pc.TAU * ref["scale"][has]).all(), (c["name"], step)
        case = dict(c["case"])
        case.update(x=pos[:, 0].copy(), y=pos[:, 1].copy(), z=pos[:, 2].copy())
        o = oracle.Oracle(case)
        o.forces(1)
        st = o.state()
        F = np.stack([st["fx"], st["fy"], st["fz"]], 1)
        err = np.sqrt(((F - ref["F"]) ** 2).sum(1))
        assert (err[~has] == 0).all()
        ratio = (err[has] / (pc.TAU * ref["scale"][has])).astype(np.float64)
        worst = max(worst, ratio.max())
        assert ratio.max() <= 1.0, (c["name"], step, ratio.max())
    print("%s: oracle worst err / (TAU sum S_F r) = %.3g" % (c["name"], worst))
