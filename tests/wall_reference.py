"""The first half of a step - drift, periodic wrap, wall-crossing counters, wall momenta - stated once, for tests/wall_cases.py: numpy only.

run() carries the gas in EXACT arithmetic: every input is a double, dt is a power of two, the forces are zero, so positions, image indices and the momenta
m |v| are integers in units of 2^-256 (Python integers in numpy object arrays; nothing rounds).  Two rules, one per schedule:

  "every"   put_periodic after every drift (box.cpp:230-295, oracle/aztot_oracle.c:531) with the documented deviation that a coordinate >= L after the shift
            becomes 0 (SURVEY C-6): x < 0 is a crossing of the lower wall, x > L one of the upper wall, x == L is none and is reported as 0.0.
  "image"   what image_of (csrc/kernels.hip.h) states for the lazy schedule: coordinates stay unwrapped between two rebuilds, a wall is crossed when the
            image index changes, and [0, L] is image 0.  Steps that rebuild the cells (`rebuild_steps`) wrap as the every-step rule does, and an engine
            that computes initial forces wraps the initial state the same way, counting nothing (`initial_fold`).
The two differ for an atom that lands exactly on L and moves on: "every" sets it to 0 and never counts it, "image" counts it one step later - unless the
landing step rebuilt the cells.  With rebuild_steps = every step the image rule IS the every-step rule.

The image index itself is exact here, floor(x / L), where the kernels take (int)(x * (1 / L)).  The two agree away from the multiples of L (wall_cases keeps
every generic atom 1e-9 A and more from one: `margin`); the reported coordinate is compared modulo L, and the count of a crossing does not depend on it.

Bounds (TAU = pair_cases.TAU; the worst chain is a dozen roundings of magnitude <= L, about 1.3e-15 L):
  position   |x_gpu - x_ref| taken to the nearest multiple of L  <=  TAU (L + sum over the steps of |v dt|)
  momentum   |mom_gpu - mom_ref|  <=  TAU sum of m |v| over the crossings of that wall
  coordinates whose chain is exact in fp64 (wall_cases.exact_axes) are held to EQUALITY with the double nearest to the exact value - the one rounding the
  rule's own shift by L can make -, and counts are integers.
kernel_step() restates the kernels' rule in float64, atom by atom in launch order with the workgroup / wave / thread-pair structure of the sums; the CPU
test applies the MUTATIONS to it and shows that the designed classes catch each.  one_step_ld() is the longdouble statement of one step WITH forces, for
the kicked atoms of a liquid.
"""
from fractions import Fraction

import numpy as np

import wall_cases as wc

LD = np.longdouble
TAU = wc.TAU
SH = 256
ONE = 1 << SH
WALLS = ("Xn", "Xp", "Yn", "Yp", "Zn", "Zp")
MARGIN = 1e-9
MUTATIONS = ("ge_for_gt", "no_plus_1_on_the_negative_side", "momentum_before_the_kick", "frozen_atoms_counted", "second_atom_of_a_pair_lost", "only_wave_0_summed")


def to_int(a):
    """float64 array -> object array of exact integers in units of 2^-256"""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx, val in np.ndenumerate(a):
        f = Fraction(float(val)) * ONE
        assert f.denominator == 1, ("not a multiple of 2^-256", val)
        out[idx] = f.numerator
    return out


def to_float(a, shift=SH):
    """object array of integers in units of 2^-shift -> the nearest doubles"""
    a = np.asarray(a, dtype=object)
    out = np.empty(a.shape, dtype=np.float64)
    for idx, val in np.ndenumerate(a):
        out[idx] = float(Fraction(int(val), 1 << shift))
    return out


def _image(col, L):
    out = np.zeros(len(col), dtype=object)
    neg, big = (col < 0).astype(bool), (col > L).astype(bool)
    out[neg] = -((-col[neg]) // L + 1)
    out[big] = col[big] // L
    return out


def _wrap(col, L):
    col = col.copy()
    neg, big = (col < 0).astype(bool), (col > L).astype(bool)
    col[neg] = col[neg] + ((-col[neg]) // L + 1) * L
    col[big] = col[big] - (col[big] // L) * L
    col[(col >= L).astype(bool)] = 0
    return col


def reported(stored, box_int):
    """what state() hands out for stored (possibly unwrapped) exact coordinates: wrapped by the rule, rounded once, and a value that rounds to L folded to 0.0"""
    out = np.empty(stored.shape, dtype=np.float64)
    for ax in range(3):
        w = to_float(_wrap(stored[:, ax], box_int[ax]))
        w[w >= wc.BOX[ax]] = 0.0
        out[:, ax] = w
    return out


def run(x0, v, types, nsteps, rule="every", rebuild_steps=None, initial_fold=False):
    """`nsteps` force-free steps from (x0, v) - v (N, 3) constant, or a list of one (N, 3) array per step (the velocity the drift of that step uses) - under
    `rule`.  Returns a list of nsteps + 1 dicts (index = step number, 0 = the initial state):
      "stored"   exact coordinates as the device keeps them (object array)      "unwrapped"  exact coordinates never wrapped
      "wrapped"  what state() reports, float64 in [0, L)                          "flags"      (N, 6) bool, walls in the order Xn Xp Yn Yp Zn Zp
      "margin"   (N, 3) float64: distance of the coordinate after the drift from the nearest multiple of L
      "cnt" (6,), "spec" (n_species, 6): cumulative counts;  "mom" (6,) float64 and "mom_scale" (6,): cumulative sum of m |v| over the crossings, exact then
      rounded once;  "travel" (N, 3): cumulative sum of |v dt|"""
    N = len(types)
    types = np.asarray(types)
    box_int = [int(Fraction(L) * ONE) for L in wc.BOX]
    m_int = to_int(wc.masses())[types]
    frozen = np.array(wc.FROZEN, dtype=bool)[types]
    X = to_int(x0)
    if initial_fold:
        for ax in range(3):
            X[:, ax] = _wrap(X[:, ax], box_int[ax])
    U = X.copy()
    every = rule == "every"
    assert every or rule == "image"
    cnt, spec, mom = np.zeros(6, dtype=np.int64), np.zeros((len(wc.SPECIES), 6), dtype=np.int64), [0] * 6
    travel = np.zeros((N, 3))
    steps = [{"stored": X, "unwrapped": U, "wrapped": reported(X, box_int), "flags": np.zeros((N, 6), dtype=bool), "margin": np.full((N, 3), np.inf), "cnt": cnt.copy(),
              "spec": spec.copy(), "mom": np.zeros(6), "mom_scale": np.zeros(6), "travel": travel.copy()}]
    v_const = to_int(v) if not isinstance(v, (list, tuple)) else None
    for s in range(1, nsteps + 1):
        vi = v_const if v_const is not None else to_int(v[s - 1])
        assert all(int(q) % 512 == 0 for q in vi.flat)
        d = vi // 512                                             # dt = 2^-9
        d[frozen] = 0
        X1, U = X.copy(), U + d
        flags, margin = np.zeros((N, 6), dtype=bool), np.empty((N, 3))
        for ax in range(3):
            L = box_int[ax]
            i0 = _image(X[:, ax], L)
            col = X[:, ax] + d[:, ax]
            c = _image(col, L) - i0
            flags[:, 2 * ax], flags[:, 2 * ax + 1] = (c < 0).astype(bool), (c > 0).astype(bool)
            r = col % L
            margin[:, ax] = to_float(np.minimum(r, L - r))
            margin[(d[:, ax] == 0).astype(bool), ax] = np.inf     # a coordinate that does not move makes no decision
            for w in (2 * ax, 2 * ax + 1):
                hit = np.flatnonzero(flags[:, w])
                cnt[w] += len(hit)
                np.add.at(spec[:, w], types[hit], 1)
                mom[w] += sum(int(m_int[i]) * abs(int(vi[i, ax])) for i in hit)
            X1[:, ax] = _wrap(col, L) if (every or (rebuild_steps is not None and s in rebuild_steps)) else col
        X = X1
        travel = travel + np.abs(to_float(d))
        mf = to_float(np.array(mom, dtype=object), 2 * SH)
        steps.append({"stored": X, "unwrapped": U, "wrapped": reported(X, box_int), "flags": flags, "margin": margin, "cnt": cnt.copy(), "spec": spec.copy(),
                      "mom": mf, "mom_scale": mf.copy(), "travel": travel.copy()})
    return steps


def position_ratio(x_gpu, step, exact):
    """(worst |x_gpu - x_ref| mod L / (TAU (L + travel)) over all coordinates, number of exact coordinates that are not EQUAL to the reference's double)"""
    x_gpu = np.asarray(x_gpu, dtype=np.float64)
    worst = 0.0
    for ax in range(3):
        L = int(Fraction(wc.BOX[ax]) * ONE)
        diff = (to_int(x_gpu[:, ax]) - step["stored"][:, ax]) % L
        err = to_float(np.minimum(diff, L - diff))
        worst = max(worst, float((err / (TAU * (wc.BOX[ax] + step["travel"][:, ax]))).max()))
    unequal = int(((x_gpu != step["wrapped"]) & exact).sum())
    return worst, unequal


def momentum_ratio(mom_gpu, step):
    """worst |mom_gpu - mom_ref| / (TAU sum m |v|) over the six walls; a wall nobody crossed must report exactly 0"""
    worst = 0.0
    for k in range(6):
        if step["mom_scale"][k] == 0.0:
            assert mom_gpu[k] == 0.0, (WALLS[k], mom_gpu[k])
        else:
            worst = max(worst, abs(float(mom_gpu[k]) - float(step["mom"][k])) / (TAU * float(step["mom_scale"][k])))
    return worst


def undecided(steps, exact):
    """(step, atom, axis) of every generic coordinate whose drift ends within MARGIN of a multiple of L: must be empty"""
    out = []
    for s, st in enumerate(steps):
        bad = (st["margin"] < MARGIN) & ~exact
        out += [(s, int(i), int(ax)) for i, ax in zip(*np.nonzero(bad))]
    return out


def cells(wrapped, dims):
    return wc.sorted_order(wrapped, dims)[1]


# ---- the kernels' rule in float64, with the structure of their sums ------------------------------------------------------------------------------------
def _image_fp(x, L, invL, mutate):
    big = (x >= L) if mutate == "ge_for_gt" else (x > L)
    plus = 0 if mutate == "no_plus_1_on_the_negative_side" else 1
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, -(np.trunc(-x * invL) + plus), np.where(big, np.trunc(x * invL), 0.0)).astype(np.int64)


def _wrap_fp(x, L, invL):
    x = x.copy()
    neg, big = x < 0, x > L
    x[neg] = x[neg] + (np.trunc(-x[neg] * invL) + 1) * L
    x[big] = x[big] - np.trunc(x[big] * invL) * L
    x[x >= L] = 0.0
    return x


def kernel_step(x, v, f, types, rM, m, frozen, order, wrap, body="one", pending=False, box=wc.BOX, dt=wc.DT, mutate=None):
    """One opening of a step as k_integrate1_bin (body "one": a thread per atom) or integrate_plain2_body (body "two": two atoms per thread) performs it, in
    float64: x, v, f (N, 3) in id order, `order` the ids in launch order, rM / m / frozen per species.  Returns (x1, v1, cnt (6,), mom (6,), spec)."""
    x, v, f = (np.asarray(a, dtype=np.float64) for a in (x, v, f))
    N = len(x)
    k = (rM[types])[:, None] * f
    vk = v + k
    if pending:
        vk = vk + k
    vm = v if mutate == "momentum_before_the_kick" else vk
    d = vk * dt
    moved = np.where(frozen[types][:, None], 0.0, d)
    x1 = x + moved
    probe = x + d if mutate == "frozen_atoms_counted" else x1
    flags, contrib = np.zeros((N, 6), dtype=bool), np.zeros((N, 6))
    for ax in range(3):
        L, invL = box[ax], 1.0 / box[ax]
        c = _image_fp(probe[:, ax], L, invL, mutate) - _image_fp(x[:, ax], L, invL, mutate)
        flags[:, 2 * ax], flags[:, 2 * ax + 1] = c < 0, c > 0
        contrib[:, 2 * ax] = m[types] * (-vm[:, ax])
        contrib[:, 2 * ax + 1] = m[types] * vm[:, ax]
        if wrap:
            x1[:, ax] = _wrap_fp(x1[:, ax], L, invL)
    contrib = np.where(flags, contrib, 0.0)
    fl, co, ty = flags[order], contrib[order], np.asarray(types)[order]
    if body == "two" and mutate == "second_atom_of_a_pair_lost":
        last_pair = N - (N % 2)
        fl[1:last_pair:2] = False
        co[1:last_pair:2] = 0.0
    spec = np.zeros((len(rM), 6), dtype=np.int64)
    for w in range(6):
        np.add.at(spec[:, w], ty[fl[:, w]], 1)
    per_wave, per_block = (64, 256) if body == "one" else (128, 512)
    cnt, mom = np.zeros(6, dtype=np.int64), np.zeros(6)
    for b in range(0, N, per_block):
        waves = range(b, min(b + per_block, N), per_wave)
        for q, w0 in enumerate(waves):
            if mutate == "only_wave_0_summed" and q > 0:
                continue
            cnt += fl[w0:w0 + per_wave].sum(0)
            mom += co[w0:w0 + per_wave].sum(0)
    return x1, vk, cnt, mom, spec


# ---- one step WITH forces, in longdouble (the kicked atoms of a liquid) --------------------------------------------------------------------------------
def one_step_ld(s0, s1, types, rM, m, frozen, box, dt, wrapped_input=True):
    """From two states an engine returned one step apart ({"x", "v", "f"}: (N, 3) float64): the velocity identity v1 = v0 + rM f0 + rM f1, the position identity
    x1 == x0 + (v0 + rM f0) dt (mod L), and what the rule decides for the step from x0, v0, f0.  Returns worst err / (TAU sum of the magnitudes of the terms)
    for v and x, the flags, the margin of every decision, and per wall the momentum with its scale."""
    x0, v0, f0, v1, f1, x1 = (np.asarray(a).astype(LD) for a in (s0["x"], s0["v"], s0["f"], s1["v"], s1["f"], s1["x"]))
    r, mm, fr = rM[types].astype(LD)[:, None], m[types].astype(LD), frozen[types]
    k0, k1 = r * f0, r * f1
    with np.errstate(invalid="ignore"):                            # (an atom at rest without a force: 0 / 0, no statement)
        rv = np.abs(v1 - (v0 + k0 + k1)) / (LD(TAU) * (np.abs(v0) + np.abs(k0) + np.abs(k1)))
    vh = v0 + k0
    d = np.where(fr[:, None], LD(0), vh * LD(dt))
    xu = x0 + d
    Lb = np.array(box).astype(LD)[None, :]
    dx = x1 - xu
    dx = dx - Lb * np.round(dx / Lb)
    rx = np.abs(dx) / (LD(TAU) * (np.abs(x0) + np.abs(d) + Lb))
    neg, pos = xu < 0, xu > Lb                                     # x0 is wrapped: image 0
    rem = xu - Lb * np.floor(xu / Lb)
    margin = np.minimum(rem, Lb - rem).astype(np.float64)
    flags = np.zeros((len(types), 6), dtype=bool)
    mom, scale = np.zeros(6, dtype=LD), np.zeros(6, dtype=LD)
    for ax in range(3):
        flags[:, 2 * ax], flags[:, 2 * ax + 1] = neg[:, ax], pos[:, ax]
        for w, sg in ((2 * ax, -1), (2 * ax + 1, 1)):
            hit = flags[:, w]
            mom[w] = (mm[hit] * (sg * vh[hit, ax])).sum()
            scale[w] = (mm[hit] * np.abs(vh[hit, ax])).sum()
    return {"v": float(np.nanmax(rv)), "x": float(rx.max()), "flags": flags, "margin": margin, "mom": mom, "mom_scale": scale}
