"""High-precision reference of one atom's step under the radiative thermostat (post_tstat_atom and its four launch forms, csrc/kernels.hip.h,
csrc/pair_list.hip.h), restated from user-level numbers only: the mass in the engine's units, the species' (radA, radB, mxEng), the photon energy, the
preset unit vector, the integer draws, revLight = 3.33567e-5, radFrac = 0.9, radThr = 1e-4, numPi = 3.14159, dt.  Forces are zero (tests/thermostat_cases.py).

One step, in the order the engine takes it:
  drift      x += v dt                  (the step's first stage; the half-kicks add exactly nothing)
  kinetic    1/2 m v^2 is booked BEFORE the thermostat (and before the equilibration factor)
  scaling    v *= k on an equilibration step, k = sqrt(0.25 tKin / E_kin)
  absorption ermc_abs = photon revLight / m,  v1 = v + ermc_abs u,  U_mid = U + photon + 1/2 m (v^2 - v1^2)
  emission   if U_mid > radThr: ph = radFrac U_mid, ermc_rad = ph revLight / m, e = ermc_rad / |v1|;
             e >= 1: d = -v1 / |v1|;  else cos_phi = r1 / 1024 (1 - e) - 1, theta = r2 / 1024 numPi and d = angled_vector(v1, cos_phi, theta), the basis
             (v2, v3) constructed literally as the kernel does, on the exact velocity;  v2 = v1 + ermc_rad d,  U = U_mid - (ph + 1/2 m (v2^2 - v1^2))
  radius     radA / (radB - min(U, mxEng))
Written twice: step() in numpy, for whole arrays, in numpy.longdouble (the chains of the tests) or in float64 (the restatement the mutations are applied
to); atom_step_mp() in mpmath at 50 digits, atom by atom (the committed fixture tests/golden/thermostat_atoms.npz).  The GPU test needs numpy only.

Condition scales - the bound on every quantity is |gpu - ref| <= TAU * scale with TAU = pair_cases.TAU and nothing else:
  velocity, per component   S_v = |v_c| + ermc_abs + ermc_rad kappa
      kappa = C0 + sin_phi kappa_b + C1 |cos_phi| / sin_phi      (C0 = 16, C1 = 4; the last term is 0 where r1 == 0: cos_phi == -1 exactly, sin_phi == 0 exactly)
      C0 covers the roundings of v1 / |v1|, of the two normalisations, of theta = r2 / 1024 numPi (up to 6.3: its rounding moves sin / cos by 6 eps) and of
      sin / cos themselves.  C1 |cos_phi| / sin_phi: cos_phi carries a few eps of absolute error, and sin_phi = sqrt(1 - cos_phi^2) turns d cos_phi into
      |cos_phi| / sin_phi d cos_phi.  kappa_b is the amplification of the basis construction, per branch of angled_vector (a = v1 / |v1|):
        branch 1 (a_x != 0): v2 = (-(a_y + a_z) / a_x, 1, 1).  Relative noise eps on a_y, a_z leaves eps (|a_y| + |a_z|) on the sum, whatever is left of it
          after the cancellation, and the division by a_x makes that eps (|a_y| + |a_z|) / |a_x| on v2_x; normalising divides by |v2|.  v3 = a x v2
          has |v3| = |v2| and takes the same noise through a_z v2_x and a_y v2_x, times |a_z|, |a_y| <= 1:
              kappa_b = 1 + (|a_y| + |a_z|) / (|a_x| |v2|)
          An entry (1e-10, 0.38, 0.92) gives v2_x ~ 1e10 = |v2|: kappa_b ~ 2, well-conditioned; (7e-14, -0.7071, 0.7071) gives |v2| ~ 1.4 and 1e13.
        branch 2 (a_x == 0, a_y != 0): v2 = (1, -a_z / a_y, 1), v3 = (a_y + a_z^2 / a_y, a_z, -a_y): one division, no cancellation (both terms of v3_x
          have the sign of a_y): kappa_b = 1
        branch 3 (a = (0, 0, +-1)): v2 = (1, 0, 0), v3 = (0, a_z, 0), exact: kappa_b = 1
      An atom with kappa > ILL = 1e-6 / TAU (its componentwise bound would exceed 1e-6 of ermc_rad) is ill-conditioned: it is held through the two
      invariants alone, and the tests cap the number of such atoms by the number designed to be so.
  invariants of the emission, for every emitting atom, without kappa_b: with dv = v_out - v1 (v1 from the reference),
      | |dv| - ermc_rad |  and  | dv . v1 / |v1| - ermc_rad cos_phi |  <=  TAU S_inv,   S_inv = |v| + ermc_abs + C0 ermc_rad
      (whatever the noise does to v2_x, the kernel's (a, v2 / |v2|, v3 / |v3|) is orthonormal to a few eps: a . v2 is the rounding of one sum, v3 is the
       cross product of the two)
  U        S_U = |U_in| + photon + 1/2 m (v^2 + v1^2) [+ ph + 1/2 m (v1^2 + v2^2) where it emits]: the ledger subtracts nearly equal squares
  radius   S_r = |r| + radA / (radB - min(U, mxEng))^2 S_U; an atom clearly in the clamp has the fp64 value of radA / (radB - mxEng) exactly
  position S_x = |x_c| + |v_c| dt; positions are compared modulo the box
Chains.  A call of n steps is held to the longdouble chain started from the state the engine returned before the call, and the bounds of the input
propagate as a SUM of per-step bounds, each carried through the later steps' sensitivities (first order, with |d(v . u)| <= sqrt(3) e_v):
      e_Umid = e_U + m ermc_abs sqrt(3) e_v;   e_ermc = radFrac revLight / m e_Umid;   e_a = 2 sqrt(3) e_v / |v1|;
      e_cos = 2 (e_ermc + e sqrt(3) e_v) / |v1|;   e_d = e_a (1 + kappa_b sin_phi) + e_cos (1 + |cos_phi| / sin_phi)      [e >= 1: e_d = e_a]
      e_v' = e_v + e_ermc + ermc_rad e_d + TAU max_c S_v;   e_U' = (1 - radFrac) e_Umid + m (e_ermc (|v1| + ermc_rad) + ermc_rad (sqrt(3) e_v + |v1| e_d)) + TAU S_U
      e_x' = e_x + e_v dt + TAU max_c S_x
An atom that is ill-conditioned at some step of a chain is left out of that chain's componentwise checks from there on (and counted against the cap).
Atoms that have slowed down to |v| ~ ermc_rad (the atoms at rest, the stopped ones, the slowest moving ones) are chaotic: every emission nearly stops them,
cos_phi -> -1, and the sensitivities above grow by an order of magnitude per step.  Where the propagated bound of an atom comes within RISK = 1e-2 of a
branch margin (|U_mid - radThr|, |e - 1|) no first-order bound holds any more and the chain does not judge that atom ("unbounded"); a chain may lose at
most CHAIN_LOSS = 5 % of the atoms that way (65 of 3000 in the 9-step chains of the tests), a single step none.
The no-tie margins of thermostat_cases keep fp64 and the reference on the same branches.
"""
import os

import numpy as np

import thermostat_cases as tc

LD = np.longdouble
TAU = tc.TAU
C0, C1 = 16.0, 4.0
ILL = 1e-6 / TAU
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thermostat_atoms.npz")
MUTATIONS = ("draws_2_and_3_swapped", "emission_draws_mod_3072", "cos_phi_without_minus_1", "pi_in_theta", "photon_index_without_step",
             "mass_of_species_0", "mxEng_of_species_0", "clamp_omitted", "draws_keyed_by_opening_step", "stop_branch_aims_at_plus_v")


def require_longdouble():
    assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended type on this machine"


def photon_table(seed=tc.SEED):
    """the model's photon energies for `seed` (host code of the library; no GPU needed)"""
    from aztotmd_amd import api
    return api.Model.from_case(tc.gas_case()).query("photons", seed=seed)


def species_arrays(dtype, mutate=None):
    tp = np.arange(tc.N) % 2
    tm = np.zeros_like(tp) if mutate == "mass_of_species_0" else tp
    tx = np.zeros_like(tp) if mutate == "mxEng_of_species_0" else tp
    m = tc.masses()[tm].astype(dtype)
    A, B = (np.array([r[k] for r in tc.RADII])[tp].astype(dtype) for k in (0, 1))
    MX = np.array([r[2] for r in tc.RADII])[tx].astype(dtype)
    return m, A, B, MX


def _norm(a):
    return np.sqrt((a * a).sum(1))


def step(x, v, U, step_no, photons, seed=tc.SEED, vscale=None, err=None, dtype=LD, mutate=None):
    """One step of all N atoms from (x, v, U) - arrays of any float type, taken exactly - at step number `step_no` (1-based: the number of the step
    being closed keys the draws).  Returns a dict: the new state, the intermediate values, the scales and the propagated bounds of the module text."""
    T = dtype
    N = tc.N
    ids = np.arange(N)
    x, v, U = np.asarray(x).astype(T), np.asarray(v).astype(T), np.asarray(U).astype(T)
    m, A, B, MX = species_arrays(T, mutate)
    rl, frac, thr, dt = T(tc.REV_LIGHT), T(tc.RAD_FRAC), T(tc.RAD_THR), T(tc.DT)
    npi = T(np.pi) if mutate == "pi_in_theta" else T(tc.NUM_PI)
    key = step_no + 1 if mutate == "draws_keyed_by_opening_step" else step_no
    uv = tc.unit_table()
    pe = np.asarray(photons)[(ids + (0 if mutate == "photon_index_without_step" else key)) % N].astype(T)
    mod = tc.N_UVECT if mutate == "emission_draws_mod_3072" else 2048
    r1, r2 = tc.draws(seed, key, ids, 2) % mod, tc.draws(seed, key, ids, 3) % mod
    if mutate == "draws_2_and_3_swapped":
        r1, r2 = r2, r1
    u = uv[tc.draws(seed, key, ids, 1) % tc.N_UVECT].astype(T)
    one, half = T(1), T(0.5)

    x1 = x + v * dt
    S_x = np.abs(x) + np.abs(v) * dt
    kin = half * m * (v * v).sum(1)
    v_pre = v
    if vscale is not None:
        v = v * T(vscale)
    v02 = (v * v).sum(1)
    ea = pe * rl / m
    va = v + ea[:, None] * u
    v12 = (va * va).sum(1)
    Umid = U + pe + half * m * (v02 - v12)
    emit = Umid > thr
    v0 = np.sqrt(v12)
    assert (v0[emit] > 0).all()                                   # (the kernel's v0 == 0 branch needs a photon of energy 0: not reachable)
    with np.errstate(divide="ignore", invalid="ignore"):
        ph = np.where(emit, frac * Umid, T(0))
        er = ph * rl / m
        e = np.where(emit, er / v0, T(0))
        stop = emit & (e >= one)
        cosphi = r1.astype(T) / T(1024) * (one - e)
        if mutate != "cos_phi_without_minus_1":
            cosphi = cosphi - one
        theta = r2.astype(T) / T(1024) * npi
        # angled_vector, literally
        a = va / v0[:, None]
        ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
        b1 = ax != 0
        b2 = ~b1 & (ay != 0)
        zero = np.zeros(N, dtype=T)
        w2 = np.stack([np.where(b1, -(ay + az) / ax, one), np.where(b1, one, np.where(b2, -az / ay, zero)), np.where(b1 | b2, one, zero)], 1)
        w3 = np.stack([ay * w2[:, 2] - az * w2[:, 1], -ax * w2[:, 2] + az * w2[:, 0], ax * w2[:, 1] - ay * w2[:, 0]], 1)
        l2, l3 = _norm(w2), _norm(w3)
        n2, n3 = w2 / l2[:, None], w3 / l3[:, None]
        sinphi = np.sqrt(one - cosphi * cosphi)
        d = a * cosphi[:, None] + sinphi[:, None] * (np.cos(theta)[:, None] * n2 + np.sin(theta)[:, None] * n3)
        d = np.where(stop[:, None], (a if mutate == "stop_branch_aims_at_plus_v" else -a), d)
        kb = np.where(b1, one + (np.abs(ay) + np.abs(az)) / (np.abs(ax) * l2), one)
        ctg = np.where(sinphi > 0, np.abs(cosphi) / sinphi, T(0))
    cosphi = np.where(stop | ~emit, -one, cosphi)
    sinphi = np.where(stop | ~emit, T(0), sinphi)
    kb = np.where(stop | ~emit, one, kb)
    ctg = np.where(stop | ~emit, T(0), ctg)
    kappa = T(C0) + sinphi * kb + T(C1) * ctg
    d = np.where(emit[:, None], d, T(0))
    vout = va + er[:, None] * d
    v22 = (vout * vout).sum(1)
    Uout = np.where(emit, Umid - (ph + half * m * (v22 - v12)), Umid)
    clamp = ~(Uout < MX)
    restr = Uout if mutate == "clamp_omitted" else np.where(clamp, MX, Uout)
    rad = A / (B - restr)
    slope = A / ((B - restr) * (B - restr))

    S_v = np.abs(v) + (ea + er * kappa)[:, None]
    S_inv = np.sqrt(v02) + ea + T(C0) * er
    S_U = np.abs(U) + pe + half * m * (v02 + v12) + np.where(emit, ph + half * m * (v12 + v22), T(0))
    S_r = np.abs(rad) + slope * S_U
    with np.errstate(divide="ignore", invalid="ignore"):
        tie_thr = np.abs(Umid - thr) / thr
        tie_stop = np.where(emit, np.abs(e - one), one)

    # propagated bounds (module text)
    if err is None:
        err = {"v": np.zeros(N, dtype=T), "U": np.zeros(N, dtype=T), "x": np.zeros(N, dtype=T)}
    sq3 = np.sqrt(T(3))
    ev = err["v"] * (T(vscale) if vscale is not None else one)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_Umid = err["U"] + m * ea * sq3 * ev
        e_er = np.where(emit, frac * rl / m * e_Umid, T(0))
        e_a = 2 * sq3 * ev / v0
        e_cos = 2 * (e_er + e * sq3 * ev) / v0
        e_d = np.where(stop, e_a, e_a * (one + kb * sinphi) + e_cos * (one + ctg))
        P_v = np.where(emit, ev + e_er + er * e_d, ev)
        P_U = np.where(emit, (one - frac) * e_Umid + m * (e_er * (v0 + er) + er * (sq3 * ev + v0 * e_d)), e_Umid)
    P_x = err["x"] + err["v"] * dt
    tau = T(TAU)
    new_err = {"v": P_v + tau * S_v.max(1), "U": P_U + tau * S_U, "x": P_x + tau * S_x.max(1)}
    rel_in = np.where(emit, e_Umid / np.abs(Umid - thr) + (e_er + e * sq3 * ev) / v0 / np.maximum(tie_stop, T(1e-300)), e_Umid / np.abs(Umid - thr))
    return {"x": x1, "v": vout, "U": Uout, "rad": rad, "v_in": v_pre, "v_abs": va, "v0": v0, "ermc_abs": ea, "ermc_rad": er, "cos_phi": cosphi, "U_mid": Umid,
            "emit": emit, "stop": stop, "clamp": clamp, "branch": np.where(b1, 1, np.where(b2, 2, 3)), "kappa": kappa, "ill": emit & ~stop & (kappa > ILL),
            "kin": kin, "S_v": S_v, "S_inv": S_inv, "S_U": S_U, "S_r": S_r, "S_x": S_x, "slope": slope, "MX": MX, "A": A, "B": B,
            "tie_thr": tie_thr, "tie_stop": tie_stop, "e_v_in": err["v"], "P_v": P_v, "P_U": P_U, "P_x": P_x, "err": new_err, "branch_risk": rel_in, "step": step_no}


RISK = 0.01                                                       # a propagated bound above this fraction of a branch margin: the first-order bound ends there
CHAIN_LOSS = 0.05                                                 # at most this fraction of the atoms may be lost to that in a chain


def chain(x, v, U, first_step, n, photons, seed=tc.SEED, vscale_at=None, dtype=LD):
    """n steps from (x, v, U), the first numbered `first_step`; vscale_at: {step number: factor}.  Returns the last step's result with the bounds of the
    whole chain in it, "ill_ever" (ill-conditioned at some step), "unbounded" (the propagated bound of the atom came within RISK of a branch margin at
    some step: an atom that has slowed down to |v| ~ ermc_rad, where cos_phi -> -1 and 1 / sin_phi amplify every step; no first-order bound holds
    for it from there on, so the chain does not judge it) and the smallest no-tie margins met."""
    err, ill, lost, ties = None, np.zeros(tc.N, dtype=bool), np.zeros(tc.N, dtype=bool), [np.inf, np.inf]
    for s in range(first_step, first_step + n):
        r = step(x, v, U, s, photons, seed, (vscale_at or {}).get(s), err, dtype)
        x, v, U, err = r["x"], r["v"], r["U"], r["err"]
        ill |= r["ill"]
        lost |= ~(r["branch_risk"] < RISK)
        ties = [min(ties[0], float(r["tie_thr"].min())), min(ties[1], float(r["tie_stop"].min()))]
    r["ill_ever"], r["unbounded"], r["ties"], r["n"] = ill, lost & ~ill, ties, n
    return r


def compare(ref, got, box=tc.L, only=None):
    """Every quantity of the state `got` ({"x": (N, 3), "v": (N, 3), "U", "rad"} in fp64) against a step or chain result: {quantity: (worst err / bound
    over the atoms it applies to, index of that atom)}, bound = TAU * scale + what the chain propagated, and the number of ill-conditioned atoms.
    Ill-conditioned atoms are held through the invariants (one step) or left out (chain: the invariants need the state before the last emission)."""
    tau = LD(TAU)
    ill = ref.get("ill_ever", ref["ill"])
    lost = ref.get("unbounded", np.zeros(tc.N, dtype=bool))
    ok = ~ill & ~lost
    sel = np.ones(tc.N, dtype=bool) if only is None else np.asarray(only)
    single = ref.get("n", 1) == 1
    gv, gU, gr, gx = (np.asarray(got[k]).astype(LD) for k in ("v", "U", "rad", "x"))
    out = {}

    def worst(name, errs, bound, mask):
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(errs == 0, LD(0), errs / bound)
        ratio = np.where(np.isfinite(errs), ratio, LD(np.inf))        # (a NaN is beyond every bound)
        ratio = np.where(mask & (sel if mask.ndim == 1 else sel[:, None]), ratio, LD(0))
        assert not np.isnan(ratio).any(), name
        flat = int(np.argmax(ratio))
        out[name] = (float(ratio.flat[flat]), flat // (ratio.size // tc.N))

    worst("v", np.abs(gv - ref["v"]), tau * ref["S_v"] + ref["P_v"][:, None], ok[:, None] & np.ones((1, 3), dtype=bool))
    if single:
        dv = gv - ref["v_abs"]
        em = ref["emit"]
        with np.errstate(divide="ignore", invalid="ignore"):
            along = (dv * ref["v_abs"]).sum(1) / ref["v0"]
        bound = tau * ref["S_inv"] + np.sqrt(LD(3)) * ref["P_v"]
        worst("|dv_rad|", np.abs(_norm(dv) - ref["ermc_rad"]), bound, em)
        worst("dv_rad.v", np.abs(np.where(em, along, LD(0)) - ref["ermc_rad"] * ref["cos_phi"]), bound, em)
        worst("U_dark", np.abs(gU - ref["U"]), tau * ref["S_U"] + ref["P_U"], ~em)
        sure = ref["clamp"] & (ref["U"] - ref["MX"] > tau * ref["S_U"] + ref["P_U"])
        exact = (ref["A"].astype(np.float64) / (ref["B"].astype(np.float64) - ref["MX"].astype(np.float64)))
        out["clamped_radius_exact"] = (float((np.asarray(got["rad"])[sure] != exact[sure]).sum()), int(sure.sum()))
    every = np.ones(tc.N, dtype=bool) if single else ok           # (U, radius and position of one step do not depend on the basis)
    worst("U", np.abs(gU - ref["U"]), tau * ref["S_U"] + ref["P_U"], every)
    worst("radius", np.abs(gr - ref["rad"]), tau * ref["S_r"] + ref["slope"] * ref["P_U"], every)
    dx = gx - ref["x"]
    dx = dx - LD(box) * np.round(dx / LD(box))
    worst("x", np.abs(dx), tau * ref["S_x"] + ref["P_x"][:, None], (np.ones(tc.N, dtype=bool) if single else ok)[:, None] & np.ones((1, 3), dtype=bool))
    out["n_ill"], out["n_unbounded"] = int(ill.sum()), int(lost.sum())
    return out


def energy_ratios(ref, eng_kin, eng_temp, scaled_to=None):
    """(engKin, engTemp) against the sums of the last step: err / (TAU * sum |terms| + what the chain propagated).  engKin is the kinetic energy BEFORE
    the thermostat; on an equilibration step the engine reports tKin instead (engKin := tKin), passed as `scaled_to`."""
    tau = LD(TAU)
    if scaled_to is None:
        m = species_arrays(LD)[0]
        bound = tau * np.abs(ref["kin"]).sum() + (m * _norm(ref["v_in"]) * np.sqrt(LD(3)) * ref["e_v_in"]).sum()
        rk = abs(LD(eng_kin) - ref["kin"].sum()) / bound
    else:
        rk = abs(LD(eng_kin) - LD(scaled_to)) / (tau * abs(LD(scaled_to)))
    rt = abs(LD(eng_temp) - ref["U"].sum()) / (tau * np.abs(ref["U"]).sum() + ref["P_U"].sum())
    return float(rk), float(rt)


# ---- the forms the tests run, on any engine (the GPU engine, the CPU oracle) -------------------------------------------------------------------
COUNTS = ("n_ill", "n_unbounded", "clamped_radius_exact")


def stack(s, rad_key="radius"):
    """state dict of api.Engine.state() / oracle.Oracle.state() -> {"x", "v", "U", "rad", "f"}"""
    return {"x": np.stack([s["x"], s["y"], s["z"]], 1), "v": np.stack([s["vx"], s["vy"], s["vz"]], 1), "U": np.asarray(s["U"]),
            "rad": np.asarray(s[rad_key] if rad_key in s else s["rad"]), "f": np.stack([s["fx"], s["fy"], s["fz"]], 1)}


def designed_state(photons, seed=tc.SEED):
    v, U, cls = tc.assign(photons, seed)
    return {"x": tc.positions(), "v": v, "U": U}, cls


def ill_cap(cls):
    """the atoms designed to be ill-conditioned: the cancelling and the tiny-|x| classes"""
    return int(((cls == "cancel") | (cls == "tiny")).sum())


def run_calls(eng, photons, calls, start, cls, vscale_for=None, label="", check_first=None, after_call=None):
    """Drive `eng` (step(n), state() -> stack()-able dict, energies() -> (engKin, engTemp)) through `calls` = [n_steps, ...] from the exact fp64 state
    `start` at step 0, each call held to the longdouble chain from the state the previous call returned.  vscale_for(step, state_before_call) gives the
    equilibration factor of a step or None; after_call(steps done before, steps of the call) runs right behind the call (kernel timers); check_first(reference,
    state) after the first.  Prints every figure, then asserts; returns {quantity: worst ratio}."""
    prev, done, worst = start, 0, {}
    for n in calls:
        vs = {}
        if vscale_for is not None:
            for s in range(done + 1, done + n + 1):
                k = vscale_for(s, prev)
                if k is not None:
                    assert s == done + 1, "an equilibration step must open its call: its factor is restated from the state before the call"
                    vs[s] = k
        ref = chain(prev["x"], prev["v"], prev["U"], done + 1, n, photons, vscale_at=vs)
        eng.step(n)
        if after_call is not None:
            after_call(done, n)
        got = stack(eng.state())
        assert (got["f"] == 0.0).all(), (label, "forces are not exactly 0")
        res = compare(ref, got)
        last_scaled = (done + n) in vs
        rk, rt = energy_ratios(ref, *eng.energies(), scaled_to=tc.t_kin() if last_scaled else None)
        res["engKin"], res["engTemp"] = (rk, -1), (rt, -1)
        print("%s steps %d..%d: " % (label, done + 1, done + n) + "  ".join("%s %.3e" % (k, v[0]) for k, v in res.items() if k not in COUNTS)
              + "  ill-conditioned %d (cap %d)  unbounded %d  no-tie margins %.1e %.1e" % (res["n_ill"], ill_cap(cls), res["n_unbounded"], ref["ties"][0], ref["ties"][1]))
        assert ref["ties"][0] >= tc.TIE_MARGIN and ref["ties"][1] >= tc.TIE_MARGIN, (label, ref["ties"])
        assert res["n_unbounded"] <= (0 if n == 1 else CHAIN_LOSS * tc.N), (label, "atoms whose propagated bound comes near a branch", res["n_unbounded"])
        assert res["n_ill"] <= ill_cap(cls), (label, res["n_ill"], ill_cap(cls))
        if done > 0:
            assert res["n_ill"] == 0, (label, "only the atoms at rest of step 1 are designed to be ill-conditioned", res["n_ill"])
        for k, val in res.items():
            if k in ("n_ill", "n_unbounded"):
                continue
            if k == "clamped_radius_exact":
                assert val[0] == 0 and (done > 0 or val[1] >= tc.MIN_PER_CLASS), (label, k, val)
                continue
            assert val[0] <= 1.0, (label, "steps %d..%d" % (done + 1, done + n), k, "atom %d" % val[1], val[0])
            worst[k] = max(worst.get(k, 0.0), val[0])
        if check_first is not None and done == 0:
            check_first(ref, got)
        prev, done = got, done + n
    return worst


# ---- mpmath, atom by atom -----------------------------------------------------------------------------------------------------------------------
def atom_step_mp(x, v, U, m, radii, pe, u, r1, r2, dt=tc.DT, vscale=None):
    """One atom's step at 50 digits from exact fp64 inputs; the values and scales of step(), as mpmath numbers"""
    import mpmath as mp
    with mp.workdps(50):
        f = mp.mpf
        x, v, u = [f(float(c)) for c in x], [f(float(c)) for c in v], [f(float(c)) for c in u]
        U, m, pe, dt = f(float(U)), f(float(m)), f(float(pe)), f(float(dt))
        A, B, MX = (f(float(c)) for c in radii)
        rl, frac, thr, npi = f(tc.REV_LIGHT), f(tc.RAD_FRAC), f(tc.RAD_THR), f(tc.NUM_PI)
        dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
        x1 = [x[k] + v[k] * dt for k in range(3)]
        S_x = [abs(x[k]) + abs(v[k]) * dt for k in range(3)]
        kin = m * dot(v, v) / 2
        if vscale is not None:
            v = [c * f(vscale) for c in v]
        v02 = dot(v, v)
        ea = pe * rl / m
        va = [v[k] + ea * u[k] for k in range(3)]
        v12 = dot(va, va)
        Umid = U + pe + m * (v02 - v12) / 2
        emit = Umid > thr
        v0 = mp.sqrt(v12)
        er, ph, cosphi, kappa, stop, branch = f(0), f(0), f(-1), f(C0), False, 0
        vout = list(va)
        if emit:
            ph = frac * Umid
            er = ph * rl / m
            e = er / v0
            a = [c / v0 for c in va]
            if e >= 1:
                stop, d = True, [-c for c in a]
            else:
                cosphi = f(int(r1)) / 1024 * (1 - e) - 1
                theta = f(int(r2)) / 1024 * npi
                kb = f(1)
                if a[0] != 0:
                    branch = 1
                    w2 = [-(a[1] * 1 + a[2] * 1) / a[0], f(1), f(1)]
                elif a[1] != 0:
                    branch = 2
                    w2 = [f(1), -(a[2] * 1) / a[1], f(1)]
                else:
                    branch = 3
                    w2 = [f(1), f(0), f(0)]
                w3 = [a[1] * w2[2] - a[2] * w2[1], -a[0] * w2[2] + a[2] * w2[0], a[0] * w2[1] - a[1] * w2[0]]
                l2, l3 = mp.sqrt(dot(w2, w2)), mp.sqrt(dot(w3, w3))
                if branch == 1:
                    kb = 1 + (abs(a[1]) + abs(a[2])) / (abs(a[0]) * l2)
                sinphi = mp.sqrt(1 - cosphi * cosphi)
                ct, st = mp.cos(theta), mp.sin(theta)
                d = [a[k] * cosphi + sinphi * (ct * w2[k] / l2 + st * w3[k] / l3) for k in range(3)]
                kappa = C0 + sinphi * kb + (C1 * abs(cosphi) / sinphi if sinphi > 0 else 0)
            vout = [va[k] + er * d[k] for k in range(3)]
        v22 = dot(vout, vout)
        Uout = Umid - (ph + m * (v22 - v12) / 2) if emit else Umid
        restr = Uout if Uout < MX else MX
        rad = A / (B - restr)
        S_v = [abs(v[k]) + ea + er * kappa for k in range(3)]
        S_U = abs(U) + pe + m * (v02 + v12) / 2 + ((ph + m * (v12 + v22) / 2) if emit else 0)
        return {"x": x1, "v": vout, "U": Uout, "rad": rad, "v_abs": va, "ermc_rad": er, "cos_phi": cosphi, "kappa": kappa, "kin": kin, "S_x": S_x, "S_v": S_v,
                "S_U": S_U, "S_r": abs(rad) + A / (B - restr) ** 2 * S_U, "S_inv": mp.sqrt(v02) + ea + C0 * er, "emit": emit, "stop": stop, "branch": branch,
                "clamp": not (Uout < MX)}


def mp_inputs(i, state, step_no, photons, seed=tc.SEED):
    """the user-level numbers of atom i at step `step_no`: arguments of atom_step_mp"""
    tp = i % 2
    uv = tc.unit_table()
    return dict(x=state["x"][i], v=state["v"][i], U=state["U"][i], m=tc.masses()[tp], radii=tc.RADII[tp], pe=photons[(i + step_no) % tc.N],
                u=uv[tc.rng_draw(seed, step_no, i, 1) % tc.N_UVECT], r1=tc.rng_draw(seed, step_no, i, 2) % 2048, r2=tc.rng_draw(seed, step_no, i, 3) % 2048)


def to_ld(vals):
    """mpmath numbers -> longdouble array (through hi + lo pairs of float64: 106 bits, more than longdouble holds)"""
    hi, lo = split2(vals)
    return hi.astype(LD) + lo.astype(LD)


def split2(vals):
    """mpmath numbers -> (hi, lo) float64 arrays, hi + lo carrying 106 bits"""
    import mpmath as mp
    hi = np.array([float(c) for c in vals])
    lo = np.array([float(c - mp.mpf(float(h))) for c, h in zip(vals, hi)])
    return hi, lo


VECTORS = ("x", "v", "v_abs", "S_v", "S_x")
SCALARS = ("U", "rad", "ermc_rad", "cos_phi", "kappa", "S_U", "S_r", "S_inv")
HI_ONLY = ("S_v", "S_x", "kappa", "S_U", "S_r", "S_inv")        # scales: fp64 is enough
_MP = {}


def mp_rows(atoms, state, photons):
    """atom_step_mp of step 1 for the given atoms of the designed state (kept: the agreement test and the fixture share them)"""
    for i in atoms:
        if int(i) not in _MP:
            _MP[int(i)] = atom_step_mp(**mp_inputs(int(i), state, 1, photons))
    return [_MP[int(i)] for i in atoms]


def chosen_atoms(state, cls, at_rest=None, per_class=24):
    """designed atoms of every kind: the first `at_rest` atoms at rest of the x0 and tiny classes (None: all) and every one of the z and cancel classes,
    the first `per_class` of every other class, 8 moving atoms with a velocity component of exactly 0, the last 16 ids (the photon index wraps)"""
    pick = set(range(tc.N - 16, tc.N)) | set(np.flatnonzero(np.isin(cls, ("z", "cancel"))).tolist())
    for k in ("x0", "tiny"):
        pick |= set(np.flatnonzero(cls == k)[:at_rest].tolist())
    for k in ("moving", "dark", "stop", "clamp", "below"):
        pick |= set(np.flatnonzero(cls == k)[:per_class].tolist())
    pick |= set(np.flatnonzero((cls == "moving") & (state["v"] == 0).any(1))[:8].tolist())
    return np.array(sorted(pick), dtype=np.int32)


def fixture_atoms(state, cls):
    return chosen_atoms(state, cls, at_rest=24, per_class=12)


def rows_as_arrays(rows):
    """{quantity: longdouble array over the rows} + "flags" (emit, stop, clamp, branch of angled_vector or 0)"""
    out = {k: np.stack([to_ld([r[k][c] for r in rows]) for c in range(3)], 1) for k in VECTORS}
    out.update({k: to_ld([r[k] for r in rows]) for k in SCALARS})
    out["flags"] = np.array([[r["emit"], r["stop"], r["clamp"], r["branch"]] for r in rows], dtype=np.int8)
    return out


def make_fixture(path=None):
    """tests/golden/thermostat_atoms.npz: for the atoms of fixture_atoms() their designed (x, v, U), the photon of step 1, and step 1 at 50 digits - values as
    hi + lo pairs of float64, scales in float64"""
    photons = photon_table()
    state, cls = designed_state(photons)
    atoms = fixture_atoms(state, cls)
    rows = mp_rows(atoms, state, photons)
    arrays = {"seed": np.int64(tc.SEED), "atoms": atoms, "in_x": state["x"][atoms], "in_v": state["v"][atoms], "in_U": state["U"][atoms],
              "photon": np.asarray(photons)[(atoms + 1) % tc.N], "flags": np.array([[r["emit"], r["stop"], r["clamp"], r["branch"]] for r in rows], dtype=np.int8)}
    for k in VECTORS:
        for c in range(3):
            hi, lo = split2([r[k][c] for r in rows])
            arrays["%s%d_hi" % (k, c)] = hi
            if k not in HI_ONLY:
                arrays["%s%d_lo" % (k, c)] = lo
    for k in SCALARS:
        hi, lo = split2([r[k] for r in rows])
        arrays[k + "_hi"] = hi
        if k not in HI_ONLY:
            arrays[k + "_lo"] = lo
    if path:
        np.savez_compressed(path, **arrays)
    return arrays


_FIX = None


def fixture():
    """the committed fixture; values recombined in longdouble (hi + lo)"""
    global _FIX
    if _FIX is None:
        z = dict(np.load(FIXTURE))
        out = {k: z[k] for k in ("seed", "atoms", "in_x", "in_v", "in_U", "photon", "flags")}
        part = lambda name: z[name + "_hi"].astype(LD) + (z[name + "_lo"].astype(LD) if name + "_lo" in z else LD(0))
        for k in VECTORS:
            out[k] = np.stack([part("%s%d" % (k, c)) for c in range(3)], 1)
        for k in SCALARS:
            out[k] = part(k)
        _FIX = out
    return _FIX


def fixture_matches(state, photons):
    """the committed inputs are the designed ones"""
    F = fixture()
    at = F["atoms"]
    return (int(F["seed"]) == tc.SEED and np.array_equal(F["in_x"], state["x"][at]) and np.array_equal(F["in_v"], state["v"][at])
            and np.array_equal(F["in_U"], state["U"][at]) and np.array_equal(F["photon"], np.asarray(photons)[(at + 1) % tc.N]))


def against_rows(ref, atoms, R):
    """a longdouble step-1 result against 50-digit values R (rows_as_arrays or fixture()) of `atoms`: worst |ld - mp| / scale per quantity, the scales
    against each other relatively (those that carry kappa: on the well-conditioned atoms)"""
    at = np.asarray(atoms)
    out = {}
    for k, s in (("v", "S_v"), ("x", "S_x"), ("v_abs", "S_v"), ("U", "S_U"), ("rad", "S_r"), ("ermc_rad", "S_inv")):
        out[k] = float((np.abs(ref[k][at] - R[k]) / R[s]).max())
    out["cos_phi"] = float(np.abs(ref["cos_phi"][at] - R["cos_phi"]).max())
    well = ~ref["ill"][at]
    for k in ("S_U", "S_r", "S_inv", "S_x"):
        out[k + " (relative)"] = float((np.abs(ref[k][at] - R[k]) / np.maximum(R[k], LD(1e-300))).max())
    for k in ("kappa", "S_v"):
        out[k + " (relative, well-conditioned)"] = float((np.abs(ref[k][at] - R[k]) / R[k])[well].max())
    flags = np.stack([ref["emit"][at], ref["stop"][at], ref["clamp"][at], np.where(ref["emit"][at] & ~ref["stop"][at], ref["branch"][at], 0)], 1).astype(np.int8)
    assert np.array_equal(flags, R["flags"]), "the longdouble step takes other branches than the 50-digit one"
    return out


def hold_to_fixture(got):
    """an engine's state after step 1 against the 50-digit values of the fixture's atoms: {quantity: worst err / (TAU scale)}; velocities of the
    well-conditioned atoms componentwise, the two invariants for every emitting atom"""
    F = fixture()
    at = F["atoms"]
    tau = LD(TAU)
    gv, gU, gr, gx = (np.asarray(got[k])[at].astype(LD) for k in ("v", "U", "rad", "x"))
    well = ~(F["flags"][:, 0].astype(bool) & ~F["flags"][:, 1].astype(bool) & (F["kappa"] > ILL))
    em = F["flags"][:, 0].astype(bool)
    dv = gv - F["v_abs"]
    v0 = _norm(F["v_abs"])
    dx = gx - F["x"]
    dx = dx - LD(tc.L) * np.round(dx / LD(tc.L))
    return {"v": float((np.abs(gv - F["v"]) / (tau * F["S_v"]))[well].max()), "U": float((np.abs(gU - F["U"]) / (tau * F["S_U"])).max()),
            "radius": float((np.abs(gr - F["rad"]) / (tau * F["S_r"])).max()), "x": float((np.abs(dx) / (tau * F["S_x"])).max()),
            "|dv_rad|": float((np.abs(_norm(dv) - F["ermc_rad"]) / (tau * F["S_inv"]))[em].max()),
            "dv_rad.v": float((np.abs((dv * F["v_abs"]).sum(1) / v0 - F["ermc_rad"] * F["cos_phi"]) / (tau * F["S_inv"]))[em].max())}
