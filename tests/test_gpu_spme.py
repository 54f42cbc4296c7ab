"""GPU tests of 'elec spme' (csrc/spme.hip.h) against tests/spme_model.py, stage by stage: a failure names its kernel.

  integer mesh   k_spme_spread      against the long-double Q 2^40: |d| <= 0.51 c(g) + 1, c(g) the contributions at g
  spectrum       k_spme_fft         against numpy.fft.fftn of the device's own mesh: max |d| <= TAU sum |Q|
  phi            convolve + inverse against the same from the device's own spectrum and G: max |d| <= TAU scale sum |G FQ|
  G              host, long double  against the model to 2 ulp
  forces, energy k_spme_gather ...  against the fp64 route of the model within BOUND_F S_F,i / BOUND_E S_E (four times what tests/test_spme_model.py
                                    measures between the model's two routes; both exceed TAU because the mesh is quantised to 2^-40 e)
Atoms of the isolated systems lie farther apart than rReal: forces() is the reciprocal part alone.
"""
import os
import subprocess

import numpy as np
import pytest

import ewald_reference as er
import pair_cases as pc
import spme_model as sm
from aztotmd_amd import api, inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPME_KERNELS = ("spme_spread", "spme_fft_fwd", "spme_convolve", "spme_fft_inv", "spme_gather")
LD = np.longdouble


def evaluate(case, meshes=False, **opts):
    """one force evaluation: forces (N, 3), stats, kernel timers of that evaluation [, the meshes and G]"""
    e = api.Engine(api.Model.from_case(case), profile=1, **opts)
    e.reset_kernel_times()
    e.forces()
    kt = e.kernel_times()
    st, stats = e.state(), e.stats()
    out = {"F": np.stack([st["fx"], st["fy"], st["fz"]], 1), "stats": stats, "kt": kt}
    if meshes:
        out.update(Qi=e.spme_mesh("charge"), FQ=e.spme_mesh("spectrum"), phi=e.spme_mesh("potential"), G=e.spme_influence())
        st2 = e.state()                                         # the read-back runs the stages again: it must not touch the forces
        assert all(np.array_equal(st[k], st2[k]) for k in ("fx", "fy", "fz")) and e.stats()["engCoulRec"] == stats["engCoulRec"]
        assert np.array_equal(e.spme_mesh("charge"), out["Qi"])                 # ... and leaves the integer mesh clear for the next evaluation
    e.close()
    return out


def hold_stages(name, case, r):
    ld, f64 = sm.spme(case, "ld"), sm.spme(case, "fp64")
    for k in SPME_KERNELS:
        assert k in r["kt"] and r["kt"][k]["calls"] == 1, (name, k, {a: b["calls"] for a, b in r["kt"].items()})
    assert r["stats"]["engCoul"] == 0.0 and r["stats"]["engVdW"] == 0.0
    # integer mesh
    dq = np.abs(r["Qi"].astype(LD) - ld["Q"] * LD(sm.FIX))
    assert (dq <= 0.51 * ld["count"] + 1).all(), (name, "integer mesh", float((dq - 0.51 * ld["count"]).max()))
    assert (r["Qi"][ld["count"] == 0] == 0).all()
    # spectrum of the device's own mesh
    q0 = r["Qi"].astype(np.float64) / sm.FIX
    dFQ = float(np.abs(r["FQ"] - np.fft.fftn(q0)).max() / np.abs(q0).sum())
    # phi from the device's own spectrum and G
    scale = float(ld["scale"])
    mine = np.fft.ifftn(scale * r["G"] * r["FQ"]) * r["G"].size
    dphi = float(np.abs(r["phi"] - mine).max() / (scale * np.abs(r["G"] * r["FQ"]).sum()))
    # G
    G64 = ld["G"].astype(np.float64)
    ulps = float((np.abs(r["G"] - G64) / np.maximum(np.spacing(np.abs(G64)), 5e-324)).max())
    rF, rE = sm.worst_ratios(r["F"], r["stats"]["engCoulRec"], f64)
    print("%s: mesh == fp64 model's: %s   spectrum %.3e sum|Q|   phi %.3e scale sum|G FQ|   G %.1f ulp   forces %.3e S_F   energy %.3e S_E"
          % (name, np.array_equal(r["Qi"], f64["Qint"]), dFQ, dphi, ulps, rF, rE))
    assert dFQ <= pc.TAU, (name, "spectrum", dFQ)
    assert dphi <= pc.TAU, (name, "phi", dphi)
    assert ulps <= 2.0 and r["G"][0, 0, 0] == 0.0, (name, "G", ulps)
    assert np.isfinite(r["F"]).all() and (r["F"][er.charges(case) == 0.0] == 0.0).all()
    assert rF <= sm.BOUND_F, (name, "forces", rF)
    assert rE <= sm.BOUND_E, (name, "energy", rE)
    assert abs(r["stats"]["engCoulConst"]) > 0.0
    return ld


@pytest.mark.parametrize("name", list(sm.ISOLATED))
def test_isolated_systems_stage_by_stage(name):
    case = sm.isolated_case(name)
    hold_stages(name, case, evaluate(case, meshes=True))


def test_forces_against_the_converged_plain_sum():
    """the box the discretisation error was measured on (tests/test_spme_model.py), 32^3 / p = 6: within four times that"""
    base = sm.jittered_rocksalt()
    assert er.min_image_distance(base) > base["rReal"]
    ref = sm.converged_plain_sum(base)
    for K, order in ((32, 6), (32, 8)):
        r = evaluate(sm.as_spme(base, (K, K, K), order))
        err = sm.rel_rms(r["F"], ref["F"])
        print("%d^3 / %d: relative rms force error against the plain sum %.3e (model: %.3e)" % (K, order, err, sm.DISCRETISATION[(K, order)]))
        assert r["stats"]["engCoul"] == 0.0 and err <= 4 * sm.DISCRETISATION[(K, order)]


@pytest.mark.parametrize("name", ["n65a", "n769b", "n4097"])
def test_bitwise_between_handles_and_under_permutation(name):
    case = sm.isolated_case(name)
    a, b = evaluate(case, meshes=True), evaluate(case, meshes=True)
    assert np.array_equal(a["Qi"], b["Qi"]) and np.array_equal(a["F"], b["F"]) and a["stats"]["engCoulRec"] == b["stats"]["engCoulRec"] != 0.0
    assert np.array_equal(a["FQ"], b["FQ"]) and np.array_equal(a["phi"], b["phi"])
    N = len(case["types"])
    perm = np.random.Generator(np.random.PCG64(11)).permutation(N)
    pcase = dict(case)
    for k in ("types", "x", "y", "z", "vx", "vy", "vz"):
        pcase[k] = np.ascontiguousarray(np.asarray(case[k])[perm])
    p = evaluate(pcase, meshes=True)
    assert np.array_equal(p["Qi"], a["Qi"])                     # integer sums: the order the atoms arrive in cannot show (float atomics would)
    assert p["stats"]["engCoulRec"] == a["stats"]["engCoulRec"] and np.array_equal(p["F"], a["F"][perm])
    SF = sm.spme(case, "fp64")["SF"][perm]
    d = np.linalg.norm((p["F"] - a["F"][perm]).astype(LD), axis=1)
    assert (d <= 2 * pc.TAU * SF).all()


def coulomb(stats):
    return stats["engCoul"] + stats["engCoulRec"] + stats["engCoulConst"]


@pytest.mark.parametrize("K, order", [(32, 6), (64, 8)])
def test_madelung_constant_through_the_engine(K, order):
    case = sm.as_spme(er.rocksalt_case(), (K, K, K), order)
    r = evaluate(case)
    assert set(SPME_KERNELS) <= {k for k, v in r["kt"].items() if v["calls"] > 0}
    e = coulomb(r["stats"])
    expect = -1.7475645946 * pc.FCOUL / 2.82 * (len(case["types"]) / 2)
    rel = abs(e - expect) / abs(expect)
    print("rock salt %d^3 / %d: E = %.12e, -M k q^2 / r0 N / 2 = %.12e, relative difference %.3e" % (K, order, e, expect, rel))
    assert rel <= 4 * sm.MADELUNG[(K, order)]
    assert np.abs(r["F"]).max() < 1e-4                          # a perfect lattice is force-free


def test_total_coulomb_energy_at_two_alphas():
    d = er.dense_case()
    ea, eb = (coulomb(evaluate(sm.as_spme(d, (32, 32, 32), 8, alpha=al))["stats"]) for al in (0.45, 0.40))
    print("dense_case: E(alpha 0.45) = %.10e, E(alpha 0.40) = %.10e, relative difference %.3e" % (ea, eb, abs(ea - eb) / abs(ea)))
    assert abs(ea - eb) <= 4 * sm.TWO_ALPHA * abs(ea)
    model = sm.coulomb_total_model(sm.as_spme(d, (32, 32, 32), 8, alpha=0.45), "fp64")
    assert abs(ea - model["total"]) <= 1e-9 * abs(ea)           # (the real-space sum of the model is plain fp64)


# ---- dynamics ---------------------------------------------------------------------------------------------------------------------------------
def run(case, steps, **opts):
    e = api.Engine(api.Model.from_case(case), **opts)
    e.step(10)
    e0 = e.stats()["engTot"]                                    # (from a step's own bookkeeping, not from the start-up evaluation)
    e.step(steps - 10)
    st, s = e.state(), e.stats()
    e.close()
    return e0, s, np.stack([st[k] for k in ("x", "y", "z", "vx", "vy", "vz")], 1)


def test_100_nve_steps():
    """drift against converged 'elec pme' (the yardstick, measured here); lazy against every-step schedule; graph replay against plain launches"""
    d = er.dense_case()
    L = d["box"][0]
    kmax = 16                                                   # exp(-(1.05 * 16 * 2 pi / L)^2 / 4 alpha^2) = 2e-9 at L = 26.3, alpha = 0.45 ...
    pme = dict(d, ewald_k=(kmax, kmax, kmax))
    assert np.exp(-(1.05 * kmax * 2 * pc.PI / L) ** 2 / (4 * d["alpha"] ** 2)) < 1e-8
    spme = sm.as_spme(d, (64, 64, 64), 8)
    p0, ps, _ = run(pme, 100, use_graph=0)
    s0, ss, Xs = run(spme, 100, use_graph=0)
    dp, ds = abs(ps["engTot"] - p0), abs(ss["engTot"] - s0)
    print("100 NVE steps: |drift| elec pme (%d^3 harmonics) %.3e, elec spme 64^3 / 8 %.3e (engTot %.6e)" % (kmax, dp, ds, s0))
    assert ss["step"] == 100 and ds <= 2 * dp
    _, s1, X1 = run(spme, 100, use_graph=0, sort_every=1)
    assert np.abs(Xs - X1).max() <= 1e-9 * max(1.0, np.abs(X1).max()) and abs(ss["engTot"] - s1["engTot"]) <= 1e-9 * abs(s1["engTot"])
    _, sg, Xg = run(spme, 100, use_graph=1)
    assert np.array_equal(Xg, Xs) and sg["engTot"] == ss["engTot"] and sg["engCoulRec"] == ss["engCoulRec"]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_slab_handle_and_overflow_guard_refused():
    case = inputs.lj_case((42, 5, 5), a=5.735, seed=31, rc=8.5, vel_T=8.0, charges=(0.2, -0.2), elec="fenn", r_real=8.5, alpha=0.35)
    case = sm.as_spme(case, (64, 16, 16), 6)
    for slab in ({"rank": 1, "nranks": 2, "loopback": True}, {"rank": 0, "nranks": 2, "loopback": True, "replicated": True}):
        with pytest.raises(api.AztotError) as e:
            api.Engine(api.Model.from_case(case), slab=slab)
        assert e.value.code == -2 and "elec spme" in str(e.value) and "one GPU" in str(e.value), str(e.value)
    big = sm.isolated_case("two")
    big["species"] = [(20.18, 0.0), (22.99, 2.0 ** 21), (35.45, -2.0 ** 21)]
    with pytest.raises(api.AztotError) as e:
        api.Engine(api.Model.from_case(big))
    assert e.value.code == -2 and "2^22" in str(e.value), str(e.value)
    big["species"] = [(20.18, 0.0), (22.99, 2.0 ** 20), (35.45, -2.0 ** 20)]       # 2 atoms * 2^20 < 2^22: accepted
    api.Engine(api.Model.from_case(big)).close()
    # the same model on one GPU is accepted and steps
    eng = api.Engine(api.Model.from_case(case))
    eng.step(3)
    assert eng.stats()["step"] == 3 and eng.stats()["engCoulRec"] > 0.0
    eng.close()


def test_stress_refused_other_samplers_unaffected():
    eng = api.Engine(api.Model.from_case(sm.as_spme(er.dense_case(), (32, 32, 32), 6)))
    with pytest.raises(api.AztotError) as e:
        eng.stress_setup()
    assert e.value.code == -2 and "elec spme" in str(e.value)
    with pytest.raises(api.AztotError) as e:
        eng.stress_sample()
    assert e.value.code == -4                                   # no sampler was left behind
    eng.rdf_setup(6.0, 0.05)
    eng.rdf_sample()
    eng.step(3)
    assert eng.stats()["step"] == 3
    L = api.lib()
    assert L.aztot_spme_mesh(None, 0, None, 0) == -4 and L.aztot_spme_mesh(eng.h, 3, None, 0) == -4 and L.aztot_spme_influence(None, None, 0) == -4
    small = np.zeros(8)
    assert L.aztot_spme_mesh(eng.h, 0, small.ctypes.data_as(api.C.c_void_p), 8) == -4
    assert L.aztot_spme_mesh(eng.h, 1, None, 0) == 2 * 32 ** 3 and L.aztot_spme_influence(eng.h, None, 0) == 32 ** 3
    eng.close()
    plain = api.Engine(api.Model.from_case(er.dense_case()))    # 'elec pme': no mesh to read
    assert L.aztot_spme_mesh(plain.h, 0, None, 0) == -4
    plain.close()


# ---- command-line program ---------------------------------------------------------------------------------------------------------------------
def test_cli_runs_elec_spme(tmp_path):
    case = dict(sm.as_spme(er.dense_case(), (32, 32, 32), 6), nsteps=10, stress=5)
    d = inputs.write_input_files(case, str(tmp_path / "spme"), stat=5)
    assert "elec\tspme\t" in open(os.path.join(d, "control.txt")).read()
    exe = os.path.join(ROOT, "aztotmd_amd", "aztotmd")
    r = subprocess.run([exe, d, "--out", d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "WARNING: stress directive not usable" in r.stderr and "elec spme" in r.stderr and not os.path.exists(os.path.join(d, "stress.dat"))
    rows = [l.split("\t") for l in open(os.path.join(d, "stat.dat")).read().splitlines()]
    rows = [l for l in rows if l[1] in ("5", "10")]
    assert [l[1] for l in rows] == ["5", "10"]
    eng = api.Engine(api.Model.from_dir(d), initial_forces=0)
    for row in rows:
        eng.step(5)
        s = eng.stats()
        assert row[2:7] == ["%f" % s[k] for k in ("engTot", "engKin", "engVdW", "engCoul", "engCoulRec")], (row, s)
        assert s["engCoulRec"] > 0.0
    eng.close()
