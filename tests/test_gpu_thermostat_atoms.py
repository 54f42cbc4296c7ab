"""post_tstat_atom (csrc/kernels.hip.h) through its four launch forms - k_integrate2_post, k_integrate2 + k_post, k_boundary_radi, the closing epilogue
of k_pair_list - atom by atom against the high-precision reference of tests/thermostat_reference.py, on the designed atoms of tests/thermostat_cases.py:
every branch of the thermostat and of angled_vector is taken by atoms chosen for it, two species, the photon index wraps.  Bounds are
|gpu - ref| <= TAU * scale with TAU = pair_cases.TAU and the scales of thermostat_reference (velocity per component, the two basis-independent invariants
of the emission, U, radius, position, engKin, engTemp); step 1 is held to the committed 50-digit fixture as well.  A call is held to the longdouble chain
started from the state the previous call returned.  kernel_times() proves which kernels ran.  Every run prints its worst err / (TAU * scale) per quantity
before it asserts.  This file needs numpy only; tests/test_thermostat_model.py holds the CPU oracle to the same bounds on the same runs.
"""
import numpy as np
import pytest

import thermostat_cases as tc
import thermostat_reference as tr
from aztotmd_amd import api
from aztotmd_amd.api import DebugBit

pytestmark = pytest.mark.gpu
_C = {}


def photons():
    if "ph" not in _C:
        _C["ph"] = tr.photon_table()
    return _C["ph"]


def designed():
    if "state" not in _C:
        tr.require_longdouble()
        _C["state"], _C["cls"] = tr.designed_state(photons())
    return _C["state"], _C["cls"]


class GpuEngine:
    """api.Engine behind the interface thermostat_reference.run_calls drives; kernel timers of the last call in .kt"""

    def __init__(self, case, U, variant=2, debug=0, sort_every=0):
        self.e = api.Engine(api.Model.from_case(case), seed=tc.SEED, pair_variant=variant, debug=debug, sort_every=sort_every, profile=1)
        self.e.set_state(U=U)
        self.kt = {}

    def step(self, n):
        self.e.reset_kernel_times()
        self.e.step(n)
        self.kt = {k: v["calls"] for k, v in self.e.kernel_times().items() if v["calls"] > 0}

    def state(self):
        return self.e.state()

    def energies(self):
        st = self.e.stats()
        assert st["pairs_dropped"] == 0 and st["engVdW"] == 0.0 and st["engCoul"] == 0.0, st
        return st["engKin"], st["engTemp"]


def fixture_check(label):
    def check(ref, got):
        w = tr.hold_to_fixture(got)
        print("%s step 1 against the 50-digit fixture: " % label + "  ".join("%s %.3e" % kv for kv in w.items()))
        for k, v in w.items():
            assert v <= 1.0, (label, "fixture", k, v)
    return check


def test_tables_and_inputs_are_the_models():
    """the restated unit-vector table, the masses and tKin are the model's; the fixture holds the designed inputs and the model's photons"""
    state, cls = designed()
    m = api.Model.from_case(tc.gas_case(photons()))
    assert np.array_equal(m.query("uvects").reshape(3, -1).T, tc.unit_table())
    assert np.array_equal(m.query("species").reshape(-1, 10)[:, 1], tc.masses()) and m.query("tkin")[0] == tc.t_kin()
    assert tr.fixture_matches(state, photons()), "the case generator or the photon table drifted away from the committed fixture"


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("form", ["integrate2_post", "integrate2 + post_tstat"])
def test_one_step_per_call(form, variant):
    """cells rebuilt every step, three calls of one step: k_integrate2_post alone, or k_integrate2 and k_post (DBG_KICK_POST_SPLIT); each call against the
    fixture (step 1) and the longdouble step from the state the call before returned"""
    state, cls = designed()
    split = form != "integrate2_post"
    g = GpuEngine(tc.gas_case(photons()), state["U"], variant, DebugBit.DBG_NO_FUSE_NEXT | (DebugBit.DBG_KICK_POST_SPLIT if split else 0), sort_every=1)

    def timers(done, n):
        if split:
            assert g.kt.get("integrate2") == 1 and g.kt.get("post_tstat") == 1 and "integrate2_post" not in g.kt and "boundary" not in g.kt, g.kt
        else:
            assert g.kt.get("integrate2_post") == 1 and "post_tstat" not in g.kt and "integrate2" not in g.kt and "boundary" not in g.kt, g.kt

    label = "%s [pair_variant %d]" % (form, variant)
    tr.run_calls(g, photons(), [1, 1, 1], state, cls, label=label, check_first=fixture_check(label), after_call=timers)


def test_boundary_kernel():
    """default lazy schedule without the pair kernel's epilogue: once the interval has opened (the look behind the first call), a call of 9 steps closes
    8 of them in k_boundary_radi, whose draws are keyed by the number of the step being closed - derived from the step being opened"""
    state, cls = designed()
    g = GpuEngine(tc.gas_case(photons()), state["U"], 2, DebugBit.DBG_NO_FUSE_NEXT)

    def timers(done, n):
        if done > 0:
            assert g.e.stats()["sort_interval"] > 1
            assert g.kt.get("boundary", 0) >= 1 and g.kt.get("boundary") + g.kt.get("integrate2_post", 0) == n and "post_tstat" not in g.kt, g.kt
            print("boundary kernel: %s" % g.kt)

    tr.run_calls(g, photons(), [1, 9], state, cls, label="k_boundary_radi", check_first=fixture_check("k_boundary_radi"), after_call=timers)


def test_list_kernel_epilogue():
    """default schedule: the plain steps of the later calls are closed (and the next ones opened) by k_pair_list itself; neither the boundary kernel nor
    k_integrate2_post appears on them - only the call's last step is closed on its own"""
    state, cls = designed()
    g = GpuEngine(tc.gas_case(photons()), state["U"], 2)

    def timers(done, n):
        if done == 10:
            st = g.e.stats()
            assert st["pair_lists"] == 1 and st["sort_interval"] > 1, st
            assert g.kt.get("pair_list") == n and "boundary" not in g.kt and g.kt.get("integrate2_post") == 1 and "post_tstat" not in g.kt and "integrate2" not in g.kt, g.kt
            print("list kernel epilogue: %s" % g.kt)

    tr.run_calls(g, photons(), [1, 9, 9], state, cls, label="k_pair_list epilogue", check_first=fixture_check("k_pair_list epilogue"), after_call=timers)


def test_equilibration_scaling_meets_the_thermostat():
    """nEq = 2, freqEq = 2: step 2 scales the velocities by sqrt(0.25 tKin / E_kin) and then runs the thermostat on them (k_integrate2, k_scale_decision,
    k_post) - the only place vscale != 1 meets tstat == 2.  E_kin of step 2 is what a twin engine without equilibration reports for that step (the
    engine itself reports engKin := tKin after a scaling step); the factor is restated from it in longdouble."""
    state, cls = designed()
    twin = GpuEngine(tc.gas_case(photons()), state["U"], 2)
    after_1 = {}
    tr.run_calls(twin, photons(), [1, 1], state, cls, label="twin without equilibration", after_call=lambda done, n: after_1.update(twin.e.state()) if done == 0 else None)
    k = np.sqrt(tr.LD(0.25) * tr.LD(tc.t_kin()) / tr.LD(twin.energies()[0]))
    print("equilibration factor of step 2: %.17g" % float(k))
    g = GpuEngine(tc.gas_case(photons(), n_eq=2, freq_eq=2), state["U"], 2)

    def timers(done, n):
        if done == 0:                                             # the twin's step 2 starts from the same state, bit for bit
            s1 = g.e.state()
            assert all(np.array_equal(s1[q], after_1[q]) for q in ("x", "y", "z", "vx", "vy", "vz", "U", "radius"))
        else:
            assert g.kt.get("scale_decision") == 1 and g.kt.get("post_tstat", 0) >= 1 and g.kt.get("integrate2", 0) >= 1, g.kt

    tr.run_calls(g, photons(), [1, 3], state, cls, vscale_for=lambda s, prev: k if s == 2 else None, label="equilibration", after_call=timers)
    assert g.e.stats()["step"] == 4
