"""Which kernels a step launches, call by call (csrc/engine.hip: Engine::plan_step decides, launch_step_kernels / sort_and_forces / launch_pair execute).

Per-kernel timing counts launches by name.  A table of small engines - the smallest systems on which each step path exists, all of them used elsewhere
in the suite - runs one sequence of calls with the counters cleared before each call, and every count must equal the one recorded in
tests/golden/step_launches.json: the kernel names, the counters 'fold_drift' and 'narrow_lists' among them, times ignored.  The table was recorded from the
commit before the step plan existed, so it holds the host code that chooses a step's launches to exactly what that code chose.

Recording (on the commit whose launches are to be the yardstick, with only this file copied in):  python tests/test_gpu_step_launches.py --record FILE
"""
import json
import os
import sys

import pytest

if __name__ == "__main__":              # (run as a script, nobody has put the repository on the path: tests/conftest.py does under pytest)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aztotmd_amd import api
from aztotmd_amd.api import DebugBit
from test_gpu_fold_kick import no_fold_case
from util import wall_liquid

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_launches.json")
# (the first look falls at 8 steps; 76 steps in all, looks and rebuilds inside the longer calls)
CALLS = [("step", 8), ("step", 5), ("step", 1), ("step", 1), ("forces", 0), ("step", 9), ("step", 12), ("step", 40)]
LARGE_PATH = DebugBit.DBG_NO_FUSE_NEXT | DebugBit.DBG_LARGE_KICK_PATH


def equil_liquid():
    c = wall_liquid()
    c.update(nEq=30, freqEq=7)          # steps 7, 14, 21 and 28 rescale the velocities; the other 72 do not, the last 46 lie behind the equilibration period
    return c, {}


def liquid():
    return wall_liquid(), {}


# name -> (case maker, engine keywords)
ENGINES = {
    "liquid": (liquid, {}),
    "liquid_large_path": (liquid, dict(debug=LARGE_PATH)),
    "liquid_fold_kick": (liquid, dict(debug=LARGE_PATH | DebugBit.DBG_FOLD_KICK)),
    "liquid_fold_drift": (liquid, dict(debug=LARGE_PATH | DebugBit.DBG_FOLD_KICK | DebugBit.DBG_FOLD_DRIFT)),
    "liquid_energies_every_step": (liquid, dict(energies_every_step=1)),
    "liquid_sort_every_1": (liquid, dict(sort_every=1)),
    "liquid_sort_every_3": (liquid, dict(sort_every=3)),
    "liquid_pair_atom": (liquid, dict(pair_variant=1)),
    "radiative": (lambda: no_fold_case("radiative"), {}),
    "radiative_no_fuse_next": (lambda: no_fold_case("radiative"), dict(debug=DebugBit.DBG_NO_FUSE_NEXT)),
    "radiative_no_boundary": (lambda: no_fold_case("radiative"), dict(debug=DebugBit.DBG_NO_FUSE_NEXT | DebugBit.DBG_NO_BOUNDARY_RADI)),
    "radiative_kick_post_split": (lambda: no_fold_case("radiative"), dict(debug=DebugBit.DBG_NO_FUSE_NEXT | DebugBit.DBG_KICK_POST_SPLIT)),
    "nose": (lambda: no_fold_case("nose"), {}),
    "bonded": (lambda: no_fold_case("bonded"), {}),
    "ewald": (lambda: no_fold_case("ewald"), {}),
    "equilibration": (equil_liquid, {}),
    "slab": (lambda: no_fold_case("slab"), {}),
}

# Names left out of the comparison, per engine: those whose count is not a function of the calls alone.
# slab / pair_cleanup: a slab rank skips the clean-up launch once the read-back of "cells without a list" has landed and says none; the host polls for
# it when it launches a plain step, so the step from which the launch is skipped depends on how far the host runs ahead of the device.  (Two recordings
# of the table agreed in every count, this one included - 3 launches behind each rebuild; it is left out because nothing holds it there.)
UNSTABLE = {"slab": ("pair_cleanup",)}


def launches(name):
    """[{kernel name: calls} per call of CALLS] of one engine"""
    make, kw = ENGINES[name]
    case, more = make()
    e = api.Engine(api.Model.from_case(case), use_graph=0, **dict(more, **kw))
    e.set_profile(1)
    out = []
    for what, n in CALLS:
        e.reset_kernel_times()
        if what == "step":
            e.step(n)
        else:
            e.forces()
        out.append({k: int(v["calls"]) for k, v in e.kernel_times().items() if v["calls"]})
    e.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(ENGINES))
def test_every_call_launches_what_it_did(name, golden):
    got, want = launches(name), golden[name]
    assert len(got) == len(want) == len(CALLS)
    skip = UNSTABLE.get(name, ())
    for call, g, w in zip(CALLS, got, want):
        g = {k: v for k, v in g.items() if k not in skip}
        w = {k: v for k, v in w.items() if k not in skip}
        assert g == w, (name, call, {k: (g.get(k, 0), w.get(k, 0)) for k in set(g) | set(w) if g.get(k, 0) != w.get(k, 0)})


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_step_launches.py --record FILE")
    table = {}
    for engine in ENGINES:
        table[engine] = launches(engine)
        print(engine, table[engine][-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        f.write("{\n" + ",\n".join('"%s":%s' % (k, json.dumps(v, sort_keys=True, separators=(",", ":"))) for k, v in table.items()) + "\n}\n")
