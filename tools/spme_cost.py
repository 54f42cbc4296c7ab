"""Cost of smooth particle-mesh Ewald ('elec spme', spme.hip.h) on one GPU, beside the long-range methods the project had before it:
  E2  40 000 ions, 'elec pme 8.5 0.35 12 12 14' as it stands (the plain Ewald sum, 4 231 k-vectors) against 'elec spme' at 64^3 / p = 6, with each
      one's reciprocal force error against the numpy model at 128^3 / p = 8, evaluated on the CPU (the same ions without Lennard-Jones and with
      rReal inside the nearest-neighbour distance: forces() is then the reciprocal part alone; it does not depend on rReal)
  C3  1 000 188 ions, Fennell/DSF as it stands against 'elec spme' at 128^3 / p = 6: the price of true long range on the headline size
ms/step is wall time over `--steps` steps between two aztot_sync (no profiling); the per-kernel means come from aztot_kernel_times
(options.profile = 1) over the same number of steps of a second handle.  The spread kernel's atomic traffic is ions * p^3 * 8 bytes per step.

Usage: python tools/spme_cost.py [--steps 200] [--skip-c3] [--out FILE]
Every block is printed as one JSON line; --out also writes the whole record to FILE.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from aztotmd_amd import api  # noqa: E402
from aztotmd_amd import inputs  # noqa: E402


def spme(case, K, order, **over):
    return dict(case, elec_type=4, spme_mesh=(K, K, K), spme_order=order, **over)


def ms_per_step(case, steps):
    eng = api.Engine(api.Model.from_case(case))
    eng.step(steps)
    eng.sync()
    t = time.perf_counter()
    eng.step(steps)
    eng.sync()
    wall = (time.perf_counter() - t) / steps * 1e3
    s = eng.stats()
    eng.close()
    return wall, s


def kernel_means(case, steps):
    eng = api.Engine(api.Model.from_case(case), profile=1)
    eng.step(20)
    eng.sync()
    eng.reset_kernel_times()
    eng.step(steps)
    eng.sync()
    kt = eng.kernel_times()
    eng.close()
    return {k: {"ms_per_call": v["ms"] / v["calls"], "ms_per_step": v["ms"] / steps} for k, v in kt.items() if v["calls"]}


def measure(case, steps):
    wall, s = ms_per_step(case, steps)
    kt = kernel_means(case, steps)
    out = {"ms_per_step": wall, "kernels": kt, "engCoulRec": s["engCoulRec"], "sort_interval": s["sort_interval"]}
    if case["elec_type"] == 4:
        q = np.array([c for _, c in case["species"]])[np.asarray(case["types"])]
        nbytes = int((q != 0).sum()) * case["spme_order"] ** 3 * 8
        out["spread_atomic_bytes_per_step"] = nbytes
        out["spread_atomic_TB_per_s"] = nbytes / (kt["spme_spread"]["ms_per_call"] * 1e-3) / 1e12
        out["spme_ms_per_step"] = sum(v["ms_per_step"] for k, v in kt.items() if k.startswith("spme_"))
        out["slowest_spme_kernel"] = max((k for k in kt if k.startswith("spme_")), key=lambda k: kt[k]["ms_per_step"])
    else:
        out["ewald_ms_per_step"] = sum(v["ms_per_step"] for k, v in kt.items() if k.startswith("ewald_"))
    return out


def forces(case, reciprocal_only=True):
    eng = api.Engine(api.Model.from_case(case))
    eng.forces()
    st, s = eng.state(), eng.stats()
    eng.close()
    assert not reciprocal_only or (s["engCoul"] == 0.0 and s["engVdW"] == 0.0)
    return np.stack([st["fx"], st["fy"], st["fz"]], 1)


def rms(F):
    return float(np.sqrt((np.asarray(F, dtype=np.float64) ** 2).sum(1).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--out", default=None, help="also write the whole record as JSON to this file")
    a = ap.parse_args()
    import spme_model as sm
    out = {"version": api.lib().aztot_version().decode(), "steps": a.steps}
    e2 = inputs.config("E2")
    blk = {"n_atoms": len(e2["types"]), "elec_pme_12_12_14": measure(e2, a.steps), "elec_spme_64_6": measure(spme(e2, 64, 6), a.steps)}
    # reciprocal force errors: the same ions alone
    bare = dict(e2, vdw=[], rReal=1.0)
    ref = sm.spme(spme(bare, 128, 8), "fp64")["F"]
    for key, c in (("elec_pme_12_12_14", bare), ("elec_spme_64_6", spme(bare, 64, 6)), ("elec_spme_128_8", spme(bare, 128, 8))):
        blk.setdefault(key, {})["rel_rms_force_error_vs_model_128_8"] = sm.rel_rms(forces(c), ref)
    # (what the errors are relative to: on this near-lattice of alternating charges the reciprocal force is a small part of an ion's force)
    blk["rms_reciprocal_force_model_128_8"], blk["rms_total_force"] = rms(ref), rms(forces(spme(e2, 128, 8), reciprocal_only=False))
    out["E2"] = blk
    print(json.dumps({"E2": blk}), flush=True)
    if not a.skip_c3:
        c3 = inputs.config("C3")
        steps = max(a.steps // 2, 20)
        blk = {"n_atoms": len(c3["types"]), "elec_fenn": measure(c3, steps), "elec_spme_128_6": measure(spme(c3, 128, 6), steps)}
        out["C3"] = blk
        print(json.dumps({"C3": blk}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
