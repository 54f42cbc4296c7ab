"""Cost of the RDF sampler (aztot_rdf_sample, rdf.hip.h) on one GPU.

  1. k_rdf_* kernel times from aztot_kernel_times (options.profile = 1) for C4 at rmax 8.5 A / dr 0.02, case study 1 (rmax 14, nucl) and case study 2
     (rmax 8): the mean over `--samples` samples after two warm-up samples.
  2. C4 ms/step of a run that samples every 20 steps against one that does not (profiling off, host clock around work that ends in a synchronise;
     the two are alternated `--reps` times and the median of each is reported).

Usage: python tools/rdf_cost.py [--samples 20] [--reps 3] [--windows 10] [--out FILE]
Every block is printed as one JSON line; --out also writes the whole record to FILE.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from aztotmd_amd import api, inputs  # noqa: E402


def kernel_cost(model, rmax, dr, nuclei, samples, **kw):
    eng = api.Engine(model, profile=1, **kw)
    eng.rdf_setup(rmax, dr, nuclei=nuclei)
    for _ in range(2):
        eng.rdf_sample()
    eng.sync()
    eng.reset_kernel_times()
    for _ in range(samples):
        eng.rdf_sample()
    t = {k: v["ms"] / max(v["calls"], 1) for k, v in eng.kernel_times().items() if k.startswith("k_rdf_") and v["calls"]}
    t["total_per_sample"] = sum(t.values())
    eng.close()
    return t


def step_cost(case, windows, reps):
    model = api.Model.from_case(case)
    eng = api.Engine(model)
    eng.rdf_setup(8.5, 0.02)
    eng.step(200)                        # warm: the sort interval has settled, graphs are captured
    eng.rdf_sample()
    eng.sync()
    res = {"plain": [], "sampling": []}
    for _ in range(reps):
        for mode in ("plain", "sampling"):
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(windows):
                eng.step(20)
                if mode == "sampling":
                    eng.rdf_sample()
            eng.sync()
            res[mode].append((time.perf_counter() - t0) * 1e3 / (20 * windows))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    return {"ms_per_step": med, "all": res, "overhead": med["sampling"] / med["plain"] - 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the whole record as JSON to this file")
    a = ap.parse_args()
    import util
    out = {"version": api.lib().aztot_version().decode()}
    c4 = inputs.config("C4")
    out["C4_rmax8.5"] = kernel_cost(api.Model.from_case(c4), 8.5, 0.02, False, a.samples)
    print(json.dumps({"C4_rmax8.5": out["C4_rmax8.5"]}), flush=True)
    with tempfile.TemporaryDirectory() as d:
        for k, rmax, nucl in ((1, 14.0, True), (2, 8.0, False)):
            m = api.Model.from_dir(util.materialise_case_study(k, os.path.join(d, "cs%d" % k)))
            out["case_study_%d" % k] = kernel_cost(m, rmax, 0.02, nucl, a.samples, initial_forces=0)
            print(json.dumps({"case_study_%d" % k: out["case_study_%d" % k]}), flush=True)
    out["C4_step_every20"] = step_cost(c4, a.windows, a.reps)
    print(json.dumps({"C4_step_every20": out["C4_step_every20"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
