"""Cost of the pressure-tensor sampler (aztot_stress_sample, stress.hip.h) on one GPU, beside two baselines from the same run:
  k_cn_pairs at R = rMax          the same grid_walk (grid.hip.h) without the force arithmetic (coordination-number sampler, one column);
  pair_tile of a sort_every = 1   the same arithmetic on the engine's own tiles (every step rebuilds the cells and stages every cell).
  step of the same box

k_stress_* kernel times from aztot_kernel_times (options.profile = 1), the mean over `--samples` samples after two warm-up samples, for C4 and
case study 2.  "binning" is k_stress_bin + _scan + _ids + _rank + _place + _gather; "totals" is k_stress_chunks + k_stress_fold.

Usage: python tools/stress_cost.py [--samples 20] [--out FILE]
Every block is printed as one JSON line; --out also writes the whole record to FILE.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from aztotmd_amd import api  # noqa: E402
from aztotmd_amd import inputs  # noqa: E402


def mean_times(eng, prefix):
    return {k: v["ms"] / max(v["calls"], 1) for k, v in eng.kernel_times().items() if k.startswith(prefix) and v["calls"]}


def kernel_cost(model, samples, **kw):
    R = float(model.query("rmax")[0])
    eng = api.Engine(model, profile=1, **kw)
    out = {"n_atoms": eng.N, "rmax": R}
    eng.stress_setup()
    for _ in range(2):
        eng.stress_sample()
    eng.sync()
    eng.reset_kernel_times()
    for _ in range(samples):
        eng.stress_sample()
    t = mean_times(eng, "k_stress_")
    out["stress"] = dict(t, binning=sum(t.get("k_stress_" + k, 0.0) for k in ("bin", "scan", "ids", "rank", "place", "gather")),
                         totals=t.get("k_stress_chunks", 0.0) + t.get("k_stress_fold", 0.0), total_per_sample=sum(t.values()))
    s = eng.stress()
    out["pairs"] = int(s["pairs"])
    eng.cn_setup("species", [(0, 0, R)])
    for _ in range(2):
        eng.cn_sample("species")
    eng.sync()
    eng.reset_kernel_times()
    for _ in range(samples):
        eng.cn_sample("species")
    out["k_cn_pairs"] = mean_times(eng, "k_cn_")["k_cn_pairs"]
    eng.close()
    # the engine's own pair kernel on the same box, every step a rebuild
    eng = api.Engine(model, profile=1, sort_every=1, pair_variant=2, **kw)
    eng.step(2)
    eng.sync()
    eng.reset_kernel_times()
    eng.step(samples)
    t = mean_times(eng, "pair_")
    out["pair_kernels_per_step"] = t
    out["pair_tile"] = t["pair_tile"]
    eng.close()
    out["k_stress_pairs_over_k_cn_pairs"] = out["stress"]["k_stress_pairs"] / out["k_cn_pairs"]
    out["k_stress_pairs_over_pair_tile"] = out["stress"]["k_stress_pairs"] / out["pair_tile"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the whole record as JSON to this file")
    a = ap.parse_args()
    import util
    out = {"version": api.lib().aztot_version().decode()}
    out["C4"] = kernel_cost(api.Model.from_case(inputs.config("C4")), a.samples)
    print(json.dumps({"C4": out["C4"]}), flush=True)
    with tempfile.TemporaryDirectory() as d:
        m = api.Model.from_dir(util.materialise_case_study(2, os.path.join(d, "cs2")))
        out["case_study_2"] = kernel_cost(m, a.samples, initial_forces=0)
        print(json.dumps({"case_study_2": out["case_study_2"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
