"""Cost of the bond-angle sampler (aztot_adf_sample, adf.hip.h) on one GPU, beside one step of the same box from the same run.

Two boxes: C4 (1 000 188 Ar, one column Ar-Ar-Ar at R = 5 A: 12 neighbours, 66 pairs per atom) and B3 (1 000 188 ions of two species, three
columns at the first-shell radius 4.6 A).  Per box:
  kernels        adf_* times from aztot_kernel_times (options.profile = 1), the mean over `--samples` samples, each sample right behind five steps
                 ("busy": the clocks are up) and each behind a pause of `--pause` seconds ("idle": a sample is a burst of a few ms, and a run that
                 samples every few hundred steps of a small system meets the GPU in this state); "binning" is adf_bin + adf_scan + adf_place
  wall           host clock around aztot_adf_sample (it returns with the device drained) and around aztot_step on an engine without the profile
                 switch, busy and idle as above
  lanes          adf_triplets with the lanes per central atom forced to 4 / 8 / 16 / 32 / 64 (AZTOT_ADF_LANES) and as the rule of Samplers::adf_sample
                 chooses them, busy, at several radii (every column at that radius): what the rule was fitted to

Usage: python tools/adf_cost.py [--samples 20] [--pause 0.5] [--out FILE]
Every block is printed as one JSON line; --out also writes the whole record to FILE.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aztotmd_amd import api, inputs  # noqa: E402


def mean_times(eng, prefix):
    return {k: v["ms"] / max(v["calls"], 1) for k, v in eng.kernel_times().items() if k.startswith(prefix) and v["calls"]}


def kernels(eng, samples, pause):
    """mean adf_* kernel times per sample: behind five steps (pause == 0) or behind a pause"""
    eng.sync()
    eng.reset_kernel_times()
    for _ in range(samples):
        if pause:
            time.sleep(pause)
        else:
            eng.step(5)
        eng.adf_sample()
    t = mean_times(eng, "adf_")
    return dict(t, binning=sum(t.get("adf_" + k, 0.0) for k in ("bin", "scan", "place")), total_per_sample=sum(t.values()))


def wall(eng, samples, pause):
    """host milliseconds per aztot_adf_sample and per step, the GPU busy or idle before each"""
    ts, tp = [], []
    for _ in range(samples):
        eng.step(5)
        eng.sync()
        if pause:
            time.sleep(pause)
        t0 = time.perf_counter()
        eng.adf_sample()
        ts.append((time.perf_counter() - t0) * 1e3)
        if pause:
            time.sleep(pause)
        t0 = time.perf_counter()
        eng.step(20)
        eng.sync()
        tp.append((time.perf_counter() - t0) * 1e3 / 20)
    ts.sort()
    tp.sort()
    return {"sample_ms_median": ts[len(ts) // 2], "sample_ms_min": ts[0], "sample_ms_max": ts[-1], "step_ms_median": tp[len(tp) // 2]}


def cost(case, n_bins, cols, samples, pause, sweep):
    model = api.Model.from_case(case)
    out = {"n_bins": n_bins, "columns": cols}
    eng = api.Engine(model, profile=1)
    out["n_atoms"] = eng.N
    eng.adf_setup(n_bins, cols)
    eng.step(20)
    for _ in range(2):
        eng.adf_sample()
    neigh = eng.adf_neighbours()
    out["neighbours_mean"] = float(neigh[neigh >= 0].mean())
    out["neighbours_max"] = int(neigh.max())
    eng.adf_reset()
    eng.adf_sample()
    out["triplets_per_sample"] = int(eng.adf_counts()[1].sum())
    out["kernels_busy"] = kernels(eng, samples, 0.0)
    out["kernels_idle"] = kernels(eng, samples, pause)
    out["lanes"] = {}
    for R in sweep:
        eng.adf_setup(n_bins, [(c, a, b, R, R) for c, a, b, _, _ in cols])
        eng.adf_sample()
        neigh = eng.adf_neighbours()
        row = out["lanes"]["R=%g" % R] = {"neighbours_mean": float(neigh[neigh >= 0].mean())}
        for lanes in (4, 8, 16, 32, 64):
            os.environ["AZTOT_ADF_LANES"] = str(lanes)
            eng.adf_sample()
            row[str(lanes)] = kernels(eng, max(samples // 3, 3), 0.0)["adf_triplets"]
        del os.environ["AZTOT_ADF_LANES"]
        row["rule"] = kernels(eng, max(samples // 3, 3), 0.0)["adf_triplets"]
    eng.adf_setup(n_bins, cols)
    eng.sync()
    eng.reset_kernel_times()
    eng.step(40)
    out["step_kernels_ms"] = sum(v["ms"] for v in eng.kernel_times().values()) / 40
    eng.close()
    eng = api.Engine(model)
    eng.adf_setup(n_bins, cols)
    eng.step(40)
    eng.adf_sample()
    out["wall_busy"] = wall(eng, samples, 0.0)
    out["wall_idle"] = wall(eng, samples, pause)
    eng.close()
    out["sample_over_step_busy"] = out["wall_busy"]["sample_ms_median"] / out["wall_busy"]["step_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--pause", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write the whole record as JSON to this file")
    a = ap.parse_args()
    out = {"version": api.lib().aztot_version().decode()}
    out["C4"] = cost(inputs.config("C4"), 180, [(0, 0, 0, 5.0, 5.0)], a.samples, a.pause, (5.0, 6.5, 7.5, 8.5))
    print(json.dumps({"C4": out["C4"]}), flush=True)
    out["B3"] = cost(inputs.config("B3"), 180, [(0, 1, 1, 4.6, 4.6), (1, 0, 0, 4.6, 4.6), (0, 0, 1, 4.6, 4.6)], a.samples, a.pause, (4.6, 6.5))
    print(json.dumps({"B3": out["B3"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
