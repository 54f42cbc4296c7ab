"""Cost of the structure-factor sampler (aztot_sk_sample, sk.hip.h) on one GPU, beside one step of the same box from the same run.

Two boxes: C4 (1 000 188 Ar) and B3 (1 000 188 ions of two species).  With 48 harmonics per axis at the most, kmax is bounded by 49 * 2 pi / L: the sets are
chosen as fractions of that bound, `--harmonics` of the longest edge.  Per box and per (kmax, max_per_bin) choice - a set thinned to 64 vectors per bin, the
unthinned set at half that kmax and the unthinned set at the full one:
  kernels        k_sk_* times from aztot_kernel_times (options.profile = 1), the mean over `--samples` samples, each right behind five steps
  work           the amplitude kernel against its counted fp64 work: n_k x N complex multiply-adds (each two complex products and two adds: 10 fp64
                 instructions as written, 14 flops), in 1e9 per second
  wall           host clock around aztot_sk_sample (it returns with the device drained) and around aztot_step on an engine without the profile switch
  tile           the amplitude kernel with the atoms per LDS tile forced to 16 / 32 / 64 (AZTOT_SK_TILE), where they fit

Usage: python tools/sk_cost.py [--samples 5] [--harmonics 40] [--out FILE]
Every block is printed as one JSON line; --out also writes the whole record to FILE.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aztotmd_amd import api, inputs  # noqa: E402


def kernels(eng, samples):
    """mean k_sk_* kernel times per sample, each sample behind five steps"""
    eng.sync()
    eng.reset_kernel_times()
    for _ in range(samples):
        eng.step(5)
        eng.sk_sample()
    t = {k: v["ms"] / samples for k, v in eng.kernel_times().items() if k.startswith("k_sk_") and v["calls"]}
    return dict(t, total_per_sample=sum(t.values()))


def wall(eng, samples):
    ts, tp = [], []
    for _ in range(samples):
        eng.step(5)
        eng.sync()
        t0 = time.perf_counter()
        eng.sk_sample()
        ts.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.step(20)
        eng.sync()
        tp.append((time.perf_counter() - t0) * 1e3 / 20)
    ts.sort()
    tp.sort()
    return {"sample_ms_median": ts[len(ts) // 2], "sample_ms_min": ts[0], "sample_ms_max": ts[-1], "step_ms_median": tp[len(tp) // 2]}


def cost(case, harmonics, samples):
    model = api.Model.from_case(case)
    g = 2.0 * math.pi / max(case["box"])
    top = harmonics * g
    out = {"box": list(case["box"]), "kmax_bound": 49 * g, "sets": {}}
    prof = api.Engine(model, profile=1)
    plain = api.Engine(model)
    out["n_atoms"] = prof.N
    prof.step(20)
    plain.step(40)
    for name, kmax, cap in (("thinned_64", top, 64), ("unthinned_half_kmax", 0.5 * top, 0), ("unthinned", top, 0)):
        dk = kmax / 50.5
        row = out["sets"][name] = {"kmax": kmax, "dk": dk, "max_per_bin": cap}
        row["n_vectors"] = prof.sk_setup(kmax, dk, cap)
        plain.sk_setup(kmax, dk, cap)
        lmn, _ = prof.sk_vectors()
        row["harmonics"] = [int(v) for v in abs(lmn).max(0)]
        prof.sk_sample()
        row["kernels"] = kernels(prof, samples)
        cmadd = float(row["n_vectors"]) * prof.N
        row["work"] = {"complex_multiply_adds": cmadd, "Gcmadd_per_s": cmadd / (row["kernels"]["k_sk_amplitudes"] * 1e-3) / 1e9}
        row["tile"] = {}
        for tile in (16, 32, 64):
            if tile * (sum(row["harmonics"]) + 3) * 16 > 49152:
                continue
            os.environ["AZTOT_SK_TILE"] = str(tile)
            row["tile"][str(tile)] = kernels(prof, max(samples // 2, 2))["k_sk_amplitudes"]
            del os.environ["AZTOT_SK_TILE"]
        plain.sk_sample()
        row["wall"] = wall(plain, samples)
        row["sample_over_step"] = row["wall"]["sample_ms_median"] / row["wall"]["step_ms_median"]
        print(json.dumps({name: row}), flush=True)
    prof.close()
    plain.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--harmonics", type=float, default=40.0, help="kmax of the full sets in units of 2 pi / the longest box edge (below 49)")
    ap.add_argument("--boxes", default="C4,B3")
    ap.add_argument("--out", default=None, help="also write the whole record as JSON to this file")
    a = ap.parse_args()
    out = {"version": api.lib().aztot_version().decode()}
    for box in a.boxes.split(","):
        out[box] = cost(inputs.config(box), a.harmonics, a.samples)
        print(json.dumps({box: out[box]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
