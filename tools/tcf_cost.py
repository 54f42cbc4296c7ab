"""Cost of the time-correlation sampler (aztot_tcf_sample, tcf.hip.h) on one GPU, beside what a user paid before it existed: reading the six
per-atom arrays back with Engine.state() at every sample.

k_tcf_* kernel times from aztot_kernel_times (options.profile = 1), the mean over `--samples` samples after the ring has filled and two more warm-up
samples, for C4 (1 000 188 atoms) and a 40 000-atom box at n_origins M in {1, 8, 64} with origin_every = 1 (every sample is an origin: the dearest
case).  With them the bytes each kernel must move, the share of the HBM peak bench.py uses that this amounts to, the wall time of one
aztot_tcf_sample call and, from the same engine in the same process, the wall time of Engine.state(("x", "y", "z", "vx", "vy", "vz")).

Usage: python tools/tcf_cost.py [--samples 20] [--out FILE]
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

HBM_PEAK = 8.0e12            # B/s, as bench.py
SIX = ("x", "y", "z", "vx", "vy", "vz")


def must_move(N, M, n_spec):
    """bytes per sample in the steady state (ring full, the sample is an origin)"""
    chunks = -(-N // 256)
    pad = 1
    while pad < chunks:
        pad *= 2
    return {
        # x y z vx vy vz type id in slot order; the six arrays twice (current state, ring slot) and the type by id
        "k_tcf_gather": N * (6 * 8 + 4 + 4) + N * (2 * 6 * 8 + 4),
        # the current state and the type once, every origin once, the chunk sums
        "k_tcf_correlate": N * (6 * 8 + 4) + M * N * 6 * 8 + M * 2 * n_spec * chunks * 8,
        # every level of the fold reads two halves and writes one
        "k_tcf_fold": M * 2 * n_spec * pad * 8 * 3 // 2,
    }


def block(model, M, samples):
    eng = api.Engine(model, profile=1)
    eng.step(20)
    eng.tcf_setup(M, 1)
    for _ in range(M + 2):
        eng.tcf_sample()
    eng.sync()
    eng.reset_kernel_times()
    t0 = time.perf_counter()
    for _ in range(samples):
        eng.tcf_sample()
    wall = (time.perf_counter() - t0) / samples * 1e3
    kt = {k: v["ms"] / max(v["calls"], 1) for k, v in eng.kernel_times().items() if k.startswith("k_tcf_") and v["calls"]}
    n_spec = eng.tcf_shape()[1]
    out = {"n_atoms": eng.N, "n_origins": M, "kernel_ms": kt, "kernels_ms_per_sample": sum(kt.values()), "sample_wall_ms": wall, "bytes": must_move(eng.N, M, n_spec)}
    out["hbm_share"] = {k: out["bytes"][k] / (kt[k] * 1e-3) / HBM_PEAK for k in kt}
    for _ in range(2):
        eng.state(SIX)
    t0 = time.perf_counter()
    for _ in range(5):
        eng.state(SIX)
    out["state_six_arrays_wall_ms"] = (time.perf_counter() - t0) / 5 * 1e3
    out["sample_cheaper_than_state"] = bool(wall < out["state_six_arrays_wall_ms"])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the whole record as JSON to this file")
    a = ap.parse_args()
    out = {"version": api.lib().aztot_version().decode(), "hbm_peak_Bps": HBM_PEAK}
    cases = (("C4", inputs.config("C4")), ("lj_40000", inputs.lj_case((25, 20, 20), seed=7, vel_T=85.0)))
    for name, case in cases:
        model = api.Model.from_case(case)
        for M in (1, 8, 64):
            key = "%s_M%d" % (name, M)
            out[key] = block(model, M, a.samples)
            print(json.dumps({key: out[key]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
