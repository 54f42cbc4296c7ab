"""Cost of the coordination-number sampler (aztot_cn_sample, cn.hip.h) on one GPU, beside the RDF sampler's pair walk at the same radius.

k_cn_* and k_rdf_* kernel times from aztot_kernel_times (options.profile = 1), the mean over `--samples` samples after two warm-up samples, for
C4 (R = 8.5 A, one Ar-Ar column) and case study 2 (R = 8 A), both kinds of CN and the RDF in ONE engine, so the numbers come from the same run.
"binning" is k_cn_bin + k_cn_scan + k_cn_place + k_cn_ids; "table" is k_cn_range + k_cn_table.

Usage: python tools/cn_cost.py [--samples 20] [--out FILE]
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

from aztotmd_amd import api, inputs  # noqa: E402


def mean_times(eng, prefix):
    return {k: v["ms"] / max(v["calls"], 1) for k, v in eng.kernel_times().items() if k.startswith(prefix) and v["calls"]}


def kernel_cost(model, R, samples, **kw):
    eng = api.Engine(model, profile=1, **kw)
    eng.rdf_setup(R, 0.02)
    out = {"n_atoms": eng.N, "radius": R}
    for kind in ("species", "nuclei"):
        eng.cn_setup(kind, [(0, 0, R)])
        for _ in range(2):
            eng.cn_sample(kind)
        eng.sync()
        eng.reset_kernel_times()
        for _ in range(samples):
            eng.cn_sample(kind)
        t = mean_times(eng, "k_cn_")
        out["cn_" + kind] = dict(t, binning=sum(t.get(k, 0.0) for k in ("k_cn_bin", "k_cn_scan", "k_cn_place", "k_cn_ids")),
                                 table=t.get("k_cn_range", 0.0) + t.get("k_cn_table", 0.0), total_per_sample=sum(t.values()))
    for _ in range(2):
        eng.rdf_sample()
    eng.sync()
    eng.reset_kernel_times()
    for _ in range(samples):
        eng.rdf_sample()
    t = mean_times(eng, "k_rdf_")
    out["rdf"] = dict(t, total_per_sample=sum(t.values()))
    out["k_cn_pairs_over_k_rdf_pairs"] = {kind: out["cn_" + kind]["k_cn_pairs"] / t["k_rdf_pairs"] for kind in ("species", "nuclei")}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the whole record as JSON to this file")
    a = ap.parse_args()
    import util
    out = {"version": api.lib().aztot_version().decode()}
    out["C4_R8.5"] = kernel_cost(api.Model.from_case(inputs.config("C4")), 8.5, a.samples)
    print(json.dumps({"C4_R8.5": out["C4_R8.5"]}), flush=True)
    with tempfile.TemporaryDirectory() as d:
        m = api.Model.from_dir(util.materialise_case_study(2, os.path.join(d, "cs2")))
        out["case_study_2_R8"] = kernel_cost(m, 8.0, a.samples, initial_forces=0)
        print(json.dumps({"case_study_2_R8": out["case_study_2_R8"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
