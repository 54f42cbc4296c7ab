"""Cost of the bond-orientational order sampler (aztot_boo_sample, boo.hip.h) on one GPU, beside one step and one bond-angle sample of the same run.

One set-up, orders (4, 6), R = 5 A (the first minimum of g(r) of the Ar lattice: 12 neighbours), one species central and ligand, on two boxes: C2
(40 000 Ar) and C4 (1 000 188 Ar).  Per box:
  kernels        k_boo_* times from aztot_kernel_times (options.profile = 1), the mean over `--samples` samples, each right behind five steps ("busy": the
                 clocks are up) and each behind a pause of `--pause` seconds ("idle"); k_boo_qlm and k_boo_average are the two launches (one per order) together
  wall           host clock around aztot_boo_sample (it returns with the device drained), around aztot_adf_sample (180 bins, one column at the same radius:
                 the method of tools/adf_cost.py) and around aztot_step on an engine without the profile switch, busy and idle
  vgprs          VGPR count of every k_boo_qlm<L> and k_boo_average<L> in the gfx950 code object of the library (from its metadata notes)

Usage: python tools/boo_cost.py [--samples 20] [--pause 0.5] [--out FILE]
Every block is printed as one JSON line; --out also writes the whole record to FILE.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aztotmd_amd import api, inputs  # noqa: E402

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
RADIUS, ORDERS, BINS = 5.0, (4, 6), 100


def vgpr_counts(so):
    """{kernel<L>: VGPRs} of the k_boo_qlm / k_boo_average instances: every offload bundle of the library's .hip_fatbin section is unbundled for gfx950 and
    the kernel metadata of its notes is read"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
        data = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), data)]
        for k, at in enumerate(starts):
            piece, co = os.path.join(d, "b%d" % k), os.path.join(d, "c%d.co" % k)
            open(piece, "wb").write(data[at:starts[k + 1] if k + 1 < len(starts) else len(data)])
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + piece,
                                "--output=" + co], capture_output=True)
            if r.returncode or not os.path.exists(co) or not os.path.getsize(co):
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
            name = None
            for line in notes.splitlines():
                m = re.search(r"\.name:\s+(\S+)", line)
                if m:
                    name = m.group(1)
                m = re.search(r"\.vgpr_count:\s+(\d+)", line)
                if m and name:
                    k2 = re.match(r"_ZN5aztot\d+(k_boo_qlm|k_boo_average)ILi(\d+)E", name)
                    if k2:
                        out["%s<%s>" % (k2.group(1), k2.group(2))] = int(m.group(1))
                    name = None
    return dict(sorted(out.items(), key=lambda kv: (kv[0].split("<")[0], int(kv[0].split("<")[1][:-1]))))


def mean_times(eng, prefix):
    return {k: v["ms"] / max(v["calls"], 1) for k, v in eng.kernel_times().items() if k.startswith(prefix) and v["calls"]}


def kernels(eng, samples, pause):
    """mean k_boo_* kernel times per sample: behind five steps (pause == 0) or behind a pause"""
    eng.sync()
    eng.reset_kernel_times()
    for _ in range(samples):
        if pause:
            time.sleep(pause)
        else:
            eng.step(5)
        eng.boo_sample()
    t = mean_times(eng, "k_boo_")
    return dict(t, total_per_sample=sum(t.values()))


def wall(eng, samples, pause):
    """host milliseconds per aztot_boo_sample, per aztot_adf_sample and per step, the GPU busy or idle before each"""
    tb, ta, tp = [], [], []
    for _ in range(samples):
        for call, acc in ((eng.boo_sample, tb), (eng.adf_sample, ta)):
            eng.step(5)
            eng.sync()
            if pause:
                time.sleep(pause)
            t0 = time.perf_counter()
            call()
            acc.append((time.perf_counter() - t0) * 1e3)
        if pause:
            time.sleep(pause)
        t0 = time.perf_counter()
        eng.step(20)
        eng.sync()
        tp.append((time.perf_counter() - t0) * 1e3 / 20)
    for v in (tb, ta, tp):
        v.sort()
    return {"boo_sample_ms_median": tb[len(tb) // 2], "boo_sample_ms_min": tb[0], "boo_sample_ms_max": tb[-1], "adf_sample_ms_median": ta[len(ta) // 2],
            "step_ms_median": tp[len(tp) // 2]}


def cost(case, samples, pause):
    model = api.Model.from_case(case)
    out = {"radius": RADIUS, "orders": list(ORDERS), "n_bins": BINS}
    eng = api.Engine(model, profile=1)
    out["n_atoms"] = eng.N
    eng.boo_setup(RADIUS, ORDERS, BINS, 1, 1)
    eng.step(20)
    for _ in range(2):
        eng.boo_sample()
    n, q = eng.boo_per_atom()
    out["neighbours_mean"] = float(n[n >= 0].mean())
    out["neighbours_max"] = int(n.max())
    out["q_mean"] = {"q%d" % l: float(q[:, o, 0].mean()) for o, l in enumerate(ORDERS)}
    out["kernels_busy"] = kernels(eng, samples, 0.0)
    out["kernels_idle"] = kernels(eng, samples, pause)
    eng.close()
    eng = api.Engine(model)
    eng.boo_setup(RADIUS, ORDERS, BINS, 1, 1)
    eng.adf_setup(180, [(0, 0, 0, RADIUS, RADIUS)])
    eng.step(40)
    eng.boo_sample()
    eng.adf_sample()
    out["wall_busy"] = wall(eng, samples, 0.0)
    out["wall_idle"] = wall(eng, samples, pause)
    eng.close()
    out["sample_over_step_busy"] = out["wall_busy"]["boo_sample_ms_median"] / out["wall_busy"]["step_ms_median"]
    out["sample_over_adf_sample_busy"] = out["wall_busy"]["boo_sample_ms_median"] / out["wall_busy"]["adf_sample_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--pause", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write the whole record as JSON to this file")
    a = ap.parse_args()
    out = {"version": api.lib().aztot_version().decode(), "vgprs": vgpr_counts(api.library_path())}
    print(json.dumps({"vgprs": out["vgprs"]}), flush=True)
    for box in ("C2", "C4"):
        out[box] = cost(inputs.config(box), a.samples, a.pause)
        print(json.dumps({box: out[box]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
