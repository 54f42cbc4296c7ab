"""CPU tests of the time-correlation sampler's contract and input surface: the summation tree of tests/tcf_model.py against an exact sum, the ring of
origins against the brute-force set of (sample, origin) pairs, the 'vaf' directive of control.txt (read_sim, sys_init.cpp:883-884) with its model
query, and the argument checks of the aztot_tcf_* entry points that need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from aztotmd_amd import api, inputs

import tcf_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TCF = ("aztot_tcf_setup", "aztot_tcf_sample", "aztot_tcf_reset", "aztot_tcf_shape", "aztot_tcf_sums", "aztot_tcf_values")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4000, 40000, 1000188])
@pytest.mark.parametrize("kind", ["squares", "products"])
def test_tree_sum_against_exact_sum(n, kind):
    """the textbook bound of pairwise summation, |tree - exact| <= levels * 2^-52 * sum |t|, levels = 6 + 2 + log2(padded chunk count)"""
    rng = np.random.default_rng(1000 + n)
    a = rng.normal(size=n) * 3.0
    t = a * a if kind == "squares" else a * rng.normal(size=n)
    exact = math.fsum(t.tolist())
    levels = tcf_model.tree_levels(n)
    bound = levels * 2.0 ** -52 * math.fsum(np.abs(t).tolist())
    err = abs(tcf_model.tree_sum(t) - exact)
    print("n = %d %s: error %.3g, bound %.3g (%d levels)" % (n, kind, err, bound, levels))
    assert err <= bound


def test_tree_sum_is_the_stated_tree():
    """a case small enough to write the tree out by hand: 300 ids -> two chunks, the second with 44 ids"""
    t = np.random.default_rng(5).normal(size=300)
    a = np.zeros(512)
    a[:300] = t

    def halve(v):
        v = list(v)
        while len(v) > 1:
            h = len(v) // 2
            v = [v[j] + v[j + h] for j in range(h)]
        return v[0]

    chunk = []
    for c in range(2):
        w = [halve(a[256 * c + 64 * r:256 * c + 64 * r + 64]) for r in range(4)]
        chunk.append((w[0] + w[2]) + (w[1] + w[3]))
    assert tcf_model.tree_sum(t) == chunk[0] + chunk[1]
    assert tcf_model.tree_levels(300) == 9 and tcf_model.tree_levels(256) == 8 and tcf_model.tree_levels(40000) == 16


@pytest.mark.parametrize("M,E,n", [(1, 1, 5), (1, 100, 7), (3, 2, 20), (4, 1, 11), (2, 5, 23), (5, 3, 4)])
def test_ring_against_brute_force(M, E, n):
    s = tcf_model.Sampler(M, E, np.zeros(3, dtype=np.int32), 1, (10.0, 10.0, 10.0))
    for _ in range(n):
        s.sample()
    want = {(c, o) for c in range(n) for o in range(0, c + 1, E) if c - o < M * E}
    assert set(s.pairs) == want and len(s.pairs) == len(want)
    count = np.zeros(M * E, dtype=np.int64)
    for c, o in want:
        count[c - o] += 1
    assert np.array_equal(s.count, count)
    # within one sample all live origins have different lags
    for c in range(n):
        lags = [c - o for (cc, o) in s.pairs if cc == c]
        assert len(lags) == len(set(lags))
    s.reset()
    s.sample()
    assert s.pairs == [(0, 0)] and s.count.sum() == 1


FIELD = """spec 2
Ar  Ar   39.9   0.0   0.0
Kr  Kr   83.8   0.0   0.0
red-ox 0
vdw 1
Ar  Ar  lnjs 4.0    0.01006 3.3952
"""
CONTROL = """timestep 0.002 ps
nstep 1234
nequil 100
eqfreq 10
temperature 298.0\tnone
init_vel\tzero
cell_list\t85.0
elec\tnone
rdf 8.0 0.02 10 5000
%s
stat\t\t200
"""
KEYS = ("n_atoms", "n_species", "box", "dt", "nstep", "nequil", "eqfreq", "temperature", "tstat_type", "elec_type", "stat", "rdf", "outcn", "ncn", "types", "x")


def write_dir(d, lines):
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "field.txt"), "w").write(FIELD)
    open(os.path.join(d, "control.txt"), "w").write(CONTROL % lines)
    open(os.path.join(d, "cuda.txt"), "w").write("nstep stat 50\n")
    names = ["Ar", "Kr", "Kr", "Ar", "Ar"]
    with open(os.path.join(d, "atoms.xyz"), "w") as f:
        f.write("%d\n1 40.000000 41.000000 42.000000\n" % len(names))
        for i, nm in enumerate(names):
            f.write("%s\t%f\t%f\t%f\n" % (nm, 1.5 * i + 0.25, 2.0 * i, 39.0 - i))
    return d


def test_vaf_directive(tmp_path):
    with_vaf = api.Model.from_dir(write_dir(str(tmp_path / "a"), "vaf 25"))
    without = api.Model.from_dir(write_dir(str(tmp_path / "b"), "// no such line"))
    assert list(with_vaf.query("vaf")) == [25]
    assert list(without.query("vaf")) == [0]
    assert list(api.Model.from_dir(write_dir(str(tmp_path / "c"), "vaf\t0")).query("vaf")) == [0]
    # everything else parses as before
    for k in KEYS:
        assert list(with_vaf.query(k)) == list(without.query(k)), k
    assert list(with_vaf.query("stat")) == [200] and list(with_vaf.query("nequil")) == [100]


def test_negative_vaf_is_refused(tmp_path):
    with pytest.raises(api.AztotError) as e:
        api.Model.from_dir(write_dir(str(tmp_path / "d"), "vaf -5"))
    assert "ERROR[414]" in str(e.value) and e.value.code == -2        # AZTOT_ERR_INPUT


def test_created_model_has_no_vaf():
    assert list(api.Model.from_case(inputs.lj_case((4, 4, 4), charges=(0.0, 0.0))).query("vaf")) == [0]


def test_write_input_files_key(tmp_path):
    case = inputs.lj_case((4, 4, 4), charges=(0.0, 0.0))
    plain = inputs.write_input_files(case, str(tmp_path / "a"))
    with_vaf = inputs.write_input_files(dict(case, vaf=5), str(tmp_path / "b"))
    assert list(api.Model.from_dir(with_vaf).query("vaf")) == [5] and list(api.Model.from_dir(plain).query("vaf")) == [0]
    # a case without the key writes what it always wrote
    assert open(os.path.join(plain, "control.txt")).read() == "".join(l for l in open(os.path.join(with_vaf, "control.txt")) if not l.startswith("vaf"))


def test_tcf_entry_points_refuse_null_handles():
    L = api.lib()
    a, b, c = C.c_int32(), C.c_int32(), C.c_int64()
    assert L.aztot_tcf_setup(None, 1, 1) == -4
    assert L.aztot_tcf_sample(None) == -4
    assert L.aztot_tcf_reset(None) == -4
    assert L.aztot_tcf_shape(None, C.byref(a), C.byref(b), C.byref(c)) == -4
    assert L.aztot_tcf_sums(None, 0, 1, None, None, None, 0) == -4
    assert L.aztot_tcf_values(None, 0, 1, None, None, 0) == -4
    assert b"null handle" in L.aztot_last_error()


def test_exports_and_declarations():
    header = open(os.path.join(ROOT, "include", "aztot.h")).read()
    for n in TCF:
        assert n in api.EXPORTS and hasattr(api.lib(), n)
        assert re.search(r"\bint %s\(aztot_md \*md" % n, header), n
    assert re.search(r"#define AZTOT_TCF_MAX_LAGS \(1 << 24\)", header)
    for name in ("tcf_setup", "tcf_sample", "tcf_reset", "tcf_shape", "tcf_sums", "tcf_values"):
        assert callable(getattr(api.Engine, name))
