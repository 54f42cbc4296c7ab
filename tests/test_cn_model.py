"""CPU tests of the coordination-number input surface: the 'outCN' directive (read_sim, sys_init.cpp:889-932) and the 'ncn' block (out_ncn,
out_md.cpp:216-271) of control.txt, the model queries "outcn" / "ncn", and the argument checks of the aztot_cn_* entry points that need no device."""
import ctypes as C
import os

import pytest

from aztotmd_amd import api, inputs

import util

FIELD = """spec 3
Ar  Ar   39.9   0.0   0.0
Ar+ Ar   39.9   0.0   0.0
Cl- Cl   35.45  0.0   0.0
red-ox 0
vdw 1
Ar  Ar  lnjs 4.0    0.01006 3.3952
"""
CONTROL = """timestep 0.002 ps
nstep 1234
temperature 298.0\tnone
init_vel\tzero
cell_list\t85.0
elec\tnone
rdf 8.0 0.02 10 5000
%s
stat\t\t200
"""
NCN = "ncn 3\nAr Cl 3.5\nCl Ar 4.25\nCl Cl 5.0"


def write_dir(d, lines):
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "field.txt"), "w").write(FIELD)
    open(os.path.join(d, "control.txt"), "w").write(CONTROL % lines)
    open(os.path.join(d, "cuda.txt"), "w").write("nstep stat 50\n")
    names = ["Ar", "Ar+", "Cl-", "Cl-", "Ar", "Cl-"]
    with open(os.path.join(d, "atoms.xyz"), "w") as f:
        f.write("%d\n1 40.000000 41.000000 42.000000\n" % len(names))
        for i, nm in enumerate(names):
            f.write("%s\t%f\t%f\t%f\n" % (nm, 1.5 * i + 0.25, 2.0 * i, 39.0 - i))
    return d


def test_directives(tmp_path):
    m = api.Model.from_dir(write_dir(str(tmp_path / "d"), "outCN 3.5 2 Ar Ar+ 1 Cl-\n" + NCN))
    # present, R, nCentral, nLigand, central species ids, ligand species ids
    assert list(m.query("outcn")) == [1, 3.5, 2, 1, 0, 1, 2]
    # n, then per line: central nucleus, ligand nucleus, R (nuclei: Ar = 0 (Ar, Ar+), Cl = 1)
    assert list(m.query("ncn")) == [3, 0, 1, 3.5, 1, 0, 4.25, 1, 1, 5.0]
    assert list(m.query("rdf")) == [1, 8.0, 0.02, 10, 5000, 0]


def test_order_of_names_is_kept(tmp_path):
    m = api.Model.from_dir(write_dir(str(tmp_path / "d"), "outCN\t4.0\t2\tCl-\tAr\t3\tAr+\tCl-\tAr"))
    assert list(m.query("outcn")) == [1, 4.0, 2, 3, 2, 0, 1, 2, 0]
    assert list(m.query("ncn")) == [0]


def test_no_directive(tmp_path):
    m = api.Model.from_dir(write_dir(str(tmp_path / "d"), "// neither"))
    assert list(m.query("outcn")) == [0, 0, 0, 0]
    assert list(m.query("ncn")) == [0]


@pytest.mark.parametrize("k", [1, 2, "src"])
def test_case_studies_have_neither(tmp_path, k):
    m = api.Model.from_dir(util.materialise_case_study(k, str(tmp_path / "cs")))
    assert m.query("outcn")[0] == 0 and m.query("ncn")[0] == 0


@pytest.mark.parametrize("lines,code", [
    ("outCN 3.5 2 Ar Xe 1 Cl-", "ERROR[201]"),                  # unknown central species (sys_init.cpp:907)
    ("outCN 3.5 2 Ar Ar+ 1 Xe", "ERROR[202]"),                  # unknown ligand species (sys_init.cpp:924)
    ("outCN 3.5 2 Ar Ar 1 Cl-", "ERROR[201]"),                  # a central species twice: a hole in the reference's tables
    ("outCN 3.5 1 Ar 2 Cl- Cl-", "ERROR[202]"),
    ("ncn 2\nAr Cl 3.5\nXe Cl 3.5", "ERROR[b010]"),             # out_md.cpp:248
    ("ncn 2\nAr Cl 3.5\nCl Ar+ 3.5", "ERROR[b011]"),            # out_md.cpp:253 (Ar+ is a species, not a nucleus)
    ("ncn 2\nAr Cl 3.5\nAr Cl 4.5", "ERROR[b010]"),             # the same directed pair twice
])
def test_bad_names_are_refused(tmp_path, lines, code):
    with pytest.raises(api.AztotError) as e:
        api.Model.from_dir(write_dir(str(tmp_path / "d"), lines))
    assert code in str(e.value)
    if "Xe" in lines:
        assert "Unknown" in str(e.value)


def test_unknown_nucleus_message_is_the_references(tmp_path):
    with pytest.raises(api.AztotError) as e:
        api.Model.from_dir(write_dir(str(tmp_path / "d"), "ncn 2\nAr Cl 3.5\nXe Cl 3.5"))
    assert "ERROR[b010] Unknown nuclei name(Xe) in ncn section of control file! Line 2: Xe Cl 3.500000" in str(e.value)


def test_created_model_has_neither():
    m = api.Model.from_case(inputs.lj_case((4, 4, 4), charges=(0.2, -0.2)))
    assert list(m.query("outcn")) == [0, 0, 0, 0] and list(m.query("ncn")) == [0]


def test_write_input_files_keys(tmp_path):
    case = inputs.lj_case((4, 4, 4), charges=(0.0, 0.0))
    plain = inputs.write_input_files(case, str(tmp_path / "a"))
    with_cn = inputs.write_input_files(dict(case, outCN=(4.5, ["A"], ["A", "B"]), ncn=[("A", "B", 4.0), ("B", "A", 5.5)]), str(tmp_path / "b"))
    m = api.Model.from_dir(with_cn)
    assert list(m.query("outcn")) == [1, 4.5, 1, 2, 0, 0, 1]
    assert list(m.query("ncn")) == [2, 0, 1, 4.0, 1, 0, 5.5]
    # a case without the keys writes what it always wrote
    ctl = open(os.path.join(plain, "control.txt")).read()
    assert "outCN" not in ctl and "ncn" not in ctl
    assert ctl == "".join(l for l in open(os.path.join(with_cn, "control.txt")) if not l.startswith(("outCN", "ncn", "A B", "B A")))
    m0 = api.Model.from_dir(plain)
    assert m0.query("outcn")[0] == 0 and m0.query("ncn")[0] == 0


def test_cn_entry_points_refuse_null_handles():
    L = api.lib()
    col = api._CnColumn(0, 0, 3.5)
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    for kind in (0, 1):
        assert L.aztot_cn_setup(None, kind, C.byref(col), 1) == -4
        assert L.aztot_cn_sample(None, kind) == -4
        assert L.aztot_cn_shape(None, kind, C.byref(a), C.byref(b), C.byref(c)) == -4
        assert L.aztot_cn_per_atom(None, kind, None, 0) == -4
        assert L.aztot_cn_table(None, kind, None, 0) == -4


def test_exports_and_struct():
    for n in ("aztot_cn_setup", "aztot_cn_sample", "aztot_cn_shape", "aztot_cn_per_atom", "aztot_cn_table"):
        assert n in api.EXPORTS and hasattr(api.lib(), n)
    assert C.sizeof(api._CnColumn) == 16            # int32, int32, double
