"""CPU tests of the RDF input surface: the 'rdf rmax dr every out_every [nucl]' directive of control.txt (read_rdf, rdf.cpp:14-37), the nuclei
table of read_spec (sys_init.cpp:86-103) and the argument checks of the aztot_rdf_* entry points that need no device."""
import ctypes as C
import os

import numpy as np
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
%s
stat\t\t200
"""


def write_dir(d, rdf_line):
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "field.txt"), "w").write(FIELD)
    open(os.path.join(d, "control.txt"), "w").write(CONTROL % rdf_line)
    open(os.path.join(d, "cuda.txt"), "w").write("nstep stat 50\n")
    names = ["Ar", "Ar+", "Cl-", "Cl-", "Ar", "Cl-"]
    with open(os.path.join(d, "atoms.xyz"), "w") as f:
        f.write("%d\n1 40.000000 41.000000 42.000000\n" % len(names))
        for i, nm in enumerate(names):
            f.write("%s\t%f\t%f\t%f\n" % (nm, 1.5 * i + 0.25, 2.0 * i, 39.0 - i))
    return d


@pytest.mark.parametrize("line,want", [
    ("rdf\t14.0   0.02\t50\t500000\tnucl", [1, 14.0, 0.02, 50, 500000, 1]),
    ("rdf 8.0 0.02 10 5000 -nucl", [1, 8.0, 0.02, 10, 5000, 0]),
    ("rdf 8.0 0.02 10 5000", [1, 8.0, 0.02, 10, 5000, 0]),           # the next word ('stat') is not 'nucl'
    ("rdf 6.5 0.05 3 7 nuclei", [1, 6.5, 0.05, 3, 7, 0]),            # only the exact word turns nuclei on
    ("// no rdf line", [0, 0, 0, 0, 0, 0]),
])
def test_rdf_directive(tmp_path, line, want):
    m = api.Model.from_dir(write_dir(str(tmp_path / "d"), line))
    assert list(m.query("rdf")) == want


@pytest.mark.parametrize("k,want", [(1, [1, 14.0, 0.02, 50, 500000, 1]), (2, [1, 8.0, 0.02, 10, 5000, 0]), ("src", [1, 8.0, 0.02, 20, 50000, 0])])
def test_case_study_rdf_lines(tmp_path, k, want):
    m = api.Model.from_dir(util.materialise_case_study(k, str(tmp_path / "cs")))
    assert list(m.query("rdf")) == want
    assert list(m.query("nuclei")) == [0] and m.query("n_nuclei")[0] == 1 and m.nucleus_name(0) == "Ar"


def test_shared_nucleus(tmp_path):
    m = api.Model.from_dir(write_dir(str(tmp_path / "d"), "rdf 8.0 0.1 1 1 nucl"))
    assert list(m.query("nuclei")) == [0, 0, 1]
    assert m.query("n_nuclei")[0] == 2
    assert [m.nucleus_name(i) for i in range(2)] == ["Ar", "Cl"]
    assert [m.species_name(i) for i in range(3)] == ["Ar", "Ar+", "Cl-"]
    with pytest.raises(api.AztotError) as e:
        m.nucleus_name(2)
    assert e.value.code == -4


def test_created_model_nucleus_is_species():
    case = inputs.lj_case((4, 4, 4), charges=(0.2, -0.2))
    case["names"] = ["Na", "Cl"]
    m = api.Model.from_case(case)
    assert list(m.query("nuclei")) == [0, 1] and m.query("n_nuclei")[0] == 2
    assert [m.nucleus_name(i) for i in range(2)] == ["Na", "Cl"]
    assert m.query("rdf")[0] == 0


def test_rdf_entry_points_refuse_null_handles():
    L = api.lib()
    assert L.aztot_rdf_setup(None, 8.0, 0.02, 0) == -4
    assert L.aztot_rdf_sample(None) == -4
    assert L.aztot_rdf_reset(None) == -4
    assert L.aztot_rdf_counts(None, 0, None, None, 0) == -4
    assert L.aztot_rdf_values(None, 0, None, None, 0) == -4
    nb, npair = C.c_int32(), C.c_int32()
    assert L.aztot_rdf_shape(None, 0, C.byref(nb), C.byref(npair)) == -4
