"""ctypes front-end of the C ABI in include/aztot.h (mirrors the reference's host seam:
init_md -> init_cudaMD -> [step loop] -> md_to_host -> free_device_md; main.cu:239-463)."""
import ctypes as C
import enum
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

STAT_FIELDS = ("step", "time", "engTot", "engKin", "engVdW", "engCoul", "engElecField", "engTemp", "engPot", "temperature",
               "posMom", "negMom", "posCross", "negCross", "pressure", "pairs_dropped", "n_cells", "nose_chit", "nose_conint",
               "engBond", "engAngle", "engCoulRec", "engCoulConst", "sort_interval", "sort_violations", "pair_lists", "cells_without_list", "rebuilds", "skin")


class AztotError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("aztot error %d: %s" % (code, msg))
        self.code = code


class _Species(C.Structure):
    _fields_ = [("name", C.c_char * 8), ("mass_amu", C.c_double), ("charge", C.c_double), ("frozen", C.c_int32),
                ("radA", C.c_double), ("radB", C.c_double), ("mxEng", C.c_double)]


class _Vdw(C.Structure):
    _fields_ = [("spec_a", C.c_int32), ("spec_b", C.c_int32), ("type", C.c_int32), ("rcut", C.c_double), ("p", C.c_double * 5)]


class _Control(C.Structure):
    _fields_ = [("timestep", C.c_double), ("nstep", C.c_int32), ("nequil", C.c_int32), ("eqfreq", C.c_int32),
                ("temperature", C.c_double), ("tstat_type", C.c_int32), ("tstat_tau", C.c_double), ("elec_type", C.c_int32),
                ("r_real", C.c_double), ("alpha", C.c_double), ("init_vel", C.c_int32), ("init_vel_par", C.c_double * 3),
                ("elecfield", C.c_double * 3), ("use_cell_list", C.c_int32), ("cell_list", C.c_double), ("stat", C.c_int32),
                ("ewald_k", C.c_int32 * 3), ("spme_mesh", C.c_int32 * 3), ("spme_order", C.c_int32)]


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class _System(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("n_species", C.c_int32), ("n_vdw", C.c_int32), ("box", C.c_double * 3),
                ("types", _ip), ("x", _dp), ("y", _dp), ("z", _dp), ("vx", _dp), ("vy", _dp), ("vz", _dp),
                ("species", C.POINTER(_Species)), ("vdw", C.POINTER(_Vdw)), ("control", _Control)]


class _BondType(C.Structure):
    _fields_ = [("spec_a", C.c_int32), ("spec_b", C.c_int32), ("type", C.c_int32), ("p", C.c_double * 5)]


class _AngleType(C.Structure):
    _fields_ = [("central", C.c_int32), ("type", C.c_int32), ("k", C.c_double), ("cos0", C.c_double)]


class _Bonded(C.Structure):
    _fields_ = [("n_bond_types", C.c_int32), ("n_angle_types", C.c_int32), ("n_bonds", C.c_int32), ("n_angles", C.c_int32),
                ("bond_types", C.POINTER(_BondType)), ("angle_types", C.POINTER(_AngleType)),
                ("bond_a", _ip), ("bond_b", _ip), ("bond_type", _ip),
                ("angle_c", _ip), ("angle_l1", _ip), ("angle_l2", _ip), ("angle_type", _ip)]


class _Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("initial_forces", C.c_int32), ("center_box", C.c_int32), ("seed", C.c_uint64),
                ("pair_variant", C.c_int32), ("cell_size", C.c_double), ("use_graph", C.c_int32), ("profile", C.c_int32),
                ("sort_every", C.c_int32), ("skin", C.c_double), ("waves_per_cell", C.c_int32), ("energies_every_step", C.c_int32),
                ("loopback_ranks", C.c_int32), ("reserved", C.c_int32 * 5)]


class _Stats(C.Structure):
    _fields_ = [("step", C.c_int64), ("time", C.c_double), ("engTot", C.c_double), ("engKin", C.c_double), ("engVdW", C.c_double),
                ("engCoul", C.c_double), ("engElecField", C.c_double), ("engTemp", C.c_double), ("engPot", C.c_double),
                ("temperature", C.c_double), ("posMom", C.c_double * 3), ("negMom", C.c_double * 3), ("posCross", C.c_int64 * 3),
                ("negCross", C.c_int64 * 3), ("pressure", C.c_double), ("pairs_dropped", C.c_int64), ("n_cells", C.c_int64),
                ("nose_chit", C.c_double), ("nose_conint", C.c_double), ("engBond", C.c_double), ("engAngle", C.c_double),
                ("engCoulRec", C.c_double), ("engCoulConst", C.c_double), ("sort_interval", C.c_int64), ("sort_violations", C.c_int64),
                ("pair_lists", C.c_int64), ("cells_without_list", C.c_int64), ("rebuilds", C.c_int64), ("skin", C.c_double)]


class _CnColumn(C.Structure):
    _fields_ = [("central", C.c_int32), ("ligand", C.c_int32), ("radius", C.c_double)]


class _AdfColumn(C.Structure):
    _fields_ = [("central", C.c_int32), ("ligand_a", C.c_int32), ("ligand_b", C.c_int32), ("reserved", C.c_int32), ("radius_a", C.c_double), ("radius_b", C.c_double)]


class _BooParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("central_mask", C.c_int32), ("ligand_mask", C.c_int32), ("n_orders", C.c_int32), ("orders", C.c_int32 * 4),
                ("n_bins", C.c_int32), ("reserved", C.c_int32)]


class _Stress(C.Structure):
    _fields_ = [("step", C.c_int64), ("time", C.c_double), ("volume", C.c_double), ("kinetic", C.c_double * 6), ("virial", C.c_double * 6),
                ("pressure", C.c_double * 6), ("pressure_iso", C.c_double), ("eng_vdw", C.c_double), ("eng_coul", C.c_double),
                ("pairs", C.c_int64), ("pairs_dropped", C.c_int64)]


class _Clock(C.Structure):
    _fields_ = [("step", C.c_int64), ("nose_chit", C.c_double), ("nose_conint", C.c_double), ("eng_kin", C.c_double)]


class _State(C.Structure):
    _fields_ = [("n_atoms", C.c_int32)] + [(k, _dp) for k in ("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz", "U", "radius")] + [("types", _ip)]


SENDRECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64))
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _dp, C.c_int)

EXPORTS = ("aztot_device_count", "aztot_device_synchronize", "aztot_init_md", "aztot_model_create", "aztot_model_set_bonded", "aztot_model_query", "aztot_model_species_name", "aztot_model_nucleus_name", "aztot_free_md", "aztot_default_options",
           "aztot_init_device", "aztot_free_device", "aztot_step", "aztot_sync", "aztot_forces", "aztot_get_stats", "aztot_species_crossings", "aztot_md_to_host",
           "aztot_set_state", "aztot_get_clock", "aztot_set_clock", "aztot_cell_table", "aztot_kernel_times", "aztot_reset_kernel_times", "aztot_set_profile", "aztot_comm_id_bytes", "aztot_comm_make_id", "aztot_comm_selftest", "aztot_comm_ranks",
           "aztot_init_device_slab", "aztot_rdf_setup", "aztot_rdf_sample", "aztot_rdf_reset", "aztot_rdf_shape", "aztot_rdf_counts", "aztot_rdf_values",
           "aztot_cn_setup", "aztot_cn_sample", "aztot_cn_shape", "aztot_cn_per_atom", "aztot_cn_table",
           "aztot_tcf_setup", "aztot_tcf_sample", "aztot_tcf_reset", "aztot_tcf_shape", "aztot_tcf_sums", "aztot_tcf_values",
           "aztot_stress_setup", "aztot_stress_sample", "aztot_stress_get", "aztot_stress_per_atom",
           "aztot_adf_setup", "aztot_adf_sample", "aztot_adf_reset", "aztot_adf_shape", "aztot_adf_edges", "aztot_adf_counts", "aztot_adf_values",
           "aztot_adf_neighbours",
           "aztot_sk_setup", "aztot_sk_sample", "aztot_sk_reset", "aztot_sk_shape", "aztot_sk_vectors", "aztot_sk_amplitudes", "aztot_sk_sums", "aztot_sk_values",
           "aztot_boo_setup", "aztot_boo_sample", "aztot_boo_reset", "aztot_boo_shape", "aztot_boo_per_atom", "aztot_boo_qlm", "aztot_boo_counts", "aztot_boo_values",
           "aztot_spme_mesh", "aztot_spme_influence",
           "aztot_last_error", "aztot_version")

SPME_MESHES = {"charge": 0, "spectrum": 1, "potential": 2}      # AZTOT_SPME_CHARGE / _SPECTRUM / _POTENTIAL

RDF_KINDS = {"species": 0, "nuclei": 1}       # AZTOT_RDF_SPECIES / AZTOT_RDF_NUCLEI
CN_KINDS = {"species": 0, "nuclei": 1}        # AZTOT_CN_SPECIES (outCN rules) / AZTOT_CN_NUCLEI (ncn rules)


class DebugBit(enum.IntFlag):
    """Engine(debug=...): the measurement / test switches of `enum DebugBit` in csrc/device_md.h, which says what each one does
    (tests/test_debug_bits.py holds the two lists to each other)."""
    DBG_BUILD_PHASE_MASK = 3
    DBG_ALWAYS_CLEANUP = 4
    DBG_FOLD_DRIFT = 8
    DBG_NO_FOLD_DRIFT = 16
    DBG_WIDE_ENTRIES = 32
    DBG_HITS_BESIDE_TILE = 64
    DBG_KICK_EVERY_STEP = 128
    DBG_LARGE_KICK_PATH = 256
    DBG_GENERIC_PAIR = 512
    DBG_KEEP_VDW_CUT_TEST = 1024
    DBG_STAGE_ONLY = 2048
    DBG_SLAB_GRAPH = 4096
    DBG_FIXED_INTERVAL = 8192
    DBG_OVERLAP_HALO = 16384
    DBG_NO_LISTS = 32768
    DBG_SHORT_LISTS = 65536
    DBG_NO_FUSE_NEXT = 131072
    DBG_FUSE_NEXT = 262144
    DBG_CHECK_EVERY_ATOM = 524288
    DBG_LIST_STATS = 2097152
    DBG_KICK_POST_SPLIT = 4194304
    DBG_GRAPH_ALWAYS = 8388608
    DBG_PLAIN_ONE_ATOM = 16777216
    DBG_NO_BOUNDARY_RADI = 33554432
    DBG_ONE_WAVE_PER_CELL = 67108864
    DBG_ENERGIES_EVERY_STEP = 134217728
    DBG_SETTLE_EVERY_CALL = 268435456
    DBG_NO_FOLD_KICK = 536870912
    DBG_FOLD_KICK = 1073741824


def library_path():
    # AZTOT_LIB lets an experiment load another build of the SAME library (kernel A/B comparisons); never a fallback
    return os.environ.get("AZTOT_LIB") or os.path.join(_HERE, "libaztot.so")


def build_library(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    so = library_path()
    newest = max(os.path.getmtime(os.path.join(src_dir, f)) for f in os.listdir(src_dir) if f.endswith((".h", ".hip", ".cpp")) or f == "Makefile")
    hdr = os.path.join(os.path.dirname(_HERE), "include", "aztot.h")
    newest = max(newest, os.path.getmtime(hdr))
    def stale():
        return force or not os.path.exists(so) or os.path.getmtime(so) < newest

    if stale():
        # N ranks started against a stale library would run N makes over the same object files: one builds, the others wait and find it done
        import fcntl
        with open(os.path.join(src_dir, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if stale():
                    subprocess.check_call(["make", "-C", src_dir, "all"], stdout=subprocess.DEVNULL)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    return so


def lib():
    """Load libaztot.so.  There is deliberately no fallback: a missing library is an error."""
    global _LIB
    if _LIB is None:
        so = library_path()
        if not os.path.exists(so):
            raise ImportError("aztotmd_amd: %s is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path." % so)
        L = C.CDLL(so)
        L.aztot_last_error.restype = C.c_char_p
        L.aztot_version.restype = C.c_char_p
        L.aztot_init_md.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.aztot_model_create.argtypes = [C.POINTER(_System), C.POINTER(C.c_void_p)]
        L.aztot_model_query.argtypes = [C.c_void_p, C.c_char_p, _dp, C.c_int]
        L.aztot_model_set_bonded.argtypes = [C.c_void_p, C.POINTER(_Bonded)]
        L.aztot_free_md.argtypes = [C.c_void_p]
        L.aztot_free_md.restype = None
        L.aztot_default_options.argtypes = [C.POINTER(_Options)]
        L.aztot_default_options.restype = None
        L.aztot_init_device.argtypes = [C.c_void_p, C.POINTER(_Options), C.POINTER(C.c_void_p)]
        L.aztot_init_device_slab.argtypes = [C.c_void_p, C.POINTER(_Options), C.c_int, C.c_int, C.c_void_p, SENDRECV_FN, ALLREDUCE_FN,
                                             C.c_void_p, C.POINTER(C.c_void_p)]
        L.aztot_free_device.argtypes = [C.c_void_p]
        L.aztot_free_device.restype = None
        L.aztot_step.argtypes = [C.c_void_p, C.c_int]
        L.aztot_sync.argtypes = [C.c_void_p]
        L.aztot_forces.argtypes = [C.c_void_p]
        L.aztot_get_stats.argtypes = [C.c_void_p, C.POINTER(_Stats)]
        L.aztot_species_crossings.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int]
        L.aztot_md_to_host.argtypes = [C.c_void_p, C.POINTER(_State)]
        L.aztot_set_state.argtypes = [C.c_void_p, C.POINTER(_State)]
        L.aztot_get_clock.argtypes = [C.c_void_p, C.POINTER(_Clock)]
        L.aztot_set_clock.argtypes = [C.c_void_p, C.POINTER(_Clock)]
        L.aztot_cell_table.argtypes = [C.c_void_p, _ip, _ip, C.c_int, _ip, C.c_int]
        L.aztot_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _dp, C.POINTER(C.c_int64), C.c_int]
        L.aztot_reset_kernel_times.argtypes = [C.c_void_p]
        L.aztot_set_profile.argtypes = [C.c_void_p, C.c_int]
        L.aztot_comm_make_id.argtypes = [C.c_void_p]
        L.aztot_comm_selftest.argtypes = [C.c_int]
        L.aztot_comm_ranks.argtypes = [C.c_void_p]
        L.aztot_model_species_name.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
        L.aztot_model_nucleus_name.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
        L.aztot_rdf_setup.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int]
        L.aztot_rdf_sample.argtypes = [C.c_void_p]
        L.aztot_rdf_reset.argtypes = [C.c_void_p]
        L.aztot_rdf_shape.argtypes = [C.c_void_p, C.c_int, _ip, _ip]
        L.aztot_rdf_counts.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_int]
        L.aztot_rdf_values.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int]
        L.aztot_cn_setup.argtypes = [C.c_void_p, C.c_int, C.POINTER(_CnColumn), C.c_int]
        L.aztot_cn_sample.argtypes = [C.c_void_p, C.c_int]
        L.aztot_cn_shape.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip]
        L.aztot_cn_per_atom.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int]
        L.aztot_cn_table.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]
        L.aztot_tcf_setup.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.aztot_tcf_sample.argtypes = [C.c_void_p]
        L.aztot_tcf_reset.argtypes = [C.c_void_p]
        L.aztot_tcf_shape.argtypes = [C.c_void_p, _ip, _ip, C.POINTER(C.c_int64)]
        L.aztot_tcf_sums.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), _dp, _dp, C.c_int]
        L.aztot_tcf_values.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int]
        L.aztot_stress_setup.argtypes = [C.c_void_p]
        L.aztot_stress_sample.argtypes = [C.c_void_p]
        L.aztot_stress_get.argtypes = [C.c_void_p, C.POINTER(_Stress)]
        L.aztot_stress_per_atom.argtypes = [C.c_void_p, _dp, C.c_int]
        L.aztot_adf_setup.argtypes = [C.c_void_p, C.c_int, C.POINTER(_AdfColumn), C.c_int]
        L.aztot_adf_sample.argtypes = [C.c_void_p]
        L.aztot_adf_reset.argtypes = [C.c_void_p]
        L.aztot_adf_shape.argtypes = [C.c_void_p, _ip, _ip, C.POINTER(C.c_int64)]
        L.aztot_adf_edges.argtypes = [C.c_void_p, _dp, C.c_int]
        L.aztot_adf_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_int]
        L.aztot_adf_values.argtypes = [C.c_void_p, _dp, _dp, C.c_int]
        L.aztot_adf_neighbours.argtypes = [C.c_void_p, _ip, C.c_int]
        L.aztot_sk_setup.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int]
        L.aztot_sk_sample.argtypes = [C.c_void_p]
        L.aztot_sk_reset.argtypes = [C.c_void_p]
        L.aztot_sk_shape.argtypes = [C.c_void_p, _ip, _ip, _ip, C.POINTER(C.c_int64)]
        L.aztot_sk_vectors.argtypes = [C.c_void_p, _ip, _ip, C.c_int]
        L.aztot_sk_amplitudes.argtypes = [C.c_void_p, _dp, C.c_int]
        L.aztot_sk_sums.argtypes = [C.c_void_p, C.POINTER(C.c_int64), _dp, C.c_int]
        L.aztot_sk_values.argtypes = [C.c_void_p, _dp, _ip, _dp, _dp, C.c_int]
        L.aztot_boo_setup.argtypes = [C.c_void_p, C.POINTER(_BooParams)]
        L.aztot_boo_sample.argtypes = [C.c_void_p]
        L.aztot_boo_reset.argtypes = [C.c_void_p]
        L.aztot_boo_shape.argtypes = [C.c_void_p, _ip, _ip, _ip, _ip, C.POINTER(C.c_int64)]
        L.aztot_boo_per_atom.argtypes = [C.c_void_p, _ip, _dp, C.c_int]
        L.aztot_boo_qlm.argtypes = [C.c_void_p, _dp, C.c_int]
        L.aztot_boo_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), _dp, C.POINTER(C.c_uint64), C.c_int]
        L.aztot_boo_values.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int]
        L.aztot_spme_mesh.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        L.aztot_spme_mesh.restype = C.c_int64
        L.aztot_spme_influence.argtypes = [C.c_void_p, _dp, C.c_int64]
        L.aztot_spme_influence.restype = C.c_int64
        _LIB = L
    return _LIB


def _check(rc):
    if rc < 0:
        raise AztotError(rc, lib().aztot_last_error().decode("utf-8", "replace"))
    return rc


def _f8(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Model:
    """Host model (reference: Atoms/Field/Sim/Elec/TStat/Box after init_md, sys_init.cpp:1036)."""

    def __init__(self, handle, keep=None):
        self.h = handle
        self._keep = keep

    @classmethod
    def from_dir(cls, directory):
        h = C.c_void_p()
        _check(lib().aztot_init_md(os.fsencode(directory), C.byref(h)))
        return cls(h)

    @classmethod
    def from_case(cls, case):
        """`case`: dict as produced by aztotmd_amd.inputs.lj_case (input units)."""
        N = len(case["types"])
        types = np.ascontiguousarray(case["types"], dtype=np.int32)
        arrs = {k: _f8(case[k]) for k in ("x", "y", "z", "vx", "vy", "vz")}
        nsp = len(case["species"])
        sp = (_Species * nsp)()
        names = case.get("names") or ["S%d" % i for i in range(nsp)]
        radii = case.get("radii") or [(0.0, 0.0, 0.0)] * nsp
        frozen = case.get("frozen") or [0] * nsp
        for i, (m, q) in enumerate(case["species"]):
            sp[i].name = names[i].encode()[:7]
            sp[i].mass_amu, sp[i].charge, sp[i].frozen = m, q, int(frozen[i])
            sp[i].radA, sp[i].radB, sp[i].mxEng = radii[i]
        vd = (_Vdw * max(len(case["vdw"]), 1))()
        for i, (a, b, t, rc, p) in enumerate(case["vdw"]):
            vd[i].spec_a, vd[i].spec_b, vd[i].type, vd[i].rcut = a, b, t, rc
            for k, v in enumerate(list(p)[:5]):
                vd[i].p[k] = v
        s = _System()
        s.n_atoms, s.n_species, s.n_vdw = N, nsp, len(case["vdw"])
        s.box = (C.c_double * 3)(*case["box"])
        s.types = types.ctypes.data_as(_ip)
        for k in ("x", "y", "z", "vx", "vy", "vz"):
            setattr(s, k, arrs[k].ctypes.data_as(_dp))
        s.species, s.vdw = sp, vd
        c = s.control
        c.timestep, c.nstep, c.nequil, c.eqfreq = case["dt"], int(case.get("nsteps", 0)), int(case.get("nEq", 0)), int(case.get("freqEq", 1))
        c.temperature, c.tstat_type = float(case.get("T", 0.0)), int(case.get("tstat_type", 0))
        c.tstat_tau = float(case.get("tau", 0.0))
        c.elec_type, c.r_real, c.alpha = int(case.get("elec_type", 0)), float(case.get("rReal", 0.0)), float(case.get("alpha", 0.0))
        c.ewald_k = (C.c_int32 * 3)(*[int(v) for v in case.get("ewald_k", (0, 0, 0))])
        c.spme_mesh = (C.c_int32 * 3)(*[int(v) for v in case.get("spme_mesh", (0, 0, 0))])
        c.spme_order = int(case.get("spme_order", 0))
        c.init_vel = 0
        c.elecfield = (C.c_double * 3)(case.get("Ux", 0.0), case.get("Uy", 0.0), case.get("Uz", 0.0))
        c.use_cell_list = int(case.get("use_clist", 1))
        c.cell_list = float(case.get("cell_list", 0.0) or 0.0)
        c.stat = int(case.get("stat", 200))
        h = C.c_void_p()
        _check(lib().aztot_model_create(C.byref(s), C.byref(h)))
        m = cls(h)
        if case.get("bond_types") or case.get("angle_types"):
            m.set_bonded(case.get("bond_types") or [], case.get("angle_types") or [], case.get("bonds"), case.get("angles"))
        return m

    def set_bonded(self, bond_types, angle_types, bonds=None, angles=None):
        """bond_types: [(specA, specB, type_id, [p..])], angle_types: [(central, type_id, [k, cos0])],
        bonds: (n,3) int array (at1, at2, type id 1-based) = bonds.txt, angles: (n,4) (central, lig1, lig2, type id) = angles.txt."""
        bt = (_BondType * max(len(bond_types), 1))()
        for i, (a, b, t, p) in enumerate(bond_types):
            bt[i].spec_a, bt[i].spec_b, bt[i].type = a, b, t
            for k, v in enumerate(list(p)[:5]):
                bt[i].p[k] = v
        at = (_AngleType * max(len(angle_types), 1))()
        for i, (c, t, p) in enumerate(angle_types):
            at[i].central, at[i].type, at[i].k, at[i].cos0 = c, t, p[0], p[1]
        b = np.ascontiguousarray(bonds if bonds is not None else np.zeros((0, 3)), dtype=np.int32).reshape(-1, 3)
        a = np.ascontiguousarray(angles if angles is not None else np.zeros((0, 4)), dtype=np.int32).reshape(-1, 4)
        bc = [np.ascontiguousarray(b[:, k]) for k in range(3)]
        ac = [np.ascontiguousarray(a[:, k]) for k in range(4)]
        d = _Bonded()
        d.n_bond_types, d.n_angle_types, d.n_bonds, d.n_angles = len(bond_types), len(angle_types), len(b), len(a)
        d.bond_types, d.angle_types = bt, at
        d.bond_a, d.bond_b, d.bond_type = [c.ctypes.data_as(_ip) for c in bc]
        d.angle_c, d.angle_l1, d.angle_l2, d.angle_type = [c.ctypes.data_as(_ip) for c in ac]
        _check(lib().aztot_model_set_bonded(self.h, C.byref(d)))

    def query(self, key, seed=None):
        n = _check(lib().aztot_model_query(self.h, key.encode(), None, 0))
        out = np.zeros(max(n, 1))
        if seed is not None:
            out[0] = float(seed)
        _check(lib().aztot_model_query(self.h, key.encode(), out.ctypes.data_as(_dp), n))
        return out[:n]

    def species_name(self, i):
        buf = C.create_string_buffer(64)
        _check(lib().aztot_model_species_name(self.h, int(i), buf, 64))
        return buf.value.decode()

    def nucleus_name(self, i):
        """name of nucleus i (aztot_model_nucleus_name); query("nuclei") gives the nucleus of each species"""
        buf = C.create_string_buffer(64)
        _check(lib().aztot_model_nucleus_name(self.h, int(i), buf, 64))
        return buf.value.decode()

    def close(self):
        if self.h:
            lib().aztot_free_md(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """Device state + step driver (reference: cudaMD + the loop body of main.cu:281-410)."""

    def __init__(self, model, device=0, initial_forces=1, center_box=0, seed=12345, pair_variant=0, cell_size=0.0, use_graph=1,
                 profile=0, slab=None, debug=0, sort_every=0, split=0, skin=0.0, energies_every_step=0):
        """slab: None or dict(rank=, nranks=, rccl_id=bytes) or dict(rank=, nranks=, sendrecv=callable, allreduce=callable) or
        dict(rank=, nranks=, loopback=True[, replicated=True]) (options.loopback_ranks 1 / 2, include/aztot.h).
        debug: measurement / test switches (DebugBit above, from csrc/device_md.h); they are not part of the ABI - the library reads them from the
        environment variable AZTOT_DEBUG when the device handle is created, so it is set around that call here."""
        L = lib()
        o = _Options()
        L.aztot_default_options(C.byref(o))
        o.device, o.initial_forces, o.center_box, o.seed = device, initial_forces, center_box, seed
        o.pair_variant, o.cell_size, o.use_graph, o.profile = pair_variant, cell_size, use_graph, profile
        o.sort_every = sort_every           # 0: adaptive lazy re-sort (default), 1: rebuild the cells every step, n: at most every n-th step
        o.skin = skin                       # Verlet skin in A (0: automatic, < 0: none)
        o.waves_per_cell = split            # staging kernel: waves per cell (0: the engine decides; 1, 2, 4, 8: forced - measurements)
        o.energies_every_step = energies_every_step
        self.model = model
        self.N = int(model.query("n_atoms")[0])
        self.h = C.c_void_p()
        self._cb = None
        old_dbg = os.environ.get("AZTOT_DEBUG")
        if debug:
            os.environ["AZTOT_DEBUG"] = str(int(debug) | int(old_dbg or "0", 0))
        try:
            self._create(L, model, o, slab)
        finally:
            if debug:
                if old_dbg is None:
                    os.environ.pop("AZTOT_DEBUG", None)
                else:
                    os.environ["AZTOT_DEBUG"] = old_dbg

    def _create(self, L, model, o, slab):
        if slab is None:
            _check(L.aztot_init_device(model.h, C.byref(o), C.byref(self.h)))
        else:
            idb = slab.get("rccl_id")
            if slab.get("loopback"):
                # measurement aid: one rank of an N-rank decomposition exchanging with itself (see LoopbackExchanger); "replicated": the model is a box
                # of nranks exact copies of one period along x (copy k of atom j has id j * nranks + k) and ids follow the copies
                o.loopback_ranks = 2 if slab.get("replicated") else 1
                _check(L.aztot_init_device_slab(model.h, C.byref(o), slab["rank"], slab["nranks"], None, SENDRECV_FN(), ALLREDUCE_FN(), None,
                                                C.byref(self.h)))
            elif idb is not None:
                buf = C.create_string_buffer(bytes(idb), len(idb))
                self._cb = (buf,)
                _check(L.aztot_init_device_slab(model.h, C.byref(o), slab["rank"], slab["nranks"], C.cast(buf, C.c_void_p),
                                                SENDRECV_FN(), ALLREDUCE_FN(), None, C.byref(self.h)))
            else:
                sr_py, ar_py = slab["sendrecv"], slab["allreduce"]

                def _sr(ctx, speer, sbuf, sbytes, rpeer, rbuf, rcap, rbytes):
                    try:
                        data = C.string_at(sbuf, sbytes)
                        got = sr_py(speer, data, rpeer, rcap)
                        C.memmove(rbuf, got, len(got))
                        rbytes[0] = len(got)
                        return 0
                    except Exception:   # noqa: BLE001 - reported through the C return code
                        import traceback
                        traceback.print_exc()
                        return 1

                def _ar(ctx, buf, n):
                    try:
                        a = np.ctypeslib.as_array(buf, shape=(n,))
                        a[:] = ar_py(a.copy())
                        return 0
                    except Exception:   # noqa: BLE001
                        import traceback
                        traceback.print_exc()
                        return 1

                self._cb = (SENDRECV_FN(_sr), ALLREDUCE_FN(_ar))
                _check(L.aztot_init_device_slab(model.h, C.byref(o), slab["rank"], slab["nranks"], None, self._cb[0], self._cb[1], None,
                                                C.byref(self.h)))

    def step(self, n=1):
        _check(lib().aztot_step(self.h, int(n)))

    def sync(self):
        """everything earlier calls queued or deferred has happened when this returns (aztot_sync): the end of a timed region"""
        _check(lib().aztot_sync(self.h))

    def forces(self):
        _check(lib().aztot_forces(self.h))

    def stats(self):
        s = _Stats()
        _check(lib().aztot_get_stats(self.h, C.byref(s)))
        d = {}
        for k in STAT_FIELDS:
            v = getattr(s, k)
            d[k] = list(v) if hasattr(v, "__len__") else v
        return d

    def species_crossings(self):
        """(n_species, 6) int array: crossings of the walls Xn, Xp, Yn, Yp, Zn, Zp per species (the columns of msd.dat)."""
        ns = int(self.model.query("n_species")[0])
        out = np.zeros(6 * ns, dtype=np.int64)
        _check(lib().aztot_species_crossings(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), out.size))
        return out.reshape(ns, 6)

    def state(self, keys=("x", "y", "z", "vx", "vy", "vz", "fx", "fy", "fz", "U", "radius")):
        """Per-atom arrays in ORIGINAL atom order.  On a slab rank only the owned atoms are filled (others NaN)."""
        st = _State()
        st.n_atoms = self.N
        out = {}
        for k in keys:
            out[k] = np.full(self.N, np.nan)
            setattr(st, k, out[k].ctypes.data_as(_dp))
        out["types"] = np.full(self.N, -1, dtype=np.int32)
        st.types = out["types"].ctypes.data_as(_ip)
        _check(lib().aztot_md_to_host(self.h, C.byref(st)))
        out["n_owned"] = st.n_atoms
        return out

    def set_state(self, **arrays):
        st = _State()
        st.n_atoms = self.N
        keep = []
        for k, v in arrays.items():
            a = _f8(v)
            keep.append(a)
            setattr(st, k, a.ctypes.data_as(_dp))
        _check(lib().aztot_set_state(self.h, C.byref(st)))

    def clock(self):
        """step number + thermostat scalars: with state() everything a restart needs (aztot_clock)"""
        c = _Clock()
        _check(lib().aztot_get_clock(self.h, C.byref(c)))
        return {"step": c.step, "nose_chit": c.nose_chit, "nose_conint": c.nose_conint, "eng_kin": c.eng_kin}

    def set_clock(self, step, nose_chit=0.0, nose_conint=0.0, eng_kin=0.0):
        c = _Clock(int(step), float(nose_chit), float(nose_conint), float(eng_kin))
        _check(lib().aztot_set_clock(self.h, C.byref(c)))

    def cell_table(self):
        """(dims, cell_start[n_cells + 1], atom_id[resident atoms]) of the sorted cell list the device holds."""
        dims = np.zeros(3, dtype=np.int32)
        n = _check(lib().aztot_cell_table(self.h, dims.ctypes.data_as(_ip), None, 0, None, 0))
        start = np.zeros(n + 1, dtype=np.int32)
        _check(lib().aztot_cell_table(self.h, dims.ctypes.data_as(_ip), start.ctypes.data_as(_ip), n + 1, None, 0))
        ids = np.zeros(max(int(start[-1]), 1), dtype=np.int32)
        _check(lib().aztot_cell_table(self.h, dims.ctypes.data_as(_ip), start.ctypes.data_as(_ip), n + 1, ids.ctypes.data_as(_ip), ids.size))
        return tuple(int(v) for v in dims), start, ids[:int(start[-1])]

    def comm_ranks(self):
        """ranks of the RCCL communicator carrying the halo (0: no RCCL in use)."""
        return _check(lib().aztot_comm_ranks(self.h))

    def kernel_times(self):
        names = C.create_string_buffer(4096)
        ms = (C.c_double * 64)()
        calls = (C.c_int64 * 64)()
        n = _check(lib().aztot_kernel_times(self.h, names, 4096, ms, calls, 64))
        parts = names.raw.split(b"\0")
        return {parts[i].decode(): {"ms": ms[i], "calls": calls[i]} for i in range(n)}

    def spme_mesh(self, which="charge"):
        """A mesh of the last force evaluation of an 'elec spme' model (aztot_spme_mesh), indexed [gx, gy, gz]: "charge" the integer charge
        mesh (int64, units of 2^-40 e), "spectrum" its forward DFT, "potential" phi after the inverse transform (both complex128)."""
        kx, ky, kz = (int(v) for v in self.model.query("spme")[:3])
        n = _check(lib().aztot_spme_mesh(self.h, SPME_MESHES[which], None, 0))
        out = np.zeros(n, dtype=np.int64 if which == "charge" else np.float64)
        _check(lib().aztot_spme_mesh(self.h, SPME_MESHES[which], out.ctypes.data_as(C.c_void_p), n))
        if which != "charge":
            out = out.view(np.complex128)
        return out.reshape(kz, ky, kx).transpose(2, 1, 0)

    def spme_influence(self):
        """The influence function G of an 'elec spme' model (aztot_spme_influence), indexed [mx, my, mz]."""
        kx, ky, kz = (int(v) for v in self.model.query("spme")[:3])
        n = _check(lib().aztot_spme_influence(self.h, None, 0))
        out = np.zeros(n)
        _check(lib().aztot_spme_influence(self.h, out.ctypes.data_as(_dp), n))
        return out.reshape(kz, ky, kx).transpose(2, 1, 0)

    def reset_kernel_times(self):
        _check(lib().aztot_reset_kernel_times(self.h))

    def set_profile(self, on):
        _check(lib().aztot_set_profile(self.h, int(bool(on))))

    # ---- radial distribution functions (aztot_rdf_*) ----
    def rdf_setup(self, rmax, dr, nuclei=False):
        """(re)allocate and zero the RDF histograms; returns the number of bins, (int)(min(rmax, L_x) / dr)"""
        return _check(lib().aztot_rdf_setup(self.h, float(rmax), float(dr), int(bool(nuclei))))

    def rdf_sample(self):
        _check(lib().aztot_rdf_sample(self.h))

    def rdf_reset(self):
        _check(lib().aztot_rdf_reset(self.h))

    def _rdf_shape(self, kind):
        nb, npair = C.c_int32(), C.c_int32()
        _check(lib().aztot_rdf_shape(self.h, RDF_KINDS[kind], C.byref(nb), C.byref(npair)))
        return nb.value, npair.value

    def rdf_counts(self, kind="species"):
        """(samples, counts[n_bins, n_pairs]) - uint64 totals, pairs in the column order of rdf.dat"""
        nb, npair = self._rdf_shape(kind)
        out = np.zeros(max(nb * npair, 1), dtype=np.uint64)
        samples = C.c_int64()
        _check(lib().aztot_rdf_counts(self.h, RDF_KINDS[kind], C.byref(samples), out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size))
        return samples.value, out[:nb * npair].reshape(nb, npair)

    def rdf(self, kind="species"):
        """(r[n_bins], g[n_bins, n_pairs], pair_names): bin centres, normalised g(r) (copy_rdf / out_rdf) and the 'A-B' column names"""
        nb, npair = self._rdf_shape(kind)
        r = np.zeros(max(nb, 1))
        g = np.zeros(max(nb * npair, 1))
        _check(lib().aztot_rdf_values(self.h, RDF_KINDS[kind], r.ctypes.data_as(_dp), g.ctypes.data_as(_dp), g.size))
        if kind == "species":
            names = [self.model.species_name(i) for i in range(int(self.model.query("n_species")[0]))]
        else:
            names = [self.model.nucleus_name(i) for i in range(int(self.model.query("n_nuclei")[0]))]
        pairs = ["%s-%s" % (names[a], names[b]) for a in range(len(names)) for b in range(a, len(names))]
        return r[:nb], g[:nb * npair].reshape(nb, npair), pairs

    # ---- coordination numbers (aztot_cn_*; the rules of the two kinds are stated in include/aztot.h) ----
    def cn_setup(self, kind, columns):
        """columns: [(central group, ligand group, radius)], groups being species ("species", outCN rules) or nuclei ("nuclei", ncn rules)"""
        cols = (_CnColumn * max(len(columns), 1))()
        for i, (a, b, r) in enumerate(columns):
            cols[i].central, cols[i].ligand, cols[i].radius = int(a), int(b), float(r)
        _check(lib().aztot_cn_setup(self.h, CN_KINDS[kind], cols, len(columns)))

    def cn_sample(self, kind="species"):
        """a snapshot of the current configuration: replaces the previous sample of `kind`"""
        _check(lib().aztot_cn_sample(self.h, CN_KINDS[kind]))

    def cn_shape(self, kind="species"):
        """(n_cols, cn_min, cn_max): the columns and the first and last row of the file"""
        nc, mn, mx = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().aztot_cn_shape(self.h, CN_KINDS[kind], C.byref(nc), C.byref(mn), C.byref(mx)))
        return nc.value, mn.value, mx.value

    def cn_per_atom(self, kind="species"):
        """int32 [n_atoms, n_cols] in ORIGINAL atom order; -1 where the atom is not of the column's central group"""
        n = _check(lib().aztot_cn_per_atom(self.h, CN_KINDS[kind], None, 0))
        out = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().aztot_cn_per_atom(self.h, CN_KINDS[kind], out.ctypes.data_as(_ip), n))
        return out[:n].reshape(self.N, -1) if n else out[:0].reshape(self.N, 0)

    def cn_table(self, kind="species"):
        """(cn_min, table[cn - cn_min, column]): central atoms of each column with each coordination number"""
        nc, mn, mx = self.cn_shape(kind)
        n = _check(lib().aztot_cn_table(self.h, CN_KINDS[kind], None, 0))
        out = np.zeros(max(n, 1), dtype=np.int64)
        _check(lib().aztot_cn_table(self.h, CN_KINDS[kind], out.ctypes.data_as(C.POINTER(C.c_int64)), n))
        return mn, out[:n].reshape(-1, nc)

    # ---- time correlation functions (aztot_tcf_*; terms, summation tree and ring of origins are stated in include/aztot.h) ----
    def tcf_setup(self, n_origins=1, origin_every=1):
        """a ring of n_origins time origins, one taken every origin_every samples; forgets an earlier set-up.  Returns n_lags = n_origins * origin_every"""
        return _check(lib().aztot_tcf_setup(self.h, int(n_origins), int(origin_every)))

    def tcf_sample(self):
        """one sample of the current state: correlated with every live origin, and stored as an origin when its number is a multiple of origin_every"""
        _check(lib().aztot_tcf_sample(self.h))

    def tcf_reset(self):
        """zero sums and counts and forget the origins: the next sample is sample 0"""
        _check(lib().aztot_tcf_reset(self.h))

    def tcf_shape(self):
        """(n_lags, n_species, samples since the set-up or the last reset)"""
        nl, ns, sm = C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().aztot_tcf_shape(self.h, C.byref(nl), C.byref(ns), C.byref(sm)))
        return nl.value, ns.value, sm.value

    def _tcf_range(self, lag0, n):
        nl, ns, _ = self.tcf_shape()
        return (nl - lag0 if n is None else int(n)), ns

    def tcf_sums(self, lag0=0, n=None):
        """raw accumulators of lags [lag0, lag0 + n) (default: to the last): count int64 [n], msd_sum and vaf_sum fp64 [n, n_species]"""
        n, ns = self._tcf_range(lag0, n)
        need = _check(lib().aztot_tcf_sums(self.h, lag0, n, None, None, None, 0))
        cnt, a, b = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(need, 1)), np.zeros(max(need, 1))
        _check(lib().aztot_tcf_sums(self.h, lag0, n, cnt.ctypes.data_as(C.POINTER(C.c_int64)), a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), need))
        return cnt[:n], a[:need].reshape(n, ns), b[:need].reshape(n, ns)

    def tcf_values(self, lag0=0, n=None):
        """(msd, vaf) [n, n_species]: sums / (count * atoms of the species), 0 where that is 0"""
        n, ns = self._tcf_range(lag0, n)
        need = _check(lib().aztot_tcf_values(self.h, lag0, n, None, None, 0))
        a, b = np.zeros(max(need, 1)), np.zeros(max(need, 1))
        _check(lib().aztot_tcf_values(self.h, lag0, n, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), need))
        return a[:need].reshape(n, ns), b[:need].reshape(n, ns)

    # ---- pressure tensor (aztot_stress_*; pair set, terms and the order of the sums are stated in include/aztot.h) ----
    def stress_setup(self):
        """allocate the pressure-tensor sampler; refused (code -2) for slab handles, models with bonded terms and 'elec pme'"""
        _check(lib().aztot_stress_setup(self.h))

    def stress_sample(self):
        """one snapshot of the current state; replaces the previous sample"""
        _check(lib().aztot_stress_sample(self.h))

    def stress(self):
        """the totals of the last sample: 6-vectors (xx yy zz xy xz yz) as numpy arrays, kinetic and virial in eV, pressure in atm"""
        s = _Stress()
        _check(lib().aztot_stress_get(self.h, C.byref(s)))
        out = {k: getattr(s, k) for k in ("step", "time", "volume", "pressure_iso", "eng_vdw", "eng_coul", "pairs", "pairs_dropped")}
        for k in ("kinetic", "virial", "pressure"):
            out[k] = np.array(getattr(s, k), dtype=np.float64)
        return out

    def stress_per_atom(self):
        """w[atom id, component] of the last sample, eV: (N, 6) float64"""
        n = _check(lib().aztot_stress_per_atom(self.h, None, 0))
        out = np.zeros(max(n, 1))
        _check(lib().aztot_stress_per_atom(self.h, out.ctypes.data_as(_dp), n))
        return out[:n].reshape(-1, 6)

    # ---- bond-angle distributions (aztot_adf_*; columns, separation and the bin rule are stated in include/aztot.h) ----
    def adf_setup(self, n_bins, cols):
        """cols: [(central, ligand_a, ligand_b, R_a, R_b)] with species indices; (re)allocates and zeroes, returns n_bins"""
        c = (_AdfColumn * max(len(cols), 1))()
        for i, (ce, a, b, ra, rb) in enumerate(cols):
            c[i].central, c[i].ligand_a, c[i].ligand_b, c[i].reserved, c[i].radius_a, c[i].radius_b = int(ce), int(a), int(b), 0, float(ra), float(rb)
        return _check(lib().aztot_adf_setup(self.h, int(n_bins), c, len(cols)))

    def adf_sample(self):
        """add the triplets of the current configuration to the totals; refused (code -2, nothing added) when an atom has more than 256 neighbours"""
        _check(lib().aztot_adf_sample(self.h))

    def adf_reset(self):
        _check(lib().aztot_adf_reset(self.h))

    def adf_shape(self):
        """(n_bins, n_cols, samples)"""
        nb, nc, sm = C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().aztot_adf_shape(self.h, C.byref(nb), C.byref(nc), C.byref(sm)))
        return nb.value, nc.value, sm.value

    def adf_edges(self):
        """the n_bins + 1 edge values T_b = cos |cos| of the bin rule"""
        n = _check(lib().aztot_adf_edges(self.h, None, 0))
        out = np.zeros(n)
        _check(lib().aztot_adf_edges(self.h, out.ctypes.data_as(_dp), n))
        return out

    def adf_counts(self):
        """(samples, counts[n_bins, n_cols]) - uint64 totals"""
        nb, nc, _ = self.adf_shape()
        out = np.zeros(nb * nc, dtype=np.uint64)
        samples = C.c_int64()
        _check(lib().aztot_adf_counts(self.h, C.byref(samples), out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size))
        return samples.value, out.reshape(nb, nc)

    def adf_values(self):
        """(theta[n_bins] in degrees, p[n_bins, n_cols]): bin centres and the probability density per degree of each column"""
        nb, nc, _ = self.adf_shape()
        theta, p = np.zeros(nb), np.zeros(nb * nc)
        _check(lib().aztot_adf_values(self.h, theta.ctypes.data_as(_dp), p.ctypes.data_as(_dp), p.size))
        return theta, p.reshape(nb, nc)

    def adf_neighbours(self):
        """int32 [n_atoms] in ORIGINAL atom order: neighbours at the last sample (a refused one included), -1 where the atom is central to no column"""
        n = _check(lib().aztot_adf_neighbours(self.h, None, 0))
        out = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().aztot_adf_neighbours(self.h, out.ctypes.data_as(_ip), n))
        return out[:n]

    # ---- static structure factors (aztot_sk_*; the vector set, the order of the sums and the values are stated in include/aztot.h) ----
    def sk_setup(self, kmax, dk, max_per_bin=0):
        """k-vectors with |k| <= kmax in bins of width dk, at most max_per_bin per bin (0: all); (re)allocates and zeroes, returns the number of vectors"""
        return _check(lib().aztot_sk_setup(self.h, float(kmax), float(dk), int(max_per_bin)))

    def sk_sample(self):
        """the per-species amplitudes of the current configuration; adds Re rho_a rho_b* to the sums"""
        _check(lib().aztot_sk_sample(self.h))

    def sk_reset(self):
        _check(lib().aztot_sk_reset(self.h))

    def sk_shape(self):
        """(n_vectors, n_bins, n_pairs, samples)"""
        nk, nb, npair, sm = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().aztot_sk_shape(self.h, C.byref(nk), C.byref(nb), C.byref(npair), C.byref(sm)))
        return nk.value, nb.value, npair.value, sm.value

    def sk_vectors(self):
        """(lmn[n_vectors, 3], bin[n_vectors]) - int32, in ascending lexicographic order of (l, m, n)"""
        nk = self.sk_shape()[0]
        lmn, b = np.zeros(3 * nk, dtype=np.int32), np.zeros(nk, dtype=np.int32)
        _check(lib().aztot_sk_vectors(self.h, lmn.ctypes.data_as(_ip), b.ctypes.data_as(_ip), nk))
        return lmn.reshape(nk, 3), b

    def sk_amplitudes(self):
        """rho[n_vectors, n_species, 2] of the last sample: (re, im) of sum_j exp(i k r_j) over the atoms of each species"""
        nk = self.sk_shape()[0]
        n = _check(lib().aztot_sk_amplitudes(self.h, None, 0))
        out = np.zeros(n)
        _check(lib().aztot_sk_amplitudes(self.h, out.ctypes.data_as(_dp), n))
        return out.reshape(nk, -1, 2)

    def sk_sums(self):
        """(samples, acc[n_vectors, n_pairs]): Re rho_a rho_b* summed over the samples, pairs a <= b in the RDF's pair order"""
        nk, _, npair, _ = self.sk_shape()
        out = np.zeros(nk * npair)
        samples = C.c_int64()
        _check(lib().aztot_sk_sums(self.h, C.byref(samples), out.ctypes.data_as(_dp), out.size))
        return samples.value, out.reshape(nk, npair)

    def sk_values(self):
        """(k[n_bins], n_in_bin[n_bins], S[n_bins], S_ab[n_bins, n_pairs]): bin centres, kept vectors per bin, the total and the Ashcroft-Langreth partials
        (means over the vectors of a bin; 0 where n_in_bin is 0)"""
        _, nb, npair, _ = self.sk_shape()
        k, cnt, tot, part = np.zeros(nb), np.zeros(nb, dtype=np.int32), np.zeros(nb), np.zeros(nb * npair)
        _check(lib().aztot_sk_values(self.h, k.ctypes.data_as(_dp), cnt.ctypes.data_as(_ip), tot.ctypes.data_as(_dp), part.ctypes.data_as(_dp), part.size))
        return k, cnt, tot, part.reshape(nb, npair)

    # ---- bond-orientational order (aztot_boo_*; bonds, values, the order of the sums and the totals are stated in include/aztot.h) ----
    def boo_setup(self, radius, orders, n_bins, central_mask, ligand_mask, reserved=0):
        """Steinhardt q_l and the neighbour-averaged form for the given orders l; the masks have bit s for species s; (re)allocates and zeroes, returns n_bins"""
        p = _BooParams()
        p.radius, p.central_mask, p.ligand_mask, p.n_orders, p.n_bins, p.reserved = float(radius), int(central_mask), int(ligand_mask), len(orders), int(n_bins), int(reserved)
        for o, l in enumerate(list(orders)[:4]):
            p.orders[o] = int(l)
        return _check(lib().aztot_boo_setup(self.h, C.byref(p)))

    def boo_sample(self):
        """the per-atom values of the current configuration; adds them to the totals"""
        _check(lib().aztot_boo_sample(self.h))

    def boo_reset(self):
        _check(lib().aztot_boo_reset(self.h))

    def boo_shape(self):
        """(orders, n_bins, n_species, samples)"""
        no, nb, ns, sm = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        orders = np.zeros(4, dtype=np.int32)
        _check(lib().aztot_boo_shape(self.h, C.byref(no), orders.ctypes.data_as(_ip), C.byref(nb), C.byref(ns), C.byref(sm)))
        return tuple(int(l) for l in orders[:no.value]), nb.value, ns.value, sm.value

    def boo_per_atom(self):
        """(n[n_atoms] int32, q[n_atoms, n_orders, 2]) of the last sample in ORIGINAL atom order: neighbours (-1: not central), q_l (kind 0) and q-bar_l (kind 1)"""
        no = len(self.boo_shape()[0])
        n = _check(lib().aztot_boo_per_atom(self.h, None, None, 0))
        cnt, q = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1) * no * 2)
        _check(lib().aztot_boo_per_atom(self.h, cnt.ctypes.data_as(_ip), q.ctypes.data_as(_dp), n))
        return cnt[:n], q[:n * no * 2].reshape(n, no, 2)

    def boo_qlm(self):
        """complex q_lm[n_atoms, n_orders, 13] of the last sample in ORIGINAL atom order, m = 0 ... 12 (zeros past m = l)"""
        no = len(self.boo_shape()[0])
        n = _check(lib().aztot_boo_qlm(self.h, None, 0))
        out = np.zeros(max(n, 1))
        _check(lib().aztot_boo_qlm(self.h, out.ctypes.data_as(_dp), n))
        out = out[:n].reshape(-1, no, 13, 2)
        return out[..., 0] + 1j * out[..., 1]

    def boo_counts(self):
        """(samples, hist[2, n_orders, n_species, n_bins] uint64, sums[2, n_orders, n_species], entered[n_species] uint64)"""
        orders, nb, ns, _ = self.boo_shape()
        no = len(orders)
        hist, sums, entered = np.zeros(2 * no * ns * nb, dtype=np.uint64), np.zeros(2 * no * ns), np.zeros(ns, dtype=np.uint64)
        samples = C.c_int64()
        u64 = C.POINTER(C.c_uint64)
        _check(lib().aztot_boo_counts(self.h, C.byref(samples), hist.ctypes.data_as(u64), sums.ctypes.data_as(_dp), entered.ctypes.data_as(u64), hist.size))
        return samples.value, hist.reshape(2, no, ns, nb), sums.reshape(2, no, ns), entered

    def boo_values(self):
        """(centre[n_bins], density[2, n_orders, n_species, n_bins] per unit q, mean[2, n_orders, n_species])"""
        orders, nb, ns, _ = self.boo_shape()
        no = len(orders)
        centre, dens, mean = np.zeros(nb), np.zeros(2 * no * ns * nb), np.zeros(2 * no * ns)
        _check(lib().aztot_boo_values(self.h, centre.ctypes.data_as(_dp), dens.ctypes.data_as(_dp), mean.ctypes.data_as(_dp), dens.size))
        return centre, dens.reshape(2, no, ns, nb), mean.reshape(2, no, ns)

    def close(self):
        if getattr(self, "h", None):
            lib().aztot_free_device(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    """HIP devices visible to this process (through libaztot, i.e. the system ROCm runtime: importing torch into a process that later
    brings up RCCL would put torch's bundled, un-initialised HSA copy in front of it)."""
    return int(lib().aztot_device_count())


def device_synchronize(device=0):
    """hipDeviceSynchronize through libaztot (the bracket of a timed region; no torch needed in the process)"""
    _check(lib().aztot_device_synchronize(int(device)))


def rccl_unique_id():
    L = lib()
    n = L.aztot_comm_id_bytes()
    buf = C.create_string_buffer(n)
    _check(L.aztot_comm_make_id(buf))
    return buf.raw


def rccl_selftest(device=0):
    """One-rank RCCL communicator: ring exchange with itself + all-reduces (raises AztotError if RCCL is unusable here)."""
    _check(lib().aztot_comm_selftest(device))
