// C ABI (include/aztot.h) over the C++ host side.  Every entry point catches exceptions and turns them
// into an error code + thread-local message (the reference prints "ERROR[..]" and returns 0).
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "engine.h"
#include "exchange.h"
#include "model.h"

using namespace aztot;

struct aztot_model { Model m; bool finished = false; };
struct aztot_md
{
    std::unique_ptr<Exchanger> xch;
    std::unique_ptr<Engine> eng;
};

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

int classify(const std::string& msg)
{
    if (msg.find("out of scope") != std::string::npos) return AZTOT_ERR_INPUT;
    if (msg.find("can't open") != std::string::npos) return AZTOT_ERR_IO;
    if (msg.find("HIP") != std::string::npos) return AZTOT_ERR_DEVICE;
    if (msg.find("RCCL") != std::string::npos || msg.find("slab") != std::string::npos) return AZTOT_ERR_COMM;
    return AZTOT_ERR_INPUT;
}

template <typename F>
int guarded(F&& f)
{
    try { f(); g_err.clear(); return AZTOT_OK; }
    catch (const ArgError& e) { return fail(AZTOT_ERR_ARG, e.what()); }
    catch (const std::exception& e) { return fail(classify(e.what()), e.what()); }
    catch (...) { return fail(AZTOT_ERR_ARG, "unknown exception"); }
}
}  // namespace

extern "C" {

const char* aztot_last_error(void) { return g_err.c_str(); }
#ifndef AZTOT_SRC_HASH
#define AZTOT_SRC_HASH "unknown"
#endif
// "... src <16 hex digits>": a digest of every source file the library was compiled from (csrc/Makefile)
const char* aztot_version(void) { return "aztotmd_amd 0.4 (gfx950, fp64) src " AZTOT_SRC_HASH; }

int aztot_init_md(const char* dir, aztot_model** out)
{
    if (!dir || !out) return fail(AZTOT_ERR_ARG, "null argument");
    *out = nullptr;
    return guarded([&] {
        auto h = std::make_unique<aztot_model>();
        init_md(dir, h->m);
        *out = h.release();
    });
}

int aztot_model_create(const aztot_system* sys, aztot_model** out)
{
    if (!sys || !out) return fail(AZTOT_ERR_ARG, "null argument");
    *out = nullptr;
    return guarded([&] {
        auto h = std::make_unique<aztot_model>();
        model_from_system(*sys, h->m);
        *out = h.release();
    });
}

int aztot_model_set_bonded(aztot_model* h, const aztot_bonded* b)
{
    if (!h || !b) return fail(AZTOT_ERR_ARG, "null argument");
    if (b->n_bond_types < 0 || b->n_angle_types < 0 || b->n_bonds < 0 || b->n_angles < 0) return fail(AZTOT_ERR_ARG, "negative count in aztot_bonded");
    if ((b->n_bond_types && !b->bond_types) || (b->n_angle_types && !b->angle_types) || (b->n_bonds && !(b->bond_a && b->bond_b && b->bond_type)) ||
        (b->n_angles && !(b->angle_c && b->angle_l1 && b->angle_l2 && b->angle_type)))
        return fail(AZTOT_ERR_ARG, "null array in aztot_bonded");
    return guarded([&] {
        Model m = h->m;                 // all-or-nothing: the model is replaced only if every line is accepted
        m.bondTypes.clear(); m.angleTypes.clear();
        for (int i = 0; i < b->n_bond_types; i++) add_bond_type(m, b->bond_types[i].spec_a, b->bond_types[i].spec_b, b->bond_types[i].type, b->bond_types[i].p);
        for (int i = 0; i < b->n_angle_types; i++) add_angle_type(m, b->angle_types[i].central, b->angle_types[i].type, b->angle_types[i].k, b->angle_types[i].cos0);
        set_bond_list(m, b->n_bonds, b->bond_a, b->bond_b, b->bond_type);
        set_angle_list(m, b->n_angles, b->angle_c, b->angle_l1, b->angle_l2, b->angle_type);
        h->m = std::move(m);
    });
}

void aztot_free_md(aztot_model* m) { delete m; }

int aztot_model_species_name(const aztot_model* m, int i, char* buf, int cap)
{
    if (!m || !buf || cap <= 0 || i < 0 || i >= m->m.nSpec()) return fail(AZTOT_ERR_ARG, "bad argument");
    std::snprintf(buf, (size_t)cap, "%s", m->m.species[i].name.c_str());
    return AZTOT_OK;
}

int aztot_model_nucleus_name(const aztot_model* m, int i, char* buf, int cap)
{
    if (!m || !buf || cap <= 0) return fail(AZTOT_ERR_ARG, "bad argument");
    const Nuclei n = nuclei_of(m->m);
    if (i < 0 || i >= (int)n.names.size()) return fail(AZTOT_ERR_ARG, "bad argument");
    std::snprintf(buf, (size_t)cap, "%s", n.names[i].c_str());
    return AZTOT_OK;
}

// Keys (all values returned as doubles):
//  n_atoms n_species box dt nstep nequil eqfreq temperature tstat_type elec_type r_real alpha scale scale2 daipi2
//  rmax r2max degfree tkin cell_list use_cell_list stat init_vel elecfield nthread kB m_scale fcoul
//  species (per species: mass_amu, mass, charge, charged, frozen, rMass_hdt, radA, radB, mxEng, number)
//  vdw (per ordered species pair a*nSpec+b: type, r2cut, p0..p4, use_radii)
//  ewald (kx, ky, kz, mr4a2, rkcut2, engElec1, number of k-vectors)  kvecs (l, m, n, rkx, rky, rkz, akk per k-vector)
//  spme (Kx, Ky, Kz, order, scale: the 'elec spme' line of control.txt, our extension, and the el_scale its energy and potential carry; zeros without one)
//  n_bonded (bond types, angle types, bonds, angles)  bond_types (type, spec1, spec2, p0..p4)  angle_types (type, central, k, cos0)
//  bonds (at1, at2, type id per bond, after the turn of read_bondlist)  angles (central, lig1, lig2, type id)
//  rdf (present, rmax, dr, every, out_every, nucl: the 'rdf' line of control.txt; present = 0 without one)
//  nuclei (nucleus index of each species)  n_nuclei
//  outcn (present, R, nCentral, nLigand, central species ids..., ligand species ids...: the 'outCN' line of control.txt; 0, 0, 0, 0 without one)
//  ncn (n, then per line: central nucleus, ligand nucleus, R: the 'ncn' block of control.txt; n = 0 without one)
//  vaf (steps between two rows of vaf.dat: the 'vaf' line of control.txt; 0 without one)
//  stress (steps between two rows of stress.dat: the 'stress' line of control.txt, our extension; 0 without one)
//  adf (n_bins, every, n, then per line: central, ligand_a, ligand_b species ids, R_a, R_b: the 'adf' block of control.txt, our extension; 0, 0, 0 without one)
//  boo (R, n_bins, every, central_mask, ligand_mask, n_orders, then the orders: the 'boo' line of control.txt, our extension; n_bins = 0 without one)
//  sk (kmax, dk, every, max_per_bin: the 'strfac' line of control.txt, our extension; kmax = 0 without one)
//  types x y z vx vy vz   (per atom)    photons uvx uvy uvz (radiative thermostat tables; seed = first element of `out` on entry for photons)
int aztot_model_query(const aztot_model* h, const char* key, double* out, int cap)
{
    if (!h || !key) return fail(AZTOT_ERR_ARG, "null argument");
    Model m = h->m;                       // derived values are computed on a copy: querying never mutates the model
    int rc = AZTOT_ERR_ARG;
    const uint64_t seed_in = (out && cap > 0 && out[0] >= 0 && out[0] < 1.8e19) ? (uint64_t)out[0] : 12345;
    int status = guarded([&] {
        finish_model(m, 12345);
        std::vector<double> v;
        const std::string k = key;
        auto per_atom = [&](const std::vector<double>& a) { v = a; };
        if (k == "n_atoms") v = {(double)m.nAt};
        else if (k == "n_species") v = {(double)m.nSpec()};
        else if (k == "box") v = {m.L[0], m.L[1], m.L[2]};
        else if (k == "dt") v = {m.tSt};
        else if (k == "nstep") v = {(double)m.nSt};
        else if (k == "nequil") v = {(double)m.nEq};
        else if (k == "eqfreq") v = {(double)m.freqEq};
        else if (k == "temperature") v = {m.Temp};
        else if (k == "tstat_type") v = {(double)m.tstat_type};
        else if (k == "elec_type") v = {(double)m.elec_type};
        else if (k == "r_real") v = {m.rReal};
        else if (k == "alpha") v = {m.alpha};
        else if (k == "scale") v = {m.el_scale};
        else if (k == "scale2") v = {m.el_scale2};
        else if (k == "daipi2") v = {m.daipi2};
        else if (k == "rmax") v = {m.rMax};
        else if (k == "r2max") v = {m.r2Max};
        else if (k == "degfree") v = {(double)m.degFree};
        else if (k == "tkin") v = {m.tKin};
        else if (k == "cell_list") v = {m.desired_cell_size};
        else if (k == "use_cell_list") v = {(double)m.use_clist};
        else if (k == "stat") v = {(double)m.stat};
        else if (k == "init_vel") v = {(double)m.init_vel, m.init_vel_par[0], m.init_vel_par[1], m.init_vel_par[2]};
        else if (k == "elecfield") v = {m.E[0], m.E[1], m.E[2]};
        else if (k == "nthread") v = {(double)m.nthread_a, (double)m.nthread_b, (double)m.nstep_stat};
        else if (k == "kB") v = {units::kB};
        else if (k == "m_scale") v = {units::m_scale};
        else if (k == "fcoul") v = {units::Fcoul_scale};
        else if (k == "n_warnings") v = {(double)m.warnings.size()};
        else if (k == "species")
            for (const auto& s : m.species)
            { double r[] = {s.mass_amu, s.mass, s.charge, (double)s.charged, (double)s.frozen, s.rMass_hdt, s.radA, s.radB, s.mxEng, (double)s.number}; v.insert(v.end(), r, r + 10); }
        else if (k == "vdw")
            for (const auto& p : m.pairpots)
            { double r[] = {(double)p.type, p.r2cut, p.p0, p.p1, p.p2, p.p3, p.p4, (double)p.use_radii}; v.insert(v.end(), r, r + 8); }
        else if (k == "ewald") { v = {(double)m.ewald_k[0], (double)m.ewald_k[1], (double)m.ewald_k[2], m.mr4a2, m.rkcut2, m.engElec1, (double)m.kvecs.size()}; }
        else if (k == "spme") v = {(double)m.spme_mesh[0], (double)m.spme_mesh[1], (double)m.spme_mesh[2], (double)m.spme_order, m.elec_type == AZTOT_ELEC_SPME ? m.el_scale : 0.0};
        else if (k == "kvecs")
            for (const auto& q : m.kvecs) { double r[] = {(double)q.l, (double)q.m, (double)q.n, q.rkx, q.rky, q.rkz, q.akk}; v.insert(v.end(), r, r + 7); }
        else if (k == "n_bonded") v = {(double)m.bondTypes.size(), (double)m.angleTypes.size(), (double)m.bondA.size(), (double)m.angC.size()};
        else if (k == "bond_types")
            for (const auto& b : m.bondTypes)
            { double r[] = {(double)b.type, (double)b.spec1, (double)b.spec2, b.p[0], b.p[1], b.p[2], b.p[3], b.p[4]}; v.insert(v.end(), r, r + 8); }
        else if (k == "angle_types")
            for (const auto& a : m.angleTypes) { double r[] = {(double)a.type, (double)a.central, a.k, a.cos0}; v.insert(v.end(), r, r + 4); }
        else if (k == "bonds")
            for (size_t i = 0; i < m.bondA.size(); i++) { v.push_back(m.bondA[i]); v.push_back(m.bondB[i]); v.push_back(m.bondT[i]); }
        else if (k == "angles")
            for (size_t i = 0; i < m.angC.size(); i++) { v.push_back(m.angC[i]); v.push_back(m.angL1[i]); v.push_back(m.angL2[i]); v.push_back(m.angT[i]); }
        else if (k == "rdf") v = {(double)m.rdf_present, m.rdf_rmax, m.rdf_dr, (double)m.rdf_every, (double)m.rdf_out_every, (double)m.rdf_nucl};
        else if (k == "outcn")
        {
            v = {(double)m.outcn_present, m.outcn_radius, (double)m.outcn_central.size(), (double)m.outcn_ligand.size()};
            for (int j : m.outcn_central) v.push_back(j);
            for (int j : m.outcn_ligand) v.push_back(j);
        }
        else if (k == "ncn")
        {
            v = {(double)m.ncn_central.size()};
            for (size_t i = 0; i < m.ncn_central.size(); i++) { v.push_back(m.ncn_central[i]); v.push_back(m.ncn_ligand[i]); v.push_back(m.ncn_radius[i]); }
        }
        else if (k == "vaf") v = {(double)m.vaf};
        else if (k == "stress") v = {(double)m.stress};
        else if (k == "adf")
        {
            v = {(double)m.adf_bins, (double)m.adf_every, (double)m.adf_cols.size()};
            for (const auto& c : m.adf_cols) { v.push_back(c.central); v.push_back(c.ligand_a); v.push_back(c.ligand_b); v.push_back(c.radius_a); v.push_back(c.radius_b); }
        }
        else if (k == "sk") v = {m.sk_kmax, m.sk_dk, (double)m.sk_every, (double)m.sk_max_per_bin};
        else if (k == "boo")
        {
            v = {m.boo.radius, (double)m.boo.n_bins, (double)m.boo_every, (double)m.boo.central_mask, (double)m.boo.ligand_mask, (double)m.boo.n_orders};
            for (int o = 0; o < m.boo.n_orders; o++) v.push_back(m.boo.orders[o]);
        }
        else if (k == "nuclei") { for (int j : nuclei_of(m).of) v.push_back(j); }
        else if (k == "n_nuclei") v = {(double)nuclei_of(m).names.size()};
        else if (k == "types") { v.resize(m.nAt); for (int i = 0; i < m.nAt; i++) v[i] = m.types[i]; }
        else if (k == "x") per_atom(m.x);
        else if (k == "y") per_atom(m.y);
        else if (k == "z") per_atom(m.z);
        else if (k == "vx") per_atom(m.vx);
        else if (k == "vy") per_atom(m.vy);
        else if (k == "vz") per_atom(m.vz);
        else if (k == "photons") { v.resize(m.nAt); photon_engs(m.nAt, v.data(), m.Temp, seed_in); }
        else if (k == "uvects") { v.resize(3 * kNumUnitVectors); unit_vectors(v.data(), v.data() + kNumUnitVectors, v.data() + 2 * kNumUnitVectors); }
        else throw std::runtime_error(std::string("unknown query key: ") + key);
        rc = (int)v.size();
        if (out && cap >= rc) std::memcpy(out, v.data(), sizeof(double) * v.size());
    });
    return status == AZTOT_OK ? rc : status;
}

int aztot_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n < 0 ? 0 : n;
}

int aztot_device_synchronize(int device)
{
    return guarded([&] {
        check_hip(hipSetDevice(device), "hipSetDevice");
        check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
    });
}

void aztot_default_options(aztot_options* opt)
{
    if (!opt) return;
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (uint32_t)sizeof(*opt);
    opt->device = 0;
    opt->initial_forces = 1;
    opt->center_box = 0;
    opt->seed = 12345;
    opt->pair_variant = 0;
    opt->cell_size = 0.0;
    opt->use_graph = 1;
    opt->profile = 0;
    opt->sort_every = 0;
    opt->skin = 0.0;
}

static int init_device_common(const aztot_model* h, const aztot_options* opt, int rank, int nranks, const void* id_bytes,
                              aztot_sendrecv_fn sr, aztot_allreduce_fn ar, void* ctx, aztot_md** out)
{
    if (!h || !out) return fail(AZTOT_ERR_ARG, "null argument");
    *out = nullptr;
    aztot_options o;
    if (opt)
    {
        if (opt->struct_size != (uint32_t)sizeof(aztot_options))
            return fail(AZTOT_ERR_ARG, "aztot_options.struct_size does not match this library (start from aztot_default_options)");
        o = *opt;
        for (int r : o.reserved) if (r != 0) return fail(AZTOT_ERR_ARG, "aztot_options.reserved must be zero");
        if (o.pair_variant < 0 || o.pair_variant > 2) return fail(AZTOT_ERR_ARG, "aztot_options.pair_variant: 0 (automatic), 1 or 2 (variant 3 was retired: measured slower than 2)");
    }
    else aztot_default_options(&o);
    return guarded([&] {
        Model m = h->m;
        finish_model(m, o.seed);
        if (o.center_box) center_box(m);
        auto md = std::make_unique<aztot_md>();
        if (nranks > 1)
        {
            if (rank < 0 || rank >= nranks) throw std::runtime_error("slab: bad rank");
            if (id_bytes)
            {
                int ndev = 0;
                if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw std::runtime_error("no HIP device available: the azTotMD hot path has no CPU fallback");
                check_hip(hipSetDevice(o.device), "hipSetDevice");
                md->xch.reset(new RcclExchanger(rank, nranks, id_bytes));
            }
            else if (sr && ar) md->xch.reset(new CallbackExchanger(sr, ar, ctx));
            else if (!o.loopback_ranks) throw std::runtime_error("slab: neither an RCCL id nor exchange callbacks were given");
        }
        md->eng.reset(new Engine(m, o, rank, nranks, md->xch.get()));
        *out = md.release();
    });
}

int aztot_init_device(const aztot_model* m, const aztot_options* opt, aztot_md** out)
{
    return init_device_common(m, opt, 0, 1, nullptr, nullptr, nullptr, nullptr, out);
}

int aztot_init_device_slab(const aztot_model* m, const aztot_options* opt, int rank, int nranks, const void* rccl_id_bytes,
                           aztot_sendrecv_fn sendrecv, aztot_allreduce_fn allreduce, void* ctx, aztot_md** out)
{
    return init_device_common(m, opt, rank, nranks, rccl_id_bytes, sendrecv, allreduce, ctx, out);
}

void aztot_free_device(aztot_md* md) { delete md; }

int aztot_step(aztot_md* md, int nsteps)
{
    if (!md) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->step(nsteps); });
}

int aztot_sync(aztot_md* md)
{
    if (!md) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->sync_all(); });
}

int aztot_forces(aztot_md* md)
{
    if (!md) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->forces(); });
}

int aztot_get_stats(aztot_md* md, aztot_stats* out)
{
    if (!md || !out) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { md->eng->get_stats(*out); });
}

int aztot_species_crossings(aztot_md* md, int64_t* out, int cap)
{
    if (!md || !md->eng || !out) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { md->eng->species_crossings(out, cap); });
}

int aztot_md_to_host(aztot_md* md, aztot_state* out)
{
    if (!md || !out) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { md->eng->md_to_host(*out); });
}

int aztot_set_state(aztot_md* md, const aztot_state* in)
{
    if (!md || !in) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { md->eng->set_state(*in); });
}

int aztot_get_clock(aztot_md* md, aztot_clock* out)
{
    if (!md || !out) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { md->eng->get_clock(*out); });
}

int aztot_set_clock(aztot_md* md, const aztot_clock* in)
{
    if (!md || !in) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { md->eng->set_clock(*in); });
}

int aztot_cell_table(aztot_md* md, int32_t dims[3], int32_t* cell_start, int cap_cells, int32_t* atom_id, int cap_atoms)
{
    if (!md || !md->eng || !dims) return fail(AZTOT_ERR_ARG, "null argument");
    int n = 0;
    const int rc = guarded([&] { n = md->eng->cell_table(dims, cell_start, cap_cells, atom_id, cap_atoms); });
    return rc < 0 ? rc : n;
}

int aztot_kernel_times(aztot_md* md, char* names, int cap, double* ms, int64_t* calls, int max_kernels)
{
    if (!md) return fail(AZTOT_ERR_ARG, "null handle");
    int n = 0;
    int status = guarded([&] {
        std::vector<KernelTimer> t;
        n = md->eng->kernel_times(t);
        int pos = 0;
        for (int i = 0; i < n && i < max_kernels; i++)
        {
            if (ms) ms[i] = t[i].ms;
            if (calls) calls[i] = t[i].calls;
            const int len = (int)t[i].name.size() + 1;
            if (names && pos + len <= cap) { std::memcpy(names + pos, t[i].name.c_str(), len); pos += len; }
        }
        if (names && pos < cap) names[pos] = 0;
    });
    return status == AZTOT_OK ? n : status;
}

int64_t aztot_spme_mesh(aztot_md* md, int which, void* out, int64_t cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    long long n = 0;
    const int rc = guarded([&] { n = md->eng->spme_mesh(which, out, cap); });
    return rc < 0 ? rc : n;
}

int64_t aztot_spme_influence(aztot_md* md, double* out, int64_t cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    long long n = 0;
    const int rc = guarded([&] { n = md->eng->spme_influence(out, cap); });
    return rc < 0 ? rc : n;
}

int aztot_reset_kernel_times(aztot_md* md)
{
    if (!md) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->reset_kernel_times(); });
}

int aztot_set_profile(aztot_md* md, int on)
{
    if (!md) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->set_profile(on != 0); });
}

int aztot_comm_id_bytes(void) { return RcclExchanger::id_bytes(); }
int aztot_comm_make_id(void* id_bytes)
{
    if (!id_bytes) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { RcclExchanger::make_id(id_bytes); });
}

int aztot_comm_ranks(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int n = 0;
    const int rc = guarded([&] { n = md->eng->comm_ranks(); });
    return rc < 0 ? rc : n;
}

int aztot_comm_selftest(int device)
{
    return guarded([&] { RcclExchanger::selftest(device); });
}

int aztot_rdf_setup(aztot_md* md, double rmax, double dr, int nuclei)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int n = 0;
    const int rc = guarded([&] { n = md->eng->samplers().rdf_setup(rmax, dr, nuclei != 0); });
    return rc < 0 ? rc : n;
}

int aztot_rdf_sample(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().rdf_sample(); });
}

int aztot_rdf_reset(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().rdf_reset(); });
}

int aztot_rdf_shape(aztot_md* md, int kind, int* n_bins, int* n_pairs)
{
    if (!md || !md->eng || !n_bins || !n_pairs) return fail(AZTOT_ERR_ARG, "null argument");
    long long samples = 0;
    return guarded([&] { md->eng->samplers().rdf_counts(kind, *n_bins, *n_pairs, samples, nullptr); });
}

int aztot_rdf_counts(aztot_md* md, int kind, int64_t* samples, uint64_t* counts, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nb = 0, np = 0;
        long long s = 0;
        md->eng->samplers().rdf_counts(kind, nb, np, s, nullptr);
        need = nb * np;
        if (samples) *samples = s;
        if (counts && cap >= need)
        {
            std::vector<unsigned long long> c;
            md->eng->samplers().rdf_counts(kind, nb, np, s, &c);
            for (int k = 0; k < need; k++) counts[k] = c[k];
        }
    });
    return rc < 0 ? rc : need;
}

int aztot_rdf_values(aztot_md* md, int kind, double* r, double* g, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nb = 0, np = 0;
        long long s = 0;
        md->eng->samplers().rdf_counts(kind, nb, np, s, nullptr);
        need = nb * np;
        if (cap < need) return;
        std::vector<double> rv, gv;
        md->eng->samplers().rdf_values(kind, rv, gv);
        if (r) std::memcpy(r, rv.data(), sizeof(double) * rv.size());
        if (g) std::memcpy(g, gv.data(), sizeof(double) * gv.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_cn_setup(aztot_md* md, int kind, const aztot_cn_column* cols, int n_cols)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().cn_setup(kind, cols, n_cols); });
}

int aztot_cn_sample(aztot_md* md, int kind)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().cn_sample(kind); });
}

int aztot_cn_shape(aztot_md* md, int kind, int* n_cols, int* cn_min, int* cn_max)
{
    if (!md || !md->eng || !n_cols || !cn_min || !cn_max) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { md->eng->samplers().cn_shape(kind, *n_cols, *cn_min, *cn_max); });
}

int aztot_cn_per_atom(aztot_md* md, int kind, int32_t* counts, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nc = 0, mn = 0, mx = 0;
        md->eng->samplers().cn_shape(kind, nc, mn, mx);
        const long long want = (long long)md->eng->n_atoms_global() * nc;
        if (want > 0x7fffffffLL) throw ArgError("cn: atoms x columns does not fit the int this call returns");
        need = (int)want;
        if (!counts || cap < need) return;
        std::vector<int32_t> v;
        md->eng->samplers().cn_per_atom(kind, v);
        std::memcpy(counts, v.data(), sizeof(int32_t) * v.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_cn_table(aztot_md* md, int kind, int64_t* table, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nc = 0, mn = 0, mx = 0;
        md->eng->samplers().cn_shape(kind, nc, mn, mx);
        need = std::max(0, mx - mn + 1) * nc;
        if (!table || cap < need) return;
        std::vector<long long> v;
        md->eng->samplers().cn_table(kind, v);
        for (int k = 0; k < need; k++) table[k] = v[k];
    });
    return rc < 0 ? rc : need;
}

int aztot_tcf_setup(aztot_md* md, int n_origins, int origin_every)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int nLags = 0;
    const int rc = guarded([&] { nLags = md->eng->samplers().tcf_setup(n_origins, origin_every); });
    return rc < 0 ? rc : nLags;
}

int aztot_tcf_sample(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().tcf_sample(); });
}

int aztot_tcf_reset(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().tcf_reset(); });
}

int aztot_tcf_shape(aztot_md* md, int* n_lags, int* n_species, int64_t* samples)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] {
        int nl = 0, ns = 0;
        long long sm = 0;
        md->eng->samplers().tcf_shape(nl, ns, sm);
        if (n_lags) *n_lags = nl;
        if (n_species) *n_species = ns;
        if (samples) *samples = sm;
    });
}

int aztot_tcf_sums(aztot_md* md, int lag0, int n, int64_t* count, double* msd_sum, double* vaf_sum, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nl = 0, ns = 0;
        long long sm = 0;
        md->eng->samplers().tcf_shape(nl, ns, sm);
        const bool fill = cap >= (long long)std::max(n, 0) * ns;
        std::vector<long long> c;
        std::vector<double> a, b;
        // (the range is checked whether or not anything is filled)
        md->eng->samplers().tcf_sums(lag0, n, fill && count ? &c : nullptr, fill && msd_sum ? &a : nullptr, fill && vaf_sum ? &b : nullptr);
        need = n * ns;
        for (size_t k = 0; k < c.size(); k++) count[k] = c[k];
        if (!a.empty()) std::memcpy(msd_sum, a.data(), a.size() * sizeof(double));
        if (!b.empty()) std::memcpy(vaf_sum, b.data(), b.size() * sizeof(double));
    });
    return rc < 0 ? rc : need;
}

int aztot_tcf_values(aztot_md* md, int lag0, int n, double* msd, double* vaf, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nl = 0, ns = 0;
        long long sm = 0;
        md->eng->samplers().tcf_shape(nl, ns, sm);
        if (cap < (long long)std::max(n, 0) * ns || (!msd && !vaf)) { md->eng->samplers().tcf_sums(lag0, n, nullptr, nullptr, nullptr); need = n * ns; return; }
        std::vector<double> a, b;
        md->eng->samplers().tcf_values(lag0, n, a, b);
        need = n * ns;
        if (msd && !a.empty()) std::memcpy(msd, a.data(), a.size() * sizeof(double));
        if (vaf && !b.empty()) std::memcpy(vaf, b.data(), b.size() * sizeof(double));
    });
    return rc < 0 ? rc : need;
}

int aztot_stress_setup(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().stress_setup(); });
}

int aztot_stress_sample(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().stress_sample(); });
}

int aztot_stress_get(aztot_md* md, aztot_stress* out)
{
    if (!md || !md->eng || !out) return fail(AZTOT_ERR_ARG, "null argument");
    return guarded([&] { md->eng->samplers().stress_get(*out); });
}

int aztot_stress_per_atom(aztot_md* md, double* w, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        aztot_stress probe;
        md->eng->samplers().stress_get(probe);          // (refuses before the set-up or a sample)
        const long long want = 6LL * md->eng->n_atoms_global();
        if (want > 0x7fffffffLL) throw ArgError("stress: 6 x atoms does not fit the int this call returns");
        need = (int)want;
        if (!w && cap <= 0) return;
        if (!w || cap < need) throw ArgError("stress: cap < 6 * n_atoms");
        std::vector<double> v;
        md->eng->samplers().stress_per_atom(v);
        std::memcpy(w, v.data(), sizeof(double) * v.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_adf_setup(aztot_md* md, int n_bins, const aztot_adf_column* cols, int n_cols)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int nb = 0;
    const int rc = guarded([&] { nb = md->eng->samplers().adf_setup(n_bins, cols, n_cols); });
    return rc < 0 ? rc : nb;
}

int aztot_adf_sample(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().adf_sample(); });
}

int aztot_adf_reset(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().adf_reset(); });
}

int aztot_adf_shape(aztot_md* md, int* n_bins, int* n_cols, int64_t* samples)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] {
        int nb = 0, nc = 0;
        long long sm = 0;
        md->eng->samplers().adf_shape(nb, nc, sm);
        if (n_bins) *n_bins = nb;
        if (n_cols) *n_cols = nc;
        if (samples) *samples = sm;
    });
}

int aztot_adf_edges(aztot_md* md, double* T, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        std::vector<double> v;
        md->eng->samplers().adf_edges(v);
        need = (int)v.size();
        if (!T && cap <= 0) return;
        if (!T || cap < need) throw ArgError("adf: cap < n_bins + 1");
        std::memcpy(T, v.data(), sizeof(double) * v.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_adf_counts(aztot_md* md, int64_t* samples, uint64_t* counts, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nb = 0, nc = 0;
        long long sm = 0;
        md->eng->samplers().adf_shape(nb, nc, sm);
        need = nb * nc;
        if (counts && cap < need) throw ArgError("adf: cap < n_bins * n_cols");
        if (samples) *samples = sm;
        if (!counts) return;
        std::vector<unsigned long long> c;
        md->eng->samplers().adf_counts(c);
        for (int k = 0; k < need; k++) counts[k] = c[k];
    });
    return rc < 0 ? rc : need;
}

int aztot_adf_values(aztot_md* md, double* theta, double* p, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nb = 0, nc = 0;
        long long sm = 0;
        md->eng->samplers().adf_shape(nb, nc, sm);
        need = nb * nc;
        if ((theta || p) && cap < need) throw ArgError("adf: cap < n_bins * n_cols");
        if (!theta && !p) return;
        std::vector<double> tv, pv;
        md->eng->samplers().adf_values(tv, pv);
        if (theta) std::memcpy(theta, tv.data(), sizeof(double) * tv.size());
        if (p) std::memcpy(p, pv.data(), sizeof(double) * pv.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_adf_neighbours(aztot_md* md, int32_t* n, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nb = 0, nc = 0;
        long long sm = 0;
        md->eng->samplers().adf_shape(nb, nc, sm);          // (refuses before the set-up)
        need = md->eng->n_atoms_global();
        if (n && cap < need) throw ArgError("adf: cap < n_atoms");
        std::vector<int32_t> v;
        md->eng->samplers().adf_neighbours(v);              // (refuses before a sample)
        if (n) std::memcpy(n, v.data(), sizeof(int32_t) * v.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_sk_setup(aztot_md* md, double kmax, double dk, int max_per_bin)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int nk = 0;
    const int rc = guarded([&] { nk = md->eng->samplers().sk_setup(kmax, dk, max_per_bin); });
    return rc < 0 ? rc : nk;
}

int aztot_sk_sample(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().sk_sample(); });
}

int aztot_sk_reset(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().sk_reset(); });
}

int aztot_sk_shape(aztot_md* md, int* n_vectors, int* n_bins, int* n_pairs, int64_t* samples)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] {
        int nk = 0, nb = 0, np = 0;
        long long sm = 0;
        md->eng->samplers().sk_shape(nk, nb, np, sm);
        if (n_vectors) *n_vectors = nk;
        if (n_bins) *n_bins = nb;
        if (n_pairs) *n_pairs = np;
        if (samples) *samples = sm;
    });
}

int aztot_sk_vectors(aztot_md* md, int32_t* lmn, int32_t* bin, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nb = 0, np = 0;
        long long sm = 0;
        md->eng->samplers().sk_shape(need, nb, np, sm);
        if ((lmn || bin) && cap < need) throw ArgError("sk: cap < n_vectors");
        if (!lmn && !bin) return;
        std::vector<int32_t> l, b;
        md->eng->samplers().sk_vectors(l, b);
        if (lmn) std::memcpy(lmn, l.data(), sizeof(int32_t) * l.size());
        if (bin) std::memcpy(bin, b.data(), sizeof(int32_t) * b.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_sk_amplitudes(aztot_md* md, double* rho, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nk = 0, nb = 0, np = 0;
        long long sm = 0;
        md->eng->samplers().sk_shape(nk, nb, np, sm);
        int ns = 0;
        while (ns * (ns + 1) / 2 < np) ns++;                // (n_pairs = n_species (n_species + 1) / 2)
        const long long want = 2LL * nk * ns;
        if (want > 0x7fffffffLL) throw ArgError("sk: 2 x vectors x species does not fit the int this call returns");
        need = (int)want;
        if (rho && cap < need) throw ArgError("sk: cap < n_vectors * n_species * 2");
        std::vector<double> v;
        md->eng->samplers().sk_amplitudes(v);               // (refuses before a sample)
        if (rho) std::memcpy(rho, v.data(), sizeof(double) * v.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_sk_sums(aztot_md* md, int64_t* samples, double* acc, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nk = 0, nb = 0, np = 0;
        long long sm = 0;
        md->eng->samplers().sk_shape(nk, nb, np, sm);
        const long long want = (long long)nk * np;
        if (want > 0x7fffffffLL) throw ArgError("sk: vectors x pairs does not fit the int this call returns");
        need = (int)want;
        if (acc && cap < need) throw ArgError("sk: cap < n_vectors * n_pairs");
        if (samples) *samples = sm;
        if (!acc) return;
        std::vector<double> v;
        md->eng->samplers().sk_sums(v);
        std::memcpy(acc, v.data(), sizeof(double) * v.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_sk_values(aztot_md* md, double* k, int32_t* n_in_bin, double* s_total, double* s_pair, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int nk = 0, nb = 0, np = 0;
        long long sm = 0;
        md->eng->samplers().sk_shape(nk, nb, np, sm);
        need = nb * np;
        const bool any = k || n_in_bin || s_total || s_pair;
        if (any && cap < need) throw ArgError("sk: cap < n_bins * n_pairs");
        if (!any) return;
        std::vector<double> kv, tv, pv;
        std::vector<int32_t> nv;
        md->eng->samplers().sk_values(kv, nv, tv, pv);
        if (k) std::memcpy(k, kv.data(), sizeof(double) * kv.size());
        if (n_in_bin) std::memcpy(n_in_bin, nv.data(), sizeof(int32_t) * nv.size());
        if (s_total) std::memcpy(s_total, tv.data(), sizeof(double) * tv.size());
        if (s_pair) std::memcpy(s_pair, pv.data(), sizeof(double) * pv.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_boo_setup(aztot_md* md, const aztot_boo_params* params)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    if (!params) return fail(AZTOT_ERR_ARG, "boo: null params");
    int nb = 0;
    const int rc = guarded([&] { nb = md->eng->samplers().boo_setup(*params); });
    return rc < 0 ? rc : nb;
}

int aztot_boo_sample(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().boo_sample(); });
}

int aztot_boo_reset(aztot_md* md)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] { md->eng->samplers().boo_reset(); });
}

int aztot_boo_shape(aztot_md* md, int* n_orders, int32_t* orders, int* n_bins, int* n_species, int64_t* samples)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    return guarded([&] {
        int no = 0, nb = 0, ns = 0, ord[AZTOT_BOO_MAX_ORDERS];
        long long sm = 0;
        md->eng->samplers().boo_shape(no, nb, ns, sm, ord);
        if (n_orders) *n_orders = no;
        if (orders) for (int o = 0; o < AZTOT_BOO_MAX_ORDERS; o++) orders[o] = ord[o];
        if (n_bins) *n_bins = nb;
        if (n_species) *n_species = ns;
        if (samples) *samples = sm;
    });
}

int aztot_boo_per_atom(aztot_md* md, int32_t* n, double* q, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int no = 0, nb = 0, ns = 0;
        long long sm = 0;
        md->eng->samplers().boo_shape(no, nb, ns, sm);          // (refuses before the set-up)
        need = md->eng->n_atoms_global();
        if ((n || q) && cap < need) throw ArgError("boo: cap < n_atoms");
        std::vector<int32_t> nv;
        std::vector<double> qv;
        md->eng->samplers().boo_per_atom(nv, qv);               // (refuses before a sample)
        if (n) std::memcpy(n, nv.data(), sizeof(int32_t) * nv.size());
        if (q) std::memcpy(q, qv.data(), sizeof(double) * qv.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_boo_qlm(aztot_md* md, double* qlm, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int no = 0, nb = 0, ns = 0;
        long long sm = 0;
        md->eng->samplers().boo_shape(no, nb, ns, sm);
        const long long want = (long long)md->eng->n_atoms_global() * no * 2 * (AZTOT_BOO_MAX_L + 1);
        if (want > 0x7fffffffLL) throw ArgError("boo: n_atoms * n_orders * 26 does not fit an int");
        need = (int)want;
        if (qlm && cap < need) throw ArgError("boo: cap < n_atoms * n_orders * 26");
        std::vector<double> v;
        md->eng->samplers().boo_qlm(v);                         // (refuses before a sample)
        if (qlm) std::memcpy(qlm, v.data(), sizeof(double) * v.size());
    });
    return rc < 0 ? rc : need;
}

int aztot_boo_counts(aztot_md* md, int64_t* samples, uint64_t* hist, double* sums, uint64_t* entered, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int no = 0, nb = 0, ns = 0;
        long long sm = 0;
        md->eng->samplers().boo_shape(no, nb, ns, sm);
        need = 2 * no * ns * nb;
        if (hist && cap < need) throw ArgError("boo: cap < 2 * n_orders * n_species * n_bins");
        if (samples) *samples = sm;
        if (!hist && !sums && !entered) return;
        std::vector<unsigned long long> h, e;
        std::vector<double> s;
        md->eng->samplers().boo_counts(h, s, e);
        if (hist) for (size_t k = 0; k < h.size(); k++) hist[k] = h[k];
        if (sums) std::memcpy(sums, s.data(), sizeof(double) * s.size());
        if (entered) for (size_t k = 0; k < e.size(); k++) entered[k] = e[k];
    });
    return rc < 0 ? rc : need;
}

int aztot_boo_values(aztot_md* md, double* centre, double* density, double* mean, int cap)
{
    if (!md || !md->eng) return fail(AZTOT_ERR_ARG, "null handle");
    int need = 0;
    const int rc = guarded([&] {
        int no = 0, nb = 0, ns = 0;
        long long sm = 0;
        md->eng->samplers().boo_shape(no, nb, ns, sm);
        need = 2 * no * ns * nb;
        if (density && cap < need) throw ArgError("boo: cap < 2 * n_orders * n_species * n_bins");
        if (!centre && !density && !mean) return;
        std::vector<double> c, d, mn;
        md->eng->samplers().boo_values(c, d, mn);
        if (centre) std::memcpy(centre, c.data(), sizeof(double) * c.size());
        if (density) std::memcpy(density, d.data(), sizeof(double) * d.size());
        if (mean) std::memcpy(mean, mn.data(), sizeof(double) * mn.size());
    });
    return rc < 0 ? rc : need;
}

}  // extern "C"
