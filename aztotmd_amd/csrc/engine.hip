// Engine: device management + step driver (see engine.h).
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <array>
#include <cstring>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <tuple>

#include "exchange.h"
#include "bonded.hip.h"
#include "ewald.hip.h"
#include "spme.hip.h"
#include "kernels.hip.h"
#include "pair_tile.hip.h"
#include "pair_list.hip.h"
#include "rdf.hip.h"
#include "cn.hip.h"
#include "adf.hip.h"
#include "sk.hip.h"
#include "tcf.hip.h"
#include "slab.hip.h"

namespace aztot {

void check_hip(hipError_t e, const char* what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}
#define HIP_CHECK(x) check_hip((x), #x)

namespace {
inline int div_up(int a, int b) { return (a + b - 1) / b; }
constexpr int kFuseKickMaxAtoms = 262144;
// volume of the points within r of a box with edges a, b, c: the box, its face slabs, edge quarter-cylinders and corner octants
inline double swept_volume(double a, double b, double c, double r) { return a * b * c + 2.0 * r * (a * b + b * c + c * a) + 3.14159265358979 * r * r * (a + b + c) + 4.18879020478639 * r * r * r; }
constexpr int kLazyCapMax = 128;         // longest sort interval (steps)
constexpr int kListCandMax = 1920;       // the LDS tile of k_pair_list holds candCap + 1 records of 32 B next to a 1 KiB table: below 64 KiB
constexpr int kListIterMax = 248;
constexpr long long kSnapshotKeepSteps = 32;     // a verified snapshot younger than this is kept at the end of a call (Engine::settle)
}  // namespace

void Engine::sync()
{
    HIP_CHECK(hipStreamSynchronize(stream_));
    if (profile_) timers_.drain();
}

void Engine::sync_all()
{
    settle();
    sync();
}

AtomArrays Engine::begin_sample()
{
    if (!failed_.empty()) throw std::runtime_error("this handle failed in an earlier call: " + failed_);
    settle();                       // the deferred end of the last aztot_step call: positions and velocities are those aztot_md_to_host would return
    return cur();
}

DevStats Engine::read_stats()
{
    sync_all();
    DevStats s;
    HIP_CHECK(hipMemcpy(&s, dStats_, sizeof(DevStats), hipMemcpyDeviceToHost));
    return s;
}

Counts Engine::read_counts()
{
    sync_all();
    Counts c;
    HIP_CHECK(hipMemcpy(&c, dCounts_, sizeof(Counts), hipMemcpyDeviceToHost));
    return c;
}

int Engine::kernel_times(std::vector<KernelTimer>& out) { sync_all(); out = timers_.totals(); return (int)out.size(); }
void Engine::reset_kernel_times() { sync_all(); timers_.reset(); }

// ---------------------------------------------------------------------------------------------------
// cell grid: split_cells (cuCellList.cu:9-34, div_type 1: edge >= requested size).  No pair tables are
// built (the reference's are O(nCell^2), cuCellList.cu:516-531): the stencil is walked on the fly with
// half-width ceil(rMax / edge) per axis (cells may be smaller than the cut-off).
// ---------------------------------------------------------------------------------------------------
void Engine::choose_cells()
{
    const Model& m = model_;
    double size = opt_.cell_size > 0 ? opt_.cell_size : ((m.use_clist && m.desired_cell_size > 0) ? m.desired_cell_size : m.rMax);
    if (!(size > 0)) size = std::max(m.L[0], std::max(m.L[1], m.L[2]));
    // Verlet skin (options.skin): the lazy re-sort keeps the cells for as long as no atom has moved farther than skin / 2, which needs a stencil that
    // reaches rc + skin.  When the user asks for cells of about the cut-off (`cell_list 8.5` next to rc 8.5: the reference's split_cells then makes
    // them L / floor(L / 8.5), cuCellList.cu:9-34 - whatever that overhangs the cut-off used to be all the slack there was: 0.05 A on the 361.305 A box,
    // nothing at all on a box of 42 x 8.5 A) the cells are sized rc + skin instead; "edge >= the requested size" still holds.  Deliberately finer or
    // coarser grids are left alone (their stencil reach is what it is).
    skinTarget_ = 0.0;
    const bool lazyWanted = opt_.sort_every != 1 && m.rMax > 0 && m.E[0] == 0.0 && m.E[1] == 0.0 && m.E[2] == 0.0 && opt_.skin >= 0.0;
    if (lazyWanted)
    {
        const double skin = opt_.skin > 0.0 ? opt_.skin : std::min(0.5, std::max(0.15, 0.036 * m.rMax));
        skinTarget_ = skin;
        if (opt_.cell_size <= 0 && size >= 0.95 * m.rMax && size < m.rMax + skin)
        {
            bool ok = true;
            for (int k = 0; k < 3; k++)
            {   // (never at the price of the lazy schedule itself: it wants 5 cells per axis on one GPU, or of a slab split that the finer grid allows)
                const int nFine = (int)std::floor(m.L[k] / size), nSkin = (int)std::floor(m.L[k] / (m.rMax + skin));
                if (nSkin < 5 && nFine >= 5) ok = false;
                if (k == 0 && nranks_ > 1 && nSkin / nranks_ < 2) ok = false;
            }
            if (ok) size = m.rMax + skin;
        }
    }
    for (int k = 0; k < 3; k++)
    {
        int n = (int)std::floor(m.L[k] / size);
        if (n < 1) n = 1;
        if (n > 1024) n = 1024;
        if (k == 0 && nranks_ > 1 && n % nranks_ != 0)
        {   // slab decomposition: the step is as slow as the rank with the most layers (41 layers on 8 ranks: seven of 5 and one of 6 - 85 % efficiency at
            // best), so a few per cent longer cells along x are the better deal when they make the layers divide evenly
            const int even = n - n % nranks_;
            if (even >= 2 * nranks_ && (double)n / even <= 1.08) n = even;
        }
        P_.nc[k] = n;
        P_.csz[k] = m.L[k] / n;
        P_.icsz[k] = n / m.L[k];
        int hw = (m.rMax > 0) ? (int)std::ceil(m.rMax / P_.csz[k] - 1e-12) : 0;
        if (hw < 0) hw = 0;
        P_.hw[k] = hw;
        P_.nOff[k] = std::min(2 * hw + 1, n);
    }
    if (nranks_ > 1)
    {
        // slab decomposition along x: contiguous, balanced runs of cell layers
        const int n = P_.nc[0], hw = std::max(P_.hw[0], 1);
        P_.hw[0] = hw;
        const int lo = (int)((long long)n * rank_ / nranks_), hi = (int)((long long)n * (rank_ + 1) / nranks_);
        if (hi - lo < 2 * hw)
            throw std::runtime_error("slab decomposition: every rank needs at least 2*ceil(rc/cell) cell layers along x");
        if ((hi - lo) + 2 * hw > n)
            throw std::runtime_error("slab decomposition: ghost layers would overlap the rank's own layers (box too small for this rank count)");
        P_.cx0 = lo - hw;
        P_.ncxLocal = (hi - lo) + 2 * hw;
        P_.xlo = lo * P_.csz[0];
        P_.xhi = hi * P_.csz[0];
        P_.nOff[0] = 2 * hw + 1;
    }
    else
    {
        P_.cx0 = 0; P_.ncxLocal = P_.nc[0]; P_.xlo = 0.0; P_.xhi = m.L[0];
    }
    P_.nCellLocal = P_.ncxLocal * P_.nc[1] * P_.nc[2];
}

Engine::Engine(const Model& model, const aztot_options& opt, int rank, int nranks, Exchanger* xch)
    : model_(model), opt_(opt), rank_(rank), nranks_(nranks), xch_(xch)
{
    try { construct(); }
    catch (...) { release(); throw; }      // ~Engine does not run for a constructor that throws: free the stream and every allocation here
}

void Engine::construct()
{
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        throw std::runtime_error("no HIP device available: the azTotMD hot path has no CPU fallback");
    if (opt_.device < 0 || opt_.device >= ndev) throw std::runtime_error("HIP device ordinal out of range");
    HIP_CHECK(hipSetDevice(opt_.device));
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    if (nranks_ > 1)
    {
        HIP_CHECK(hipStreamCreateWithFlags(&commStream_, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&evIntegrated_, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&evHalo_, hipEventDisableTiming));
    }
    profile_ = opt_.profile != 0;
    if (const char* dbg = std::getenv("AZTOT_DEBUG")) debug_ = (unsigned)std::strtoul(dbg, nullptr, 0);
    if (opt_.energies_every_step) debug_ |= DBG_ENERGIES_EVERY_STEP;
    // (the radiative thermostat kicks atoms at random - a photon's momentum E / (m c) with the reference's c -, so the longest step of the next window is
    //  not bounded by the trend of the last ones: case study 2 ran into violations at 1.15)
    if (model_.tstat_type == AZTOT_TSTAT_RADI) lazyMargin_ = 1.3;
    if (const char* e = std::getenv("AZTOT_MARGIN")) lazyMargin_ = std::max(1.0, std::atof(e));      // (experiments: K steps of the longest step seen may use slack / margin)
    if (nranks_ > 1 && !xch_ && !opt_.loopback_ranks) throw std::runtime_error("slab decomposition needs an exchanger");

    const Model& m = model_;
    if (m.elec_type == AZTOT_ELEC_SPME)
    {   // what the mesh sum cannot do is refused before anything is allocated ("out of scope" -> AZTOT_ERR_INPUT)
        if (nranks_ > 1) throw std::runtime_error("out of scope: 'elec spme' runs on one GPU only: the mesh is not decomposed over slab ranks (use elec pme or elec fenn)");
        double qmax = 0.0;
        for (int i = 0; i < m.nAt; i++) qmax = std::max(qmax, std::fabs(m.species[m.types[i]].charge));
        if (!((double)m.nAt * qmax < kSpmeChargeCap))
            throw std::runtime_error("out of scope: 'elec spme': n_atoms * max|q| = " + std::to_string((double)m.nAt * qmax) +
                                     " reaches 2^22 = 4194304: the mesh's 64-bit sums of 2^-40 e could overflow");
    }
    // (an SPME model shows the pair kernels the real-space term of the Ewald sum: no pair kernel knows of the mesh)
    const int elecPair = m.elec_type == AZTOT_ELEC_SPME ? (int)AZTOT_ELEC_EWALD : m.elec_type;
    P_.nSpec = m.nSpec();
    P_.nAtGlobal = m.nAt;
    for (int k = 0; k < 3; k++) { P_.L[k] = m.L[k]; P_.invL[k] = 1.0 / m.L[k]; P_.half[k] = m.L[k] * 0.5; P_.E[k] = m.E[k]; }
    P_.dt = m.tSt;
    P_.r2Max = m.r2Max;
    P_.elec_type = elecPair; P_.alpha = m.alpha; P_.el_scale = m.el_scale; P_.el_scale2 = m.el_scale2; P_.daipi2 = m.daipi2;
    P_.rReal = m.rReal; P_.fcoul = units::Fcoul_scale; P_.sqrtpi = std::sqrt(units::pi);
    P_.tstat = m.tstat_type; P_.nEq = m.nEq; P_.freqEq = m.freqEq; P_.tKin = m.tKin; P_.revDegFree = m.revDegFree; P_.rkB = 1.0 / units::kB;
    if (m.tstat_type == AZTOT_TSTAT_NOSE) { P_.rQmass = 0.5 / m.tKin / m.tau / m.tau; P_.qMassTau2 = 2 * m.tKin; }
    P_.revLight = 3.33567e-5;   // cuTemp.cu:225 (SURVEY C-19: 100x the physical 1/c, kept for behavioural parity)
    P_.radFrac = 0.9;           // cuTemp.cu:639
    P_.radThr = 1e-4;           // cuTemp.cu:747
    P_.numPi = 3.14159;         // cuTemp.cu:228
    P_.seed = opt_.seed;
    P_.rank = rank_; P_.nranks = nranks_;
    P_.debugMask = debug_;
    P_.use_radii = 0;
    for (const auto& p : m.pairpots) if (p.type && p.use_radii) P_.use_radii = 1;
    P_.single_lj = (m.nSpec() == 1 && m.pairpots[0].type == AZTOT_VDW_LJ && m.elec_type == AZTOT_ELEC_NONE) ? 1 : 0;
    P_.ljDropR2 = 1e300;
    if (P_.single_lj)
    {   // fer_lj (vdw.cpp:16-26): f = p2 s^3 (2 s^3 - 1) / r^2 with s = p1 / r^2 (p1 = sigma^2, p2 = 24 eps).  For s >= 1: |f| <= 3 p2 s^7 / p1,
        // so |f| <= 1e5 whenever s^7 <= 1e5 p1 / (3 p2); for s < 1: |f| < p2 / p1.  The kernel evaluates the exact f^2 > 1e10 rule only when
        // some pair of the wave is inside TWICE that r^2 (a liquid never is).
        const PairPot& lj = m.pairpots[0];
        const double ratio = 3.0 * lj.p2 / (1e5 * lj.p1);
        if (ratio > 0.0 && ratio < 1.0 && lj.p2 / lj.p1 < 1e5) P_.ljDropR2 = 2.0 * lj.p1 * std::pow(ratio, 1.0 / 7.0);
    }
    {   // kernel specialisation 2/3: few species, ONE potential family among lnjs / buck / p746 / bmhs for every defined pair, no
        // radius-dependent potential, electrostatics none / direct / Fennell / Ewald inside the domain of the erfcx fit
        int family = 0;
        bool uniform = m.nSpec() <= 4 && !P_.single_lj;
        for (const auto& p : m.pairpots)
        {
            if (p.type == 0) continue;
            if (p.use_radii || p.type < AZTOT_VDW_LJ || p.type > AZTOT_VDW_BHM) uniform = false;
            if (family == 0) family = p.type; else if (family != p.type) family = VDW_MIXED;   // mixed families, type looked up per species pair
        }
        if (family == 0) family = AZTOT_VDW_LJ;          // charges only: any family does, nothing is inside a VdW cut-off
        if ((elecPair == AZTOT_ELEC_FENNEL || elecPair == AZTOT_ELEC_EWALD) && m.alpha * m.rReal > 4.0) uniform = false;
        if (debug_ & DBG_GENERIC_PAIR) uniform = false;
        P_.potSet = uniform ? POTSET_ONE_FAMILY : POTSET_GENERIC;
        P_.vdwFamily = uniform ? family : 0;
        if (uniform && family == AZTOT_VDW_LJ)
        {   // family 6 = Lennard-Jones where EVERY species pair has a potential and none of their cut-offs lies inside the pair test's r2Max (the usual input:
            // one cut-off for everything, C3): the per-pair cut-off test - a table read, a compare and two selects per visit - always passes and is compiled out
            bool always = true;
            for (const auto& p : m.pairpots) if (p.type != AZTOT_VDW_LJ || p.r2cut < m.r2Max) always = false;
            if (always && !(debug_ & DBG_KEEP_VDW_CUT_TEST)) P_.vdwFamily = VDW_LJ_NOCUT;
        }
        if (uniform && family == AZTOT_VDW_LJ)
        {   // the same shortcut for the Lennard-Jones family with charges: |f| <= |f_LJ| + |f_Coulomb|, each held below 0.5e5 beyond its radius.  LJ part
            // as above per species pair; Coulomb part (direct, Fennell, real-space Ewald alike): |f| <= |kqq| (1/r^3 + (2 alpha/sqrt pi)/r^2 + S2/r)
            double r2 = 0.0;
            bool ok = true;
            for (const auto& p : m.pairpots)
            {
                if (p.type == 0) continue;
                const double ratio = 3.0 * p.p2 / (0.5e5 * p.p1);
                if (ratio > 0.0 && ratio < 1.0 && p.p2 / p.p1 < 0.5e5) r2 = std::max(r2, p.p1 * std::pow(ratio, 1.0 / 7.0)); else ok = false;
            }
            double qq = 0.0;
            for (int a = 0; a < m.nSpec(); a++)
                for (int b = 0; b < m.nSpec(); b++) qq = std::max(qq, std::fabs(m.species[a].charge * m.species[b].charge) * units::Fcoul_scale);
            if (m.elec_type != AZTOT_ELEC_NONE && qq > 0.0)
            {
                const double a2 = (m.elec_type == AZTOT_ELEC_DIRECT) ? 0.0 : 2.0 * std::fabs(m.alpha) / std::sqrt(units::pi);
                const double s2 = (m.elec_type == AZTOT_ELEC_FENNEL) ? std::fabs(m.el_scale2) : 0.0;
                double r = 0.01;
                while (r < 100.0 && qq * (1.0 / (r * r * r) + a2 / (r * r) + s2 / r) > 0.5e5) r *= 1.05;
                if (r >= 100.0) ok = false;
                r2 = std::max(r2, r * r);
            }
            if (ok) P_.ljDropR2 = 2.0 * r2;
        }
        // kernel specialisation 4: ONE species with the radius-dependent surk potential and no electrostatics (case study 2)
        if (m.nSpec() == 1 && m.pairpots[0].type == AZTOT_VDW_SURK && m.pairpots[0].use_radii && m.elec_type == AZTOT_ELEC_NONE && !(debug_ & DBG_GENERIC_PAIR))
            P_.potSet = POTSET_ONE_SURK;
    }
    std::memset(&S_, 0, sizeof(S_));
    for (int i = 0; i < m.nSpec(); i++)
    {
        const Species& s = m.species[i];
        S_.mass[i] = s.mass; S_.charge[i] = s.charge; S_.rMhdt[i] = s.rMass_hdt;
        S_.radA[i] = s.radA; S_.radB[i] = s.radB; S_.mxEng[i] = s.mxEng;
        S_.charged[i] = s.charged; S_.frozen[i] = s.frozen;
    }
    choose_cells();
    // which pair kernel runs: 1 per-atom gather (any geometry), 2 one wave per cell with its own LDS tile (+ the pair lists of the lazy re-sort).
    // 0 = the best one that supports the system.  (Round 2's variant 3 - four waves sharing a tile of 16-atom cell bins, measured 8 % slower than 2 - was
    // retired in round 4: NOTES.md.)
    pairVariant_ = opt_.pair_variant == 0 ? 2 : opt_.pair_variant;
    if (pairVariant_ == 2 && !pair_tile_supported(P_)) pairVariant_ = 1;
    allocate();
    upload_bonded();
    upload_ewald();
    upload_spme();
    {
        // who applies the second half-kick on plain NVE steps (nothing is added to the pair forces, nothing rescales velocities)
        const bool plainNve = !(P_.nEq > 0) && P_.tstat == AZTOT_TSTAT_NONE && !hasBonded_ && !has_recip() && !(debug_ & DBG_KICK_EVERY_STEP);
        const int variant = pair_variant();
        // small systems / slabs are bound by launch latency: the tile kernel's epilogue does it (one kernel less: C2 0.083 -> 0.063 ms).
        // Large systems are not: they fold the kick into the next step's streaming k_integrate1_bin.  (Round 2 measured 221 MB per step for that
        // 13-lane read-modify-write of the velocities in the tile kernel of the day; in today's k_pair_list the same three arrays read and three
        // written cost +3-3.7 us and +6 MB of HBM traffic per launch - KICK_BOTH, NOTES.md - which is what the folding below rests on.)
        // Large systems on one GPU that walk pair lists go one step further: on steps that book no energies and are followed by a plain step of the same
        // run, k_pair_list applies this step's second half-kick AND the next step's first and stores the velocity instead of the force (KICK_BOTH); the next
        // step is then a drift (k_drift_plain2: 76 B per atom instead of k_integrate_plain2's 124).  Above the sizes that fuse the next step (they keep what
        // they have); DBG_FOLD_KICK forces it on whatever the size - such an engine neither fuses the next step nor kicks in the tile kernel's epilogue -,
        // DBG_NO_FOLD_KICK switches it off.  Which steps fold: plan_step.
        foldKickOk_ = plainNve && nranks_ == 1 && lists_.on && variant == 2 && P_.tstat != AZTOT_TSTAT_NOSE && !(debug_ & (DBG_NO_FOLD_KICK | DBG_PLAIN_ONE_ATOM)) &&
                      (capacity_ > 2 * kFuseKickMaxAtoms || (debug_ & (DBG_FOLD_KICK | DBG_FOLD_DRIFT))) && !((debug_ & DBG_FUSE_NEXT) && !(debug_ & DBG_NO_FUSE_NEXT));
        // ... and the same lane drifts the atom too (KICK_DRIFT): the step behind a folded one then opens with no launch of its own.  Its positions go to the
        // second set of coordinate arrays next-step fusion uses, swapped in after the launch.  On by size where kick folding is, DBG_FOLD_DRIFT whatever the
        // size (it implies DBG_FOLD_KICK), DBG_NO_FOLD_DRIFT off: KICK_BOTH with k_drift_plain2 behind it, as before
        foldDriftOk_ = foldKickOk_ && !(debug_ & DBG_NO_FOLD_DRIFT) && (capacity_ > 2 * kFuseKickMaxAtoms || (debug_ & DBG_FOLD_DRIFT));
        fuseEpilogue_ = plainNve && variant >= 2 && capacity_ <= kFuseKickMaxAtoms && !(debug_ & DBG_LARGE_KICK_PATH) && !foldKickOk_;
        // (bonded and reciprocal-space forces are added behind the pair kernel and are complete before the next step's integrate kernel just the same: runs with
        //  bonds / angles / the Ewald sum defer the kick too - they cannot take the pair kernel's epilogue, which would kick with the pair forces alone.
        //  M4: one 17 us launch per step less)
        const bool kickCanWait = !(P_.nEq > 0) && P_.tstat == AZTOT_TSTAT_NONE && !(debug_ & DBG_KICK_EVERY_STEP);
        lazyKick_ = kickCanWait && !fuseEpilogue_;
        P_.boundSkip = 0;
        // next-step fusion (NextStep, pair_tile.hip.h): plain NVE (nothing happens between the forces and the next half-kick; on slab ranks the coordinate
        // exchange of the next step simply follows the pair kernel that produced the coordinates), a lazy run that walks
        // pair lists; DBG_NO_FUSE_NEXT switches it off.  Up to ~500 000 atoms per GPU, where a step is bound by launch latency (measured: 40 000 atoms 0.0230 ->
        // 0.0199 ms/step; emulated slab ranks of 143 000 / 250 000 / 333 000 atoms -9 % / -5 % / -4 %): on 1 M atoms the 13-lane stores of the epilogue cost
        // the pair kernel exactly what the streaming k_integrate1_bin<2> costs on its own (111 + 31 -> 140 us); DBG_FUSE_NEXT forces it on there
        // ... and runs with the radiative thermostat (case study 1: 40 000 atoms, two launches per step - the pair kernel and the boundary kernel that closes
        // the step with the thermostat and opens the next): the thermostat acts on one atom at a time, so the lane that closes the atom's step applies it too
        // (k_pair_list<..., TSTAT>) and a step is ONE launch.  Not where the pair kernel reads radii (the thermostat rewrites them while other waves still
        // gather: case study 2's surk potential), not with bonded terms or the Ewald sum (their forces arrive after the pair kernel).
        const bool radiFuse = P_.tstat == AZTOT_TSTAT_RADI && !hasBonded_ && !has_recip() && !(debug_ & DBG_KICK_EVERY_STEP) && !P_.use_radii && P_.potSet != POTSET_ONE_SURK && (P_.single_lj || P_.potSet == POTSET_ONE_FAMILY) &&
                              nranks_ == 1 && capacity_ <= 2 * kFuseKickMaxAtoms;
        fuseNextTstat_ = radiFuse && lists_.on && variant == 2 && !(debug_ & DBG_NO_FUSE_NEXT);
        if (((plainNve && !foldKickOk_ && (capacity_ <= 2 * kFuseKickMaxAtoms || (debug_ & DBG_FUSE_NEXT))) || radiFuse) && lists_.on && variant == 2 && !(debug_ & DBG_NO_FUSE_NEXT))
            fuseNextOk_ = true;
        if (fuseNextOk_ || foldDriftOk_)
            for (int b = 0; b < 2; b++)
                for (int d = 0; d < 3; d++) altXyz_[b][d] = dev_alloc<double>((size_t)capacity_, true);
    }
    // displacement bound instead of the per-atom check on plain steps: wherever k_integrate1_bin<2> opens every plain step (engines that fuse the next
    // step into the pair kernel keep the per-atom check there); DBG_CHECK_EVERY_ATOM switches it off
    P_.boundSkip = (lazyOn_ && !fuseNextOk_ && !(debug_ & DBG_CHECK_EVERY_ATOM)) ? 1 : 0;
    if (nranks_ > 1 && !xch_)
    {   // options.loopback_ranks: loopback measurement mode (see LoopbackExchanger); 2: the model is a box of nranks copies of one period, ids follow the copies
        int copies = 0;
        if (opt_.loopback_ranks == 2)
        {
            if (model_.nAt % nranks_ != 0 || P_.nc[0] % nranks_ != 0)
                throw std::runtime_error("slab loopback over a replicated box: atoms and cell layers along x must divide by the number of ranks");
            copies = nranks_;
        }
        ownedXch_.reset(new LoopbackExchanger((P_.ncxLocal - 2 * P_.hw[0]) * P_.csz[0], P_.L[0], rank_ == 0, rank_ == nranks_ - 1, lay_.mig_offset(), lay_.halo_offset(),
                                              sizeof(MigRec), sizeof(HaloRec), offsetof(MigRec, id), offsetof(HaloRec, id), copies));
        xch_ = ownedXch_.get();
    }
    upload_initial();
    Samplers::Box box;
    for (int k = 0; k < 3; k++) { box.L[k] = P_.L[k]; box.invL[k] = P_.invL[k]; box.half[k] = P_.half[k]; }
    samplers_.reset(new Samplers(*this, model_, box, stream_, nranks_));
}

Engine::~Engine() { release(); }

void Engine::drop_graphs()
{
    for (GraphSlot& g : graphs_)
    {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    graphs_.clear();
    graphCycle_ = 0;
}

Engine::BufState Engine::buf_state() const
{
    BufState b;
    b.cur = cur_;
    for (int k = 0; k < 2; k++)
    {
        b.xyz[k][0] = buf_[k].x; b.xyz[k][1] = buf_[k].y; b.xyz[k][2] = buf_[k].z;
        for (int d = 0; d < 3; d++) b.alt[k][d] = altXyz_[k][d];
    }
    return b;
}

void Engine::set_buf_state(const BufState& b)
{
    cur_ = b.cur;
    for (int k = 0; k < 2; k++)
    {
        buf_[k].x = b.xyz[k][0]; buf_[k].y = b.xyz[k][1]; buf_[k].z = b.xyz[k][2];
        for (int d = 0; d < 3; d++) altXyz_[k][d] = b.alt[k][d];
    }
}

// What the order of destruction cannot express: the streams drain before anything they use goes (the members free their memory, pinned blocks and
// events afterwards, in their destructors - also when the constructor throws)
void Engine::release()
{
    if (stream_) (void)hipStreamSynchronize(stream_);
    drop_graphs();
    if (evIntegrated_) (void)hipEventDestroy(evIntegrated_);
    if (evHalo_) (void)hipEventDestroy(evHalo_);
    evIntegrated_ = evHalo_ = nullptr;
    if (commStream_) { (void)hipStreamSynchronize(commStream_); (void)hipStreamDestroy(commStream_); }
    commStream_ = nullptr;
    if (stream_) (void)hipStreamDestroy(stream_);
    stream_ = nullptr;
}

// a rejected launch configuration (too much LDS, bad grid) is reported by hipGetLastError only: hipStreamSynchronize stays silent
void Engine::check_launch(const char* where)
{
    if (capturing_) return;
    check_hip(hipGetLastError(), where);
}

// the eleven double arrays of an AtomArrays in StateCopy's order (its two int32_t arrays are type, id)
static std::array<double**, 11> double_arrays(AtomArrays& A) { return {&A.x, &A.y, &A.z, &A.vx, &A.vy, &A.vz, &A.fx, &A.fy, &A.fz, &A.U, &A.rad}; }

void Engine::alloc_atoms(AtomArrays& A, bool zero)
{
    for (double** pp : double_arrays(A)) *pp = dev_alloc<double>((size_t)capacity_, zero);
    A.type = dev_alloc<int32_t>((size_t)capacity_, zero); A.id = dev_alloc<int32_t>((size_t)capacity_, zero);
}

void Engine::allocate()
{
    const int N = model_.nAt;
    if (nranks_ > 1)
    {
        // Capacities from the ACTUAL initial population of the x-layers (every rank holds the whole model, so all ranks arrive at
        // the same message size): the fixed-size message is what travels every step, so padding costs link time.
        //   halo      the fullest run of hw consecutive layers + 25 %
        //   migrants  3 % of the fullest layer (an atom moves << one cell per step: v dt / edge ~ 1e-3) + 1024
        //   arrays    this rank's window (owned + ghost layers) + one ghost run + 25 %
        const int ncx = P_.nc[0], hw = P_.hw[0];
        std::vector<long long> hist(ncx, 0);
        for (int i = 0; i < N; i++)
        {
            int gx = (int)std::floor(model_.x[i] * P_.icsz[0]);
            gx %= ncx; if (gx < 0) gx += ncx;
            hist[gx]++;
        }
        long long maxLayer = 0, maxRun = 0, window = 0;
        for (int g = 0; g < ncx; g++)
        {
            maxLayer = std::max(maxLayer, hist[g]);
            long long run = 0;
            for (int k = 0; k < hw; k++) run += hist[(g + k) % ncx];
            maxRun = std::max(maxRun, run);
        }
        for (int l = 0; l < P_.ncxLocal; l++) window += hist[(((P_.cx0 + l) % ncx) + ncx) % ncx];
        // arrays: the received atoms are appended behind the owned range while last step's left ghosts still sit in front of it, so
        // the footprint is window + one more ghost run - NOT bounded by N on a short ring (2 ranks x 3-4 layers), where the window
        // alone already covers most of the box
        capacity_ = (int)(std::ceil((window + maxRun) * 1.25) + 4096);
        lay_.haloCap = (int)std::min<double>((double)N, std::ceil(maxRun * 1.25) + 1024);
        lay_.migCap = (int)std::min<double>((double)N, std::ceil(maxLayer * 0.03) + 1024);
    }
    else capacity_ = N;
    // + 24: a split launch rounds each of its three runs up to 8 workgroups; the clean-up launches behind k_pair_list book into their own slots
    {   // few cells (less than half a residency of waves) and a stencil with columns to share out: several waves per cell in the staging kernel
        const int cells = pair_tile_cells(P_);
        int n = 1;
        if (pair_tile_supported(P_) && !(debug_ & DBG_ONE_WAVE_PER_CELL))
            while (n < 8 && cells * n * 2 <= 4096 && n * 2 <= P_.nOff[0] * P_.nOff[1]) n *= 2;
        if (n == 1 && pair_tile_supported(P_) && !(debug_ & DBG_ONE_WAVE_PER_CELL))
        {   // more cells than that, but a stencil that needs several tiles per cell (dense systems, small cells: expected candidates = density x volume
            // within the cut-off of a cell): two waves per cell, each with half the columns and fewer tile flushes (measured: S40 -8 %, M4 -9 %; four: worse)
            const double vol = swept_volume(P_.csz[0], P_.csz[1], P_.csz[2], model_.rMax);
            const double density = (double)model_.nAt / (model_.L[0] * model_.L[1] * model_.L[2]);
            if (density * vol > 1.15 * kTileCap && P_.nOff[0] * P_.nOff[1] >= 2) n = 2;
        }
        if (opt_.waves_per_cell == 1 || opt_.waves_per_cell == 2 || opt_.waves_per_cell == 4 || opt_.waves_per_cell == 8) n = opt_.waves_per_cell;      // measurements: forced
        split_.n = n;
        split_.capacity = capacity_;
    }
    const int pairBlocks = std::max(div_up(capacity_, kBlock), pair_tile_grid(P_) * std::max(split_.n, kListMaxWaves) + 24 + 3 * pair_cleanup_grid(pair_tile_cells(P_)));
    maxBlocks_ = std::max(div_up(capacity_, kBlock), pairBlocks) + 1;
    const size_t nAtoms = (size_t)capacity_, nCells = (size_t)(P_.nCellLocal + 1);
    for (AtomArrays& A : buf_) alloc_atoms(A, true);
    dCellOf_ = dev_alloc<int32_t>(nAtoms); dSlotOf_ = dev_alloc<int32_t>(nAtoms);
    dTmpId_ = dev_alloc<int32_t>(nAtoms); dTmpSrc_ = dev_alloc<int32_t>(nAtoms); dTmpCell_ = dev_alloc<int32_t>(nAtoms); dCellOfSorted_ = dev_alloc<int32_t>(nAtoms);
    dCellCount_ = dev_alloc<int32_t>(nCells, true); dCellStart_ = dev_alloc<int32_t>(nCells, true);
    dPartials_ = dev_alloc<double>((size_t)PS_COUNT * maxBlocks_, true); dStats_ = dev_alloc<DevStats>(1);
    {
        DevStats zero;
        std::memset(&zero, 0, sizeof(zero));
        zero.vscale = 1.0;          // "no scaling"; only k_scale_decision ever changes it
        zero.vscaleBegin = 1.0;
        HIP_CHECK(hipMemcpy(dStats_, &zero, sizeof(DevStats), hipMemcpyHostToDevice));
    }
    if (split_.n > 1)
    {
        const size_t nb = (size_t)split_.n * capacity_;
        split_.fx = dev_alloc<double>(nb); split_.fy = dev_alloc<double>(nb); split_.fz = dev_alloc<double>(nb);
        split_.arrived = dev_alloc<int32_t>((size_t)P_.nCellLocal, true);
    }
    dCounts_ = dev_alloc<Counts>(1); dChunkTot_ = dev_alloc<int32_t>((size_t)(div_up(P_.nCellLocal, kScanChunk) + 1));
    dEkGlobal_ = dev_alloc<double>(2); dStage_ = dev_alloc<double>((size_t)PS_COUNT * kCollectParts, true);
    if (nranks_ > 1)
    {
        for (int k = 0; k < 4; k++) dMsg_[k] = dev_alloc<char>(lay_.bytes(), true);
        dHaloInfo_ = dev_alloc<int32_t>(HI_COUNT, true);
    }
    const int ns = model_.nSpec();
    std::vector<DevPot> pots((size_t)ns * ns);
    for (int a = 0; a < ns; a++)
        for (int b = 0; b < ns; b++)
        {
            const PairPot& p = model_.pot(a, b);
            DevPot& d = pots[(size_t)a * ns + b];
            d.type = p.type; d.use_radii = p.use_radii; d.p0 = p.p0; d.p1 = p.p1; d.p2 = p.p2; d.p3 = p.p3; d.p4 = p.p4; d.r2cut = p.r2cut;
            // Lennard-Jones uses p0..p2 only (vdw.cpp:283-288: 4 eps, sigma^2, 24 eps); the two free slots carry the force law in powers of 1/r^2 for the
            // one-species kernel (pair_body, PM_ONE_LJ): f = u^4 (A2 u^3 - A1) with u = 1/r^2, A1 = 24 eps sigma^6, A2 = 48 eps sigma^12
            if (p.type == AZTOT_VDW_LJ) { const double s6 = p.p1 * p.p1 * p.p1; d.p3 = p.p2 * s6; d.p4 = 2.0 * p.p2 * s6 * s6; }
        }
    {   // lazy re-sort: no external field (its energy is booked from wrapped coordinates), a stencil that can be widened by one cell on a violation
        // (one GPU), and a slack worth having
        const Model& m = model_;
        double slack = 1e300;
        bool widenOk = true;
        for (int k = 0; k < 3; k++)
        {
            slack = std::min(slack, 0.49 * (P_.hw[k] * P_.csz[k] - m.rMax));
            if (P_.nc[k] < 2 * (P_.hw[k] + 1) + 1) widenOk = false;
        }
        const int sortEvery = opt_.sort_every;                    // 0: adaptive, 1: every step (the reference's schedule), n: at most every n-th step
        // (a slab rank cannot widen its stencil - it holds hw ghost layers -: there a violation is repaired by going back to the last look's snapshot and
        //  running the window again with the cells rebuilt every step, Engine::replay_from_snapshot; the interval keeps a factor 2 in hand)
        lazyOn_ = sortEvery != 1 && (widenOk || nranks_ > 1) && m.rMax > 0 && slack > 1e-3 && m.E[0] == 0.0 && m.E[1] == 0.0 &&
                  m.E[2] == 0.0 && pair_tile_supported(P_);
        lazyCap_ = sortEvery > 1 ? std::min(sortEvery, kLazyCapMax) : kLazyCapMax;
        if (lazyOn_ && (debug_ & DBG_FIXED_INTERVAL)) lazyK_ = lazyCap_;
        // The slack an atom may use is half the skin (both atoms of a pair move).  With a skin (options.skin >= 0) the cells were sized for it and the box
        // may give a little more for free - taken up to a quarter above the target, beyond that it would only lengthen the lists; without one
        // (options.skin < 0) it is capped at 1.2 % of the cut-off as in round 2.
        slack = std::min(slack, skinTarget_ > 0.0 ? 0.5 * 1.25 * skinTarget_ : 0.012 * m.rMax);
        lazySlack_ = lazyOn_ ? slack : 0.0;
        P_.lazySlack2 = lazySlack_ * lazySlack_;
        const double rp = m.rMax + 2.0 * lazySlack_;
        P_.pruneR2 = rp * rp * (1.0 + 1e-12);
        if (lazyOn_)
        {
            ref_.x = dev_alloc<double>(nAtoms); ref_.y = dev_alloc<double>(nAtoms); ref_.z = dev_alloc<double>(nAtoms);
            if (capacity_ < (1 << 26) && !(debug_ & DBG_NO_LISTS))          // atom index + 6 bits of image code in 32 bits
                lists_.create(P_, m, opt_, capacity_, rp, stream_, rank_);
        }
    }
    dPots_ = dev_alloc<DevPot>(pots.size());
    HIP_CHECK(hipMemcpyAsync(dPots_, pots.data(), sizeof(DevPot) * pots.size(), hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
}

// ---------------------------------------------------------------------------------------------------
// ListStore (list_store.h)
// ---------------------------------------------------------------------------------------------------
// bytes of k_pair_list's LDS tile per candidate are 24, 25 or 32 with the pair mode; tiles beyond 13 / 26 KiB, or lists beyond 96 / 192 iterations, want
// 2 / 4 waves per cell (they share the cell's tile and split its atoms): one where cells are many and their tiles small; more where the tile of a cell is
// large (LDS per wave bounds the occupancy: dense systems, wide stencils) - measured: M4 (28 atoms and 720 candidates per cell) 788 -> 514 us with two; on
// the 1 M-atom liquid (14 atoms, 320 candidates) two waves cost 102 -> 158 us: every wave pays the fixed part of a cell again.  (Few cells alone do not
// pay for more waves: C2 13.9 -> 15.2 us, an emulated rank of 8 26.8 -> 29.2 us with two.)
int ListStore::waves_wanted(double tileRecords, int iters) const
{
    const double tileBytes = tileRecords * (P_->single_lj ? 24.0 : (pair_list_tab_mode(*P_) ? 25.0 : 32.0));
    if (tileBytes > 26.0 * 1024 || iters > 192) return 4;
    return (tileBytes > 13.0 * 1024 || iters > 96) ? 2 : 1;
}

void ListStore::create(const StepParams& P, const Model& m, const aztot_options& opt, int capacity, double listRadius, hipStream_t stream, int rank)
{
    P_ = &P; stream_ = stream; capacity_ = capacity; rank_ = rank;
    forcedWaves_ = (opt.waves_per_cell == 1 || opt.waves_per_cell == 2 || opt.waves_per_cell == 4) ? opt.waves_per_cell : 0;      // measurements: forced
    if (P.ncxLocal > 1023 || P.nc[1] > 1023 || P.nc[2] > 1023) throw std::runtime_error("more than 1023 cells along an axis");
    int devLds = 0;
    HIP_CHECK(hipDeviceGetAttribute(&devLds, hipDeviceAttributeMaxSharedMemoryPerBlock, opt.device));
    ldsMax_ = (size_t)std::max(devLds, 64 * 1024);
    // capacities from the density: candidates = atoms within the list radius of a cell's box, iterations = pairs of a cell / 64 lanes, each
    // with room for a liquid's fluctuations (+ 30 % / + 50 %); cells that need more keep no list, and the store grows the lists when
    // that happens to more than a few (adapt)
    const double a = P.csz[0], b = P.csz[1], c = P.csz[2], r = listRadius;
    const double vol = swept_volume(a, b, c, r);
    const double density = (double)m.nAt / (m.L[0] * m.L[1] * m.L[2]);
    const double perCell = density * a * b * c, partners = density * 4.18879020478639 * r * r * r;
    waves = forcedWaves_ ? forcedWaves_ : waves_wanted(density * vol, 0);
    int cand = (int)(density * vol * 1.5) + 64;
    // (a cell's iterations are its atoms' partners divided by the slices each atom gets, NS = 64 / atoms; a wave of a W-wave cell serves ceil(n / W)
    //  atoms: sized for a cell 60 % fuller than the mean)
    int iters = (int)(partners * 1.25 / list_slices(list_atoms_per_wave(std::min(kWave * waves, (int)(1.6 * perCell) + 6), waves))) + 4;
    cand = std::max(kListMinCand * waves, (cand + 63) & ~63);
    iters = std::max(2 * kListMinIter, (iters + 7) & ~7);
    if (const char* e = std::getenv("AZTOT_CAND_CAP")) cand = std::atoi(e);        // (experiments / tests: start from other capacities)
    if (const char* e = std::getenv("AZTOT_ITER_CAP")) iters = std::atoi(e);
    try { allocate(cand, iters); }
    catch (const std::exception&)
    {   // (no room for the lists - hundreds of millions of cells: the run goes on without them, the steps between two rebuilds stage every cell)
        (void)hipGetLastError();
        release();
    }
}

// [nCell][candCap] candidates, [nCell][iterCap x 64] pair entries, headers.  Capacities are clipped to what the LDS of k_pair_list / k_build_lists and
// the entry format allow.
void ListStore::allocate(int candCapNew, int iterCapNew)
{
    release();
    const StepParams& P = *P_;
    // (k_pair_list asks for five groups of candidate entries per wave and two chunks of 8 iterations before it knows the cell: the arrays are never smaller)
    candCapNew = std::max(kListMinCand * waves, std::min((candCapNew + 63) & ~63, kListCandMax));
    iterCapNew = std::max(kListMinIter, std::min((iterCapNew + 7) & ~7, kListIterMax));
    PairLists probe;
    probe.candCap = probe.candLds = probe.stageLds = candCapNew; probe.iterCap = probe.iterLds = iterCapNew; probe.recBytes = pair_list_rec_bytes(P); probe.waves = waves;
    probe.buildGroups = (P.debugMask & DBG_HITS_BESIDE_TILE) ? 0 : 1;      // (the capacities are clipped for the smallest mask buffer; the buffer then takes what is left: below)
    while (candCapNew > kListMinCand && (pair_list_lds_bytes(P, probe) > ldsMax_ || build_lists_lds_bytes(probe) > ldsMax_))
    {
        candCapNew -= 64;
        probe.candCap = probe.candLds = probe.stageLds = candCapNew;
    }
    while (iterCapNew > 2 * kListMinIter && build_lists_lds_bytes(probe) > ldsMax_) { iterCapNew -= 8; probe.iterCap = probe.iterLds = iterCapNew; }
    const size_t nc = (size_t)P.nCellLocal;
    cand = mem_.alloc<uint32_t>(nc * candCapNew, true, stream_);            // every entry is an atom index at all times
    meta = mem_.alloc<int32_t>(4 * nc, false, stream_);
    pairs = mem_.alloc<uint16_t>(nc * (size_t)waves * (size_t)iterCapNew * kWave, true, stream_);   // every entry is a tile offset at all times (k_pair_list reads ahead)
    report = mem_.alloc<int32_t>(LR_COUNT, true, stream_); rel = mem_.alloc<float4>((size_t)capacity_ + kWave, true, stream_);
    candCap = candCapNew; iterCap = iterCapNew;
    candLds = stageLds = candCapNew; iterLds = iterCapNew;          // (tightened once the builder has reported what the cells really hold: tighten / adapt)
    buildGroups = groups_that_fit(4 * waves, stageLds, iterLds);    // (the worst case - 64 atoms per wave - for the first recording only)
    entryBytes = entryNext = 2;                                     // (... and 16-bit entries until then: one-byte entries go with a tile of at most 256 records)
    {   // header: -1 = no list ; second word: the cell's coordinates in the local grid (the kernels decode them with shifts)
        std::vector<int32_t> mx(4 * nc, 0);
        const int ncy = P.nc[1], ncz = P.nc[2];
        for (size_t c = 0; c < nc; c++)
        {
            const int cz = (int)(c % ncz), cy = (int)((c / ncz) % ncy), lx = (int)(c / ((size_t)ncy * ncz));
            mx[4 * c] = -1; mx[4 * c + 1] = lx | (cy << 10) | (cz << 20);
        }
        HIP_CHECK(hipMemcpyAsync(meta, mx.data(), sizeof(int32_t) * 4 * nc, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    on = true;
    if (std::getenv("AZTOT_VERBOSE"))
        std::fprintf(stderr, "aztot: pair lists for %zu cells: %d candidates, %d iterations per cell (%.1f MB), LDS %zu B (list kernel) / %zu B (builder)\n", nc, candCap, iterCap,
                     (double)(nc * ((size_t)candCap * 4 + (size_t)iterCap * 128)) / 1e6, pair_list_lds_bytes(P, pair_lists()), build_lists_lds_bytes(pair_lists()));
}

void ListStore::regrow(int candCapNew, int iterCapNew)
{
    try { allocate(candCapNew, iterCapNew); }
    catch (const std::exception& e)
    {   // (on slab ranks the other ranks would be left waiting in the look's all-reduce: ADVICE round 3)
        (void)hipGetLastError();
        release();
        if (std::getenv("AZTOT_VERBOSE")) std::fprintf(stderr, "aztot: rank %d: no room for larger pair lists (%s): the run goes on without lists\n", rank_, e.what());
    }
}

void ListStore::release() noexcept
{
    if (stream_) (void)hipStreamSynchronize(stream_);
    mem_.release();
    cand = nullptr; meta = nullptr; pairs = nullptr; report = nullptr; rel = nullptr;
    on = false;
}

PairLists ListStore::pair_lists() const
{
    PairLists pl;
    if (on)
    {
        pl.cand = cand; pl.meta = meta; pl.pairs = pairs; pl.noList = report;
        pl.candCap = candCap; pl.iterCap = iterCap; pl.candLds = candLds; pl.stageLds = stageLds; pl.iterLds = iterLds; pl.recBytes = pair_list_rec_bytes(*P_); pl.waves = waves;
        pl.buildGroups = buildGroups;
        pl.entryBytes = entryBytes; pl.entryScale = entryBytes == 1 ? 1 : pair_list_entry_scale(*P_);      // (one-byte entries are record numbers in every mode)
        pl.rel = rel;
    }
    return pl;
}

// Records of k_pair_list's LDS tile for cells that keep at most maxT candidates.  LDS per wave bounds the kernel's occupancy and the hardware hands LDS out in
// blocks of 1 280 B (gfx950: 160 KiB in 128 blocks), so the tile is the largest one that costs no more blocks than the smallest one that would do
// (largest cell + 1 % + 1): C4's largest tile of 305 candidates gives 319 records in six blocks - 21 waves per CU by LDS - where "largest + 4 % + 6" took seven.
int ListStore::tile_records_for(int maxT) const
{
    constexpr size_t kLdsBlock = 1280;
    PairLists L = pair_lists();
    // (roomy: systems that run without the clean-up launch - a cell that outgrows the tile there costs a window of steps run again, and LDS per wave is not
    //  what bounds a step of a few thousand cells: + 6 %)
    const bool roomy = P_->nranks == 1 && capacity_ <= 2 * kFuseKickMaxAtoms;
    int need = std::max(4 * kWave, std::min(candCap, roomy ? maxT + maxT / 16 + 4 : maxT + maxT / 100 + 1));
    // (one GPU, one wave per cell, every cell's record numbers still in a byte: the margin never takes the tile past the 256 records of the four-group kernel,
    //  which is the one that walks one-byte entries (narrow_fits) - from 238 kept candidates on a roomy engine's margin shrinks instead, to nothing at 255,
    //  where the byte is the limit anyway.  Whatever DBG_WIDE_ENTRIES says: the switch changes the entries' width and nothing else)
    if (maxT <= 255 && P_->nranks == 1 && waves == 1) need = 4 * kWave;
    // (a tile of up to 256 records is served by the kernel that gathers four groups of candidates up front instead of five: never a few records more than
    //  that for the sake of a full LDS block)
    if (need <= 4 * kWave) return need;
    L.candLds = need;
    const size_t blocks = (pair_list_lds_bytes(*P_, L) + kLdsBlock - 1) / kLdsBlock;
    int best = need;
    for (int c = need + 1; c <= candCap; c++)
    {
        L.candLds = c;
        if ((pair_list_lds_bytes(*P_, L) + kLdsBlock - 1) / kLdsBlock > blocks) break;
        best = c;
    }
    return best;
}

// The builder's staging area for cells that stage at most maxStaged candidates (+ 6 %; the builder rounds it up to whole mask words of 128 anyway, so this
// does too: its LDS bounds nothing that runs every step)
int ListStore::stage_records_for(int maxStaged) const
{
    return std::max(4 * kWave, std::min(candCap, (maxStaged + maxStaged / 16 + 4 + 127) & ~127));
}

// Groups of 16 atoms the builder's mask buffer holds (PairLists::buildGroups) for cells of `want` groups: no more than a cell can have, 4 x waves, and no more
// than the LDS a workgroup is granted leaves room for beside a staging area and a list buffer of these sizes - cells with more keep no list and are served by
// the clean-up launch.  LDS per wave bounds the builder's occupancy too and comes in blocks of 1 280 B (tile_records_for): the buffer takes the groups that
// cost no block more than `want` does, and no others - C4's cells of up to 32 atoms get two groups in seven blocks, 18 waves per CU, where a third would take
// an eighth.  0 with DBG_HITS_BESIDE_TILE: the builder then runs one group at a time
int ListStore::groups_that_fit(int want, int stageLdsNew, int iterLdsNew) const
{
    if (P_->debugMask & DBG_HITS_BESIDE_TILE) return 0;
    constexpr size_t kLdsBlock = 1280;
    PairLists L;
    L.stageLds = stageLdsNew; L.iterLds = iterLdsNew; L.waves = waves;
    L.buildGroups = std::max(1, std::min(want, 4 * waves));
    while (L.buildGroups > 1 && build_lists_lds_bytes(L) > ldsMax_) L.buildGroups--;
    const size_t blocks = (build_lists_lds_bytes(L) + kLdsBlock - 1) / kLdsBlock;
    while (L.buildGroups < 4 * waves)
    {
        L.buildGroups++;
        if ((build_lists_lds_bytes(L) + kLdsBlock - 1) / kLdsBlock > blocks || build_lists_lds_bytes(L) > ldsMax_) { L.buildGroups--; break; }
    }
    return L.buildGroups;
}

// LDS per wave is what bounds the occupancy of k_pair_list: its tile is sized from the largest KEPT candidate set ever recorded, not from the capacity of
// the arrays; the builder's staging area from the largest STAGED set, its list buffer from the longest list (+ 1/8), its mask buffer from the most atoms
// a cell held, in whole groups of 16
void ListStore::lds_for(const int32_t* rep, int& candLdsNew, int& stageLdsNew, int& iterLdsNew, int& groupsNew) const
{
    candLdsNew = tile_records_for(rep[LR_MAX_TILE]);
    stageLdsNew = stage_records_for(rep[LR_MAX_STAGED]);
    iterLdsNew = std::max(2 * kListMinIter, std::min(iterCap, (rep[LR_MAX_ITERS] + rep[LR_MAX_ITERS] / 8 + 2 + 7) & ~7));
    // (one-byte entries are read out sixteen iterations at a time: whole chunks where the capacity allows.  A cell's stride in `pairs`, iterCap x 128 B, holds
    //  2 iterCap one-byte iterations, so any iterCap >= 16 keeps whole chunks of them inside it)
    if (entryNext == 1 && ((iterLdsNew + 15) & ~15) <= iterCap) iterLdsNew = (iterLdsNew + 15) & ~15;
    groupsNew = groups_that_fit((rep[LR_MAX_ATOMS] + 15) / 16, stageLdsNew, iterLdsNew);
}

bool ListStore::narrow_fits(int maxTile, int candLdsNew, int wavesNew) const
{
    return P_->nranks == 1 && !(P_->debugMask & DBG_WIDE_ENTRIES) && !wideForGood_ && wavesNew == 1 && list_preload(candLdsNew) == 4 && maxTile <= 255;
}

bool ListStore::tighten(const int32_t* rep, bool* formatChanged)
{
    if (formatChanged) *formatChanged = false;
    if (rep[LR_TILE_FULL] != 0 || rep[LR_LIST_FULL] != 0 || rep[LR_KEPT_FULL] != 0 || rep[LR_MASK_FULL] != 0 || rep[LR_MAX_STAGED] <= 0) return false;
    int c, s, i, g;
    lds_for(rep, c, s, i, g);
    bool changed = false;
    if (entryNext == 2 && narrow_fits(rep[LR_MAX_TILE], std::min(candLds, c), waves))
    {   // the lists just recorded hold 16-bit entries: the caller records them again
        entryNext = 1;
        lds_for(rep, c, s, i, g);
        changed = true;
        if (formatChanged) *formatChanged = true;
    }
    if (c >= candLds && s >= stageLds && i >= iterLds && g >= buildGroups) return changed;
    candLds = std::min(candLds, c); stageLds = std::min(stageLds, s); iterLds = std::min(iterLds, i); buildGroups = std::min(buildGroups, g);
    if (std::getenv("AZTOT_VERBOSE"))
        std::fprintf(stderr, "aztot: list LDS sized from the first recording: tile %d, staging %d, %d iterations, %d mask groups: %zu B (list kernel) / %zu B (builder)\n", candLds, stageLds, iterLds,
                     buildGroups, pair_list_lds_bytes(*P_, pair_lists()), build_lists_lds_bytes(pair_lists()));
    return true;
}

// Cells that keep no list are staged by the small clean-up launch: fine for a few, slow for many (stencils wider than one tile, cells of more than
// 64 atoms) - then the plain steps go back to staging every cell.  
ListStore::Verdict ListStore::adapt(const int32_t* rep, unsigned debug)
{
    Verdict v;
    const bool frozen = debug & DBG_SHORT_LISTS;
    if (debug & DBG_LIST_STATS)
    {   // measurement aid: mean list length / tile size / atoms per cell over the cells recorded since the last look
        std::fprintf(stderr, "aztot: per cell: %.2f list iterations, %.1f candidates staged, %.1f kept, %.2f atoms; %.1f %% of the cells walk more than 16 iterations (%d-byte entries)\n",
                     (double)rep[LR_SUM_ITERS] / rep[LR_RECORDED], (double)rep[LR_SUM_STAGED] / rep[LR_RECORDED], (double)rep[LR_SUM_CANDS] / rep[LR_RECORDED],
                     (double)rep[LR_SUM_ATOMS] / rep[LR_RECORDED], 100.0 * (double)rep[LR_OVER_16] / rep[LR_RECORDED], entryBytes);
        HIP_CHECK(hipMemset(&report[LR_SUM_ITERS], 0, sizeof(int32_t) * 4));
        HIP_CHECK(hipMemset(&report[LR_OVER_16], 0, sizeof(int32_t)));
    }
    // (LR_UNLISTED_NOW stays: it describes the lists in force; the maxima are all-time)
    HIP_CHECK(hipMemsetAsync(&report[LR_UNLISTED], 0, sizeof(int32_t) * 2, stream_));
    HIP_CHECK(hipMemsetAsync(&report[LR_TILE_FULL], 0, sizeof(int32_t) * 3, stream_));
    HIP_CHECK(hipMemsetAsync(&report[LR_MASK_FULL], 0, sizeof(int32_t), stream_));
    // ("tile full": the staged candidates did not fit the builder's staging area; "kept full": the kept ones did not fit the tile of k_pair_list; "mask full":
    //  more groups of 16 atoms than the builder's mask buffer holds)
    const int tileFull = rep[LR_TILE_FULL], keptFull = rep[LR_KEPT_FULL], listFull = rep[LR_LIST_FULL], maskFull = rep[LR_MASK_FULL], recorded = rep[LR_RECORDED], unlisted = rep[LR_UNLISTED];
    if (std::getenv("AZTOT_VERBOSE"))
        std::fprintf(stderr, "aztot: lists recorded since the last look: %d cells, %d of them without a list (%d: staging full, %d: tile full, %d: list full, %d: mask buffer full); most staged %d of %d (LDS %d), largest tile %d (LDS %d), longest list %d of %d (LDS %d), most atoms %d (LDS %d groups, builder %zu B)\n",
                     recorded, unlisted, tileFull, keptFull, listFull, maskFull, rep[LR_MAX_STAGED], candCap, stageLds, rep[LR_MAX_TILE], candLds, rep[LR_MAX_ITERS], iterCap, iterLds, rep[LR_MAX_ATOMS], buildGroups,
                     build_lists_lds_bytes(pair_lists()));
    // A cell that does not fit next time keeps no list for one interval (exact: the clean-up launch serves it) and is counted; then the tiles grow again.
    int candLdsNew, stageLdsNew, iterLdsNew, groupsNew;
    lds_for(rep, candLdsNew, stageLdsNew, iterLdsNew, groupsNew);
    if (tileFull > 0) stageLdsNew = std::min(candCap, std::max(stageLdsNew, stageLds + 128));
    if (keptFull > 0) candLdsNew = std::min(candCap, std::max(candLdsNew, candLds + 32));
    if (listFull > 0) iterLdsNew = std::min(iterCap, std::max(iterLdsNew, iterLds + 8));
    // (the mask buffer follows the largest cell reported, which the cells that did not fit reported too; staging area and list buffer may have grown beside it)
    groupsNew = groups_that_fit((rep[LR_MAX_ATOMS] + 15) / 16, stageLdsNew, iterLdsNew);
    if (frozen) { candLdsNew = candLds; stageLdsNew = stageLds; iterLdsNew = iterLds; groupsNew = buildGroups; }
    // more waves per cell where the cells turn out denser than the mean density promised (a droplet in a large box - case study 2: tiles of 1 487
    // candidates, lists of 210 iterations where the homogeneous estimate said 1 wave would do): decided from what the builder recorded
    const int wWant = std::max(waves, waves_wanted((double)rep[LR_MAX_TILE], rep[LR_MAX_ITERS]));
    const int wavesNew = (wWant > waves && !forcedWaves_ && !frozen) ? wWant : waves;
    // The entry format.  One-byte entries and a cell they cannot hold (it was recorded without a list, LR_KEPT_FULL, and the clean-up launch has served it), or
    // a tile or a wave count their kernel is not built for: back to 16 bits from the next step on, which rebuilds - and for good.  16-bit entries where one
    // byte would do (an engine whose first lists were recorded by a step, not by prepare_next_call): the next rebuild, whenever it comes, records one-byte
    // entries - the lists in force serve until then, no step's schedule changes
    if (entryNext == 1 && (rep[LR_MAX_TILE] > 255 || keptFull > 0 || !narrow_fits(rep[LR_MAX_TILE], candLdsNew, wavesNew)))
    {
        entryNext = 2; wideForGood_ = true;
        v.rebuild = v.launchChanged = true;
    }
    else if (entryNext == 2 && !frozen && tileFull + keptFull + listFull + maskFull == 0 && narrow_fits(rep[LR_MAX_TILE], candLdsNew, wavesNew))
    {
        entryNext = 1;
        v.launchChanged = true;
        lds_for(rep, candLdsNew, stageLdsNew, iterLdsNew, groupsNew);
    }
    if (wWant > waves && !forcedWaves_ && !frozen)
    {   // (what was recorded describes lists that no longer exist: nothing more to decide now)
        const int itersNew = std::max(2 * kListMinIter, ((int)(rep[LR_MAX_ITERS] * (double)waves / wWant * 1.3) + 8 + 7) & ~7);
        const int candNew = std::max(candCap, kListMinCand * wWant);
        waves = wWant;
        regrow(candNew, itersNew);
        v.rebuild = v.launchChanged = true;
        return v;
    }
    const bool capFull = (tileFull > 0 && stageLds == candCap) || (keptFull > 0 && candLds == candCap) || (listFull > 0 && iterLds == iterCap);
    // (one GPU: ANY cell that does not fit costs an engine that runs without the clean-up launch a window of steps run again, so the arrays grow at once
    //  while they still can; slab ranks and the last growth wait until it is more than a handful)
    if (capFull && !frozen && (double)(tileFull + keptFull + listFull) > ((P_->nranks == 1 && growths < 3) ? 0.0 : 0.0005 * (double)recorded))
    {   // the arrays themselves are too small: larger ones if the limits allow (twice), and the next step rebuilds; else - cells of more than 64 atoms
        // never fit - the plain steps go back to staging once that is more than 2 % of the cells
        const int candNew = tileFull + keptFull > 0 ? std::min(kListCandMax, (candCap * 3 / 2 + 63) & ~63) : candCap;
        const int itersNew = listFull > 0 ? std::min(kListIterMax, (iterCap * 2 + 7) & ~7) : iterCap;
        v.launchChanged = true;
        if (growths < 3 && (candNew > candCap || itersNew > iterCap)) { growths++; regrow(candNew, itersNew); v.rebuild = true; }
    }
    else if (candLdsNew != candLds || stageLdsNew != stageLds || iterLdsNew != iterLds || groupsNew != buildGroups)
    {
        candLds = candLdsNew; stageLds = stageLdsNew; iterLds = iterLdsNew; buildGroups = groupsNew;
        v.launchChanged = true;               // (launch parameters are baked into the graphs)
    }
    if (on && (double)unlisted > 0.02 * (double)recorded && !frozen && tileFull + keptFull + listFull + maskFull < unlisted / 2)
    {   // mostly cells of more than 64 atoms: no list will ever hold them
        on = false;
        v.launchChanged = true;
    }
    return v;
}

// Static per-atom tables of the bonded terms, keyed by atom id and replicated on every rank (like the reference's
// host-side lists, cuBonds.cu / cuAngles.cu); entries of one atom keep list order, so the summation order is fixed.
void Engine::upload_bonded()
{
    const Model& m = model_;
    const size_t nb = m.bondA.size(), na = m.angC.size();
    hasBonded_ = (nb + na) > 0;
    if (!hasBonded_) return;
    const int N = m.nAt;
    auto up = [&](const void* src, size_t bytes) {
        void* p = dev_alloc<char>(bytes);
        if (bytes) HIP_CHECK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return p;
    };
    std::vector<int32_t> bs(N + 1, 0), as(N + 1, 0);
    for (size_t k = 0; k < nb; k++) { bs[m.bondA[k] + 1]++; bs[m.bondB[k] + 1]++; }
    for (size_t k = 0; k < na; k++) { as[m.angC[k] + 1]++; as[m.angL1[k] + 1]++; as[m.angL2[k] + 1]++; }
    for (int i = 0; i < N; i++) { bs[i + 1] += bs[i]; as[i + 1] += as[i]; }
    std::vector<BondEntry> be(2 * nb);
    std::vector<AngleEntry> ae(3 * na);
    {
        std::vector<int32_t> fill(bs.begin(), bs.end() - 1);
        for (size_t k = 0; k < nb; k++)
        {
            be[fill[m.bondA[k]]++] = BondEntry{m.bondB[k], m.bondT[k] | (1 << 30)};
            be[fill[m.bondB[k]]++] = BondEntry{m.bondA[k], m.bondT[k]};
        }
        fill.assign(as.begin(), as.end() - 1);
        for (size_t k = 0; k < na; k++)
        {
            const int32_t c = m.angC[k], l1 = m.angL1[k], l2 = m.angL2[k], t = m.angT[k] << 2;
            ae[fill[c]++] = AngleEntry{t | 0, c, l1, l2};
            ae[fill[l1]++] = AngleEntry{t | 1, c, l1, l2};
            ae[fill[l2]++] = AngleEntry{t | 2, c, l1, l2};
        }
    }
    std::vector<DevBondType> bt(m.bondTypes.size() + 1);
    std::memset(bt.data(), 0, sizeof(DevBondType) * bt.size());
    for (size_t k = 0; k < m.bondTypes.size(); k++)
    {
        const BondType& b = m.bondTypes[k];
        bt[k + 1] = DevBondType{b.type, 0, b.p[0], b.p[1], b.p[2], b.p[3], b.p[4]};
    }
    std::vector<DevAngleType> at(m.angleTypes.size() + 1, DevAngleType{0.0, 0.0});
    for (size_t k = 0; k < m.angleTypes.size(); k++) at[k + 1] = DevAngleType{m.angleTypes[k].k, m.angleTypes[k].cos0};
    bonded_.bondStart = (const int32_t*)up(bs.data(), sizeof(int32_t) * bs.size());
    bonded_.bondEnt = (const BondEntry*)up(be.data(), sizeof(BondEntry) * be.size());
    bonded_.angStart = (const int32_t*)up(as.data(), sizeof(int32_t) * as.size());
    bonded_.angEnt = (const AngleEntry*)up(ae.data(), sizeof(AngleEntry) * ae.size());
    bonded_.btypes = (const DevBondType*)up(bt.data(), sizeof(DevBondType) * bt.size());
    bonded_.atypes = (const DevAngleType*)up(at.data(), sizeof(DevAngleType) * at.size());
    std::vector<int32_t> none(N, -1);
    bonded_.idxOfId = (int32_t*)up(none.data(), sizeof(int32_t) * (size_t)N);
}

// k-vector table of the Ewald sum + work buffers.  The table is the host model's (finish_model, same loop as ewald_rec).
void Engine::upload_ewald()
{
    const Model& m = model_;
    hasEwald_ = m.elec_type == AZTOT_ELEC_EWALD && !m.kvecs.empty();
    if (!hasEwald_) return;
    std::vector<EwaldK> kv(m.kvecs.size());
    for (size_t k = 0; k < kv.size(); k++)
    {
        const KVec& a = m.kvecs[k];
        int flags = 0;
        if (k == 0 || m.kvecs[k - 1].l != a.l) flags |= EWK_NEW_L | EWK_NEW_LM;
        else if (m.kvecs[k - 1].m != a.m) flags |= EWK_NEW_LM;
        kv[k] = EwaldK{a.l, a.m, a.n, flags, a.rkx, a.rky, a.rkz, a.akk};
    }
    EwaldK* dkv = dev_alloc<EwaldK>(kv.size());
    HIP_CHECK(hipMemcpy(dkv, kv.data(), sizeof(EwaldK) * kv.size(), hipMemcpyHostToDevice));
    ew_.kv = dkv;
    // work items of k_ewald_sfac: (l, m, |n|) with the indices of its +n / -n members
    std::map<std::tuple<int, int, int>, int> slot;
    std::vector<EwaldW> work;
    for (size_t k = 0; k < kv.size(); k++)
    {
        const auto key = std::make_tuple(kv[k].l, kv[k].m, std::abs(kv[k].n));
        auto it = slot.find(key);
        if (it == slot.end()) { slot[key] = (int)work.size(); work.push_back(EwaldW{kv[k].l, kv[k].m, std::abs(kv[k].n), -1, -1}); it = slot.find(key); }
        if (kv[k].n >= 0) work[it->second].kPlus = (int)k; else work[it->second].kMinus = (int)k;
    }
    EwaldW* dw = dev_alloc<EwaldW>(work.size());
    HIP_CHECK(hipMemcpy(dw, work.data(), sizeof(EwaldW) * work.size(), hipMemcpyHostToDevice));
    ew_.work = dw; ew_.nW = (int)work.size();
    // work items of k_ewald_force: runs of consecutive n with the same (l, m) (the table is in ewald_rec's nested-loop order)
    std::vector<EwaldG> groups;
    for (size_t k = 0; k < kv.size(); k++)
    {
        if (!groups.empty() && groups.back().l == kv[k].l && groups.back().m == kv[k].m && groups.back().nHi + 1 == kv[k].n) groups.back().nHi = kv[k].n;
        else groups.push_back(EwaldG{kv[k].l, kv[k].m, kv[k].n, kv[k].n, (int)k});
    }
    EwaldG* dg = dev_alloc<EwaldG>(groups.size());
    HIP_CHECK(hipMemcpy(dg, groups.data(), sizeof(EwaldG) * groups.size(), hipMemcpyHostToDevice));
    ew_.groups = dg; ew_.nG = (int)groups.size();
    ew_.T = dev_alloc<double>(2 * kv.size());
    ew_.nK = (int)kv.size(); ew_.kx = m.ewald_k[0]; ew_.ky = m.ewald_k[1]; ew_.kz = m.ewald_k[2];
    ew_.nBlocksA = std::max(1, std::min(1024, div_up(capacity_, kEwTile)));
    ew_.partial = dev_alloc<double>(2 * (size_t)ew_.nK * ew_.nBlocksA);
    ew_.S = dev_alloc<double>(2 * (size_t)ew_.nK);
    HIP_CHECK(hipMemset(ew_.S, 0, sizeof(double) * 2 * (size_t)ew_.nK));
    ew_.scale = m.el_scale; ew_.scale2 = m.el_scale2;
    {   // both kernels keep the three per-atom harmonic tables in dynamic LDS: 1 KiB per harmonic (+ 12 KiB of force slices).  Beyond
        // the default 64 KiB a kernel has to be told (up to the CU's 160 KiB); beyond that the sum cannot run in this layout
        const size_t ldsTab = sizeof(double) * 2 * (size_t)kEwTile * (ew_.kx + ew_.ky + ew_.kz);
        const size_t ldsForce = ldsTab + sizeof(double) * 3 * kEwTile * kEwSlices;
        int devMax = 0;
        HIP_CHECK(hipDeviceGetAttribute(&devMax, hipDeviceAttributeMaxSharedMemoryPerBlock, opt_.device));
        const size_t hwMax = std::max<size_t>((size_t)devMax, 160 * 1024);
        if (ldsForce > hwMax)
            throw std::runtime_error("elec pme: kx + ky + kz = " + std::to_string(ew_.kx + ew_.ky + ew_.kz) + " harmonics need " + std::to_string(ldsForce) +
                                     " B of LDS per workgroup, more than the " + std::to_string(hwMax) + " B a CU has (use fewer k-vectors or elec fenn)");
        if (ldsTab > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void*)k_ewald_sfac, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsTab));
        if (ldsForce > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void*)k_ewald_force, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsForce));
    }
    DevStats s;
    HIP_CHECK(hipMemcpy(&s, dStats_, sizeof(DevStats), hipMemcpyDeviceToHost));
    s.engCoulConst = m.engElec1;
    HIP_CHECK(hipMemcpy(dStats_, &s, sizeof(DevStats), hipMemcpyHostToDevice));
}

// sim->add_elec = ewald_rec (main.cpp:99 ; GPU path main.cu:330-335): structure factors of the owned atoms, their sum over the
// ranks, then energy and per-atom forces (added to what the pair kernel wrote)
void Engine::launch_ewald()
{
    const size_t lds = sizeof(double) * 2 * (size_t)kEwTile * (ew_.kx + ew_.ky + ew_.kz);
    timed("ewald_sfac", [&] {
        hipLaunchKernelGGL(k_ewald_sfac, dim3(ew_.nBlocksA), dim3(256), lds, stream_, P_, S_, cur(), dCounts_, ew_);
        hipLaunchKernelGGL(k_ewald_reduce, dim3(div_up(ew_.nK, 64)), dim3(64 * kEwRedGroups), 0, stream_, ew_);
    });
    if (nranks_ > 1) timed("ewald_allreduce", [&] { xch_->allreduce_device(ew_.S, 2 * ew_.nK, stream_); });
    timed("ewald_energy", [&] { hipLaunchKernelGGL(k_ewald_energy, dim3(1), dim3(256), 0, stream_, ew_, dStats_); });
    timed("ewald_force", [&] {
        hipLaunchKernelGGL(k_ewald_force, dim3(div_up(capacity_, kEwTile)), dim3(kEwTile * kEwSlices), lds + sizeof(double) * 3 * kEwTile * kEwSlices,
                           stream_, P_, S_, cur(), dCounts_, ew_);
    });
    check_launch("Ewald kernels");
}

// Meshes, influence function and twiddles of 'elec spme' (spme.hip.h): everything the per-step path touches is allocated here, once
void Engine::upload_spme()
{
    const Model& m = model_;
    hasSpme_ = m.elec_type == AZTOT_ELEC_SPME;
    if (!hasSpme_) return;
    SpmeTables& T = spme_;
    for (int k = 0; k < 3; k++) { T.K[k] = m.spme_mesh[k]; T.KoverL[k] = (double)m.spme_mesh[k] / m.L[k]; }
    T.order = m.spme_order;
    T.nPts = T.K[0] * T.K[1] * T.K[2];
    T.scale = m.el_scale;
    const size_t nPts = (size_t)T.nPts;
    T.Qi = dev_alloc<long long>(nPts, true);
    T.W = dev_alloc<double>(2 * nPts, true);
    T.partial = dev_alloc<double>(nPts / kBlock, true);
    {
        std::vector<double> G;
        aztot::spme_influence(m, G);
        double* dG = dev_alloc<double>(nPts);
        HIP_CHECK(hipMemcpy(dG, G.data(), sizeof(double) * nPts, hipMemcpyHostToDevice));
        T.G = dG;
    }
    for (int a = 0; a < 3; a++)
    {
        std::vector<double> tw;
        spme_twiddles(T.K[a], tw);
        double* d = dev_alloc<double>(tw.size());
        HIP_CHECK(hipMemcpy(d, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice));
        T.tw[a] = d;
    }
    // the three passes of the transform (SpmeAxis, device_md.h): tiles of kSpmeTilePts points at the most
    const int Kx = T.K[0], Ky = T.K[1], Kz = T.K[2];
    auto log2i = [](int v) { int l = 0; while ((1 << l) < v) l++; return l; };
    {
        SpmeAxis& A = spmeAxis_[0];
        A.N = Kx; A.logN = log2i(Kx); A.LT = std::min(kSpmeTilePts / Kx, Ky * Kz); A.contiguous = 1; A.tilesPerRow = 1;
        A.nTiles = Ky * Kz / A.LT; A.outerStride = (int64_t)A.LT * Kx; A.elemStride = 1;
    }
    {
        SpmeAxis& A = spmeAxis_[1];
        A.N = Ky; A.logN = log2i(Ky); A.LT = std::min(kSpmeTilePts / Ky, Kx); A.contiguous = 0; A.tilesPerRow = Kx / A.LT;
        A.nTiles = Kz * A.tilesPerRow; A.outerStride = (int64_t)Kx * Ky; A.elemStride = Kx;
    }
    {
        SpmeAxis& A = spmeAxis_[2];
        A.N = Kz; A.logN = log2i(Kz); A.LT = std::min(kSpmeTilePts / Kz, Kx); A.contiguous = 0; A.tilesPerRow = Kx / A.LT;
        A.nTiles = Ky * A.tilesPerRow; A.outerStride = Kx; A.elemStride = (int64_t)Kx * Ky;
    }
    DevStats s;
    HIP_CHECK(hipMemcpy(&s, dStats_, sizeof(DevStats), hipMemcpyDeviceToHost));
    s.engCoulConst = m.engElec1;
    HIP_CHECK(hipMemcpy(dStats_, &s, sizeof(DevStats), hipMemcpyHostToDevice));
}

// The stages of the mesh sum on the arrays as they stand, up to and including: 0 the spread (the integer mesh is left filled), 1 the forward transform
// (the work mesh holds the spectrum), 2 the convolution (books engCoulRec) and the inverse transform (the work mesh holds phi)
void Engine::spme_stage(int upTo)
{
    const SpmeTables& T = spme_;
    const int gridAtoms = div_up(capacity_, kSpmeAtomsPerBlock), gridPts = T.nPts / kBlock;
    timed("spme_spread", [&] {
        if (T.order == 4) hipLaunchKernelGGL(k_spme_spread<4>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, T);
        else if (T.order == 6) hipLaunchKernelGGL(k_spme_spread<6>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, T);
        else hipLaunchKernelGGL(k_spme_spread<8>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, T);
    });
    if (upTo < 1) return;
    timed("spme_fft_fwd", [&] {
        hipLaunchKernelGGL(k_spme_to_complex, dim3(gridPts), dim3(kBlock), 0, stream_, T);
        for (int a = 0; a < 3; a++) hipLaunchKernelGGL(k_spme_fft<false>, dim3(spmeAxis_[a].nTiles), dim3(kBlock), 0, stream_, T.W, T.tw[a], spmeAxis_[a]);
    });
    if (upTo < 2) return;
    timed("spme_convolve", [&] {
        hipLaunchKernelGGL(k_spme_convolve, dim3(gridPts), dim3(kBlock), 0, stream_, T);
        hipLaunchKernelGGL(k_spme_energy, dim3(1), dim3(kBlock), 0, stream_, T, dStats_);
    });
    timed("spme_fft_inv", [&] {
        for (int a = 2; a >= 0; a--) hipLaunchKernelGGL(k_spme_fft<true>, dim3(spmeAxis_[a].nTiles), dim3(kBlock), 0, stream_, T.W, T.tw[a], spmeAxis_[a]);
    });
}

// the reciprocal part of 'elec spme', at launch_ewald's place in the step: energy into DevStats::engCoulRec, forces added to what the pair kernel wrote
void Engine::launch_spme()
{
    spme_stage(2);
    const SpmeTables& T = spme_;
    const int gridAtoms = div_up(capacity_, kSpmeAtomsPerBlock);
    timed("spme_gather", [&] {
        if (T.order == 4) hipLaunchKernelGGL(k_spme_gather<4>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, T);
        else if (T.order == 6) hipLaunchKernelGGL(k_spme_gather<6>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, T);
        else hipLaunchKernelGGL(k_spme_gather<8>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, T);
    });
    check_launch("SPME kernels");
}

long long Engine::spme_mesh(int which, void* out, long long cap)
{
    if (!hasSpme_) throw ArgError("aztot_spme_mesh: the model of this handle has no 'elec spme'");
    if (which < AZTOT_SPME_CHARGE || which > AZTOT_SPME_POTENTIAL) throw ArgError("aztot_spme_mesh: which is AZTOT_SPME_CHARGE, _SPECTRUM or _POTENTIAL");
    const long long words = which == AZTOT_SPME_CHARGE ? (long long)spme_.nPts : 2LL * spme_.nPts;
    if (!out && cap == 0) return words;
    if (!out || cap < words) throw ArgError("aztot_spme_mesh: the buffer is too small");
    if (!failed_.empty()) throw std::runtime_error("this handle failed in an earlier call: " + failed_);
    // the positions the handle holds are those of the last force evaluation; the stages run again on them (the same kernels, the same bits) without
    // touching the forces, and leave the integer mesh clear as a force evaluation does
    sync_all();
    spme_stage(which);
    if (which == AZTOT_SPME_CHARGE)
    {
        HIP_CHECK(hipMemcpyAsync(out, spme_.Qi, sizeof(long long) * (size_t)words, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipMemsetAsync(spme_.Qi, 0, sizeof(long long) * (size_t)words, stream_));
    }
    else HIP_CHECK(hipMemcpyAsync(out, spme_.W, sizeof(double) * (size_t)words, hipMemcpyDeviceToHost, stream_));
    check_launch("SPME read-back");
    sync();
    return words;
}

long long Engine::spme_influence(double* out, long long cap)
{
    if (!hasSpme_) throw ArgError("aztot_spme_influence: the model of this handle has no 'elec spme'");
    const long long words = spme_.nPts;
    if (!out && cap == 0) return words;
    if (!out || cap < words) throw ArgError("aztot_spme_influence: the buffer is too small");
    HIP_CHECK(hipMemcpy(out, spme_.G, sizeof(double) * (size_t)words, hipMemcpyDeviceToHost));
    return words;
}

void Engine::upload_initial()
{
    const Model& m = model_;
    const int N = m.nAt;
    // which atoms start on this rank: all of them on one GPU, the slab's cell layers otherwise
    std::vector<int32_t> ids; ids.reserve(capacity_);
    for (int i = 0; i < N; i++)
    {
        if (nranks_ > 1)
        {
            int gx = (int)std::floor(m.x[i] * P_.icsz[0]);
            gx %= P_.nc[0]; if (gx < 0) gx += P_.nc[0];
            const int lo = P_.cx0 + P_.hw[0], hi = lo + P_.ncxLocal - 2 * P_.hw[0];
            if (gx < lo || gx >= hi) continue;
        }
        ids.push_back(i);
    }
    const int n = (int)ids.size();
    if (n > capacity_) throw std::runtime_error("slab capacity exceeded at initialisation");
    AtomArrays& A = cur();
    std::vector<double> tmp(std::max(n, 1));
    auto up = [&](double* dst, const std::vector<double>& src) {
        for (int k = 0; k < n; k++) tmp[k] = src[ids[k]];
        HIP_CHECK(hipMemcpy(dst, tmp.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    };
    up(A.x, m.x); up(A.y, m.y); up(A.z, m.z); up(A.vx, m.vx); up(A.vy, m.vy); up(A.vz, m.vz);
    std::vector<int32_t> ty(std::max(n, 1));
    for (int k = 0; k < n; k++) ty[k] = m.types[ids[k]];
    HIP_CHECK(hipMemcpy(A.type, ty.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(A.id, ids.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    if (m.tstat_type == AZTOT_TSTAT_RADI)
    {   // init_cuda_tstat: cuTemp.cu:25-60 ; tables: read_tstat temperature.cpp:113-245
        std::vector<double> ph(N), ux(kNumUnitVectors), uy(kNumUnitVectors), uz(kNumUnitVectors);
        photon_engs(N, ph.data(), m.Temp, opt_.seed);
        unit_vectors(ux.data(), uy.data(), uz.data());
        auto alloc_up = [&](double*& d, const std::vector<double>& h) {
            d = dev_alloc<double>(h.size());
            HIP_CHECK(hipMemcpy(d, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
        };
        alloc_up(dPhotons_, ph); alloc_up(dUvx_, ux); alloc_up(dUvy_, uy); alloc_up(dUvz_, uz);
    }
    if (m.tstat_type == AZTOT_TSTAT_RADI || P_.use_radii)
    {   // (a radius-dependent potential without the radiative thermostat: the radii it would have drawn, cuTemp.cu:41, never unset memory)
        for (int k = 0; k < n; k++) tmp[k] = initial_radius(opt_.seed, (uint64_t)ids[k]);
        HIP_CHECK(hipMemcpy(A.rad, tmp.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    }
    Counts c{};
    c.ownedBegin = 0; c.ownedEnd = n; c.nTotal = n; c.srcBegin = 0; c.srcEnd = n;
    HIP_CHECK(hipMemcpy(dCounts_, &c, sizeof(Counts), hipMemcpyHostToDevice));
    // init_serial computes all_pairs only (sys_init.cpp:1181-1184): bonds and angles first act in step 1's force phase
    if (opt_.initial_forces) forces(false);
}

// ---------------------------------------------------------------------------------------------------
// pair kernel dispatch
// ---------------------------------------------------------------------------------------------------
PairLaunch Engine::pair_launch(const StepParams& Q) { return PairLaunch{Q, S_, dPots_, cur(), dCounts_, dCellStart_, dPartials_, maxBlocks_, stream_}; }

void Engine::launch_pair(const StepPlan& plan)
{
    int splitBlocks = 0;            // partial-sum slots a split or list launch has booked into (0: the plain tile grid)
    if (plan.pair != StepPlan::PAIR_ATOM)
    {
        StepParams Q = P_;
        Q.fuseKick = plan.tileKick;
        const PairLaunch C = pair_launch(Q);
        // (a step that records the lists records them in the entry format the store has decided on, and walks them in it)
        if (plan.lists == StepPlan::LISTS_RECORD) lists_.begin_recording();
        const PairLists pl = lists_.pair_lists();
        if (plan.overlapHalo)
        {   // interior x-layers [2 hw, ncx - 2 hw) first; then, once the neighbours' coordinates have landed, the two runs of boundary layers
            const int plane = P_.nc[1] * P_.nc[2], hw = P_.hw[0];
            PairRange in, lo, hi;
            in.first = 2 * hw * plane; in.n = (P_.ncxLocal - 4 * hw) * plane;
            lo.first = hw * plane; lo.n = hw * plane;
            hi.first = (P_.ncxLocal - 2 * hw) * plane; hi.n = hw * plane;
            const bool lists = plan.pair == StepPlan::PAIR_LIST;
            int nb = 0;
            auto run = [&](PairRange& r) {
                r.blockBase = nb;
                if (lists)
                {
                    nb += launch_pair_list(C, r, pl, NextStep(), plan.wantEnergies);
                    nb += launch_pair_cleanup(C, r, pl);
                }
                else
                {
                    launch_pair_tile(C, r, PairLists(), 0, NextStep(), split_);
                    nb += pair_range_grid(r.n) * split_.n;
                }
            };
            timed(lists ? "pair_list" : "pair_tile", [&] {
                run(in);
                HIP_CHECK(hipStreamWaitEvent(stream_, evHalo_, 0));
                run(lo);
                run(hi);
            });
            splitBlocks = nb;
        }
        else
        {
            if (plan.pair == StepPlan::PAIR_LIST)
            {   // lazy re-sort.  The step that rebuilds the cells first makes the lists (candidates of every tile, partners of every atom); then, like every
                // plain step until the next rebuild, it walks them; the clean-up launch stages the cells that keep no list
                if (plan.lists == StepPlan::LISTS_RECORD)
                {   // (k_rank_gather has cleared the count of cells without a list)
                    timed("build_lists", [&] { launch_build_lists(C, PairRange(), pl); });
                    listsValid_ = true;
                    unlistedState_ = 0;
                    if (nranks_ > 1 && !capturing_)
                    {
                        hUnlisted_.post(&pl.noList[LR_UNLISTED_NOW], sizeof(int32_t), stream_);
                        hUnlisted_.mark(stream_);
                    }
                }
                else if (plan.cleanup == StepPlan::CLEANUP_UNLESS_IDLE && unlistedState_ == 0 && hUnlisted_.landed())
                    unlistedState_ = (*hUnlisted_.as<int32_t>() == 0) ? 1 : 2;
                // (the one answer the plan leaves open: has this slab rank learnt by now that no cell is without a list?)
                const bool skipCleanup = plan.cleanup == StepPlan::CLEANUP_NONE || (plan.cleanup == StepPlan::CLEANUP_UNLESS_IDLE && unlistedState_ == 1);
                NextStep nx;
                nx.st = dStats_; nx.cnt = dCounts_; nx.R0 = ref_;
                nx.pendingAfter = plan.pendingAfter;
                if (plan.fuseNext) { nx.xn = altXyz_[cur_][0]; nx.yn = altXyz_[cur_][1]; nx.zn = altXyz_[cur_][2]; }
                if (plan.closesStep) { nx.photons = dPhotons_; nx.uvx = dUvx_; nx.uvy = dUvy_; nx.uvz = dUvz_; }
                StepParams QL = Q; QL.fuseKick = plan.listKick;
                const bool foldDrift = plan.listKick == KICK_DRIFT;
                if (foldDrift)
                {
                    nx.xd = altXyz_[cur_][0]; nx.yd = altXyz_[cur_][1]; nx.zd = altXyz_[cur_][2];
                    nx.driftBlocks = div_up(div_up(capacity_, 2), kBlock);           // (the grid of the k_drift_plain2 launch this replaces, sort_and_forces)
                    if (profile_ && !capturing_) timers_.count("fold_drift");
                }
                const PairLaunch CL = pair_launch(QL);
                if (profile_ && !capturing_ && pl.entryBytes == 1) timers_.count("narrow_lists");      // (a count, no time of its own: the launch is timed as pair_list)
                timed("pair_list", [&] { splitBlocks = launch_pair_list(CL, PairRange(), pl, nx, plan.wantEnergies); });
                if (!skipCleanup)
                    timed("pair_cleanup", [&] { splitBlocks += launch_pair_cleanup(C, PairRange(), pl, nx); });
                if (plan.fuseNext || foldDrift)
                {   // the next step's positions are in the other set of coordinate arrays now
                    AtomArrays& A = cur();
                    std::swap(A.x, altXyz_[cur_][0]); std::swap(A.y, altXyz_[cur_][1]); std::swap(A.z, altXyz_[cur_][2]);
                }
            }
            else
                timed("pair_tile", [&] { launch_pair_tile(C, PairRange(), pl, 0, NextStep(), split_); });
        }
    }
    else
        timed("pair_atom", [&] {
            hipLaunchKernelGGL(k_pair_atom, dim3(div_up(capacity_, kBlock)), dim3(kBlock), 0, stream_, P_, S_, dPots_, cur(), dCounts_, dCellStart_,
                               dCellOfSorted_, dPartials_, maxBlocks_);
        });
    notes_.pairBlocksUsed = (plan.pair != StepPlan::PAIR_ATOM) ? (splitBlocks ? splitBlocks : pair_tile_grid(P_) * split_.n) : div_up(capacity_, kBlock);
    notes_.blocksEver = std::max(notes_.blocksEver, std::max(notes_.pairBlocksUsed, div_up(capacity_, kBlock)) + 1);
}

// slab ranks: where the boundary layers sit in the sorted arrays, as read back behind the last sort
void Engine::take_halo_info()
{
    if (!haloInfoPending_) return;
    hHalo_.wait();
    haloInfoPending_ = false;
    adopt_halo_info(hHalo_.as<int32_t>());
}

// Behind every sort that opens an interval of plain steps the ranks tell each other how many boundary atoms they will send per plain step (k_rank_gather
// left {send count, ghost count} per side in the halo block, HaloInfo); the neighbours' pairs land behind them.
// Fixed-size messages: this exchange cannot itself be mismatched.
void Engine::post_count_exchange()
{
    int32_t* h = dHaloInfo_;
    xch_->exchange_counts(left(), right(), &h[HI_SEND_LEFT], &h[HI_SEND_RIGHT], &h[HI_LEFT_SENDS], &h[HI_RIGHT_SENDS], 2, stream_);
}

// ... and before the first plain step posts a send or a receive, every rank checks that its ghost ranges are exactly as long as what the neighbours
// will send: a disagreement (a protocol error - the ranges are equal by construction) is reported as an error instead of hanging in RCCL or silently
// shifting coordinates onto the wrong atoms
void Engine::adopt_halo_info(const int32_t* h)
{
    halo_[0] = h[HI_OWNED_BEGIN]; halo_[1] = h[HI_LEFT_END]; halo_[2] = h[HI_RIGHT_BEGIN]; halo_[3] = h[HI_OWNED_END]; halo_[4] = h[HI_NTOTAL];
    const int ghostsLeft = h[HI_OWNED_BEGIN], ghostsRight = h[HI_NTOTAL] - h[HI_OWNED_END], sendLeft = h[HI_SEND_LEFT], sendRight = h[HI_SEND_RIGHT];
    // (both ranks of a boundary evaluate the same two equalities, so they fail together)
    if (h[HI_RIGHT_SENDS] != ghostsRight || h[HI_RIGHT_HOLDS] != sendRight || h[HI_LEFT_SENDS] != ghostsLeft || h[HI_LEFT_HOLDS] != sendLeft)
        throw std::runtime_error("slab decomposition: the neighbours disagree about their boundary atoms (left boundary: this rank sends " + std::to_string(sendLeft) +
                                 " and holds " + std::to_string(ghostsLeft) + " ghosts, the neighbour holds " + std::to_string(h[HI_LEFT_HOLDS]) + " and sends " + std::to_string(h[HI_LEFT_SENDS]) +
                                 "; right boundary: sends " + std::to_string(sendRight) + ", holds " + std::to_string(ghostsRight) + ", the neighbour holds " +
                                 std::to_string(h[HI_RIGHT_HOLDS]) + " and sends " + std::to_string(h[HI_RIGHT_SENDS]) + "): no coordinate exchange was posted");
}

// one message to each x-neighbour: migrants + halo (packed by k_integrate1_bin; protocol in slab.hip.h)
void Engine::exchange_halo()
{
    timed("exchange", [&] { xch_->exchange(left(), right(), dMsg_[0], dMsg_[1], dMsg_[2], dMsg_[3], lay_.bytes(), stream_); });
    const int recvCap = 2 * (lay_.migCap + lay_.haloCap);
    timed("unpack_halo", [&] {
        hipLaunchKernelGGL(k_unpack, dim3(div_up(recvCap, kBlock)), dim3(kBlock), 0, stream_, P_, cur(), dCounts_, capacity_, lay_, dMsg_[2], dMsg_[3],
                           dCellOf_, dSlotOf_, dCellCount_, dMsg_[0], dMsg_[1]);
    });
}

// ---------------------------------------------------------------------------------------------------
// iter_fastCellList (cuPairs.cu:2519-2567): histogram -> [halo] -> scan -> sort -> pair forces
// ---------------------------------------------------------------------------------------------------
void Engine::sort_and_forces(const StepPlan& plan)
{
    const int gridAtoms = div_up(capacity_, kBlock);
    P_.cycleStep = plan.cycleStep;          // (the slack-violation flag is indexed by it)
    if (plan.stepMode == STEP_PLAIN)
    {   // plain step of the lazy re-sort: integrate only; slots, cells and buffers stay as they are
        if (plan.opener == StepPlan::OPEN_DRIFT)
            timed("drift", [&] {
                hipLaunchKernelGGL(k_drift_plain2, dim3(div_up(div_up(capacity_, 2), kBlock)), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dPartials_,
                                   maxBlocks_, dStats_, ref_);
            });
        else if (plan.opener == StepPlan::OPEN_PLAIN2)
            timed("integrate1", [&] {
                hipLaunchKernelGGL(k_integrate_plain2, dim3(div_up(div_up(capacity_, 2), kBlock)), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dPartials_,
                                   maxBlocks_, dStats_, ref_);
            });
        else if (plan.opener == StepPlan::OPEN_PLAIN)
        timed("integrate1", [&] {
            hipLaunchKernelGGL(k_integrate1_bin<STEP_PLAIN>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dCellOf_, dSlotOf_,
                               dCellCount_, dPartials_, maxBlocks_, lay_, dMsg_[0], dMsg_[1], dStats_, ref_);
        });
        if (nranks_ > 1)
        {   // the neighbours hold this rank's boundary atoms in the order of the last sort: only their coordinates (and radii) travel
            take_halo_info();
            AtomArrays& A = cur();
            double* arr[4] = {A.x, A.y, A.z, A.rad};
            if (plan.overlapHalo)
            {
                HIP_CHECK(hipEventRecord(evIntegrated_, stream_));
                HIP_CHECK(hipStreamWaitEvent(commStream_, evIntegrated_, 0));
            }
            hipStream_t xs = plan.overlapHalo ? commStream_ : stream_;
            timed("exchange_coords", [&] {
                xch_->exchange_ranges(left(), right(), arr, P_.use_radii ? 4 : 3, halo_[0], halo_[1] - halo_[0], halo_[2], halo_[3] - halo_[2], 0, halo_[0], halo_[3],
                                      halo_[4] - halo_[3], xs);
            });
            if (plan.overlapHalo) HIP_CHECK(hipEventRecord(evHalo_, commStream_));
        }
        sinceSort_++;
    }
    else
    {
    if (plan.opener == StepPlan::OPEN_RESORT)
        timed("integrate1_bin", [&] {
            hipLaunchKernelGGL(k_integrate1_bin<STEP_RESORT>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dCellOf_, dSlotOf_,
                               dCellCount_, dPartials_, maxBlocks_, lay_, dMsg_[0], dMsg_[1], dStats_, ref_);
        });
    else
    {
        HIP_CHECK(hipMemsetAsync(dCellCount_, 0, sizeof(int32_t) * (size_t)(P_.nCellLocal + 1), stream_));
        timed("bin", [&] {
            hipLaunchKernelGGL(k_integrate1_bin<STEP_BIN_ONLY>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dCellOf_, dSlotOf_,
                               dCellCount_, dPartials_, maxBlocks_, lay_, dMsg_[0], dMsg_[1], dStats_, ref_);
        });
    }
    if (nranks_ > 1) exchange_halo();
    const int nChunks = div_up(P_.nCellLocal, kScanChunk);
    timed("scan_cells", [&] {
        if (P_.nCellLocal <= kScanSingleMax)
            hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, stream_, P_.nCellLocal, dCellCount_, dCellStart_, dCounts_, dStats_, plan.setPending);
        else
        {
            hipLaunchKernelGGL(k_scan_totals, dim3(nChunks), dim3(kBlock), 0, stream_, P_.nCellLocal, dCellCount_, dChunkTot_);
            hipLaunchKernelGGL(k_scan_apply, dim3(nChunks), dim3(kBlock), 0, stream_, P_.nCellLocal, dCellCount_, dChunkTot_, dCellStart_, dCounts_, dStats_, plan.setPending);
        }
    });
    timed("place", [&] {
        hipLaunchKernelGGL(k_place, dim3(gridAtoms), dim3(kBlock), 0, stream_, dCounts_, dCellOf_, dSlotOf_, dCellStart_, cur().id, dTmpId_, dTmpSrc_,
                           dTmpCell_);
    });
    timed("rank_gather", [&] {
        hipLaunchKernelGGL(k_rank_gather, dim3(gridAtoms), dim3(kBlock), 0, stream_, dCounts_, dCellStart_, dTmpId_, dTmpSrc_, dTmpCell_, cur(), oth(),
                           dCellOfSorted_, (P_.tstat == AZTOT_TSTAT_RADI || P_.use_radii || thermoTouched_) ? 2 : 0, P_, dCounts_, bonded_.idxOfId, ref_,
                           dHaloInfo_, plan.lists == StepPlan::LISTS_RECORD ? &lists_.report[LR_UNLISTED_NOW] : nullptr, lists_.on ? lists_.rel : nullptr);
    });
    cur_ ^= 1;
    sinceSort_ = 0;
    if (!capturing_ && plan.stepMode == STEP_RESORT) rebuilds_++;
    listsValid_ = false;            // (until this step's launch_pair records them)
    if (nranks_ > 1 && lazyOn_ && lazyK_ > 1)
    {   // where the boundary layers sit in the sorted arrays: [ownedBegin, end of layer 2hw-1) goes left, [start of layer ncx-2hw, ownedEnd) goes right;
        // ghosts are [0, ownedBegin) and [ownedEnd, nTotal).  One small read-back per sort.
        post_count_exchange();
        hHalo_.post(dHaloInfo_, sizeof(int32_t) * HI_COUNT, stream_);
        hHalo_.mark(stream_);
        haloInfoPending_ = true;      // (no stall here: take_halo_info waits when the numbers are needed)
    }
    }
    launch_pair(plan);
    if (hasEwald_) launch_ewald();
    if (hasSpme_) launch_spme();
    if (hasBonded_ && plan.withBonded)     // exec_bondlist + exec_anglelist, main.cpp:101-104 (GPU path: main.cu:307-312,353-363)
        timed("bonded", [&] {
            if (nranks_ > 1)
                hipLaunchKernelGGL(k_bonded<true>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, cur(), dCounts_, bonded_, dPartials_, maxBlocks_);
            else
                hipLaunchKernelGGL(k_bonded<false>, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, cur(), dCounts_, bonded_, dPartials_, maxBlocks_);
        });
    check_launch("sort + force kernels");
}

void Engine::collect_and_finalize(unsigned slotMask)
{
    timed("collect", [&] {
        hipLaunchKernelGGL(k_collect, dim3(PS_COUNT * kCollectParts), dim3(256), 0, stream_, dPartials_, maxBlocks_, div_up(capacity_, kBlock), notes_.pairBlocksUsed,
                           dStage_, slotMask, notes_.ekinFromPair ? 1 : 0, notes_.blocksEver);
    });
    timed("finalize", [&] { hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, stream_, P_, dStats_, dStage_, slotMask); });
}

void Engine::forces(bool withBonded)
{
    if (!failed_.empty()) throw std::runtime_error("this handle failed in an earlier call: " + failed_);
    settle();
    snap_.valid = false;
    sinceSort_ = kNoSort;           // a sort interval does not run on through a force call (it re-bins wrapped coordinates)
    sort_and_forces(plan_forces(withBonded));
    forget_interval();
    // energies of this configuration; kinetic energy and wall counters are left untouched
    unsigned mask = (1u << PS_EVDW) | (1u << PS_ECOUL) | (1u << PS_DROPPED);
    if (hasBonded_ && withBonded) mask |= (1u << PS_EBOND) | (1u << PS_EANGLE);
    collect_and_finalize(mask);
    HIP_CHECK(hipMemsetAsync(dCellCount_, 0, sizeof(int32_t) * (size_t)(P_.nCellLocal + 1), stream_));
    sync();
    check_overflow();
}

// what a step launches (step_plan.h): decided here, once, from host state alone; executed below
StepPlan Engine::plan_forces(bool withBonded) const
{
    StepPlan p;                     // STEP_BIN_ONLY: bin + sort, no lists, no kick, energies booked, nothing closes it
    p.pair = (pair_variant() == 2) ? StepPlan::PAIR_TILE : StepPlan::PAIR_ATOM; p.withBonded = withBonded;
    return p;
}

StepPlan Engine::plan_step(int stepsLeft) const
{
    StepPlan p;
    // does this step need the all-atom kinetic energy on the device?  Nose-Hoover: every step; equilibration rescaling: the steps it acts on
    // (integrators.cpp:511-522: step <= nequil and a multiple of eqfreq) - the host knows the number of the step it is launching.  (A captured cycle is
    // replayed at many step numbers: cycles are captured only once the equilibration period is over, can_graph.)
    const long long iStep = hostStep_ + 1;
    p.scalingDue = !capturing_ && P_.nEq > 0 && iStep <= P_.nEq && P_.freqEq > 0 && (iStep % P_.freqEq) == 0;
    p.equil = p.scalingDue || P_.tstat == AZTOT_TSTAT_NOSE;
    const bool plain = lazyOn_ && sinceSort_ < lazyK_ - 1;
    p.stepMode = plain ? STEP_PLAIN : STEP_RESORT; p.cycleStep = plain ? sinceSort_ + 1 : 0;
    // is there a next step before the host looks or the cycle ends, and is it a plain one?
    const bool nextPlain = lazyOn_ && p.cycleStep < lazyK_ - 1 && stepsLeft > 0;
    const bool everyStep = debug_ & DBG_ENERGIES_EVERY_STEP;
    // -- opener.  A kicked step (KICK_BOTH: v stored, no f) takes the drift alone; one the previous pair / boundary kernel opened takes nothing
    if (left_ == StepPlan::LEFT_KICKED) p.opener = StepPlan::OPEN_DRIFT;
    else if (!plain) p.opener = StepPlan::OPEN_RESORT;
    else if (left_ == StepPlan::LEFT_OPENED) p.opener = StepPlan::OPEN_NONE;
    // one GPU (the owned range starts at 0: 16-byte loads are aligned), nothing scales the velocities at the start of the step: two atoms per thread
    else p.opener = (nranks_ == 1 && P_.tstat != AZTOT_TSTAT_NOSE && !(debug_ & DBG_PLAIN_ONE_ATOM)) ? StepPlan::OPEN_PLAIN2 : StepPlan::OPEN_PLAIN;
    p.setPending = lazyKick_ ? 1 : 0;
    // -- exchange.  A plain slab step's coordinate exchange touches the ghost ranges only, and the cells two or more layers inside the slab never read them
    // (SURVEY 8e): it may run on its own stream next to the interior cells' pair forces; the boundary cells wait for it (launch_pair).  Not while kernels
    // are being timed one by one, not with the per-atom kernel, and not when there is no interior to speak of.
    // OPT-IN (DBG_OVERLAP_HALO): measured on one rank of 7 (loopback) the two cross-stream event waits and the two extra launches cost 30 us
    // where the exchange they hide takes 7 (0.0685 -> 0.0981 ms/step), so the default is the serial order
    p.overlapHalo = plain && nranks_ > 1 && !profile_ && xch_->device_side() && pair_variant() == 2 && P_.ncxLocal - 4 * P_.hw[0] >= 1 && (debug_ & DBG_OVERLAP_HALO);
    // -- lists and pair kernel.  A step that opens an interval of plain steps records the lists and walks them, like every plain step behind it.
    // (walks_lists() holds lists_.on, and PairLists::cand is non-null exactly when the store is on - ListStore::allocate / release / pair_lists - and
    // the tile variant: a step with lists is a k_pair_list step)
    if (walks_lists()) p.lists = plain ? StepPlan::LISTS_WALK : StepPlan::LISTS_RECORD;
    p.pair = pair_variant() != 2 ? StepPlan::PAIR_ATOM : (p.lists != StepPlan::LISTS_NONE ? StepPlan::PAIR_LIST : StepPlan::PAIR_TILE);
    // pair energies are looked at through the statistics of a call's last step only (finish_steps): the list kernel of every other step books none
    // (options.energies_every_step: every step does).  Inside a graph the last step of the cycle is the one that may be the call's last
    p.wantEnergies = stepsLeft == 0 || everyStep;
    // the clean-up launch stages the cells that keep no list: none on optimistic runs (one GPU only, choose_optimism); a slab rank drops it from the plain
    // steps of an interval once it has learnt that the build left no such cell; the split launch of the overlapped exchange always carries it
    if (optimistic_) p.cleanup = StepPlan::CLEANUP_NONE;
    else if (nranks_ > 1 && plain && !capturing_ && !p.overlapHalo) p.cleanup = StepPlan::CLEANUP_UNLESS_IDLE;
    // plain NVE steps leave integrate2 to somebody else (decided once, in the constructor): small systems / slabs -> the tile
    // kernel's epilogue (fuseEpilogue_, which holds the tile variant); large ones -> the next step's k_integrate1_bin (lazyKick_, see finish_steps)
    p.tileKick = p.listKick = fuseEpilogue_ ? KICK_SECOND : KICK_NONE; p.ekinFromPair = fuseEpilogue_;
    // does this step's pair kernel also open the next step?  Only if it walks the lists (k_pair_list and its clean-up launch carry the epilogue; the split launch does not)
    p.fuseNext = fuseNextOk_ && p.pair == StepPlan::PAIR_LIST && nextPlain && !p.overlapHalo;
    // thermostat runs: only where no clean-up launch follows (it has no thermostat epilogue), on steps without equilibration scaling, never with energies on every step
    // (and one wave per cell: in the multi-wave kernels of dense systems the thermostat's registers cost the loop more than the launch saves -
    //  measured with a second radius array for case study 2's surk kernel: S40 0.076 -> 0.093 ms/step, case study 2 unchanged; not kept)
    if (fuseNextTstat_) p.fuseNext = p.fuseNext && optimistic_ && !p.equil && lists_.waves == 1 && !everyStep;
    p.closesStep = p.fuseNext && fuseNextTstat_;        // (second half-kick + thermostat in the fused epilogue: the pair launch has closed this step)
    // this step's second half-kick is owed to the next k_integrate1_bin (a call may open with a plain step, where no scan re-arms the flag)
    p.pendingAfter = (!p.closesStep && lazyKick_) ? 1 : -1;
    // ... or kick for it?  (foldKickOk_: plain NVE on ONE GPU - so never a split launch - that walks lists and never fuses the next step.)  The same walk of
    // the lists with no clean-up launch behind it (it has no such epilogue), a step that books no energies, and a plain step of this run to follow: whoever
    // else may come next - a rebuild (k_integrate1_bin and k_rank_gather need the force and the kick state they know), a look, the end of the call and
    // everything that can read the state there - finds the canonical state, velocities half-kicked, forces valid, DevStats::pendingKick as ever.
    // Both half-kicks in this launch: neither is owed.  With foldDriftOk_ the next step's drift too (KICK_DRIFT): that step is opened like a fused one
    const bool fold = foldKickOk_ && p.pair == StepPlan::PAIR_LIST && nextPlain && optimistic_ && !p.fuseNext && !p.wantEnergies;
    if (fold) { p.listKick = foldDriftOk_ ? KICK_DRIFT : KICK_BOTH; p.pendingAfter = 0; }
    // -- closer.  Radiative thermostat without equilibration scaling: nothing global happens between the second half-kick and the thermostat - one launch
    // (DBG_KICK_POST_SPLIT: two, as everywhere else); when a plain step follows, the same launch opens it (k_boundary_radi; DBG_NO_BOUNDARY_RADI: no)
    const bool kickHere = !p.closesStep && !fuseEpilogue_ && !lazyKick_;
    const bool kickAndPost = kickHere && !p.equil && P_.tstat == AZTOT_TSTAT_RADI && !(debug_ & DBG_KICK_POST_SPLIT);
    if (kickAndPost) p.closer = (nextPlain && !(debug_ & DBG_NO_BOUNDARY_RADI)) ? StepPlan::CLOSE_BOUNDARY_RADI : StepPlan::CLOSE_INTEGRATE2_POST;
    else if (kickHere) p.closer = StepPlan::CLOSE_INTEGRATE2;
    p.post = (p.equil || P_.tstat == AZTOT_TSTAT_RADI) && !kickAndPost && !p.closesStep;
    if (p.fuseNext || p.listKick == KICK_DRIFT || p.closer == StepPlan::CLOSE_BOUNDARY_RADI) p.leaves = StepPlan::LEFT_OPENED;     // -- hand-over
    else if (fold) p.leaves = StepPlan::LEFT_KICKED;
    if (p.opener == StepPlan::OPEN_DRIFT && !plain) throw std::runtime_error("a step that needs the forces follows a pair kernel that stored none");     // -- what no plan may hold
    if ((fold && (p.cleanup != StepPlan::CLEANUP_NONE || p.wantEnergies || !nextPlain)) || (p.closesStep && !p.fuseNext))
        throw std::runtime_error("step plan: a fold with a clean-up launch, with energies or without a plain step behind it, or a thermostat close without next-step fusion");
    return p;
}

// ---------------------------------------------------------------------------------------------------
// one iteration of the loop body of main.cu:281-410 (serial twin: main.cpp:89-142)
// ---------------------------------------------------------------------------------------------------
void Engine::launch_step_kernels(int stepsLeft)
{
    const StepPlan plan = plan_step(stepsLeft);
    const int gridAtoms = div_up(capacity_, kBlock);
    if (P_.tstat == AZTOT_TSTAT_NOSE) timed("nose_begin", [&] { hipLaunchKernelGGL(k_nose_begin, dim3(1), dim3(64), 0, stream_, P_, dStats_); });
    sort_and_forces(plan);
    notes_.ekinFromPair = plan.ekinFromPair;
    if (plan.closer == StepPlan::CLOSE_BOUNDARY_RADI)
    {
        StepParams Q = P_;
        Q.cycleStep = sinceSort_ + 1;              // of the step being opened
        timed("boundary", [&] {
            hipLaunchKernelGGL(k_boundary_radi, dim3(gridAtoms), dim3(kBlock), 0, stream_, Q, S_, cur(), dCounts_, dPartials_, maxBlocks_, dStats_, dPhotons_, dUvx_, dUvy_,
                               dUvz_, ref_);
        });
    }
    else if (plan.closer == StepPlan::CLOSE_INTEGRATE2_POST)
        timed("integrate2_post", [&] {
            hipLaunchKernelGGL(k_integrate2_post, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dCellCount_, P_.nCellLocal, dPartials_,
                               maxBlocks_, dStats_, dPhotons_, dUvx_, dUvy_, dUvz_);
        });
    else if (plan.closer == StepPlan::CLOSE_INTEGRATE2)
        timed("integrate2", [&] {
            hipLaunchKernelGGL(k_integrate2, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dCellCount_, P_.nCellLocal, dPartials_,
                               maxBlocks_, dStats_);
        });
    if (plan.equil)
    {
        timed("reduce_kin", [&] {
            hipLaunchKernelGGL(k_reduce_kin, dim3(1), dim3(1024), 0, stream_, P_, dPartials_, maxBlocks_, gridAtoms, dStats_, dEkGlobal_);
        });
        if (nranks_ > 1)
        {   // the scaling factor needs the kinetic energy of ALL ranks (equilibration steps only)
            double ek = 0.0;
            HIP_CHECK(hipMemcpyAsync(&ek, dEkGlobal_, sizeof(double), hipMemcpyDeviceToHost, stream_));
            HIP_CHECK(hipStreamSynchronize(stream_));
            xch_->allreduce_sum(&ek, 1, stream_);
            HIP_CHECK(hipMemcpyAsync(dEkGlobal_, &ek, sizeof(double), hipMemcpyHostToDevice, stream_));
        }
        timed("scale_decision", [&] { hipLaunchKernelGGL(k_scale_decision, dim3(1), dim3(64), 0, stream_, P_, dStats_, dEkGlobal_); });
    }
    if (plan.post)
        timed("post_tstat", [&] {
            hipLaunchKernelGGL(k_post, dim3(gridAtoms), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dStats_, dPhotons_, dUvx_, dUvy_, dUvz_,
                               dPartials_, maxBlocks_);
        });
    if (plan.scalingDue && P_.tstat != AZTOT_TSTAT_NOSE)
    {   // the factor has been applied: the steps that follow take the short path, which never decides one (DevStats::vscale is read by every thermostat kernel)
        static const double one = 1.0;
        HIP_CHECK(hipMemcpyAsync(&dStats_->vscale, &one, sizeof(double), hipMemcpyHostToDevice, stream_));
    }
    notes_.lastStepEquil = plan.equil;
    left_ = plan.leaves;
    if (!capturing_) hostStep_++;
}

// the per-block partial sums are folded into the statistics only when somebody can look at them: at the end of a
// step() call (energies are those of the last step; wall momenta / crossing counts pile up in between)
void Engine::finish_steps()
{
    if (kickOwed_)
    {   // the deferred second half-kick of the last step + its kinetic energy
        timed("integrate2", [&] {
            hipLaunchKernelGGL(k_integrate2, dim3(div_up(capacity_, kBlock)), dim3(kBlock), 0, stream_, P_, S_, cur(), dCounts_, dCellCount_, P_.nCellLocal,
                               dPartials_, maxBlocks_, dStats_);
        });
        kickOwed_ = false;
    }
    unsigned mask = (1u << PS_COUNT) - 1u;
    if (notes_.lastStepEquil) mask &= ~(1u << PS_EKIN);   // k_reduce_kin / k_scale_decision own engKin then
    if (!(P_.nEq > 0 || P_.tstat == AZTOT_TSTAT_RADI)) mask &= ~(1u << PS_ETEMP);
    if (!hasBonded_) mask &= ~((1u << PS_EBOND) | (1u << PS_EANGLE));
    collect_and_finalize(mask);
}

// may the plain steps of the next window run without the clean-up launch?  (decided at the start of a call and after every look: the answer is baked into
// kernel arguments, so a change drops the captured graphs)
void Engine::choose_optimism()
{
    // (any size since round 4: on 1 M atoms the launch cost 6.9 us of a 123 us step - the drain and refill of the chip around a kernel that finds nothing
    //  to do -, a snapshot is 100 MB = 33 us per look, and looks are up to 256 steps apart)
    const bool want = nranks_ == 1 && walks_lists() && lazyMeasured_ &&
                      safeLooks_ == 0 && !unlistedAtLook_ && unlistedState_ != 2 && !(debug_ & DBG_ALWAYS_CLEANUP);
    if (want != optimistic_)
    {
        optimistic_ = want;
        P_.optimistic = want ? 1 : 0;
        drop_graphs();
        if (!want) snap_.valid = false;
    }
}

void Engine::copy_state(DynState from, DynState to)
{
    StateCopy C;
    const auto src = double_arrays(from.A), dst = double_arrays(to.A);
    for (int k = 0; k < 11; k++) { C.srcD[k] = *src[k]; C.dstD[k] = *dst[k]; }
    C.srcI[0] = from.A.type; C.dstI[0] = to.A.type; C.srcI[1] = from.A.id; C.dstI[1] = to.A.id;
    C.srcP = from.partials; C.dstP = to.partials; C.nP = (long long)PS_COUNT * maxBlocks_;
    C.srcS[0] = (const int32_t*)from.stats; C.dstS[0] = (int32_t*)to.stats; C.nS[0] = (int)(sizeof(DevStats) / 4);
    C.srcS[1] = (const int32_t*)from.counts; C.dstS[1] = (int32_t*)to.counts; C.nS[1] = (int)(sizeof(Counts) / 4);
    hipLaunchKernelGGL(k_copy_state, dim3(div_up(capacity_, kBlock)), dim3(kBlock), 0, stream_, C, capacity_);
}

// Slab ranks: the dynamic state as it stands (the host has just looked and found no skin violation), device to device.  The arrays are those an exact
// restart needs (aztot_state + aztot_clock): everything else is rebuilt by the step that rebuilds the cells, and the replay opens with one.
void Engine::take_snapshot()
{
    if (!snap_.A.x)
    {
        alloc_atoms(snap_.A, false);
        snap_.stats = dev_alloc<DevStats>(1); snap_.counts = dev_alloc<Counts>(1); snap_.partials = dev_alloc<double>((size_t)PS_COUNT * maxBlocks_);
    }
    copy_state(live(), snap_);
    snap_.buf = buf_state();
    snap_.hostStep = hostStep_;
    snap_.valid = true;
    stepsSinceSnap_ = 0;
}

// ... and back to it: the steps since the snapshot run again with the cells rebuilt on every one of them (no atom can leave a slack that is never used)
void Engine::replay_from_snapshot()
{
    if (!snap_.valid) throw std::runtime_error("lazy re-sort on slab ranks: an atom left its cell's slack and there is no snapshot to go back to");
    sync();
    drop_graphs();
    set_buf_state(snap_.buf);
    copy_state(snap_, live());
    forget_interval(); left_ = StepPlan::LEFT_UNTOUCHED; haloInfoPending_ = false; unlistedState_ = 0;
    kickOwed_ = false;
    hostStep_ = snap_.hostStep;
    if (nranks_ > 1) lazyK_ = 1;
    else
    {   // one GPU: the same steps with the clean-up launch behind every k_pair_list (it stages the cells without a list and, from the step of a violation
        // on, every cell with the wider stencil)
        optimistic_ = false; P_.optimistic = 0;
        rollbacks_ = std::min(rollbacks_ + 1, 12);
        safeLooks_ = 4 << rollbacks_;          // 8, 16, 32 ... looks on the safe side: a system that keeps outgrowing its lists stops trying
    }
    const long long n = stepsSinceSnap_;
    if (std::getenv("AZTOT_VERBOSE")) std::fprintf(stderr, "aztot: rank %d: a skin violation (or a cell without a list) found at a look - %lld steps run again, %s\n", rank_, n, nranks_ > 1 ? "cells rebuilt every step" : "with the clean-up launch");
    if (n > 0) run_steps((int)n);
    stepsSinceSnap_ = n;
}

// An error inside a call leaves the host's picture of the device (cycles, lists, the deferred kick, its own step count) unreliable: the handle is dead
// for stepping from then on and says why; reads (aztot_get_stats, aztot_md_to_host, aztot_get_clock) still work for a post-mortem and report what the
// device holds (a secondary "step counts differ" error used to hide the first one).
void Engine::mark_failed(const char* what) noexcept
{
    if (failed_.empty()) failed_ = what ? what : "unknown error";
    unsettled_ = false;
    snap_.valid = false;
    if (stream_) (void)hipStreamSynchronize(stream_);
    (void)hipGetLastError();
    DevStats s;
    if (dStats_ && hipMemcpy(&s, dStats_, sizeof(DevStats), hipMemcpyDeviceToHost) == hipSuccess) hostStep_ = s.step;
    (void)hipGetLastError();
}

void Engine::step(int nsteps)
{
    if (nsteps <= 0) return;
    if (!failed_.empty()) throw std::runtime_error("this handle failed in an earlier call and cannot step on: " + failed_);
    try { step_body(nsteps); }
    catch (const std::exception& e) { mark_failed(e.what()); throw; }
    catch (...) { mark_failed("unknown exception"); throw; }
}

// Does this call end with the look / statistics / read-backs right away?  Slab ranks (collectives every rank must take together), bonded terms
// (an overflow flag to read back), per-kernel timing (events to drain): always.  One GPU otherwise: only when a look at the sort interval is due
// (8, 16, ... 256 steps after the last one, or never made) - else the call returns with its kernels queued, and whoever reads state or statistics next
// (or the next look) settles: a caller that steps one step at a time (the reference's loop is per step, main.cu:281-410) pays for the second half-kick
// launch, the statistics reduction, the stream synchronisation and the snapshot once per look instead of once per step.
bool Engine::settle_now() const
{
    if (nranks_ > 1 || hasBonded_ || profile_ || (debug_ & DBG_SETTLE_EVERY_CALL)) return true;
    if (!lazyOn_) return false;
    return !lazyMeasured_ || sinceLook_ >= lazyWindow_;
}

// The end of a call, possibly deferred (settle_now): the deferred second half-kick and the statistics of the last step, the look at the sort interval
// (a window of steps run again where it finds a skin violation that nothing had repaired on the spot), overflow checks on the state the caller will see,
// what the next call needs.
// A look: what the window just run has left on the device (look_sync), the sort interval and the lists from it (adapt_sort_interval), and where the window
// turns out not to have been exact (slab ranks, all together: an atom left its slack; one GPU without the clean-up launch: that, or a cell without a
// list) those steps again from the snapshot, exactly, then a look that cannot fail.  The two callers differ on purpose.  At the end of a call the
// statistics of the call's last step have been reduced already, so the steps run again owe their second half-kick (kickOwed_) and their statistics once
// more; inside a call the steps that follow pay the kick on the device (DevStats::pendingKick) and nobody has asked for statistics.  A look inside a call
// was due, so the window doubles; the end of a call stands in for a due look only if at least half a window has gone by.
void Engine::look(bool callEnd)
{
    look_sync();
    if (!lazyOn_) return;
    if (!adapt_sort_interval())
    {
        replay_from_snapshot();
        if (callEnd)
        {
            kickOwed_ = lazyKick_;
            finish_steps();
            check_launch("step kernels (run again)");
        }
        look_sync();
        if (!adapt_sort_interval()) throw std::runtime_error("lazy re-sort: a skin violation in a run that rebuilds its cells every step");
    }
    if (!callEnd || 2 * sinceLook_ >= lazyWindow_) lazyWindow_ = std::min(window_cap(), 2 * lazyWindow_);
    sinceLook_ = 0;
    if (safeLooks_ > 0) safeLooks_--;
}

void Engine::settle()
{
    if (!unsettled_ || !failed_.empty()) return;
    unsettled_ = false;
    try
    {
        finish_steps();
        check_launch("end-of-call kernels");
        look(true);
        // (on the state the caller will see: an optimistic window that had to be run again is inexact until it has been - ADVICE round 3)
        check_overflow();
        prepare_next_call();
        if (lazyOn_)
        {   // (behind prepare_next_call: it may have recorded the engine's first lists and knows whether every cell got one)
            choose_optimism();
            // The snapshot a later look may have to go back to.  A verified one that is still young is kept (going back a few steps further costs a little
            // more in the rare case, a 100 MB copy per call costs every caller that steps in short calls)
            if (!rollback_on()) snap_.valid = false;
            else if (!snap_.valid || stepsSinceSnap_ >= kSnapshotKeepSteps) take_snapshot();
        }
    }
    catch (const std::exception& e) { mark_failed(e.what()); throw; }
}

void Engine::step_body(int nsteps)
{
    // The sort interval is re-evaluated ("a look": a stream synchronisation and a few small read-backs, ~0.1 ms with the pipeline refill) at the end of every
    // call and, inside long calls, whenever lazyWindow_ steps have gone by since the last look - 8, 16, 32, ... then every 256 (a run that starts from rest speeds
    // up for a while: the looks are close together where that happens).  The count runs on across calls (sinceLook_), and a look is skipped when the call
    // ends within half a window anyway: a short call right behind a look - the driver's 20 steps after 5 of warm-up - pays for no look of its own.
    // (a call whose end was deferred - settle_now - and that nobody has looked at since: its second half-kick is still owed on the device, DevStats::pendingKick,
    //  and this call's first integrate kernel pays it exactly as it does between two steps of one call; its statistics were never asked for)
    kickOwed_ = false;
    if (!unsettled_)
    {
        choose_optimism();
        if (rollback_on() && !snap_.valid) take_snapshot();         // (the state as the caller left it: set_state / aztot_forces / the first call)
    }
    int left = nsteps;
    while (left > 0)
    {
        const int n = lazyOn_ ? std::min(left, std::max(1, lazyWindow_ - sinceLook_)) : left;
        run_steps(n);
        left -= n;
        sinceLook_ += n;
        stepsSinceSnap_ += n;
        if (left > 0 && sinceLook_ >= lazyWindow_)
        {
            if (2 * left > lazyWindow_)
            {
                look(false);
                choose_optimism();
                if (rollback_on()) take_snapshot();
            }
            else { run_steps(left); sinceLook_ += left; stepsSinceSnap_ += left; left = 0; }      // the end of the call, at most half a window away, is the look
        }
    }
    kickOwed_ = lazyKick_;          // set here, not in launch_step_kernels: a replayed graph does not pass through the host code
    check_launch("step kernels");
    unsettled_ = true;
    if (settle_now()) settle();
}

// steps per graph: one sort interval; with the cells rebuilt every step the sort ping-pongs the buffers, so it takes two steps to come back
int Engine::graph_cycle() const
{
    const int K = lazyOn_ ? lazyK_ : 1;
    return (K == 1) ? 2 : K;
}

bool Engine::can_graph() const
{
    // slab ranks: only with the loopback transport and only on request (DBG_SLAB_GRAPH) - an experiment, see DESIGN.md section 6.  Only cycles of steps
    // that all rebuild the cells (options.sort_every = 1): a plain step's coordinate exchange takes its ranges from the host's copy of the halo block
    // (take_halo_info waits for the read-back the sort posted, adopt_halo_info checks it), which a capture can neither wait for nor bake in - the ranges
    // change with every sort.  On the lazy schedule the switch does nothing and the steps are launched one by one.
    const bool slabGraph = nranks_ > 1 && ownedXch_ && (debug_ & DBG_SLAB_GRAPH) && !(P_.nEq > 0 || P_.tstat == AZTOT_TSTAT_NOSE) && !lazyOn_;
    // Replaying captured cycles pays where a step is a handful of microsecond kernels.  On 1 M atoms the kernels are long enough for plain asynchronous
    // launches to keep the GPU busy, and each hipGraphLaunch costs a 40 us bubble in front of its first kernel (rocprofv3 kernel trace): 0.1594 ms/step
    // replayed, 0.1575 launched one by one; 40 000 atoms: 0.0184 replayed, 0.0187 one by one.  (DBG_GRAPH_ALWAYS: replay whatever the size.)
    const bool worthIt = capacity_ <= 2 * kFuseKickMaxAtoms || (debug_ & DBG_GRAPH_ALWAYS);
    return opt_.use_graph && worthIt && (nranks_ == 1 || slabGraph) && !profile_ && !equil_phase();
}

// the graph of one cycle of steps for the buffer state the engine is in (captured on first use; the capture executes nothing).  One graph per buffer
// state because kernel arguments are baked in at capture time; a graph starts with a step that sorts
Engine::GraphSlot* Engine::graph_for_state(int cycle)
{
    if (graphCycle_ != cycle) { drop_graphs(); graphCycle_ = cycle; }
    const BufState now = buf_state();
    for (GraphSlot& g : graphs_)
        if (g.before.cur == now.cur && g.before.xyz[0][0] == now.xyz[0][0] && g.before.xyz[1][0] == now.xyz[1][0]) return &g;
    GraphSlot g;
    g.before = now;
    const int sinceBefore = sinceSort_;
    const LaunchNotes notesBefore = notes_;      // (the capture executes nothing: what the host knows about the last EXECUTED step must survive it)
    const int entryBytesBefore = lists_.entryBytes;       // (... the format of the lists on the device too: the captured rebuild step may record another)
    HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    capturing_ = true;
    try
    {
        sinceSort_ = kNoSort;
        left_ = StepPlan::LEFT_UNTOUCHED;
        for (int k = 0; k < cycle; k++) launch_step_kernels(cycle - 1 - k);
    }
    catch (...)
    {   // leave neither the stream in capture mode nor the engine believing it is capturing
        hipGraph_t broken = nullptr;
        (void)hipStreamEndCapture(stream_, &broken);
        if (broken) (void)hipGraphDestroy(broken);
        capturing_ = false;
        left_ = StepPlan::LEFT_UNTOUCHED;
        sinceSort_ = sinceBefore;
        lists_.entryBytes = entryBytesBefore;
        set_buf_state(now);
        adopt_launch_notes(notesBefore);
        throw;
    }
    capturing_ = false;
    HIP_CHECK(hipStreamEndCapture(stream_, &g.graph));
    HIP_CHECK(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    g.after = buf_state();
    g.notes = notes_;         // ... of the cycle's last step
    g.entryBytes = lists_.entryBytes;
    lists_.entryBytes = entryBytesBefore;
    set_buf_state(now);               // the capture itself executed nothing
    adopt_launch_notes(notesBefore);
    sinceSort_ = sinceBefore;
    graphs_.push_back(g);
    return &graphs_.back();
}

void Engine::run_steps(int nsteps)
{
    int done = 0;
    // Lazy re-sort (one GPU): the reference rebuilds its cell list every step (main.cu:300-326); here a step re-sorts only every lazyK_-th time.  That is
    // exact as long as no atom is farther than (stencil reach - rc) / 2 from where it was when the cells were built: every pair inside rc is then still
    // found in the stencil of the cell the atoms were sorted into.  Plain steps leave slots, cells and buffers alone, keep coordinates unwrapped, count
    // wall crossings when they happen, and check every atom's displacement; should one ever leave the slack (the interval is sized with a factor 1.15 to
    // spare from the largest step seen), the pair kernels reach one cell further until the next sort - slower, still exact.  The first step of
    // every call sorts (the deferred half-kick is re-armed by the scan).
    // With pair lists a sort interval runs on from the previous call when nothing has touched the state since (the lists are those of the arrays as they
    // stand; slab ranks: when all ranks agreed at the end of the previous call that they can - a rebuild step carries the full exchange, so they must
    // take it together); the plain steps that finish it are launched one by one, whole cycles are replayed as graphs after that.
    const bool carryOn = walks_lists() && (nranks_ == 1 || carryAgreed_) && listsValid_ && sinceSort_ < kNoSort / 2;
    if (!carryOn) sinceSort_ = kNoSort;
    left_ = StepPlan::LEFT_UNTOUCHED;
    while (carryOn && done < nsteps && sinceSort_ < lazyK_ - 1) { launch_step_kernels(nsteps - 1 - done); done++; }
    const int cycle = graph_cycle();
    if (can_graph() && nsteps - done >= cycle)
    {
        sinceSort_ = kNoSort;
        while (nsteps - done >= cycle)
        {
            GraphSlot* slot = graph_for_state(cycle);
            HIP_CHECK(hipGraphLaunch(slot->exec, stream_));
            done += cycle;
            hostStep_ += cycle;
            rebuilds_ += (lazyOn_ && lazyK_ > 1) ? 1 : cycle;       // (a captured cycle: one sort interval, or two every-step steps)
            set_buf_state(slot->after);           // one sort per cycle (K > 1) and the coordinate-array swaps of the fused steps
            adopt_launch_notes(slot->notes);      // where the cycle's last step left its partial sums
            lists_.entryBytes = slot->entryBytes; // the format its rebuild step recorded
            sinceSort_ = kNoSort;                 // the next cycle (or the eager remainder) starts with a sort
        }
    }
    left_ = StepPlan::LEFT_UNTOUCHED;
    for (; done < nsteps; done++) launch_step_kernels(nsteps - 1 - done);
}

// At the end of a call: what the next call will need and this one can provide without executing a step.  (1) The graph of a whole cycle for the buffer
// state the engine is in (capturing executes nothing).  (2) If the cells were rebuilt by the last step but no lists were recorded (the interval was 1
// until now: the engine had not measured the atoms' speed yet), the lists of the arrays as they stand - so that the next call opens with plain steps
// instead of rebuilding the same cells again.
void Engine::prepare_next_call()
{
    if (!lazyOn_ || !lazyMeasured_) return;
    if (walks_lists() && !listsValid_ && sinceSort_ == 0)
    {
        P_.cycleStep = 0;
        int32_t rep[LR_COUNT];
        auto record = [&] {
            HIP_CHECK(hipMemsetAsync(&lists_.report[LR_UNLISTED_NOW], 0, sizeof(int32_t), stream_));
            lists_.begin_recording();
            launch_build_lists(pair_launch(P_), PairRange(), lists_.pair_lists());
            check_launch("list building");
            sync();
            HIP_CHECK(hipMemcpy(rep, lists_.report, sizeof(rep), hipMemcpyDeviceToHost));
            unlistedState_ = (rep[LR_UNLISTED_NOW] == 0) ? 1 : 2;
        };
        record();
        // the first lists of an engine's life: size the LDS tiles from what the cells really hold right away (adapt_sort_interval does the same at
        // every look) - the next call then walks them at full occupancy - and choose the entry format from it: where one byte per entry will do, the
        // lists are recorded once more, in that format (the cells are as they were: no rebuild, nothing a caller can see)
        bool formatChanged = false;
        if (!(debug_ & DBG_SHORT_LISTS) && lists_.tighten(rep, &formatChanged)) drop_graphs();
        if (formatChanged) record();
        if (nranks_ > 1)
        {   // the plain steps' coordinate exchange needs to know where the boundary layers sit; with interval 1 nobody had asked (k_rank_gather left it ready)
            int32_t h[HI_COUNT];
            post_count_exchange();
            HIP_CHECK(hipStreamSynchronize(stream_));
            HIP_CHECK(hipMemcpy(h, dHaloInfo_, sizeof(h), hipMemcpyDeviceToHost));
            haloInfoPending_ = false;
            adopt_halo_info(h);
        }
        listsValid_ = true;
    }
    if (nranks_ > 1)
    {   // can every rank open the next call with plain steps?
        double cannot = (walks_lists() && listsValid_) ? 0.0 : 1.0;
        xch_->allreduce_sum(&cannot, 1, stream_);
        carryAgreed_ = cannot == 0.0;
    }
    if (can_graph()) (void)graph_for_state(graph_cycle());
}

// the largest step any atom made since the last look sizes the next calls' sort interval: K steps of that length use at most slack / 1.15 (Engine::lazyMargin_)
// (one GPU; a violation is handled exactly by the clean-up launch at the staging kernel's speed, so the margin is a performance choice: with half the
// slack C4 ran at K = 16, with two thirds at K = 24-28, no violation in 2 000 steps; every violation widens the margin for good - a system that heats up,
// like the Born-Mayer-Huggins melt B3, would otherwise run into one after the other) - half on slab ranks, whose repair (a window of steps run again) is dearer.
// Returns false when the slab ranks have found a violation: the caller takes every rank back to its snapshot
// A look needs the device's Counts and the list builder's report.  Two blocking copies behind a stream synchronisation were three round trips between host
// and device (~40 us of a short aztot_step call); queued into pinned memory BEFORE the synchronisation they ride on it (a small kernel writing the pinned block directly: measured, the same).
void Engine::look_sync()
{
    if (lazyOn_)
    {
        static_assert(sizeof(Counts) + sizeof(int32_t) * LR_COUNT <= PinnedReadback::kBytes, "the look's block holds Counts and the builder's report");
        hLook_.post(dCounts_, sizeof(Counts), stream_);
        if (lists_.on) hLook_.post(lists_.report, sizeof(int32_t) * LR_COUNT, stream_, sizeof(Counts));
    }
    sync();
}

// (called right behind look_sync: reads what it left in pinned memory)
bool Engine::adapt_sort_interval()
{
    Counts c = *hLook_.as<Counts>();
    bool rebuildNeeded = false;                    // this rank's lists were re-allocated: the next step must rebuild (on every rank: rebuild steps carry the full exchange)
    const int32_t* rep = hLook_.as<int32_t>(sizeof(Counts));
    if (lists_.on && rep[LR_RECORDED] > 0)
    {   // (nothing recorded since the last look: what that look found still stands)
        unlistedAtLook_ = rep[LR_UNLISTED] > 0;
        const ListStore::Verdict v = lists_.adapt(rep, debug_);
        if (v.launchChanged) drop_graphs();
        if (!lists_.on) listsValid_ = false;
        rebuildNeeded = v.rebuild;
    }
    if (nranks_ > 1)
    {   // every rank must arrive at the same interval (sort steps carry the full exchange) and at the same verdict: one slot per rank + the flags
        double v[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        v[10] = rebuildNeeded ? 1.0 : 0.0;
        double mine;
        std::memcpy(&mine, &c.maxStep2, sizeof(mine));
        if (nranks_ <= 8) v[rank_] = mine; else v[0] = 0.0;
        v[8] = c.lazyViolatedEver ? 1.0 : 0.0;
        v[9] = nranks_ > 8 ? mine : 0.0;              // more than 8 ranks: sum of squares bounds the maximum from above (conservative)
        xch_->allreduce_sum(v, 11, stream_);
        rebuildNeeded = v[10] > 0.0;
        double mx = v[9];
        for (int k = 0; k < 8; k++) mx = std::max(mx, v[k]);
        std::memcpy(&c.maxStep2, &mx, sizeof(mx));
        c.lazyViolatedEver = v[8] > 0.0 ? 1 : 0;
        if (c.lazyViolatedEver)
        {
            clear_violation_flag();
            set_interval(1);
            void_measurement();
            lazyMargin_ = std::min(4.0, lazyMargin_ * (4.0 / 3.0));
            if (rebuildNeeded) forget_interval();
            return false;             // every rank goes back to its snapshot (Engine::step)
        }
    }
    HIP_CHECK(hipMemsetAsync(&dCounts_->maxStep2, 0, sizeof(unsigned long long), stream_));      // (in stream order: no second round trip for the look)
    if (rebuildNeeded) forget_interval();
    lazyMeasured_ = true;
    int K = lazyK_;
    // one GPU without the clean-up launch: a violation, or a cell that kept no list, means the steps since the last look were not exact
    const bool goBack = optimistic_ && (c.lazyViolatedEver != 0 || unlistedAtLook_);
    if (debug_ & DBG_FIXED_INTERVAL)
    {   // debug: fixed interval whatever the speeds (exercises the wider-stencil fallback); violations are only counted
        if (c.lazyViolatedEver) clear_violation_flag();
        K = lazyCap_;
    }
    else
    {
        const bool violated = c.lazyViolatedEver != 0;
        if (violated)
        {
            clear_violation_flag();
            lazyMargin_ = std::min(4.0, lazyMargin_ * (4.0 / 3.0));      // the speeds are growing: more room from now on (1.15 -> 1.5 -> 2.0 -> 2.7 -> 3.6 -> 4)
        }
        int fromSpeed = -1;
        if (c.maxStep2 != 0)
        {
            double ms2;
            std::memcpy(&ms2, &c.maxStep2, sizeof(ms2));
            const double len = std::sqrt(ms2);
            // (slab ranks repair a violation by running up to a window of steps again with the cells rebuilt every step - dearer than the wider stencil one GPU
            //  falls back on - so they keep a factor 2 in hand at least; round 2 kept 4 and could only report the violation)
            // ... and where the speeds are still growing (a lattice released from rest, a melt heating up: the longest step of this window against the last
            // one's) the margin grows by the same factor, at most 2: the steps ahead will be longer than the ones just seen.  (With the plain margin of 1.15
            // C3 - charges on a lattice at rest - ran into a violation in its first hundred steps; a first look has nothing to compare with and takes 1.3.)
            // (a ratio below 1.1 is the noise of a maximum over a few thousand atom-steps, not a trend)
            const double growth = lastLookLen_ > 0.0 ? (len > 1.1 * lastLookLen_ ? std::min(2.0, len / lastLookLen_) : 1.0) : 1.3 / 1.15;
            lastLookLen_ = len;
            const double raw = len > 0 ? lazySlack_ / ((nranks_ > 1 ? std::max(2.0, lazyMargin_) : lazyMargin_) * growth * len) : 1e9;
            if (std::getenv("AZTOT_VERBOSE"))
                std::fprintf(stderr, "aztot: longest step %.3e A, slack %.3e A, margin %.2f%s: interval up to %.1f steps\n", len, lazySlack_, lazyMargin_, violated ? ", violated" : "", raw);
            static const int allowed[] = {128, 112, 96, 80, 64, 56, 48, 40, 36, 32, 28, 24, 20, 16, 14, 12, 10, 8, 6, 5, 4, 3, 2, 1};
            fromSpeed = 1;
            // (engines that replay whole cycles as graphs stop at 64: what is left of a call behind its last whole cycle is launched kernel by kernel -
            //  C2 with 2 000-step calls: 0.0122 ms/step at K = 64, 0.0129 at 112)
            const int cap = can_graph() ? std::min(lazyCap_, 64) : lazyCap_;
            for (int a : allowed) if (a <= cap && (double)a <= raw) { fromSpeed = a; break; }
            // (the table keeps the number of different cycle lengths - captured graphs - small; where cycles are launched kernel by kernel any whole number will do:
            //  a thermalised 1 M-atom liquid sits between 14 and 16 and gets 15)
            if (!can_graph() && raw >= 1.0) fromSpeed = std::max(fromSpeed, std::min(cap, (int)raw));
        }
        // after a violation: half the interval, or what the speeds seen now allow if that is less (a melt that heats up outruns halving)
        if (violated) K = std::max(1, fromSpeed > 0 ? std::min(K / 2, fromSpeed) : K / 2);
        else if (fromSpeed > 0) K = fromSpeed;
    }
    set_interval(K);
    return !goBack;
}

// a violation the host has seen and counted: Counts::lazyViolatedEver is sticky on the device until cleared here (a blocking copy: looks are rare)
void Engine::clear_violation_flag()
{
    const int32_t z = 0;
    HIP_CHECK(hipMemcpy(&dCounts_->lazyViolatedEver, &z, sizeof(z), hipMemcpyHostToDevice));
    lazyViolations_++;
}

void Engine::check_overflow()
{
    if (nranks_ <= 1 && !hasBonded_) return;
    Counts c;
    HIP_CHECK(hipMemcpy(&c, dCounts_, sizeof(Counts), hipMemcpyDeviceToHost));
    if (c.overflow) throw std::runtime_error("slab decomposition: a fixed-capacity halo/migration/atom buffer overflowed");
    if (c.bondedMissing)
        throw std::runtime_error("slab decomposition: a bond / angle partner was not resident on the rank that owns the atom "
                                 "(bonded terms must span less than the halo width)");
}

void Engine::get_stats(aztot_stats& out)
{
    const DevStats s = read_stats();
    // (the host decides from its own count of the steps which of them the equilibration schedule acts on: the two counts must never part)
    if (failed_.empty() && s.step != hostStep_) throw std::runtime_error("the host's step count (" + std::to_string(hostStep_) + ") and the device's (" + std::to_string(s.step) + ") differ");
    double v[24];
    v[0] = s.engKin; v[1] = s.engVdW; v[2] = s.engCoul; v[3] = s.engElecField; v[4] = s.engTemp;
    for (int k = 0; k < 6; k++) { v[5 + k] = s.mom[k]; v[11 + k] = (double)s.cross[k]; }
    v[17] = (double)s.dropped; v[18] = s.engBond; v[19] = s.engAngle;
    if (nranks_ > 1) xch_->allreduce_sum(v, 20, stream_);
    std::memset(&out, 0, sizeof(out));
    out.step = s.step;
    out.time = s.step * model_.tSt;
    out.engKin = v[0]; out.engVdW = v[1]; out.engCoul = v[2]; out.engElecField = v[3]; out.engTemp = v[4];
    out.engPot = out.engCoul + out.engVdW;
    out.engBond = v[18]; out.engAngle = v[19];
    out.engCoulRec = s.engCoulRec; out.engCoulConst = s.engCoulConst;      // global quantities: identical on every rank
    out.engTot = out.engElecField + out.engVdW + (out.engCoulConst + out.engCoulRec + out.engCoul) + out.engKin + out.engBond +
                 out.engAngle;                                             // calc_chars integrators.cpp:70-71
    out.temperature = 2.0 * out.engKin * model_.revDegFree * (1.0 / units::kB);     // integrators.cpp:67
    out.negMom[0] = v[5]; out.posMom[0] = v[6]; out.negMom[1] = v[7]; out.posMom[1] = v[8]; out.negMom[2] = v[9]; out.posMom[2] = v[10];
    out.negCross[0] = (int64_t)v[11]; out.posCross[0] = (int64_t)v[12]; out.negCross[1] = (int64_t)v[13];
    out.posCross[1] = (int64_t)v[14]; out.negCross[2] = (int64_t)v[15]; out.posCross[2] = (int64_t)v[16];
    out.pairs_dropped = (int64_t)v[17];
    out.n_cells = (int64_t)P_.nc[0] * P_.nc[1] * P_.nc[2];
    out.nose_chit = s.chit; out.nose_conint = s.conint;
    out.sort_interval = lazyOn_ ? lazyK_ : 1; out.sort_violations = lazyViolations_;
    out.pair_lists = (lists_.on && lazyOn_ && lazyK_ > 1) ? 1 : 0;
    out.rebuilds = rebuilds_;
    out.skin = 2.0 * lazySlack_;
    out.cells_without_list = 0;
    if (lists_.on)
    {
        int32_t nl = 0;
        HIP_CHECK(hipMemcpy(&nl, &lists_.report[LR_UNLISTED_NOW], sizeof(nl), hipMemcpyDeviceToHost));
        out.cells_without_list = nl;
    }
    // pressure from the wall momentum over the window since the previous evaluation (main.cpp:143-163)
    if (s.step - lastPresStep_ >= std::max(1, model_.stat))
    {
        const double dtw = (s.step - lastPresStep_) * model_.tSt;
        const double revS[6] = {1.0 / (model_.L[1] * model_.L[2]), 1.0 / (model_.L[1] * model_.L[2]), 1.0 / (model_.L[0] * model_.L[2]),
                                1.0 / (model_.L[0] * model_.L[2]), 1.0 / (model_.L[0] * model_.L[1]), 1.0 / (model_.L[0] * model_.L[1])};
        double p = 0.0;
        for (int k = 0; k < 6; k++) { p += 2.0 * units::pressure_factor * revS[k] * (v[5 + k] - lastMom_[k]) / dtw; lastMom_[k] = v[5 + k]; }
        pressure_ = p / 6.0;
        lastPresStep_ = s.step;
    }
    out.pressure = pressure_;
}

void Engine::species_crossings(int64_t* out, int cap)
{
    const int n = 6 * model_.nSpec();
    if (cap < n) throw std::runtime_error("species_crossings: output array too small");
    const DevStats s = read_stats();
    double v[kSpecCap * 6];
    for (int k = 0; k < n; k++) v[k] = (double)s.specCross[k];
    if (nranks_ > 1) xch_->allreduce_sum(v, n, stream_);
    for (int k = 0; k < n; k++) out[k] = (int64_t)(v[k] + 0.5);
}

// md_to_host (cuInit.cu:1212-1262).  The reference returns the arrays in cell-sorted order (SURVEY C-20);
// we put every atom back at its original index.  On several ranks each rank fills only the atoms it owns.
void Engine::md_to_host(aztot_state& out)
{
    const Counts c = read_counts();
    const int n = c.ownedEnd - c.ownedBegin;
    if (out.n_atoms < model_.nAt) throw std::runtime_error("md_to_host: output arrays too small");
    std::vector<int32_t> ids(std::max(n, 1));
    HIP_CHECK(hipMemcpy(ids.data(), cur().id + c.ownedBegin, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    std::vector<double> tmp(std::max(n, 1));
    auto down = [&](double* dst, const double* src) {
        if (!dst) return;
        HIP_CHECK(hipMemcpy(tmp.data(), src + c.ownedBegin, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        for (int k = 0; k < n; k++) dst[ids[k]] = tmp[k];
    };
    AtomArrays& A = cur();
    down(out.x, A.x); down(out.y, A.y); down(out.z, A.z); down(out.vx, A.vx); down(out.vy, A.vy); down(out.vz, A.vz);
    if (lazyOn_)
    {   // between two sorts of a lazy run coordinates are kept unwrapped on the device: hand out what put_periodic would have left (box.cpp:230-295)
        auto wrap = [](double x, double L) {
            const double invL = 1.0 / L;
            if (x < 0) x += ((int)(-x * invL) + 1) * L;
            else if (x > L) x -= ((int)(x * invL)) * L;
            return (x >= L) ? 0.0 : x;
        };
        double* arr[3] = {out.x, out.y, out.z};
        for (int k = 0; k < 3; k++)
            if (arr[k])
                for (int q = 0; q < n; q++) arr[k][ids[q]] = wrap(arr[k][ids[q]], model_.L[k]);
    }
    down(out.fx, A.fx); down(out.fy, A.fy); down(out.fz, A.fz); down(out.U, A.U); down(out.radius, A.rad);
    if (out.types)
    {
        std::vector<int32_t> ty(std::max(n, 1));
        HIP_CHECK(hipMemcpy(ty.data(), A.type + c.ownedBegin, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        for (int k = 0; k < n; k++) out.types[ids[k]] = ty[k];
    }
    out.n_atoms = n;   // number of atoms this rank wrote
}

// restart support: step number + thermostat scalars (see aztot_clock)
void Engine::get_clock(aztot_clock& out)
{
    const DevStats s = read_stats();
    out.step = s.step; out.nose_chit = s.chit; out.nose_conint = s.conint; out.eng_kin = s.ekSim;
}

void Engine::set_clock(const aztot_clock& in)
{
    DevStats s = read_stats();
    snap_.valid = false;
    s.step = in.step; s.stepAtSort = in.step; s.chit = in.nose_chit; s.conint = in.nose_conint; s.ekSim = in.eng_kin; s.engKin = in.eng_kin;
    s.pendingKick = 0;
    HIP_CHECK(hipMemcpy(dStats_, &s, sizeof(DevStats), hipMemcpyHostToDevice));
    lastPresStep_ = in.step;
    hostStep_ = in.step;
    forget_interval();
    drop_graphs();
}

// read-back of the sorted cell list (cudaMD::firstAtomInCell + the id of the atom in every slot)
int Engine::cell_table(int32_t dims[3], int32_t* cellStart, int capCells, int32_t* atomId, int capAtoms)
{
    sync_all();
    dims[0] = P_.ncxLocal; dims[1] = P_.nc[1]; dims[2] = P_.nc[2];
    const int nCell = P_.nCellLocal;
    if (cellStart)
    {
        if (capCells < nCell + 1) throw std::runtime_error("cell_table: cell_start needs n_cells + 1 entries");
        HIP_CHECK(hipMemcpy(cellStart, dCellStart_, sizeof(int32_t) * (size_t)(nCell + 1), hipMemcpyDeviceToHost));
    }
    if (atomId)
    {
        Counts c;
        HIP_CHECK(hipMemcpy(&c, dCounts_, sizeof(Counts), hipMemcpyDeviceToHost));
        if (capAtoms < c.nTotal) throw std::runtime_error("cell_table: atom_id array too small");
        HIP_CHECK(hipMemcpy(atomId, cur().id, sizeof(int32_t) * (size_t)c.nTotal, hipMemcpyDeviceToHost));
    }
    return nCell;
}

// overwrite per-atom state (indexed by ORIGINAL atom id); used for exact restarts and stage-wise tests
void Engine::set_state(const aztot_state& in)
{
    if (!failed_.empty()) throw std::runtime_error("this handle failed in an earlier call: " + failed_);
    const Counts c = read_counts();
    snap_.valid = false;
    forget_interval();
    if (in.vx || in.vy || in.vz || in.fx || in.fy || in.fz)
    {   // new velocities / forces: the interval measured on the old ones says nothing about them - every step rebuilds until the first look
        if (!(debug_ & DBG_FIXED_INTERVAL)) set_interval(1);
        void_measurement();
        lastLookLen_ = 0.0;
    }
    const int n = c.ownedEnd - c.ownedBegin;
    std::vector<int32_t> ids(std::max(n, 1));
    HIP_CHECK(hipMemcpy(ids.data(), cur().id + c.ownedBegin, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    std::vector<double> tmp(std::max(n, 1));
    auto up = [&](const double* src, double* dst) {
        if (!src) return;
        for (int k = 0; k < n; k++) tmp[k] = src[ids[k]];
        HIP_CHECK(hipMemcpy(dst + c.ownedBegin, tmp.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    };
    AtomArrays& A = cur();
    up(in.x, A.x); up(in.y, A.y); up(in.z, A.z); up(in.vx, A.vx); up(in.vy, A.vy); up(in.vz, A.vz);
    up(in.fx, A.fx); up(in.fy, A.fy); up(in.fz, A.fz); up(in.U, A.U); up(in.radius, A.rad);
    if ((in.U || in.radius) && !thermoTouched_)
    {   // from now on the sort carries the per-atom thermostat state along; a captured graph has the old carry mode baked in
        thermoTouched_ = true;
        drop_graphs();
    }
}

}  // namespace aztot

#include "samplers.hip.h"
