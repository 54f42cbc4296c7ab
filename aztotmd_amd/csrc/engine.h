// Step driver + device management of one rank: the MI355X-native counterpart of the reference's
// init_cudaMD / md_to_host / free_device_md (cuInit.cu:756-1374) and of the loop body of
// main.cu:281-410.  One HIP stream, no host synchronisation inside a step (the reference blocks on
// cudaThreadSynchronize 11 times per step, main.cu:290-383), optional hipGraph replay.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_md.h"
#include "device_resources.h"
#include "list_store.h"
#include "model.h"
#include "msg_layout.h"
#include "samplers.h"
#include "step_plan.h"

namespace aztot {

struct Counts;
struct PairLists; struct PairLaunch;

// a caller error that the C ABI reports as AZTOT_ERR_ARG (capi.cpp: guarded)
struct ArgError : std::runtime_error
{
    using std::runtime_error::runtime_error;
};

}  // namespace aztot
#include "exchange.h"
namespace aztot {

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// The host state machine in one table, grouped as the members are below.  API calls that touch state first complete a
// deferred call end (Engine::settle).  Transitions with a name: forget_interval() (the next step rebuilds the cells), void_measurement() (looks start
// over at 8 steps), set_interval(K), drop_graphs() (captured cycles are stale).  Memory, pinned blocks and the pair-list store say what they own in
// device_resources.h / list_store.h.
//
//  member            meaning                                              set by                                      cleared / reset by                         invalidated by (API)
//  ----------------  ---------------------------------------------------  ------------------------------------------  -----------------------------------------  ---------------------------------------
//  unsettled_        the last aztot_step returned before its end           step_body (every call)                      settle (at once when settle_now(), else     every read / write entry point settles
//                    (deferred kick, statistics, look) had happened                                                    by the next reader or the next due look)    first; mark_failed drops it
//  hostStep_         steps launched so far (== DevStats::step when the     launch_step_kernels (+1), run_steps (graph  replay_from_snapshot (snapshot's),          aztot_set_clock; mark_failed re-reads it
//                    stream has drained)                                   replay: + cycle)                            set_clock                                  from the device
// -- pair lists ---
//  lists_            the store (list_store.h); lists_.on, the LDS sizes    ListStore::create / regrow / adapt,         ListStore::release, adapt (most unlisted    - (baked into graphs: drop_graphs)
//                    and waves per cell are launch parameters              tighten                                     cells can never be listed)
//  listsValid_       the lists on the device are those of the arrays as    launch_pair (build), prepare_next_call      forget_interval; sort_and_forces until      as sinceSort_
//                    they stand (a call may open with plain steps)                                                     launch_pair has recorded the new ones
//  unlistedState_    cells without a list in the lists in force: 0 ?,      launch_pair (slab: read back behind the     launch_pair at every build (-> 0), replay    -
//                    1 none, 2 some                                        build), prepare_next_call
//  unlistedAtLook_   the last look found cells recorded without a list     adapt_sort_interval                         the next look that saw a recording          -
// -- sort interval ---
//  lazyK_            sort interval in force (1: every step)                set_interval: adapt_sort_interval (from the -> 1: set_state with new v / f, a slab      aztot_set_state (v, f); aztot_forces keeps it
//                                                                          longest step seen); constructor (debug)     violation (replay), never above lazyCap_
//  lazyMeasured_     lazyK_ comes from a measurement                       adapt_sort_interval                         void_measurement: set_state (v, f), slab    aztot_set_state (v, f)
//                                                                                                                      violation
//  lazyWindow_       steps between two looks: 8, 16 ... 256 (64 on slabs)  look (doubling)                             -> 8: void_measurement                      aztot_set_state (v, f)
//  sinceLook_        steps since the last look (runs on across calls)      step_body (+ n)                             every look (-> 0); void_measurement         aztot_set_state (v, f)
//  sinceSort_        plain steps since the last rebuild (kNoSort: none)    sort_and_forces (0 at a rebuild, +1 plain)  forget_interval                             aztot_forces, aztot_set_state, aztot_set_clock,
//                                                                                                                                                                  replay, list re-allocation, run_steps without carryOn
//  carryAgreed_      slab ranks: all agreed the next call may open with    prepare_next_call (all-reduce)              forget_interval                             as sinceSort_
//                    plain steps
//  haloInfoPending_  slab: the boundary ranges of the last sort are still  sort_and_forces                             take_halo_info, prepare_next_call, replay   -
//                    on their way to pinned memory
// -- graphs ---
//  graphs_, graphCycle_  captured cycles, valid for one buffer state and   graph_for_state                             drop_graphs: any change of lazyK_,          aztot_set_clock, aztot_set_state (U / radius
//                    one set of launch parameters                                                                       optimistic_, the list store's launch        first touched), replay
//                                                                                                                      parameters, thermoTouched_
// -- snapshot and optimism ---
//  optimistic_       plain steps run without the clean-up launch           choose_optimism (start of a settled call,   choose_optimism; replay_from_snapshot       - (P_.optimistic is baked into graphs)
//                    (P_.optimistic)                                       after every look)
//  safeLooks_        looks still to spend with the clean-up launch         constructor (1), replay (4 << rollbacks_)   every look (- 1)                            -
//  snap_.valid       a verified snapshot of the dynamic state exists       take_snapshot (start of a settled call,     choose_optimism (not optimistic any more),  aztot_forces, aztot_set_state, aztot_set_clock,
//                                                                          every clean look; kept when younger than    settle (no roll-back mode)                  mark_failed
//                                                                          kSnapshotKeepSteps)
// -- across a step boundary ---
//  kickOwed_         the last step's second half-kick has not been         step_body (= lazyKick_ at the end of a      finish_steps (k_integrate2); start of the   -
//                    applied and settle must apply it                      call), look at the end of a call (replay)   next step_body (the device flag
//                                                                                                                      DevStats::pendingKick makes the next
//                                                                                                                      integrate kernel pay it)
//  left_             how the previous step left the one being launched     launch_step_kernels (StepPlan::leaves: a    run_steps, graph capture, replay            - (a kicked step is always followed by a plain
//                    (StepPlan::Left): untouched, opened, or kicked        pair launch that opened or kicked the       (-> untouched)                              step of the same run_steps: no entry point,
//                    (v stored and no f: NOT the canonical state)          next step, k_boundary_radi)                                                             look, snapshot or rebuild ever sees it)
// ---------------------------------------------------------------------------------------------------------------------------------------------------
class Engine final : private Samplers::Host
{
public:
    Engine(const Model& model, const aztot_options& opt, int rank, int nranks, Exchanger* xch);
    ~Engine();
    Engine(const Engine&) = delete;

    void step(int nsteps);
    void forces(bool withBonded = true);    // sort + pair forces (+ bonds / angles) on the current positions
    void get_stats(aztot_stats& out);
    void species_crossings(int64_t* out, int cap);
    void md_to_host(aztot_state& out);
    void set_state(const aztot_state& in);
    void get_clock(aztot_clock& out);
    void set_clock(const aztot_clock& in);
    int cell_table(int32_t dims[3], int32_t* cellStart, int capCells, int32_t* atomId, int capAtoms);
    int kernel_times(std::vector<KernelTimer>& out);
    void reset_kernel_times();
    void set_profile(bool on) { sync_all(); profile_ = on; }
    int n_atoms_global() const { return model_.nAt; }
    int comm_ranks() const { return xch_ ? xch_->comm_ranks() : 0; }
    void sync_all();                        // everything queued or deferred by earlier calls has happened when this returns (aztot_sync)
    // debug read-back of the SPME meshes of the last force evaluation (aztot_spme_mesh / aztot_spme_influence); cap and result count 8-byte words
    long long spme_mesh(int which, void* out, long long cap);
    long long spme_influence(double* out, long long cap);    Samplers& samplers() { return *samplers_; }     // RDF, coordination numbers, time correlation functions: they see the engine as a Samplers::Host

private:
    void step_body(int nsteps);
    bool settle_now() const;
    void settle();
    void mark_failed(const char* what) noexcept;
    bool unsettled_ = false;                // the last aztot_step call returned with its end (deferred kick, statistics, look) still to come: Engine::settle
    std::string failed_;                    // first error of a step / settle: the handle no longer steps, reads still work
    void construct();
    void release();
    void check_launch(const char* where);
    void choose_cells();
    void allocate();
    void alloc_atoms(AtomArrays& A, bool zero);
    void upload_initial();
    void upload_bonded();
    void upload_ewald();
    void launch_ewald();
    void upload_spme();
    void launch_spme();
    void spme_stage(int upTo);      // spread [+ to_complex + forward transform [+ convolution + inverse transform]] on the arrays as they stand
    StepPlan plan_step(int stepsLeft) const;        // stepsLeft: steps that follow the one being launched before the host looks / the cycle ends
    StepPlan plan_forces(bool withBonded) const;    // aztot_forces: bin + sort + forces on the positions as they stand
    void sort_and_forces(const StepPlan& plan);
    void launch_step_kernels(int stepsLeft);
    void run_steps(int nsteps);
    void launch_pair(const StepPlan& plan);
    int pair_variant() const { return pairVariant_; }
    bool walks_lists() const { return lists_.on && lazyOn_ && lazyK_ > 1 && pairVariant_ == 2; }      // plain steps of this engine walk pair lists
    void exchange_halo();
    void collect_and_finalize(unsigned slotMask);
    void finish_steps();
    void check_overflow();
    void sync();
    DevStats read_stats();          // DevStats / Counts as a caller may see them: the deferred end of the last call has happened and the stream has drained
    Counts read_counts();
    template <typename F> void timed(const char* name, F&& launch) { if (!profile_ || capturing_) launch(); else timers_.timed(name, stream_, launch); }
    template <typename T> T* dev_alloc(size_t n, bool zero = false) { return mem_.alloc<T>(n, zero, stream_); }
    PairLaunch pair_launch(const StepParams& Q);    // what the pair launches of the step in flight share (Q: P_ as the launch sees it)
    AtomArrays& cur() { return buf_[cur_]; }
    AtomArrays& oth() { return buf_[cur_ ^ 1]; }
    int left() const { return (rank_ + nranks_ - 1) % nranks_; }       // x-neighbours on the ring of slab ranks
    int right() const { return (rank_ + 1) % nranks_; }
    // Samplers::Host
    void quiesce() override { sync_all(); }
    AtomArrays begin_sample() override;
    void end_sample(const char* where) override { check_launch(where); sync(); }
    void launch_timed(const char* name, const std::function<void()>& launch) override { timed(name, launch); }
    Samplers::PairTables pair_tables() override { return {P_, S_, dPots_, hostStep_}; }

    Model model_;
    aztot_options opt_;
    unsigned debug_ = 0;            // AZTOT_DEBUG (DebugBit)
    int pairVariant_ = 1;           // which pair kernel runs (construct)
    StepParams P_{};
    SpecTable S_{};
    int rank_, nranks_;
    Exchanger* xch_;
    std::unique_ptr<Exchanger> ownedXch_;

    hipStream_t stream_ = nullptr;
    hipStream_t commStream_ = nullptr;      // slab ranks, plain steps: the coordinate exchange runs here while the interior cells' pair forces run on stream_
    hipEvent_t evIntegrated_ = nullptr, evHalo_ = nullptr;
    DeviceArena mem_;               // every device buffer below except the pair lists' (ListStore); the samplers own theirs (samplers.h)
    bool profile_ = false;
    KernelTimers timers_;
    int capacity_ = 0;          // atoms that fit in the per-atom arrays (owned + ghosts + slack)
    int maxBlocks_ = 0;
    AtomArrays buf_[2]{};
    int cur_ = 0;
    DevPot* dPots_ = nullptr;
    int32_t *dCellOf_ = nullptr, *dSlotOf_ = nullptr, *dCellCount_ = nullptr, *dCellStart_ = nullptr;
    int32_t* dChunkTot_ = nullptr;
    int32_t *dTmpId_ = nullptr, *dTmpSrc_ = nullptr, *dTmpCell_ = nullptr, *dCellOfSorted_ = nullptr;
    double* dPartials_ = nullptr;
    DevStats* dStats_ = nullptr;
    Counts* dCounts_ = nullptr;
    double *dPhotons_ = nullptr, *dUvx_ = nullptr, *dUvy_ = nullptr, *dUvz_ = nullptr;
    double* dStage_ = nullptr;      // sub-totals of the two-level collect
    double* dEkGlobal_ = nullptr;   // kinetic energy over all ranks (equilibration scaling only)
    char* dMsg_[4] = {nullptr, nullptr, nullptr, nullptr};   // sendLeft, sendRight, fromLeft, fromRight
    MsgLayout lay_{};
    SplitArgs split_{};             // few cells, wide stencils: several waves per cell in the staging kernel (pair_tile.hip.h)
    BondedTables bonded_{};         // all-null when the model has no bonds / angles
    bool hasBonded_ = false;
    EwaldTables ew_{};              // reciprocal-space Ewald sum ('elec pme')
    bool hasEwald_ = false;
    SpmeTables spme_{};             // smooth particle-mesh Ewald ('elec spme'): meshes, influence function, twiddles
    SpmeAxis spmeAxis_[3]{};
    bool hasSpme_ = false;
    bool has_recip() const { return hasEwald_ || hasSpme_; }    // a reciprocal-space sum adds forces behind the pair kernel
    bool thermoTouched_ = false;    // the caller set U / radius on a run whose model does not use them: keep them attached to their atoms

    // -- pair lists of the lazy re-sort ---
    ListStore lists_;
    // a sort interval may run on from one aztot_step call into the next (one GPU, pair lists): the lists recorded at the last rebuild are those of the
    // arrays as they stand; set_state / aztot_forces end that
    bool listsValid_ = false;
    // slab ranks: how many cells the last list build left without a list, copied to pinned memory behind the build; once the copy has landed and says
    // "none", the clean-up launches of the interval are skipped (a slab rank cannot widen its stencil, so the clean-up launch has nothing else to do there)
    PinnedReadback hUnlisted_;
    int unlistedState_ = 0;         // 0 unknown (copy in flight or never made), 1 known to be zero, 2 known to be non-zero
    bool unlistedAtLook_ = false;   // the last look found cells recorded without a list

    // -- sort interval: lazy re-sort (one GPU): the cells are rebuilt only every lazyK_ steps; in between the atoms keep their slots, coordinates stay
    // unwrapped and every step checks that no atom has moved farther than lazySlack_ from where it was sorted (RefPos) - see Engine::run_steps ---
    static constexpr int kNoSort = 1 << 30;     // sinceSort_: no rebuild to count from (the next step rebuilds the cells)
    bool lazyOn_ = false;
    int lazyK_ = 1;                 // current sort interval (1: every step); adapted at every look from the largest step seen
    int lazyCap_ = 32;
    long long lazyViolations_ = 0;
    int lazyWindow_ = 8;               // steps between two looks at the speeds: 8, 16, ... 256
    int sinceLook_ = 0;                // steps since the last look (runs on across calls)
    double lazyMargin_ = 1.15;         // one GPU: K steps of the longest step seen may use slack / lazyMargin_ (1.3 until round 4: 20 000 steps of C4T and 10 000 of C3T run
                                       // without a violation at 1.05 too); widened by every violation (a system that heats up)
    bool lazyMeasured_ = false;     // the interval has been sized from a measurement at least once
    double lastLookLen_ = 0.0;      // the longest step of the window before the last look (0: none to compare with): growing speeds widen the margin
    int sinceSort_ = kNoSort;       // plain steps since the last sort
    long long rebuilds_ = 0;        // steps that rebuilt the cell list so far
    double lazySlack_ = 0.0;
    double skinTarget_ = 0.0;       // the skin the cells were sized for (0: none)
    RefPos ref_{};
    bool carryAgreed_ = false;      // slab ranks: every rank can carry the interval on (decided together at the end of the previous call)
    void forget_interval() { sinceSort_ = kNoSort; listsValid_ = false; carryAgreed_ = false; }     // the next step rebuilds the cells
    void void_measurement() { lazyMeasured_ = false; lazyWindow_ = 8; sinceLook_ = 0; }             // what the looks have learnt says nothing about the steps ahead
    void set_interval(int K) { if (K != lazyK_) { lazyK_ = K; drop_graphs(); } }
    void clear_violation_flag();
    int window_cap() const { return nranks_ > 1 ? 64 : 256; }       // (a slab rank repairs a skin violation by running the window again: it looks more often)
    void look_sync();               // what a look reads (Counts, the list builder's report) copied into pinned memory behind the queued work, then ONE stream synchronisation
    PinnedReadback hLook_;          // Counts followed by the builder's report (ListReport)
    bool adapt_sort_interval();
    void look(bool callEnd);
    void prepare_next_call();
    int halo_[5] = {0, 0, 0, 0, 0};  // slab ranks: ownedBegin, end of the left boundary layers, start of the right ones, ownedEnd, nTotal (after the last sort)
    // read back after every sort without stalling the stream: copied into pinned host memory behind the sort kernels, waited for only when the next plain
    // step needs the numbers (by then the list building and the pair kernel of the sort step are queued behind the copy)
    PinnedReadback hHalo_;           // the halo block (enum HaloInfo)
    int32_t* dHaloInfo_ = nullptr;   // the same on the device, written by k_rank_gather
    bool haloInfoPending_ = false;
    void take_halo_info();
    void post_count_exchange();
    void adopt_halo_info(const int32_t* h);

    // Equilibration rescaling (control.txt: nequil / eqfreq) acts on a handful of steps only - step numbers the host can tell (hostStep_ mirrors DevStats::step) -,
    // so only those steps take the path that sums the kinetic energy on the device, decides a factor and scales; every other step of a thermostat run takes the
    // short path of a run without equilibration (case study 2: 6 launches per step -> 2)
    long long hostStep_ = 0;        // steps launched so far (== DevStats::step once the stream has drained)
    bool equil_phase() const { return P_.nEq > 0 && hostStep_ < P_.nEq; }

    // statistics window for the wall-momentum pressure (main.cpp:143-163)
    double lastMom_[6] = {0, 0, 0, 0, 0, 0};
    double pressure_ = 0.0;
    long long lastPresStep_ = 0;

    std::unique_ptr<Samplers> samplers_;    // made once stream and box exist (construct); its arenas free their memory after release() has drained the streams

    // -- graphs: hipGraph replay of a cycle of steps.  Kernel arguments are baked in at capture time, so a graph is valid for the buffer state it was
    // captured in (which AtomArrays is current, which coordinate arrays each of them holds: the sort ping-pongs the buffers, the fused next-step epilogue
    // swaps coordinate arrays); it also remembers the state it leaves behind ---
    struct BufState { int cur; double* xyz[2][3]; double* alt[2][3]; };
    // ... and what the host notes down while it launches a step for whoever reduces the statistics afterwards (finish_steps): a replayed cycle does not pass
    // through that host code, so the slot carries the notes of its last step (found by the call-pattern fuzz of round 4: aztot_forces - whose staging launch
    // books into more partial-sum slots than the list kernel - followed by a call served entirely by replays summed stale slots into the energies)
    struct LaunchNotes
    {
        int pairBlocksUsed = 0;
        int blocksEver = 0;             // partial-sum entries any launch has booked into so far (what k_collect has to read of the accumulating rows)
        bool ekinFromPair = false;      // where the last step left its kinetic-energy partials
        bool lastStepEquil = false;     // the last step launched left its kinetic energy in DevStats::local (k_reduce_kin), not in the partial sums
    } notes_;                           // of the last step EXECUTED (launched one by one, or the last of a replayed cycle)
    // (entryBytes: the pair-list entry format the cycle's rebuild step records and its steps walk - ListStore::entryBytes once the graph has run)
    struct GraphSlot { BufState before, after; LaunchNotes notes; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; int entryBytes = 2; };
    void adopt_launch_notes(const LaunchNotes& n) { const int ever = std::max(notes_.blocksEver, n.blocksEver); notes_ = n; notes_.blocksEver = ever; }
    std::vector<GraphSlot> graphs_;
    int graphCycle_ = 0;            // steps held by the captured graphs
    bool capturing_ = false;
    // The captured graphs are stale (a launch parameter or a baked-in pointer changed).  graphCycle_ goes back to 0 with them: graph_for_state compares
    // it with the cycle it is asked for and, finding no graph either way, captures anew - so callers that used to leave it alone lose nothing
    void drop_graphs();
    BufState buf_state() const;
    GraphSlot* graph_for_state(int cycle);
    int graph_cycle() const;
    bool can_graph() const;
    void set_buf_state(const BufState& b);

    // -- what crosses a step boundary, and who applies the second half-kick (decided once, in the constructor) ---
    bool lazyKick_ = false;         // large plain-NVE runs: integrate2 is folded into the next step's integrate1 (flushed by finish_steps)
    bool kickOwed_ = false;
    bool fuseEpilogue_ = false;     // small plain-NVE runs: the tile kernel's epilogue applies integrate2
    // large plain-NVE runs on one GPU that walk pair lists: on a step that books no energies and is followed by a plain step of the same run, k_pair_list
    // applies both half-kicks (this step's second, the next step's first) and stores the velocity instead of the force; the next step is a drift
    bool foldKickOk_ = false;       // this engine may fold (decided once)
    bool foldDriftOk_ = false;      // ... and a folding launch also drifts (KICK_DRIFT; decided once): the new positions go to altXyz_ and the next step is opened, not kicked
    // next-step fusion (pair_tile.hip.h NextStep): on plain NVE steps of a lazy run on one GPU the pair kernel's epilogue also does the next step's
    // k_integrate1_bin<2>; the new positions go to a second set of coordinate arrays, swapped in after the launch
    double* altXyz_[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    bool fuseNextOk_ = false;       // this engine may fuse (decided once)
    bool fuseNextTstat_ = false;    // ... in a run with the radiative thermostat: the fused epilogue also applies it (k_pair_list<..., TSTAT>; decided once)
    StepPlan::Left left_ = StepPlan::LEFT_UNTOUCHED;    // how the previous step left the one being launched

    // -- snapshot: Slab ranks cannot repair a skin violation on the spot (they hold hw ghost layers: no wider stencil to fall back on), and the host learns
    // of one only at its next look.  So every look that finds none leaves a snapshot of the dynamic state (per-atom arrays, DevStats, Counts, partial sums -
    // what an exact restart needs, device to device), and a look that finds one goes back to it and runs the steps since again with the cells rebuilt every
    // step, which is exact whatever the speeds (all ranks together: the verdict is all-reduced).  A violation costs time, never exactness. ---
    struct DynState                 // what k_copy_state copies
    {
        AtomArrays A{};
        void *stats = nullptr, *counts = nullptr;
        double* partials = nullptr;
    };
    struct Snapshot : DynState
    {
        BufState buf{};
        long long hostStep = 0;
        bool valid = false;
    } snap_;
    long long stepsSinceSnap_ = 0;
    DynState live() { return DynState{cur(), dStats_, dCounts_, dPartials_}; }
    void copy_state(DynState from, DynState to);
    // One GPU, small systems (a step is a handful of microsecond kernels: the clean-up launch behind every k_pair_list is a quarter of a 40 000-atom step and
    // nearly always has nothing to do): the same snapshots let the plain steps run WITHOUT it.  A look that finds a violation or a cell that kept no list
    // goes back and runs the window again with the launch in place (exact as before), and the run stays on the safe side for a few looks.
    bool optimistic_ = false;
    int safeLooks_ = 1;             // looks still to be spent with the clean-up launch in place (an engine's first; 8, 16, 32 ... after a window had to be run again)
    int rollbacks_ = 0;
    void choose_optimism();
    bool rollback_on() const { return lazyOn_ && (nranks_ > 1 || optimistic_); }
    void take_snapshot();
    void replay_from_snapshot();
};

}  // namespace aztot
