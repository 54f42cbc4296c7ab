// Lists of the lazy re-sort (pair_tile.hip.h / pair_list.hip.h), recorded by the step that rebuilds the cells and walked by the plain steps: per cell the
// candidates its tile held, and per atom of the cell its partners among them, dealt evenly to the lanes.  The store owns the buffers, knows their capacities
// and the LDS sizes the kernels are launched with, and turns what the builder reports (ListReport) into new ones.  Host-only; the bodies are in engine.hip,
// the one translation unit that sees the kernels.  Whether the lists on the device are those of the arrays as they stand is the scheduler's business
// (Engine::listsValid_): whoever lets the store release or re-allocate makes the next step rebuild.
#pragma once
#include "device_resources.h"
#include "model.h"

namespace aztot {

struct StepParams; struct PairLists;

struct ListStore
{
    // what a look at the builder's report changed, for the scheduler
    struct Verdict
    {
        bool rebuild = false;       // the lists were re-allocated (or given up half-way): the next step must rebuild the cells
        bool launchChanged = false; // LDS sizes, waves per cell or `on` changed: captured graphs have the old ones baked in
    };

    bool on = false;                // lists exist and plain steps walk them (off: no room for them, or most unlisted cells can never be listed)
    uint32_t* cand = nullptr;
    int32_t* meta = nullptr;
    uint16_t* pairs = nullptr;
    int32_t* report = nullptr;      // [LR_COUNT] the builder's report (enum ListReport, pair_tile.hip.h)
    float4* rel = nullptr;          // [capacity + 64] position relative to the own cell's centre (f32) + cell z index, written by the sort for the list builder
    int candCap = 0, iterCap = 0;   // capacities of the lists per cell (PairLists); grown when too many cells turn out not to fit
    int candLds = 0, iterLds = 0;   // what the LDS tile of k_pair_list (the candidates a cell KEEPS) and the builder's list buffer are sized for (<= the capacities;
                                    // from the largest cell recorded)
    int stageLds = 0;               // what the builder's staging area is sized for: the candidates a cell STAGES before the unreachable ones are dropped (<= candCap)
    int buildGroups = 0;            // groups of 16 atoms whose hit masks the builder parks in LDS (PairLists::buildGroups): the worst case, 4 x waves, until a report says how
                                    // many atoms the largest cell holds; 0 with DBG_HITS_BESIDE_TILE
    int waves = 1;                  // waves per cell in k_pair_list (PairLists::waves)
    int growths = 0;
    // Bytes per pair-list entry (PairLists::entryBytes).  entryBytes: the format of the lists on the device, what k_pair_list is launched with; entryNext: the
    // format the next recording will leave (begin_recording makes it the one in force).  An engine starts with 2, goes to 1 where narrow_fits says so (tighten:
    // the caller records again at once ; adapt: from the next rebuild on, whenever that comes - no step's schedule changes), and back to 2 FOR GOOD when a
    // report shows a cell beyond 255 kept candidates (adapt: Verdict::rebuild).  A launch parameter: every change drops the captured graphs.
    int entryBytes = 2, entryNext = 2;

    // sizes the lists from density, cut-off and skin (listRadius = cut-off + skin) and allocates them; without room for them the run goes on with `on` false
    void create(const StepParams& P, const Model& m, const aztot_options& opt, int capacity, double listRadius, hipStream_t stream, int rank);
    // Larger lists in the middle of a run.  The old ones are released first (hundreds of megabytes on a 1 M-atom box: never two generations at once); if
    // the new ones do not fit the run goes on without lists instead of failing the call half-way through a look
    void regrow(int candCap, int iterCap);
    void release() noexcept;        // behind a stream synchronisation
    PairLists pair_lists() const;   // what the kernels are launched with (all-null when off)
    // LDS sizes that hold the largest cell of a report
    void lds_for(const int32_t* rep, int& candLds, int& stageLds, int& iterLds, int& buildGroups) const;
    // the first lists of an engine's life: tighter LDS sizes right away, if every cell fitted.  True when launch parameters changed; *formatChanged when
    // entryNext differs from the format those lists were recorded in (the caller records them again)
    bool tighten(const int32_t* rep, bool* formatChanged = nullptr);
    // One-byte entries for an engine whose largest recorded cell keeps maxTile candidates in a tile of candLdsNew records?  One GPU, one wave per cell, the
    // four-group kernel, every record number in a byte, never gone back before, DBG_WIDE_ENTRIES not set
    bool narrow_fits(int maxTile, int candLdsNew, int wavesNew) const;
    // in front of a launch of k_build_lists: the lists it leaves - and every k_pair_list launch from here on - are in the format entryNext
    void begin_recording() { entryBytes = entryNext; }
    // at a look, for a report with cells recorded: tighten or widen the LDS sizes, more waves per cell, larger arrays, or give up
    Verdict adapt(const int32_t* rep, unsigned debug);

private:
    void allocate(int candCap, int iterCap);
    int tile_records_for(int maxT) const;
    int stage_records_for(int maxStaged) const;
    int groups_that_fit(int want, int stageLds, int iterLds) const;
    int waves_wanted(double tileRecords, int iters) const;
    DeviceArena mem_;
    const StepParams* P_ = nullptr; // the engine's (outlives the store)
    hipStream_t stream_ = nullptr;
    int capacity_ = 0, rank_ = 0;
    int forcedWaves_ = 0;           // options.waves_per_cell where it names a count k_pair_list has (measurements), else 0
    bool wideForGood_ = false;      // a report once showed a cell that one-byte entries cannot hold: this engine keeps 16-bit entries (no flipping back and forth)
    size_t ldsMax_ = 0;             // dynamic LDS this device grants a workgroup
};

}  // namespace aztot
