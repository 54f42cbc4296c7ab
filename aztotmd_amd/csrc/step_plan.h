// What one time step (or one aztot_forces call) launches.  Engine::plan_step / plan_forces decide all of it from host state before the first launch;
// launch_step_kernels, sort_and_forces and launch_pair execute it and decide nothing.  The one thing left to the executor: a slab rank learns from a
// read-back, whenever the host happens to poll, that no cell is without a list (CLEANUP_UNLESS_IDLE).
#pragma once

namespace aztot {

struct StepPlan
{
    enum Opener { OPEN_NONE, OPEN_DRIFT, OPEN_PLAIN2, OPEN_PLAIN, OPEN_RESORT, OPEN_BIN };    // none: the previous pair / boundary kernel opened the step;
                            // k_drift_plain2; k_integrate_plain2; k_integrate1_bin<STEP_PLAIN>, <STEP_RESORT>, <STEP_BIN_ONLY> behind its memset
    enum Lists { LISTS_NONE, LISTS_RECORD, LISTS_WALK };            // the step that opens an interval of plain steps records the pair lists, plain steps walk them
    enum Pair { PAIR_ATOM, PAIR_TILE, PAIR_LIST };
    enum Cleanup { CLEANUP_NONE, CLEANUP_UNLESS_IDLE, CLEANUP_ALWAYS };     // pair_cleanup behind pair_list (UNLESS_IDLE: unless the rank has learnt there is nothing to clean)
    enum Closer { CLOSE_NONE, CLOSE_BOUNDARY_RADI, CLOSE_INTEGRATE2_POST, CLOSE_INTEGRATE2 };
    // how a step leaves the one behind it - the only state that crosses a step boundary (Engine::left_).  OPENED: drifted too, by the pair kernel (into the
    // second set of coordinate arrays, swapped in) or by k_boundary_radi; KICKED: k_pair_list applied both half-kicks and stored v, no f (KICK_BOTH) - NOT
    // the canonical state: the next step is a plain one of the same run and opens with k_drift_plain2
    enum Left { LEFT_UNTOUCHED, LEFT_OPENED, LEFT_KICKED };

    int stepMode = 0, cycleStep = 0;            // StepMode (kernels.hip.h); which step since the last rebuild (StepParams::cycleStep)
    Opener opener = OPEN_BIN;
    int setPending = 0;                         // a step that rebuilds the cells: what the scan leaves in DevStats::pendingKick
    bool overlapHalo = false;                   // plain slab step: the coordinate exchange runs beside the interior cells' pair forces, the pair launch is split
    Lists lists = LISTS_NONE;
    Pair pair = PAIR_TILE;
    Cleanup cleanup = CLEANUP_ALWAYS;
    bool wantEnergies = true;                   // the list kernel books pair energies
    int tileKick = 0, listKick = 0;             // StepParams::fuseKick of the tile / clean-up launches and of the list launch (KICK_*)
    bool fuseNext = false, closesStep = false;  // the pair launch opens the next step (NextStep); ... with the thermostat epilogue: it has closed this one
    int pendingAfter = -1;                      // NextStep::pendingAfter
    bool withBonded = true;
    Closer closer = CLOSE_NONE;
    bool scalingDue = false, equil = false, post = false;       // equilibration rescaling acts on this step; reduce_kin + scale_decision run; k_post runs
    Left leaves = LEFT_UNTOUCHED;
    bool ekinFromPair = false;                  // LaunchNotes (lastStepEquil is equil)
};

}  // namespace aztot
