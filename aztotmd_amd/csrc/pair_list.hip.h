// Pair lists of the lazy re-sort: the kernel that builds them on the step that rebuilds the cells (k_build_lists) and the pair-force kernel that walks
// them on every step of a lazy run (k_pair_list).  One wave64 per cell in both.
//
// Replaces the reference's cell_list5a + cell_list4b_noshared + pair_1 (cuPairs.cu:2266,1474,117).  The reference rebuilds everything every step
// (main.cu:300-326); here the cells are rebuilt every K-th step only (Engine::step) and the rebuild leaves two lists per cell:
//   * the candidates: every atom of the cell's stencil within rc + skin of at least one atom of the cell (atom index + periodic image code, tile order), and
//   * for every atom of the cell its partners among them - the candidates within rc + skin of the atom -, dealt round-robin to the lanes that
//     serve the atom.  An entry is the byte offset of the candidate's record in the LDS tile of k_pair_list.
// Until the next rebuild atoms keep their slots and nobody moves farther than skin / 2 (checked every step by whoever integrates; a violation makes
// k_pair_list stand down and the clean-up launch of k_pair_tile stage everything with a wider stencil), so no pair inside rc can be missing and a step is
//   1. gather the candidates into LDS (coordinates relative to the cell centre: same numbers, same arithmetic as k_pair_tile);
//   2. every lane walks ITS list: entry -> LDS record -> exact r^2 <= rc^2 test -> potential (pair_body, shared with k_pair_tile);
//   3. optionally the epilogue opens the next step: second half-kick, first half-kick, drift (NextStep, small systems: everything k_integrate1_bin<2>
//      does; KICK_DRIFT, large ones: the lean form below).
// Lanes are (atom slot, slice) with slot = lane / NS and NS = min(8, 64 / atoms in the cell) slices per atom: 13-16 atoms run 4 slices each, 17-21
// three, 22-32 two - whatever the cell holds, at least two thirds of the lanes work (the power-of-two layout of round 2 fell to half at 17 atoms, which
// is what a liquid's cells of rc + skin hold).  Slices of one atom are neighbouring lanes: they are folded with lane shifts in a fixed order.
// Forces: written once per atom, no atomics, fixed summation order => bit-reproducible.  All list sizes are per engine (PairLists::candCap / iterCap,
// dynamic LDS), so dense systems (hundreds of partners per atom, a thousand candidates per cell) walk lists too.
#pragma once
#include <type_traits>
#include "pair_tile.hip.h"

namespace aztot {

constexpr int kListPreload = 5;            // most groups of 64 candidate entries a wave of k_pair_list asks for before it knows the cell's T (candCap >= 320)
constexpr int kListMinCand = 64 * kListPreload;
// groups gathered up front by every wave of k_pair_list, a compile-time parameter of the kernel: four cover a tile of up to 256 records (a liquid's cells
// of rc + skin keep ~160 candidates, never more than ~210), five the larger ones; the builder pads the candidate array to that many groups
__host__ __device__ inline int list_preload(int candLds) { return candLds <= 4 * kWave ? 4 : kListPreload; }
constexpr int kListMinIter = 16;           // two chunks of 8 iterations are asked for up front
constexpr int kListMaxSlices = 32;         // slices per atom (a cell of one or two atoms still uses half a wave)

constexpr int kListMaxWaves = 4;
// a cell of n atoms served by W waves: every wave takes ceil(n / W) atoms (the last ones fewer, possibly none), each with NS = 64 / that many slices
__host__ __device__ inline int list_atoms_per_wave(int nAtoms, int W) { return (nAtoms + W - 1) >> (W >> 1); }      // (W is 1, 2 or 4: a shift, not a division)
__host__ __device__ inline int list_slices(int nAtomsOfWave) { const int n = kWave / (nAtomsOfWave > 0 ? nAtomsOfWave : 1); return n > kListMaxSlices ? kListMaxSlices : (n < 1 ? 1 : n); }

// LDS of k_pair_list by kernel mode (LDS per wave bounds its occupancy, so every byte per candidate counts):
//   one species, LJ (PM_ONE_LJ)         records {x, y, z} of 24 B; a list entry is the record's byte offset
//   table-driven modes (PM_TAB*)        [pair table 1 KiB][species bytes, kListTypeBytes][records of 24 B]; a list entry is the record NUMBER (the species byte
//                                       sits at a fixed offset + number, the record at number x 24 + base: one v_mad more per visit, 8 B less per candidate)
//   PM_ONE_SURK / PM_GENERIC            [records of 24 B][radii, 8 B each][species bytes (PM_GENERIC)]; entry = record number.  (Records of 32 B {x, y, z, radius}
//                                       were tried first: a stride of 8 banks leaves 8 distinct bank groups for 64 lanes - 90 % of the LDS cycles of the
//                                       case-study-2 kernel were bank conflicts; 24 B = 6 banks gives 32)
inline bool pair_list_tab_mode(const StepParams& P) { return P.potSet == POTSET_ONE_FAMILY && !P.single_lj; }
inline size_t pair_list_lds_bytes(const StepParams& P, const PairLists& L)
{
    const bool tab = pair_list_tab_mode(P);
    const bool generic = !P.single_lj && P.potSet == POTSET_GENERIC;
    const bool radii = !P.single_lj && !tab;                       // PM_ONE_SURK and PM_GENERIC
    size_t b = (size_t)(L.candLds + 1) * 24;
    if (tab) b += sizeof(double) * kLjSpecMax * kLjSpecMax * kPairTabStride + (((size_t)L.candLds + 1 + 15) & ~(size_t)15);
    if (radii) b += sizeof(double) * (size_t)(L.candLds + 1);
    if (generic) b += (size_t)(L.candLds + 1 + 7) & ~(size_t)7;
    return b;
}
inline int pair_list_rec_bytes(const StepParams&) { return 24; }
inline int pair_list_entry_scale(const StepParams& P) { return P.single_lj ? 24 : 1; }     // what the builder multiplies a record number by: byte offset, or the number itself

// KICK_DRIFT: the drift of the NEXT step behind the two folded kicks, by the lane that has just stored the atom's final velocity - what k_drift_plain2
// (integrate_plain2_body<false>, kernels.hip.h) does for the atom in a launch of its own, the same operations in the same order with the next step's
// values (cycle step P.cycleStep + 1), so positions, flags and counters are bit-identical.  That kernel's side effects and who takes care of each here:
//   x, y, z                      fold_drift_atom; into the second set of coordinate arrays (NextStep::xd/yd/zd: other waves still gather this step's positions)
//   DevStats::step += 1          k_pair_list's last lines
//   PS_EFIELD partials zeroed    k_pair_list's last lines, the same entries (NextStep::driftBlocks)
//   Counts::maxStep2, cycMaxRun  fold_drift_finish: integer-bit atomicMax behind a relaxed load, once per wave - and only in a wave that holds a step
//                                longer than the maxima it read when it started (after the first waves of a window: nobody)
//   Counts::lazyViolated / Ever  fold_drift_finish, numbered from the step being opened (next_step_finish's convention)
//   DevStats::specCross          fold_drift_finish, one atomic per crossing
//   wall momenta, crossing counts  fold_drift_finish, into this wave's partial slot (next_wall_sum); a wall's momentum sum is then added in another order
//                                than k_drift_plain2's workgroups add it: equal to a few ulps, the counts exactly
// Lean, because the kernel is bound by instruction issue: the reference position is read only by a lane the displacement bound cannot clear (P.boundSkip,
// as in k_drift_plain2; the bound itself is taken in f32, rounded to the safe side: it decides who looks, never what is found); a crossing is one bit, the
// sums are built by the rare wave that has one; and a wave whose cell has no periodic image in its stencil (`interior`) skips the six image_of evaluations
// as long as every one of its atoms is and stays within a cell edge and a quarter of its cell's centre - such a position lies strictly inside the box
// before and after, image 0 both times.
__device__ __forceinline__ void fold_drift_atom(const StepParams& P, const SpecTable& S, const NextStep& N, int i, int t, double x, double y, double z,
                                                double xi, double yi, double zi, double vx, double vy, double vz, bool interior, double room2,
                                                double& len2, int& cross, int& violated)
{
    const double x0 = x, y0 = y, z0 = z;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (!S.frozen[t]) { dx = vx * P.dt; dy = vy * P.dt; dz = vz * P.dt; x += dx; y += dy; z += dz; }
    len2 = dx * dx + dy * dy + dz * dz;
    bool full = !interior;
    if (interior)
    {   // (xi, yi, zi: the old position relative to the cell's centre, which the lane holds anyway)
        const double lx = 1.25 * P.csz[0], ly = 1.25 * P.csz[1], lz = 1.25 * P.csz[2];
        const bool far = fabs(xi) > lx || fabs(xi + dx) > lx || fabs(yi) > ly || fabs(yi + dy) > ly || fabs(zi) > lz || fabs(zi + dz) > lz;
        full = __any(far) != 0;                                       // (over the lanes that hold an atom)
    }
    if (full)
    {
        int c;
        c = image_of(x, P.L[0], P.invL[0]) - image_of(x0, P.L[0], P.invL[0]);
        if (c < 0) cross |= 1; else if (c > 0) cross |= 2;
        c = image_of(y, P.L[1], P.invL[1]) - image_of(y0, P.L[1], P.invL[1]);
        if (c < 0) cross |= 4; else if (c > 0) cross |= 8;
        c = image_of(z, P.L[2], P.invL[2]) - image_of(z0, P.L[2], P.invL[2]);
        if (c < 0) cross |= 16; else if (c > 0) cross |= 32;
    }
    if (!(room2 > 0.0 && len2 < room2))
    {
        const double ex = x - N.R0.x[i], ey = y - N.R0.y[i], ez = z - N.R0.z[i];
        if (ex * ex + ey * ey + ez * ez > P.lazySlack2) violated = 1;
    }
    st_f64(N.xd, i, x); st_f64(N.yd, i, y); st_f64(N.zd, i, z);
}

// once per wave, all lanes (those without an atom bring zeros): runBits / maxBits are Counts::cycMaxRun / maxStep2 as the wave read them when it started
__device__ __forceinline__ void fold_drift_finish(const StepParams& P, const SpecTable& S, const NextStep& N, int t, double vx, double vy, double vz, double len2,
                                                  int cross, int violated, unsigned long long runBits, unsigned long long maxBits,
                                                  double* __restrict__ partials, int maxBlocks, size_t pb)
{
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned long long mine = (unsigned long long)__double_as_longlong(len2);
    if (__any(mine > maxBits || (P.boundSkip && mine > runBits)))
    {
        double mx = len2;
#pragma unroll
        for (int o = kWave >> 1; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, kWave));
        if (lane == 0)
        {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(mx);
            if (bits > __hip_atomic_load(&N.cnt->maxStep2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&N.cnt->maxStep2, bits);
            if (P.boundSkip && bits > __hip_atomic_load(&N.cnt->cycMaxRun, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&N.cnt->cycMaxRun, bits);
        }
    }
    if (__any(violated) && lane == 0)
    {
        if (N.cnt->lazyViolated == 0) N.cnt->lazyViolated = P.cycleStep + 1;
        N.cnt->lazyViolatedEver = 1;
    }
    if (__any(cross != 0))
    {   // a handful of atoms in a million cross a wall on any one step.  Slots in the order Xn, Xp, Yn, Yp, Zn, Zp (PartialSlot)
#pragma unroll
        for (int d = 0; d < 6; d++) if (cross & (1 << d)) atomicAdd(&N.st->specCross[t * 6 + d], 1ULL);
        const double m = S.mass[t];
        next_wall_sum(m * (-vx), cross & 1, 1, 0, partials, maxBlocks, pb); next_wall_sum(m * vx, cross & 2, 2, 1, partials, maxBlocks, pb);
        next_wall_sum(m * (-vy), cross & 4, 4, 2, partials, maxBlocks, pb); next_wall_sum(m * vy, cross & 8, 8, 3, partials, maxBlocks, pb);
        next_wall_sum(m * (-vz), cross & 16, 16, 4, partials, maxBlocks, pb); next_wall_sum(m * vz, cross & 32, 32, 5, partials, maxBlocks, pb);
    }
}

// ENG = false: the launch books no energies (steps whose energies nobody can see: all but the last step of an aztot_step call - the statistics are those of
// the last step, finish_steps; the reference prints them every `stat` steps, cuStat.cu:308-330).  Forces are the same instructions either way: the energy
// terms feed nothing else, the compiler drops them and their two wave reductions.
// MULTI = false: one wave per cell, known when the kernel is compiled (the wave number and every multiple of W fold away: 585 -> 515 vector instructions per
// cell on the 1 M-atom liquid); true: W = PairLists::waves waves share the cell's tile.
// TSTAT = true (launches that fuse the next step in a run with the radiative thermostat; never with ENG: the call's last step does not fuse): the epilogue
// applies the thermostat between closing this step and opening the next, operation for operation what k_boundary_radi does in a launch of its own.
// PRE: groups of candidates gathered up front (list_preload: 4 for tiles of up to 256 records, else 5).
// EB: bytes per list entry (PairLists::entryBytes).  2: chunks of 8 iterations, two of them asked for up front.  1 (only !MULTI && PRE == 4, every mode): an
// entry is the record NUMBER, a chunk holds 16 iterations; chunk 0 is asked for up front and chunk 1 only by a wave whose header says nIter > 16 - one cell
// in seven of a liquid - so the pair entries of a step are 1.14 KiB per cell instead of 2.14.  The same entries are visited in the same order with the same
// arithmetic: only the encoding of a record number differs.
template <int MODE, int VDW, bool ENG, bool MULTI, bool TSTAT = false, int PRE = kListPreload, int EB = 2>
__global__ __launch_bounds__(MULTI ? kWave * kListMaxWaves : kWave) void k_pair_list(StepParams P, SpecTable S, const DevPot* __restrict__ pots, AtomArrays A,
                                                     const int32_t* __restrict__ cellStart, int firstCell, int nCellsRun,
                                                     double* __restrict__ partials, int maxBlocks, const Counts* __restrict__ counts, int blockBase, PairLists L,
                                                     NextStep N)
{
    constexpr bool kOneSpecies = pair_mode_one_species(MODE);
    constexpr bool kRadii = pair_mode_reads_radii(MODE);
    constexpr bool kTab = pair_mode_has_table(MODE);
    constexpr int RECB = 24;                                         // record {x, y, z} RELATIVE to the centre of the cell
    static_assert(EB == 2 || (EB == 1 && !MULTI && PRE == 4), "one-byte list entries: one wave per cell and the four-group tile only");
    constexpr int ESCALE = (MODE == PM_ONE_LJ && EB == 2) ? 1 : 24;          // list entry -> byte offset of the record (only the one-species LJ kernel's 16-bit entries are byte offsets)
    constexpr int VPC = 16 / EB;                                     // visits per 1 KiB chunk (16 B per lane)
    constexpr int kTabDoubles = kTab ? kLjSpecMax * kLjSpecMax * kPairTabStride : 0;
    extern __shared__ double ldsList[];
    double* const pairTab = ldsList;
    uint8_t* const ttypT = (uint8_t*)(ldsList + kTabDoubles);        // table modes: species ids by record number, at a compile-time offset
    char* const tb = (char*)(ldsList + kTabDoubles) + (kTab ? ((L.candLds + 1 + 15) & ~15) : 0);
    double* const trad = (double*)(tb + (size_t)(L.candLds + 1) * RECB);         // modes that read radii (by record number)
    uint8_t* const ttyp0 = (uint8_t*)(trad + (L.candLds + 1));                   // PM_GENERIC only: species ids (by record number)

    const int lane = threadIdx.x & (kWave - 1), wave = MULTI ? (int)(threadIdx.x >> 6) : 0;
    const int W = MULTI ? L.waves : 1;                               // waves of this workgroup = waves per cell (they share the tile, each serves its share of the atoms)
    const int per = (nCellsRun + 7) >> 3;
    const int cr = (blockIdx.x & 7) * per + (blockIdx.x >> 3);       // XCD-aware: each XCD owns a contiguous eighth of the cells
    double eV = 0.0, eC = 0.0, dropped = 0.0, eK = 0.0;
    NextAcc nacc;                                                    // (touched only in launches that fuse the next step: no initialisation on the others)
    if (N.xn) next_acc_clear(nacc);
    // everything that depends on the cell number only is requested at once, before anything is known about the cell (the loads stay inside the
    // arrays whatever they return): list header, PRE groups of candidate entries, the lane's first two list chunks.  A wave's life is then two
    // memory round trips (these, then the coordinates) and the loop
    const int cell = firstCell + min(cr, nCellsRun - 1);
    // (candidate groups are dealt to the waves round-robin: wave w gathers groups w, w + W, ...; candCap >= 64 * 5 * W keeps the preloads inside the array)
    const uint32_t* const myList = L.cand + (size_t)cell * L.candCap + lane;
    const uint4* const pl = (const uint4*)(L.pairs + ((size_t)cell * W + wave) * L.iterCap * kWave) + lane;
    // one wave and four groups: the FOURTH group's entries are asked for below, once the header has said that the group holds a candidate (T > 192).  A
    // liquid's cells keep ~160 candidates: in most of them the group is 256 B of padding that nobody needs to load (17.6 MB per launch on the 1 M-atom box)
    constexpr bool kLazyLast = PRE == 4 && !MULTI;
    uint32_t ent[PRE];
#pragma unroll
    for (int u = 0; u < PRE; u++) ent[u] = (kLazyLast && u == PRE - 1) ? 0u : myList[(wave + u * W) * kWave];
    uint4 w = pl[0];
    uint4 w1 = make_uint4(0u, 0u, 0u, 0u);
    if (EB == 2) w1 = pl[kWave];                                    // (the second chunk too: 16 iterations cover a liquid's cells, and a chunk asked for only
                                                                    //  8 iterations ahead arrives late.  One-byte entries: chunk 0 IS 16 iterations; chunk 1
                                                                    //  is asked for below, once the header has said that the cell needs it)
    // {list header, cell coordinates lx | cy << 10 | cz << 20, the cell's first atom, atoms | rcpNS << 12}: one scalar load - no look at cellStart (a second,
    // dependent round trip), no integer divisions (the builder leaves slices per atom and their reciprocal in the header)
    const int4 mx = ((const int4*)L.meta)[cell];
    // KICK_DRIFT: the longest steps so far, for the displacement bound and for fold_drift_finish (a value from before this launch's first atomic serves both)
    unsigned long long runBits = 0ULL, maxBits = 0ULL;
    if (P.fuseKick == KICK_DRIFT) { runBits = N.cnt->cycMaxRun; maxBits = N.cnt->maxStep2; }
    asm volatile("" ::: "memory");                              // (what follows is issued behind the loads above, not in front of them)
    // after a slack violation (one GPU) the clean-up launch stages every cell with the wider stencil: stand down
    const bool violated = P.nranks == 1 && !P.optimistic && slack_violated(P, counts);
    int meta = mx.x;
    if (violated || cr >= nCellsRun || !list_usable(L, meta)) meta = -1;         // (a cell that does not walk its list is served by the clean-up launch)
    if (meta > 0)
    {
        const int T = meta & 0xFFF, nIter = (meta >> 12) & 0xFF;
        // the last group up front holds a candidate (wave-uniform).  A wave that skips it loads no entries, fetches no coordinates and leaves records
        // 193 .. candLds of its tile unwritten.  No list entry of such a cell names them: k_build_lists writes whole chunks (every lane's 16 bytes of every
        // chunk below nIter), each entry the record of a KEPT candidate - n + 1 <= T - or 0, the dummy; the walk reads no chunk at or above nIter, and the
        // read ahead behind a list's last chunk is the dummy's (below) - stale entries of an older, larger list are never looked up
        const bool lastGroup = !kLazyLast || T > (PRE - 1) * kWave;
        if (kLazyLast)
        {   // (in front of the gather and behind a barrier, like chunk 1 below)
            if (lastGroup) ent[PRE - 1] = myList[(PRE - 1) * kWave];
            if (EB != 1) asm volatile("" ::: "memory");
        }
        if (EB == 1)
        {   // one-byte entries: the second chunk, for the cells that have one (wave-uniform).  Asked for here, in front of the gather, so that it travels with
            // the coordinates; the barrier keeps the compiler from sinking the load behind the LDS writes (as it once did with a conditional preload of
            // the fifth candidate group)
            if (nIter > VPC) w1 = pl[kWave];
            asm volatile("" ::: "memory");
        }
        const int ncy = P.nc[1], ncz = P.nc[2];
        const int lx = mx.y & 1023, cy = (mx.y >> 10) & 1023, cz = (mx.y >> 20) & 1023;
        const int ib = mx.z;
        const double cc0 = (lx + P.cx0) * P.csz[0] + 0.5 * P.csz[0], cc1 = cy * P.csz[1] + 0.5 * P.csz[1], cc2 = cz * P.csz[2] + 0.5 * P.csz[2];
        const DevPot lj = pots[0];
        if (kTab)
        {
            const int np = P.nSpec * P.nSpec;
            if (threadIdx.x < np)
            {
                const DevPot v = pots[lane];
                const int a = lane / P.nSpec, b = lane - a * P.nSpec;
                double* q = pairTab + lane * kPairTabStride;
                q[0] = v.p0; q[1] = v.p1; q[2] = v.p2; q[3] = v.p3; q[4] = v.p4;
                q[5] = v.type ? v.r2cut : -1.0;                                   // no potential for this pair: never inside the cut-off
                q[6] = (S.charged[a] && S.charged[b]) ? S.charge[a] * S.charge[b] * P.fcoul : 0.0;
                if (v.type == 2) q[3] = 1.0 / v.p1;                              // buck uses p0..p2 only: 1/rho rides in the p3 slot
                q[7] = (double)v.type;
            }
        }
        // ---- the cell's own atoms: this wave serves atoms [wave * aw, wave * aw + aw) of the cell; lane = slot * NS + slice
        const int ncell = mx.w & 0xFFF;                                // 1 .. 64 W (cells with more keep no list)
        const int aw = list_atoms_per_wave(ncell, W);
        const int nthis = max(0, min(aw, ncell - wave * aw));           // atoms of this wave (the last waves of a small cell may have none)
        const int NS = (meta >> 20) & 63;                               // slices per atom, list_slices(aw), and 65536 / NS + 1: left in the header by the builder
        const int rcpNS = mx.w >> 12;
        const int slot = (lane * rcpNS) >> 16, slice = lane - slot * NS;
        const bool validI = slot < nthis;
        const int myi = ib + wave * aw + slot;
        // (every lane loads - idle atom slots from the cell's first atom - so that the three loads travel together; a conditional load made the compiler
        //  wait for each of them in turn)
        const int myl = validI ? myi : ib;
        const double xr = A.x[myl], yr = A.y[myl], zr = A.z[myl];
        // NextStep: what the epilogue will need is asked for now - loaded there, at the end of the wave's life, it cost a memory round trip per wave (+30 us)
        double v0x, v0y, v0z, r0x, r0y, r0z;                         // (defined exactly where they are used: with fuseKick / NextStep)
        if (P.fuseKick || N.xn) { v0x = A.vx[myl]; v0y = A.vy[myl]; v0z = A.vz[myl]; }
        if (N.xn) { r0x = N.R0.x[myl]; r0y = N.R0.y[myl]; r0z = N.R0.z[myl]; }
        double radi = 0.0;
        int ti = 0;
        if (!kOneSpecies) ti = A.type[myl];
        if ((MODE == PM_GENERIC && P.use_radii) || MODE == PM_ONE_SURK) radi = A.rad[myl];
        // ---- gather the candidates (groups of 64; the builder padded the last group with a valid atom).  PRE groups are gathered whatever T is - but for the
        // fourth of a one-wave, four-group kernel, lastGroup above - (stale entries are atom indices too: the array starts out zeroed and only indices are ever
        // written); all their loads travel together
        const int gx0 = lx + P.cx0;
        // does any neighbour cell lie across a periodic boundary (or the seam of a slab ring)?  wave-uniform
        const bool images = gx0 - P.hw[0] < 0 || gx0 + P.hw[0] >= P.nc[0] || cy - P.hw[1] < 0 || cy + P.hw[1] >= ncy || cz - P.hw[2] < 0 || cz + P.hw[2] >= ncz;
        {
            struct Cand { double x, y, z, rad; int typ; };
            auto fetch = [&](uint32_t e) {
                Cand c;
                const int j = (int)(e & 0x3FFFFFFu);
                c.x = ld_f64(A.x, j); c.y = ld_f64(A.y, j); c.z = ld_f64(A.z, j);
                c.typ = kOneSpecies ? 0 : ld_i32(A.type, j);
                c.rad = ((MODE == PM_GENERIC && P.use_radii) || MODE == PM_ONE_SURK) ? ld_f64(A.rad, j) : 0.0;
                return c;
            };
            auto put = [&](auto IMG, int u, uint32_t e, const Cand& c) {
                // (the tile holds candLds records, not whole groups of 64: LDS per wave bounds the occupancy; the first four groups always fit)
                if ((MULTI || u >= 4) && u * kWave + lane >= L.candLds) return;      // (one wave: its first four groups always fit, candLds >= 256)
                double xj = c.x, yj = c.y, zj = c.z;
                if (decltype(IMG)::value)
                {   // image code per axis: 0 -> -L, 1 -> 0, 2 -> +L (exact: the product is +-L or 0)
                    xj += (double)((int)((e >> 26) & 3u) - 1) * P.L[0];
                    yj += (double)((int)((e >> 28) & 3u) - 1) * P.L[1];
                    zj += (double)((int)((e >> 30) & 3u) - 1) * P.L[2];
                }
                char* const r = tb + (size_t)(u * kWave + lane + 1) * RECB;       // candidate k -> record k + 1 (record 0 is the dummy)
                *(double*)r = xj - cc0; *(double*)(r + 8) = yj - cc1; *(double*)(r + 16) = zj - cc2;
                if (kTab) ttypT[u * kWave + lane + 1] = (uint8_t)c.typ;
                if (kRadii) trad[u * kWave + lane + 1] = c.rad;
                if (MODE == PM_GENERIC) ttyp0[u * kWave + lane + 1] = (uint8_t)c.typ;
            };
            // this wave's groups are wave + q W, q = 0, 1, ...  PRE of them are gathered whatever T is - straight-line code, 3 PRE loads in flight together
            // (the builder fills all PRE groups of the array: behind the last candidate with the cell's first atom, one cache line for the whole wave.
            //  Skipping only the last group's coordinate FETCH where it holds padding was measured earlier: ~1 us of 85, not kept; skipping its 256 B of
            //  entries as well - kLazyLast, above - is worth 2 us of 91 on the 1 M-atom box, NOTES.md)
            Cand cd[PRE] = {};
#pragma unroll
            for (int u = 0; u < PRE; u++) if (u < PRE - 1 || lastGroup) cd[u] = fetch(ent[u]);
            using ImgYes = std::integral_constant<bool, true>;
            using ImgNo = std::integral_constant<bool, false>;
            // (two copies of the straight-line code rather than a wave-uniform branch inside every put: interior cells - nearly all - shift nothing)
            if (images)
            {
#pragma unroll
                for (int u = 0; u < PRE; u++) if (u < PRE - 1 || lastGroup) put(ImgYes(), wave + u * W, ent[u], cd[u]);
            }
            else
            {
#pragma unroll
                for (int u = 0; u < PRE; u++) if (u < PRE - 1 || lastGroup) put(ImgNo(), wave + u * W, ent[u], cd[u]);
            }
            if (T > PRE * W * kWave)
            {   // dense systems: the rest of the tile, four groups per round trip
                for (int q0 = PRE; (wave + q0 * W) * kWave < T; q0 += 4)
                {
                    uint32_t en[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) en[q] = ((wave + (q0 + q) * W) * kWave < T) ? myList[(wave + (q0 + q) * W) * kWave] : ent[0];
                    const Cand d0 = fetch(en[0]), d1 = fetch(en[1]), d2 = fetch(en[2]), d3 = fetch(en[3]);
                    put(ImgYes(), wave + q0 * W, en[0], d0);           // (image code 1 on every axis shifts by exactly 0)
                    if ((wave + (q0 + 1) * W) * kWave < T) put(ImgYes(), wave + (q0 + 1) * W, en[1], d1);
                    if ((wave + (q0 + 2) * W) * kWave < T) put(ImgYes(), wave + (q0 + 2) * W, en[2], d2);
                    if ((wave + (q0 + 3) * W) * kWave < T) put(ImgYes(), wave + (q0 + 3) * W, en[3], d3);
                }
            }
        }
        // idle atom slots sit far away on the other side of the dummy candidate, so that nothing they meet is inside a cut-off
        const double xi = validI ? xr - cc0 : 1e30, yi = validI ? yr - cc1 : 1e30, zi = validI ? zr - cc2 : 1e30;
        // the dummy candidate the unused list entries (0) point at: far outside any cut-off, with a species and a radius the potentials can digest
        constexpr uint32_t dummyOff = 0u;
        if (threadIdx.x == 0)
        {
            char* const r = tb;
            *(double*)r = -1e30; *(double*)(r + 8) = -1e30; *(double*)(r + 16) = -1e30;
            if (kTab) ttypT[0] = 0;
            if (kRadii) trad[0] = 1.0;
            if (MODE == PM_GENERIC) ttyp0[0] = 0;
        }
        __syncthreads();                                                // (one wave: no more than the wave barrier it replaces; the branch is uniform over the workgroup)

        // ---- every lane walks its list
        PairAcc acc = {0, 0, 0, 0, 0, 0};
        int nDropHalf = 0;
        double ljDropR2 = P.ljDropR2;
        if (kTab) asm volatile("" : "+v"(ljDropR2));                   // (table-driven modes: a vector register, like the uniforms of PairHot - see there)
        const PairHot hot = kTab ? pair_hot_in_vgprs(P, lj) : (MODE == PM_ONE_LJ ? pair_hot_lj_in_vgprs(P, lj) : pair_hot(P, lj));
        const int nChunks = (nIter + VPC - 1) / VPC;
        // software-pipelined: the candidate of iteration t + 1 is read from LDS before the potential of iteration t is evaluated (entries behind a lane's
        // last one point at the dummy - the builder fills the list buffer with it - so the read ahead is always a valid one)
        double xj, yj, zj, radj = 0.0;
        int tj = 0;
        auto fetch = [&](uint32_t en, double& x, double& y, double& z, int& ty, double& rd) {
            const uint32_t ko = en * ESCALE;                           // (table modes: one v_mad_u32_u24 with the records' base)
            // (x and y leave as one ds_read2_b64, z as a ds_read_b64.  Three ds_read_b64 - the offset laundered through an empty asm between the uses, so that
            //  the compiler cannot merge them - were measured on this layout: 98-102 us against 91-93 on the 1 M-atom box, NOTES.md)
            x = *(const double*)(tb + ko);
            y = *(const double*)(tb + ko + 8);
            z = *(const double*)(tb + ko + 16);
            if (kTab) ty = ttypT[en];
            if (kRadii) rd = trad[en];
            if (MODE == PM_GENERIC) ty = ttyp0[en];
        };
        // (one-byte entries: whatever a byte holds - a stale entry of an older list, of the other format - is a record of the tile, which has candLds + 1 >= 257
        //  records: the read ahead stays inside the tile)
        fetch(nIter > 0 ? (w.x & (EB == 1 ? 0xFFu : 0xFFFFu)) : dummyOff, xj, yj, zj, tj, radj);
        for (int c = 0; c < nChunks; c++)
        {
            uint4 wn = w1;
            if (c + 2 < nChunks) w1 = pl[(c + 2) * kWave];
            const uint32_t ww[5] = {w.x, w.y, w.z, w.w, wn.x};
#pragma unroll
            for (int u = 0; u < VPC; u++)
            {
                const int t = c * VPC + u;
                if (t >= nIter) break;                                  // wave-uniform
                uint32_t kn;                                            // the next candidate's list entry: byte offset of its record, or its number
                if (EB == 1) kn = (ww[(u + 1) >> 2] >> (8 * ((u + 1) & 3))) & 0xFFu;
                else kn = ((u + 1) & 1) ? (ww[(u + 1) >> 1] >> 16) : (ww[(u + 1) >> 1] & 0xFFFFu);
                if (u == VPC - 1 && c + 1 >= nChunks) kn = dummyOff;     // (behind the list's last chunk there is nothing the builder wrote: stale entries of an older, larger tile)
                double xn, yn, zn, radn = 0.0;
                int tn = 0;
                fetch(kn, xn, yn, zn, tn, radn);
                {   // (no test of the lane's own entry count: behind its last entry a lane finds dummies)
                    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
                    const double r2 = dx * dx + dy * dy + dz * dz;
                    pair_body<MODE, VDW, true>(P, S, pots, lj, pairTab, true, dx, dy, dz, r2, ti, tj, radi, radj, ljDropR2, nDropHalf, acc, hot);
                }
                xj = xn; yj = yn; zj = zn; tj = tn; radj = radn;
            }
            w = wn;
        }
        if (MODE != PM_GENERIC) acc.dropped += 0.5 * (double)nDropHalf;

        // fold the slices of every atom (neighbouring lanes) in a fixed tree order and write the force: clear_force + pair sums
        if (NS == 4)
        {   // (the usual case: two lane exchanges inside a quad)
            acc.fx += __shfl_xor(acc.fx, 1, kWave); acc.fy += __shfl_xor(acc.fy, 1, kWave); acc.fz += __shfl_xor(acc.fz, 1, kWave);
            acc.fx += __shfl_xor(acc.fx, 2, kWave); acc.fy += __shfl_xor(acc.fy, 2, kWave); acc.fz += __shfl_xor(acc.fz, 2, kWave);
        }
        else
        {   // n partial sums left in slices 0 .. n - 1: slice i < s takes slice i + s (if there is one), then n = s; at most five steps for 32 slices
            int n = NS;
            for (int s = kListMaxSlices / 2; s >= 1; s >>= 1)
            {
                if (s >= n) continue;                                   // wave-uniform
                const double ux = __shfl_down(acc.fx, s, kWave), uy = __shfl_down(acc.fy, s, kWave), uz = __shfl_down(acc.fz, s, kWave);
                if (slice < s && slice + s < n) { acc.fx += ux; acc.fy += uy; acc.fz += uz; }
                n = s;
            }
        }
        // KICK_DRIFT: what the lane hands to its wave (fold_drift_finish); lanes without an atom bring zeros
        double dLen2 = 0.0, dvx = 0.0, dvy = 0.0, dvz = 0.0;
        int dCross = 0, dViol = 0;
        if (validI && slice == 0)
        {
            double q = 0.0;
            if (!kOneSpecies) q = S.charge[ti];
            const double fxi = -q * P.E[0] + acc.fx;   // clear_force integrators.cpp:17-39
            const double fyi = -q * P.E[1] + acc.fy;
            const double fzi = -q * P.E[2] + acc.fz;
            if (P.fuseKick >= KICK_BOTH)
            {   // this step's second half-kick and the next step's first: the two roundings k_integrate_plain2 would make from the stored force (the kick
                // it owes, then its own).  The velocity leaves instead of the force, which nobody reads before the next pair kernel: the next step is a
                // drift (k_drift_plain2, or KICK_DRIFT right here).  Never a step whose energies are booked, never with NextStep (Engine::launch_step_kernels)
                const double rM = S.rMhdt[ti];
                double vx = v0x + rM * fxi, vy = v0y + rM * fyi, vz = v0z + rM * fzi;
                vx += rM * fxi; vy += rM * fyi; vz += rM * fzi;
                st_f64(A.vx, myi, vx); st_f64(A.vy, myi, vy); st_f64(A.vz, myi, vz);      // (32-bit byte offsets: no 64-bit address arithmetic per store)
                if (P.fuseKick == KICK_DRIFT)
                {   // the displacement bound of the step being opened, squared (k_drift_plain2's roomLeft): the slack less P.cycleStep steps of the longest
                    // length so far - two f32 square roots, each rounded to the safe side by far more than their error; <= 0: every atom is checked
                    double room2 = -1.0;
                    if (P.boundSkip)
                    {
                        const float room = __builtin_amdgcn_sqrtf((float)P.lazySlack2) * 0.99999f -
                                           (float)P.cycleStep * (__builtin_amdgcn_sqrtf((float)__longlong_as_double((long long)runBits)) * 1.00001f);
                        if (room > 0.0f) room2 = (double)(room * room);
                    }
                    fold_drift_atom(P, S, N, myi, ti, xr, yr, zr, xi, yi, zi, vx, vy, vz, !images, room2, dLen2, dCross, dViol);
                    dvx = vx; dvy = vy; dvz = vz;
                }
            }
            else
            {
            A.fx[myi] = fxi; A.fy[myi] = fyi; A.fz[myi] = fzi;
            if (P.fuseKick || N.xn)
            {   // second half-kick + kinetic energy of integrate2 (integrators.cpp:486-531 ; verlet_2stage cuMDfunc.cu:521-600); with NextStep also the
                // next step's k_integrate1_bin<2>
                const double rM = S.rMhdt[ti], m = S.mass[ti];
                double vx = v0x + rM * fxi, vy = v0y + rM * fyi, vz = v0z + rM * fzi;
                if (ENG && P.fuseKick == KICK_SECOND) eK += (vx * vx + vy * vy + vz * vz) * m;     // (the kinetic energy too is looked at after a call's last step only)
                if (TSTAT && N.xn)      // close the step as k_integrate2_post does: the thermostat acts on the fully kicked velocity; its draws are keyed by this step's number
                    (void)post_tstat_atom(P, S, A, N.st, N.photons, N.uvx, N.uvy, N.uvz, myi, vx, vy, vz, N.st->stepAtSort + (long long)P.cycleStep);
                if (N.xn) next_step_atom(P, S, N, myi, ti, xr, yr, zr, fxi, fyi, fzi, vx, vy, vz, r0x, r0y, r0z, nacc);
                A.vx[myi] = vx; A.vy[myi] = vy; A.vz[myi] = vz;
            }
            }
        }
        if (P.fuseKick == KICK_DRIFT)
            fold_drift_finish(P, S, N, ti, dvx, dvy, dvz, dLen2, dCross, dViol, runBits, maxBits, partials, maxBlocks, (size_t)blockBase + (size_t)blockIdx.x * W + wave);
        if (ENG) { eV = acc.eV; eC = acc.eC; }
        dropped = acc.dropped;
    }
    // (the reductions are ~14 vector instructions each: skipped where the sum is known to be zero)
    if (ENG) eV = wave_sum(eV);
    if (ENG && !pair_mode_one_species(MODE)) eC = wave_sum(eC);
    if (__any(dropped != 0.0)) dropped = wave_sum(dropped);
    // every wave books into its own partial-sum slot (fixed order of the final sums whatever W is)
    const size_t pb = (size_t)blockBase + (size_t)blockIdx.x * W + wave;
    if (lane == 0)
    {
        if (ENG)
        {
            partials[(size_t)PS_EVDW * maxBlocks + pb] = eV;
            partials[(size_t)PS_ECOUL * maxBlocks + pb] = eC;
        }
        if (dropped != 0.0) partials[(size_t)PS_DROPPED * maxBlocks + pb] += dropped;
    }
    if (ENG && P.fuseKick == KICK_SECOND)
    {
        eK = wave_sum(eK);
        if (lane == 0) partials[(size_t)PS_EKIN * maxBlocks + pb] = 0.5 * eK;
    }
    if (N.xn)
    {
        next_step_finish(P, N, nacc, partials, maxBlocks, pb);
        // the step counter of the step being opened (main.cpp:92), and: its second half-kick is NOT owed to the next k_integrate1_bin
        if (blockIdx.x == 0 && threadIdx.x == 0) { N.st->step += 1; N.st->pendingKick = 0; }
    }
    else if (N.pendingAfter >= 0 && blockIdx.x == 0 && threadIdx.x == 0) N.st->pendingKick = N.pendingAfter;
    if (P.fuseKick == KICK_DRIFT && threadIdx.x == 0)
    {   // what k_drift_plain2 does per launch and per workgroup: the step counter of the step being opened, its PS_EFIELD partials
        if (blockIdx.x == 0) N.st->step += 1;
        for (int b = blockIdx.x; b < N.driftBlocks; b += gridDim.x) partials[(size_t)PS_EFIELD * maxBlocks + b] = 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// k_build_lists: the step that rebuilds the cells makes the lists (geometry only - independent of the potential set; no forces: k_pair_list
// computes that step's forces like any other's, so a run has ONE force kernel and one summation order).  Everything here is f32: the lists only
// have to be a SUPERSET of the pairs within rc + skin (k_pair_list applies the exact fp64 cut-off test every step), and the sort leaves every atom's
// position relative to the centre of its own cell as one float4 (PairLists::rel) - so a neighbour's position relative to THIS cell's centre is that
// plus a whole number of cell edges, whatever the periodic wrap: no image shifts, no fp64, one 16-byte load per candidate.  Per cell, one wave:
//   1. the z-runs of the stencil are looked up by the lanes in parallel; the loads of up to eight runs travel together (a wave's life is two memory
//      round trips and the arithmetic);
//   2. candidates are pruned against the box of the cell's atoms and packed ("staged") into LDS with wave ballot + popcount prefix, together with their
//      list entries (atom index + image code, which k_pair_list needs for its fp64 gather);
//   3. per group of 16 atoms of the cell ONE v_mfma_f32_16x16x4_f32 per 16 candidates tests 256 pairs against the list radius
//      (D = thr - |ri - rj|^2 with a threshold widened by the f32 error bound: conservative);
//   4. every lane pops its hits (staged candidate numbers) into its atom's stretch of a compact per-cell array, and the hit masks are ORed over the
//      cell's atoms;
//   5. only the candidates that some atom of the cell hit are KEPT (the dilated box holds ~30 % more than the union of the atoms' spheres): they
//      are renumbered in tile order - so the gathers of k_pair_list stay runs of consecutive atoms and every atom's hit sequence is what it was -
//      and leave as the cell's candidate list, T = the kept count;
//   6. every lane of k_pair_list's layout (lane = atom * NS + slice) reads ITS entries out of the hit array (entry slice + t NS of its atom), maps
//      them to the kept candidates' records, and the list leaves as whole 1 KiB chunks.
// A cell whose staged candidates exceed the staging area (PairLists::stageLds), whose kept ones exceed the tile of k_pair_list (candLds), whose lists
// exceed iterCap or that holds more than 64 atoms per wave keeps no list (header -1): the clean-up launch of k_pair_tile stages it on every step, and
// the engine grows the capacities when that happens.  A cell whose atoms reach nobody keeps a list with T = 0: k_pair_list writes its forces as zero.
// ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kBuildEntRegsBeside = 8;     // ... 512 with DBG_HITS_BESIDE_TILE, as that layout always had
constexpr int kBuildEntRegs = 12;          // k_build_lists: list entries of up to 768 staged candidates wait in registers while the filter runs
struct BuildLds
{
    int capS;            // floats per coordinate array: stageLds rounded up to whole mask words (the matrix filter reads 8 blocks of 16 candidates at a time)
    int nWords;          // 32-bit hit-mask words per lane and atom group: capS / 128
    int hitCap;          // entries of the compact hit array: iterLds x 64 x waves per cell
    int nTab;            // entries of each of the three small tables (staging table: <= 64 runs ; per atom of the cell: <= 64 x waves)
    int groups;          // groups of 16 atoms whose hit masks are parked (PairLists::buildGroups); 0: one in flight, and the hit array beside the tile
    __host__ __device__ BuildLds(int stageLds, int iterLds, int waves, int buildGroups)
        : capS((stageLds + 127) & ~127), nWords((stageLds + 127) / 128), hitCap(iterLds * kWave * waves), nTab(kWave * waves), groups(buildGroups) {}
    // LDS per wave bounds the builder's occupancy (a chain of dependent LDS round trips: its time goes as 1 / waves per CU), so nothing lives longer than it
    // must.  The TILE serves the matrix filter and nothing else: every group's filter runs before the first hit is popped, the groups' hit masks wait in the
    // mask buffer, and the compact hit array then takes the tile's bytes - behind the first 2 capS of them, where the keep pass writes the renumbering while
    // the hit array is live.  The staged candidates' list ENTRIES outlive the filter (only then is it known who is kept).  Up to kBuildEntRegs x 64 staged
    // candidates they wait in registers meanwhile, and their place in LDS is the mask buffer's (a liquid's cells); larger staging areas keep both.
    //   front:  tile 16 capS  |  renumbering 2 capS, hit array 2 hitCap        (whichever is larger)
    //   middle: entries 4 capS  |  masks 256 nWords groups                      (entries in registers: whichever is larger ; else both)
    //   tables: 3 x 4 nTab
    // groups == 0 (DBG_HITS_BESIDE_TILE), the layout this one replaced: tile, entries | hit array (in registers: whichever is larger ; else both), the masks of
    // the one group in flight, tables
    __host__ __device__ bool ent_in_regs() const { return capS <= (beside() ? kBuildEntRegsBeside : kBuildEntRegs) * kWave; }
    __host__ __device__ bool beside() const { return groups == 0; }
    __host__ __device__ size_t tile_bytes() const { return sizeof(float) * 4 * (size_t)capS; }
    __host__ __device__ size_t ent_bytes() const { return sizeof(uint32_t) * (size_t)capS; }
    __host__ __device__ size_t hit_bytes() const { return (sizeof(uint16_t) * (size_t)hitCap + 15) & ~(size_t)15; }
    __host__ __device__ size_t remap_bytes() const { return sizeof(uint16_t) * (size_t)capS; }                  // (capS is a multiple of 128: 16-byte aligned)
    __host__ __device__ size_t mask_bytes() const { return sizeof(uint32_t) * (size_t)nWords * kWave * (size_t)(groups > 0 ? groups : 1); }
    __host__ __device__ size_t ent_off() const { return beside() || tile_bytes() > remap_bytes() + hit_bytes() ? tile_bytes() : remap_bytes() + hit_bytes(); }
    __host__ __device__ size_t hit_off() const { return !beside() ? remap_bytes() : ent_in_regs() ? ent_off() : ent_off() + ent_bytes(); }
    __host__ __device__ size_t mask_off() const
    {
        if (!beside()) return ent_in_regs() ? ent_off() : ent_off() + ent_bytes();
        return ent_off() + (ent_in_regs() ? (ent_bytes() > hit_bytes() ? ent_bytes() : hit_bytes()) : ent_bytes() + hit_bytes());
    }
    __host__ __device__ size_t tab_off() const
    {
        if (!beside() && ent_in_regs()) return ent_off() + (ent_bytes() > mask_bytes() ? ent_bytes() : mask_bytes());
        return mask_off() + mask_bytes();
    }
    __host__ __device__ size_t bytes() const { return tab_off() + sizeof(int32_t) * 3 * (size_t)nTab; }
};

__global__ __launch_bounds__(kWave) void k_build_lists(StepParams P, const int32_t* __restrict__ cellStart, int firstCell, int nCellsRun, PairLists L)
{
    extern __shared__ float ldsBuild[];
    const int W = L.waves;
    const BuildLds G(L.stageLds, L.iterLds, W, L.buildGroups);
    char* const lds = (char*)ldsBuild;
    float4* const tile = (float4*)ldsBuild;                         // {x, y, z, -(x^2 + y^2 + z^2)} of every staged candidate, relative to the cell centre: one 16-byte store each;
                                                                    // lane (row c, component k) of the matrix operand reads float 4 (16 b + perm(c)) + k: 64 different banks
    uint16_t* const remap = (uint16_t*)ldsBuild;                    // ... and, once the filter has run: staged candidate number -> list entry of its record in k_pair_list's tile
    uint32_t* const tent = (uint32_t*)(lds + G.ent_off());          // list entries of the staged candidates (atom index | image code << 26), tile order ...
    const bool entInRegs = G.ent_in_regs();                         // ... which wait in registers while the filter runs, if they are few enough (BuildLds)
    const bool beside = G.beside();                                 // (DBG_HITS_BESIDE_TILE)
    uint16_t* const hits = (uint16_t*)(lds + G.hit_off());          // the compact hit array (staged candidate numbers, atom by atom): in the tile's bytes once every group's filter has run
    uint32_t* const maskBuf = (uint32_t*)(lds + G.mask_off());      // [groups][nWords][64] hit masks of the cell's atom groups
    int32_t* const entJ = (int32_t*)(lds + G.tab_off());            // staging table: first atom, count (<= 64), codes ; later, per atom of the cell:
    int32_t* const entN = entJ + G.nTab;                            //   tile slot, then hit counts of its quarters / offset / hit count
    int32_t* const entC = entN + G.nTab;

    const int lane = threadIdx.x;
    const int per = (nCellsRun + 7) >> 3;
    const int cr = (blockIdx.x & 7) * per + (blockIdx.x >> 3);       // the mapping of k_pair_list: a cell is built and walked on the same XCD
    if (blockIdx.x == 0 && lane == 0) atomicAdd(&L.noList[LR_RECORDED], nCellsRun);      // cells recorded (one atomic per launch)
    if (cr >= nCellsRun) return;
    const int cell = firstCell + cr;
    const int ncy = P.nc[1], ncz = P.nc[2];
    const int cxyz = L.meta[4 * cell + 1];
    const int lx = cxyz & 1023, cy = (cxyz >> 10) & 1023, cz = (cxyz >> 20) & 1023;
    const int ib = cellStart[cell], ie = cellStart[cell + 1];
    const int nthis = ie - ib;
    if (nthis == 0) { if (lane == 0) L.meta[4 * cell] = 0; return; }            // an empty cell: a list with nothing in it
    auto no_list = [&](int why) { if (lane == 0) { L.meta[4 * cell] = -1; atomicAdd(&L.noList[LR_UNLISTED], 1); atomicAdd(&L.noList[LR_UNLISTED_NOW], 1); if (why != LR_NONE) atomicAdd(&L.noList[why], 1); } };
    auto report_atoms = [&]() { if (lane == 0 && nthis > L.noList[LR_MAX_ATOMS]) atomicMax(&L.noList[LR_MAX_ATOMS], nthis); };
    if (nthis > kWave * W) { report_atoms(); no_list(LR_NONE); return; }      // (W waves of k_pair_list share the cell: up to 64 atoms each)
    // (more groups of 16 atoms than the mask buffer holds: no list this time - the clean-up launch serves the cell -, and the engine sizes the buffer from the
    //  largest cell reported at its next look)
    if (!beside && nthis > 16 * G.groups) { report_atoms(); no_list(LR_MASK_FULL); return; }
    const int RECB = L.entryScale;                                  // record number -> list entry (k_pair_list's mode decides: byte offset or number)
    const int stageLds = L.stageLds;
    const float cs0 = (float)P.csz[0], cs1 = (float)P.csz[1], cs2 = (float)P.csz[2];
    // f32 pruning radius: the list radius + what rounding can do to a coordinate (an atom's own-cell offset is rounded to f32, |x| < a few cell edges:
    // 2^-22 relative on the square is far more than that)
    const float pruneF = (float)(P.pruneR2 * (1.0 + 1e-5));
    // The candidates are pruned against the bounding box of the cell's ATOMS, not against the cell: a dozen atoms leave on average an eighth of the cell's
    // edge empty on either side, and the box dilated by the list radius holds 15 % fewer candidates (C4: 299 -> 255) - less to filter here.  Conservative: an
    // atom farther than the list radius from the box is farther than that from every atom inside it.  (What k_pair_list gathers is smaller still: only
    // the staged candidates that the filter finds within the list radius of some atom of the cell are kept, below.)
    float bc0, bc1, bc2, bh0, bh1, bh2;
    {
        float lo0 = 3e38f, lo1 = 3e38f, lo2 = 3e38f, hi0 = -3e38f, hi1 = -3e38f, hi2 = -3e38f;
        for (int a = lane; a < nthis; a += kWave)
        {
            const float4 m = L.rel[ib + a];
            lo0 = fminf(lo0, m.x); hi0 = fmaxf(hi0, m.x); lo1 = fminf(lo1, m.y); hi1 = fmaxf(hi1, m.y); lo2 = fminf(lo2, m.z); hi2 = fmaxf(hi2, m.z);
        }
#pragma unroll
        for (int o = kWave >> 1; o >= 1; o >>= 1)
        {
            lo0 = fminf(lo0, __shfl_xor(lo0, o, kWave)); hi0 = fmaxf(hi0, __shfl_xor(hi0, o, kWave));
            lo1 = fminf(lo1, __shfl_xor(lo1, o, kWave)); hi1 = fmaxf(hi1, __shfl_xor(hi1, o, kWave));
            lo2 = fminf(lo2, __shfl_xor(lo2, o, kWave)); hi2 = fmaxf(hi2, __shfl_xor(hi2, o, kWave));
        }
        // (half-widths rounded up by more than the f32 error of centre and difference)
        bc0 = 0.5f * (lo0 + hi0); bh0 = 0.5f * (hi0 - lo0) * 1.000001f + 1e-5f;
        bc1 = 0.5f * (lo1 + hi1); bh1 = 0.5f * (hi1 - lo1) * 1.000001f + 1e-5f;
        bc2 = 0.5f * (lo2 + hi2); bh2 = 0.5f * (hi2 - lo2) * 1.000001f + 1e-5f;
    }

    // ---- staging: all z-runs are looked up by the lanes in parallel, packed into a table, loaded eight at a time
    int T = 0;
    bool overflow = false;
    const int nSegTot = P.nOff[0] * P.nOff[1] * 3;
    const int rcpOff1 = 65536 / P.nOff[1] + 1;
    for (int sg0 = 0; sg0 < nSegTot && !overflow; sg0 += kWave)
    {
        int rjb = 0, rn = 0, rcode = 0;
        {
            const int sg = sg0 + lane;
            const int col = (sg * 21846) >> 16, seg = sg - 3 * col;
            const int ox = (col * rcpOff1) >> 16, oy = col - ox * P.nOff[1];
            int nx = lx + ox - P.hw[0], cxs = 1;                      // image codes (for k_pair_list's fp64 gather): 0 -> -L, 1 -> 0, 2 -> +L
            if (P.nranks > 1)
            {   // slab window: ghost layers are resident; their coordinates are global, so k_pair_list shifts across the seam
                const int gx = nx + P.cx0;
                if (gx < 0) cxs = 0; else if (gx >= P.nc[0]) cxs = 2;
            }
            else if (nx < 0) { nx += P.nc[0]; cxs = 0; }
            else if (nx >= P.nc[0]) { nx -= P.nc[0]; cxs = 2; }
            int ny = cy + oy - P.hw[1], cys = 1;
            if (ny < 0) { ny += ncy; cys = 0; } else if (ny >= ncy) { ny -= ncy; cys = 2; }
            const int zlo = cz - P.hw[2], zhi = cz + P.hw[2];
            int zs, ze, czs = 1;
            bool have = sg < nSegTot;
            if (seg == 0) { zs = max(zlo, 0); ze = min(zhi, ncz - 1); }
            else if (seg == 1) { have = have && zlo < 0; zs = zlo + ncz; ze = ncz - 1; czs = 0; }
            else { have = have && zhi >= ncz; zs = 0; ze = zhi - ncz; czs = 2; }
            if (have)
            {
                const int colBase = (nx * ncy + ny) * ncz;
                rjb = cellStart[colBase + zs];
                rn = cellStart[colBase + ze + 1] - rjb;
                // image code (6 bits) | x offset of the column in cells + 32 (6 bits) | y offset + 32 (6 bits)
                rcode = cxs | (cys << 2) | (czs << 4) | ((ox - P.hw[0] + 32) << 6) | ((oy - P.hw[1] + 32) << 12);
            }
        }
        while (__any(rn > 0) && !overflow)
        {
            const unsigned long long emask = __ballot(rn > 0);
            const int nEnt = __popcll(emask);
            if (rn > 0)
            {
                const int pe = lanes_below(emask);
                entJ[pe] = rjb; entN[pe] = min(rn, kWave); entC[pe] = rcode;
                rjb += kWave; rn -= kWave;
            }
            __builtin_amdgcn_wave_barrier();
            for (int e = 0; e < nEnt && !overflow; e += 8)
            {
                const int le = min(e + (lane & 7), nEnt - 1);
                const int vj = entJ[le], vn = entN[le], vc = entC[le];
                float4 g[8];
                int gjn[8];
#pragma unroll
                for (int u = 0; u < 8; u++)
                {
                    const int j = __builtin_amdgcn_readlane(vj, u) + lane;
                    gjn[u] = (e + u < nEnt) ? __builtin_amdgcn_readlane(vn, u) : 0;
                    g[u] = L.rel[j];                                   // (unconditional: the array is padded by a wave's width, lanes beyond the run are dropped below)
                }
#pragma unroll
                for (int u = 0; u < 8; u++)
                {
                    if (gjn[u] > 0 && !overflow)
                    {
                        const int code = __builtin_amdgcn_readlane(vc, u);
                        const float offx = (float)(((code >> 6) & 63) - 32) * cs0, offy = (float)(((code >> 12) & 63) - 32) * cs1;
                        const float dzc = (float)((((code >> 4) & 3) - 1) * ncz - cz);          // cells along z between the candidate's cell (its own index rides in .w) and this one
                        const float xf = g[u].x + offx, yf = g[u].y + offy, zf = fmaf(g[u].w + dzc, cs2, g[u].z);
                        // distance from the box of the cell's atoms: atoms farther than the list radius cannot be anybody's partner
                        const float bx = fmaxf(fabsf(xf - bc0) - bh0, 0.0f), by = fmaxf(fabsf(yf - bc1) - bh1, 0.0f), bz = fmaxf(fabsf(zf - bc2) - bh2, 0.0f);
                        const bool keep = (lane < gjn[u]) && (bx * bx + by * by + bz * bz) <= pruneF;
                        const unsigned long long mask = __ballot(keep);
                        const int nk = __popcll(mask);
                        if (T + nk > stageLds) { overflow = true; }
                        else
                        {
                            if (keep)
                            {
                                const int pp = T + lanes_below(mask);
                                tile[pp] = make_float4(xf, yf, zf, -(xf * xf + yf * yf + zf * zf));
                                tent[pp] = (uint32_t)(__builtin_amdgcn_readlane(vj, u) + lane) | ((uint32_t)(code & 63) << 26);
                            }
                            T += nk;
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (overflow) { no_list(LR_TILE_FULL); return; }
    if ((P.debugMask & DBG_BUILD_PHASE_MASK) == 1) return;                                 // (phase timing: staging only)

    // far-away, finite dummies behind the last candidate up to the end of its mask word: the filter reads whole words of 8 x 16 candidates, without guards
    for (int q = T + lane; q < ((T + 127) & ~127); q += kWave) tile[q] = make_float4(-1e18f, 0.0f, 0.0f, -3e38f);
    // where the cell's own atoms sit in the tile (they are candidates too, unshifted): found by their list entries
    for (int q = lane; q < T; q += kWave)
    {
        const uint32_t en = tent[q];
        const int rel = (int)(en & 0x3FFFFFFu) - ib;
        if ((en >> 26) == 0x15u && rel >= 0 && rel < nthis) entJ[rel] = q;
    }
    uint32_t te[kBuildEntRegs];                                     // entries of the staged candidates 64 u + lane
#pragma unroll
    for (int u = 0; u < kBuildEntRegs; u++) te[u] = (entInRegs && u * kWave < T) ? tent[u * kWave + lane] : 0u;
    __builtin_amdgcn_wave_barrier();                                // (from here on the entries' place may hold the hit array)
    // hit masks ORed over all atoms of the cell: the word of (mask word wd, quarter kq) - candidate 128 wd + kq + 4 p at bit 31 - p - is kept by lane 16 kq + wd
    // (at most 15 mask words: 1 920 candidates)
    uint32_t keepAcc = 0u;

    // ---- filter + compaction, one group of 16 atoms at a time.  Matrix operand maps (gfx950, v_mfma_f32_16x16x4_f32): A[row l & 15][k l >> 4],
    // B[k l >> 4][col l & 15], C/D[row 4 (l >> 4) + reg][col l & 15].  Rows are fed in the order perm(c) = (c >> 2) + 4 (c & 3), which makes register r
    // of lane (atom l & 15, quarter kq = l >> 4) the candidate 16 b + kq + 4 r of block b; the -|rj|^2 of those four arrive as the C operand.
    const double h0 = 0.5 * P.csz[0], h1 = 0.5 * P.csz[1], h2 = 0.5 * P.csz[2];
    const double rList = sqrt(P.pruneR2);
    const double ext2 = (h0 + rList) * (h0 + rList) + (h1 + rList) * (h1 + rList) + (h2 + rList) * (h2 + rList);
    const float thrList = (float)(P.pruneR2 + 1.9073486328125e-06 * (4.0 * ext2 + P.pruneR2));       // list radius^2 + 2^-19 x a bound of the f32 error
    const int aw = list_atoms_per_wave(nthis, W);                   // k_pair_list: wave w serves atoms [w aw, w aw + aw), lane = (atom - w aw) * NS + slice
    const int NS = list_slices(aw);
    const int rcpNS = 65536 / NS + 1;
    const int nBlk = (T + 15) >> 4;
    const int nW = (nBlk + 7) >> 3;
    const int c16 = lane & 15, kq = lane >> 4;
    const int permc = (c16 >> 2) + ((c16 & 3) << 2);
    // A[cand][k] = (xj, yj, zj, -|rj|^2), B[k][atom] = (2 xi, 2 yi, 2 zi, 1), C[cand][atom] = thr - |ri|^2 (the same in a lane's four registers, for every block):
    // the per-candidate term rides in the A operand, so a block costs ONE LDS read per lane and no operand selects
    const float* const pa = (const float*)tile + 4 * permc + kq;
    int nIter = 0, hitBase = 0, tooLong = 0;
    // one group's matrix filter: its hit masks go to mb, its atoms' offsets and counts to the tables; returns where this lane's hits go in the hit array
    auto filter_group = [&](int g0, uint32_t* mb) -> int
    {
        const int a = g0 + c16;
        const bool validA = a < nthis;
        // idle atom slots sit at 1e18: their column of the filter is hugely negative ("outside") whatever the candidate
        float4 me = make_float4(1e18f, 1e18f, 1e18f, 0.f);
        if (validA) me = L.rel[ib + a];
        const float fB = (kq == 0) ? 2.0f * me.x : (kq == 1) ? 2.0f * me.y : (kq == 2) ? 2.0f * me.z : 1.0f;
        const float cAtom = thrList - (me.x * me.x + me.y * me.y + me.z * me.z);
        const float4_t cw = {cAtom, cAtom, cAtom, cAtom};
        const int kSelf = validA ? entJ[a] : -1;
        int h = 0;
        for (int wd = 0; wd < nW; wd++)
        {
            // all operands of the word's eight blocks first (the tile is padded with dummies to the end of the word), then the eight matrix instructions,
            // then the sign bits: no guards, so the reads of one block do not wait for the arithmetic of the one before
            float av[8];
#pragma unroll
            for (int q = 0; q < 8; q++) av[q] = pa[(8 * wd + q) * 64];
            uint32_t miss = 0u;                                      // one bit per candidate of the lane, 1 = outside; newest candidate in bit 0
#pragma unroll
            for (int q = 0; q < 8; q++)
            {
                const float4_t d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], fB, cw, 0, 0, 0);
                miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(d[0]), 31);
                miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(d[1]), 31);
                miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(d[2]), 31);
                miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(d[3]), 31);
            }
            // candidate number p of this word (p = 4 (block & 7) + r) sits at bit 31 - p; the dummies behind the last candidate are misses
            uint32_t m = ~miss;
            // the atom itself is a candidate of its own tile (always a hit): not a partner
            if (kSelf >= 0 && (kSelf & 3) == kq && (kSelf >> 7) == wd) m &= ~(0x80000000u >> ((kSelf & 127) >> 2));
            mb[wd * kWave + lane] = m;
            h += __popc(m);
            // who is hit by anybody: OR over the 16 atoms of the group (the lanes of one kq are one DPP row: four rotations), then into the cell's keep word
            uint32_t any = m;
            any |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)any, 0x128, 0xF, 0xF, false);      // row_ror:8
            any |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)any, 0x124, 0xF, 0xF, false);      // row_ror:4
            any |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)any, 0x122, 0xF, 0xF, false);      // row_ror:2
            any |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)any, 0x121, 0xF, 0xF, false);      // row_ror:1
            if (c16 == wd) keepAcc |= any;
        }
        // where this lane's hits go: behind those of the lower quarters of its atom, which come behind the atoms before it
        int below = 0, total = 0, quarters = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
        {
            const int hq = __shfl(h, c16 | (q << 4), kWave);
            below += (q < kq) ? hq : 0;
            total += hq;
            if (q < 3) quarters |= hq << (10 * q);                   // (a quarter holds at most 32 candidates per mask word, 15 words: 480)
        }
        if (!validA) total = 0;
        int incl = total;                                            // inclusive scan over the 16 atoms of the group (every quarter computes the same)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { const int up = __shfl_up(incl, o, 16); if (c16 >= o) incl += up; }
        const int myOff = hitBase + incl - total;
        hitBase += __shfl(incl, 15, 16);
        // (the atom's tile slot has served - every quarter read it above -: its place keeps the quarters' hit counts for the pop that comes after every group's filter)
        if (validA && kq == 0) { entJ[a] = quarters; entN[a] = myOff; entC[a] = total; }
        nIter = max(nIter, ((total + NS - 1) * rcpNS) >> 16);
        if (hitBase > G.hitCap) tooLong = 1;                         // (wave-uniform)
        return myOff + below;
    };
    // ... and its compaction: every lane pops its hits, in the order quarter, word, bit.  Bit 31 - p of word wd is the staged candidate 128 wd + kq + 4 p
    auto pop_group = [&](const uint32_t* mb, int at)
    {
        uint16_t* dst = hits + at;
        for (int wd = 0; wd < nW; wd++)
        {
            uint32_t cur = mb[wd * kWave + lane];
            const int base = 128 * wd + kq;
            while (cur != 0u)
            {
                const int p = __clz(cur);
                cur &= ~(0x80000000u >> p);
                *dst++ = (uint16_t)(base + p * 4);
            }
        }
    };
    const bool compact = (P.debugMask & DBG_BUILD_PHASE_MASK) != 2;                        // (phase timing: no compaction)
    if (beside)
    {   // (DBG_HITS_BESIDE_TILE) group by group: the hit array lives beside the tile
        for (int g0 = 0; g0 < nthis && !tooLong; g0 += 16)
        {
            const int at = filter_group(g0, maskBuf);
            if (!tooLong && compact) pop_group(maskBuf, at);
            __builtin_amdgcn_wave_barrier();
        }
    }
    else
    {
        const int groupWords = G.nWords * kWave;
        uint32_t* mb = maskBuf;
        for (int g0 = 0; g0 < nthis && !tooLong; g0 += 16, mb += groupWords) filter_group(g0, mb);
        __builtin_amdgcn_wave_barrier();                            // (the tile has served: its place takes the hit array)
        if (!tooLong && compact)
        {
            mb = maskBuf;
            for (int g0 = 0; g0 < nthis; g0 += 16, mb += groupWords)
            {
                const int a = g0 + c16;
                int at = 0;
                if (a < nthis)
                {   // (idle atom slots hit nobody)
                    const int quarters = entJ[a];
                    at = entN[a] + (kq > 0 ? quarters & 1023 : 0) + (kq > 1 ? (quarters >> 10) & 1023 : 0) + (kq > 2 ? quarters >> 20 : 0);
                }
                pop_group(mb, at);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if ((P.debugMask & DBG_BUILD_PHASE_MASK) >= 2) return;                                 // (phase timing: no read-out)
    nIter = wave_max_int(nIter);
    // (DBG_SHORT_LISTS, tests: lists hold 14 iterations only - part of a liquid's cells then keep no list and go through the clean-up launch)
    bool usable = !tooLong && nIter <= ((P.debugMask & DBG_SHORT_LISTS) ? 14 : L.iterCap);
    // ---- the candidates some atom of the cell reaches are kept, in tile order: kept candidate n sits in record n + 1 of k_pair_list's tile.  They are
    // written out in whole groups of 64 (k_pair_list gathers whole groups: the last one is filled with a valid atom, the cell's first)
    int kept = 0;
    if (usable)
    {
        __builtin_amdgcn_wave_barrier();                            // (the tile has served: its place takes the renumbering)
        uint32_t* const myList = L.cand + (size_t)cell * L.candCap;
        auto keep_chunk = [&](int q0, uint32_t entry) {
            const int q = q0 + lane;
            const uint32_t kw = (uint32_t)__shfl((int)keepAcc, ((q & 3) << 4) | (q >> 7), kWave);
            const bool keep = q < T && ((kw << ((q & 127) >> 2)) & 0x80000000u) != 0u;
            const unsigned long long mask = __ballot(keep);
            if (keep)
            {
                const int n = kept + lanes_below(mask);
                remap[q] = (uint16_t)((n + 1) * RECB);
                myList[n] = entry;
            }
            kept += __popcll(mask);
        };
        if (entInRegs)
        {
#pragma unroll
            for (int u = 0; u < kBuildEntRegs; u++) if (u * kWave < T) keep_chunk(u * kWave, te[u]);
        }
        else
            for (int q0 = 0; q0 < T; q0 += kWave) keep_chunk(q0, tent[min(q0 + lane, T - 1)]);
        const int Tpad = max((kept + kWave - 1) & ~(kWave - 1), list_preload(L.candLds) * W * kWave);      // (k_pair_list gathers that many groups per wave whatever T is)
        for (int q = kept + lane; q < Tpad; q += kWave) myList[q] = (uint32_t)ib | (0x15u << 26);
        __builtin_amdgcn_wave_barrier();
    }
    // (staged, filtered, and still too many for the walk's tile - or, with one-byte entries, for a record number: served by the clean-up launch until the tile
    //  has grown, or the engine has gone back to 16-bit entries)
    const bool narrow = L.entryBytes == 1;
    const bool keptFull = usable && (kept > L.candLds || (narrow && kept > 255));
    if (keptFull) usable = false;
    if (usable)
    {   // every lane of k_pair_list's layout collects ITS entries: lane = slot * NS + slice of wave w walks entries slice, slice + NS, ... of atom w aw + slot;
        // 0 = no candidate
        const int slot = (lane * rcpNS) >> 16, slice = lane - slot * NS;
        for (int w = 0; w < W; w++)
        {
            const int atom = w * aw + slot;
            int off = 0, cnt = 0;
            if (slot < aw && atom < nthis) { off = entN[atom]; cnt = entC[atom]; }
            const uint16_t* const src = hits + off;
            uint4* const out = (uint4*)(L.pairs + ((size_t)cell * W + w) * L.iterCap * kWave) + lane;
            if (narrow)
            {   // record numbers (entryScale is 1: remap holds n + 1 <= 255), sixteen iterations per lane and chunk
                for (int c = 0; c * 16 < nIter; c++)
                {
                    uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int u = 0; u < 16; u++)
                    {
                        const int e = (c * 16 + u) * NS + slice;
                        const uint32_t r = (e < cnt) ? (uint32_t)remap[src[e]] : 0u;
                        v[u >> 2] |= r << (8 * (u & 3));
                    }
                    out[c * kWave] = make_uint4(v[0], v[1], v[2], v[3]);
                }
                continue;
            }
            for (int c = 0; c * 8 < nIter; c++)
            {
                uint32_t v[8];
#pragma unroll
                for (int u = 0; u < 8; u++)
                {
                    const int e = (c * 8 + u) * NS + slice;
                    v[u] = (e < cnt) ? (uint32_t)remap[src[e]] : 0u;
                }
                out[c * kWave] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
            }
        }
    }
    if (lane == 0)
    {
        // header: candidates | iterations << 12 | slices per atom << 20 ; then the cell's first atom and atoms | (65536 / slices + 1) << 12 - all k_pair_list needs to
        // know about the cell arrives in one 16-byte scalar load
        L.meta[4 * cell] = usable ? (kept | (nIter << 12) | (NS << 20)) : -1;
        L.meta[4 * cell + 2] = ib;
        L.meta[4 * cell + 3] = nthis | (rcpNS << 12);
        if (T > L.noList[LR_MAX_STAGED]) atomicMax(&L.noList[LR_MAX_STAGED], T);       // (a read first: after the first few cells nobody has a new record to report)
        if (kept > L.noList[LR_MAX_TILE]) atomicMax(&L.noList[LR_MAX_TILE], kept);
        if (usable && nIter > L.noList[LR_MAX_ITERS]) atomicMax(&L.noList[LR_MAX_ITERS], nIter);
        if (nthis > L.noList[LR_MAX_ATOMS]) atomicMax(&L.noList[LR_MAX_ATOMS], nthis);
        if (P.debugMask & DBG_LIST_STATS)
        {   // measurement aid (slow)
            atomicAdd(&L.noList[LR_SUM_ITERS], nIter); atomicAdd(&L.noList[LR_SUM_CANDS], kept); atomicAdd(&L.noList[LR_SUM_ATOMS], nthis); atomicAdd(&L.noList[LR_SUM_STAGED], T);
            if (nIter > 16) atomicAdd(&L.noList[LR_OVER_16], 1);
        }
        if (!usable) { atomicAdd(&L.noList[LR_UNLISTED], 1); atomicAdd(&L.noList[LR_UNLISTED_NOW], 1); atomicAdd(&L.noList[keptFull ? LR_KEPT_FULL : LR_LIST_FULL], 1); }
    }
}

// the step that rebuilds the cells: candidates and pair lists of every cell (no forces; k_pair_list follows)
inline void launch_build_lists(const PairLaunch& C, PairRange R, PairLists L)
{
    pair_range_default(C.P, R);
    if (R.n == 0) return;
    const BuildLds G(L.stageLds, L.iterLds, L.waves, L.buildGroups);
    hipLaunchKernelGGL(k_build_lists, dim3(pair_range_grid(R.n)), dim3(kWave), G.bytes(), C.stream, C.P, C.cellStart, R.first, R.n, L);
}
inline size_t build_lists_lds_bytes(const PairLists& L) { return BuildLds(L.stageLds, L.iterLds, L.waves, L.buildGroups).bytes(); }

template <int MODE, int VDW>
inline void launch_pair_list_as(const PairLaunch& C, PairRange R, PairLists L, NextStep N, bool energies)
{
    const size_t lds = pair_list_lds_bytes(C.P, L);
    const dim3 grid(pair_range_grid(R.n)), block(kWave * L.waves);
    // thermostat-fused epilogue: modes that do not read radii (the thermostat rewrites them while other waves would still be gathering), never on a step
    // whose energies are wanted (Engine::launch_step_kernels)
    constexpr bool kCanFuseTstat = !pair_mode_reads_radii(MODE);
    const bool four = list_preload(L.candLds) == 4;                 // groups gathered up front: compiled in
    // one-byte entries: instantiated for one wave per cell and the four-group tile only (ListStore::narrow_fits holds the engine to that)
    const bool narrow = L.entryBytes == 1;
    if (narrow && (!four || L.waves != 1)) throw std::runtime_error("k_pair_list: one-byte list entries need one wave per cell and a tile of at most 256 records");
#define AZTOT_LAUNCH_LIST_PRE(E, M, T, G, B) hipLaunchKernelGGL((k_pair_list<MODE, VDW, E, M, T, G, B>), grid, block, lds, C.stream, C.P, C.S, C.pots, C.A, C.cellStart, R.first, R.n, C.partials, C.maxBlocks, C.cnt, R.blockBase, L, N)
#define AZTOT_LAUNCH_LIST(E, M, T) do { if (narrow) AZTOT_LAUNCH_LIST_PRE(E, false, T, 4, 1); else if (four) AZTOT_LAUNCH_LIST_PRE(E, M, T, 4, 2); else AZTOT_LAUNCH_LIST_PRE(E, M, T, kListPreload, 2); } while (0)
    if (N.photons)
    {
        if (energies || !kCanFuseTstat) throw std::runtime_error("k_pair_list: the thermostat cannot be fused into this launch");
        if (L.waves == 1) AZTOT_LAUNCH_LIST(false, false, kCanFuseTstat); else AZTOT_LAUNCH_LIST(false, true, kCanFuseTstat);
    }
    else if (L.waves == 1) { if (energies) AZTOT_LAUNCH_LIST(true, false, false); else AZTOT_LAUNCH_LIST(false, false, false); }
    else { if (energies) AZTOT_LAUNCH_LIST(true, true, false); else AZTOT_LAUNCH_LIST(false, true, false); }
#undef AZTOT_LAUNCH_LIST
#undef AZTOT_LAUNCH_LIST_PRE
}

// a plain step: the list kernel for every cell (launch_pair_list), then the clean-up launch of the staging kernel for the cells that keep no list
// (launch_pair_cleanup; it books into the partial-sum slots behind the list kernel's).  Each returns the number of partial-sum slots it uses.
inline int launch_pair_list(const PairLaunch& C, PairRange R, PairLists L, NextStep N = NextStep(), bool energies = true)
{
    pair_range_default(C.P, R);
    if (R.n == 0) return 0;
    AZTOT_PAIR_DISPATCH(C.P, launch_pair_list_as, C, R, L, N, energies);
    return pair_range_grid(R.n) * L.waves;
}

inline int launch_pair_cleanup(const PairLaunch& C, PairRange R, PairLists L, NextStep N = NextStep())
{
    pair_range_default(C.P, R);
    if (R.n == 0) return 0;
    R.blockBase += pair_range_grid(R.n) * L.waves;
    launch_pair_tile(C, R, L, 2, N);
    return pair_cleanup_grid(R.n);
}

}  // namespace aztot
