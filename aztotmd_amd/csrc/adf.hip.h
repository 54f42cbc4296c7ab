// Bond-angle distributions (aztot_adf_*, include/aztot.h) on the samplers' kind of private cell grid.  The reference has no such output: the directive is ours.
//
//  k_grid_bin + k_scan_* + k_grid_place (grid.hip.h) counting sort of the current positions into cells with an edge >= the largest radius
//  k_grid_slot_ids                                   the slot -> atom id map of that sort
//  k_adf_neigh                                       neighbours of every central atom (lanes = (atom, slice of the candidates), grid_walk) and the
//                                                    largest count with its atom id: the host sizes the tile from it and refuses a sample over the cap
//  k_adf_triplets                                    per central atom: its neighbours gathered into an LDS tile (u, r2, species, fp64), the pairs of the tile
//                                                    dealt to the atom's lanes, the bin by binary search over the edge table, uint32 sub-histogram in LDS
//                                                    flushed once per workgroup into the uint64 totals (or 64-bit global atomics where it does not fit)
//
// A column is (central species c, ligand species a <= b, R_a, R_b).  colOf[c][x][y] (symmetric in x, y) names the column of a neighbour pair of species
// x and y around c, -1: none.  Only engine state is READ; every total is an integer, so the results do not depend on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>

#include "grid.hip.h"

namespace aztot {

constexpr int kAdfMaxBins = 3600, kAdfMaxCols = 64, kAdfMaxNeigh = 256;    // AZTOT_ADF_MAX_* of include/aztot.h
constexpr int kAdfMaxBlocks = 1024;         // k_adf_triplets walks the atoms grid-stride: at most this many LDS histograms are flushed per sample ...
constexpr int kAdfAtomsPerFlush = 65536;    // ... unless a workgroup's share of the atoms would exceed this (see the overflow bound at k_adf_triplets)
constexpr int kAdfLdsBudget = 59392;        // bytes of dynamic LDS of k_adf_triplets, histogram and tiles together (58 KiB: with its 5.4 KiB of tables under 64 KiB)
constexpr int kAdfLdsComfort = 36864;       // what the lane rule keeps it under where it can (four workgroups per CU; adf_cost.py: beyond it the kernel slows by half)
constexpr int kAdfHistBudget = 20480;       // of which the uint32 sub-histogram may take this much (5120 cells); beyond it: 64-bit global atomics.  What is
                                            // left holds 4 tiles of 256 neighbours (one wave per atom) whatever the histogram
constexpr int kAdfTileBytes = 4 * 8 + 4;    // per neighbour: u_x u_y u_z r2 (fp64), species (int32)

// which neighbours an atom of species g keeps, and which column a pair of them belongs to
struct AdfTables
{
    double rowMax2[kSpecCap];                       // square of the largest radius of any column g is central to; < 0: central to nothing
    int32_t ligMask[kSpecCap];                      // bit h: species h is a ligand of a column g is central to
    double ra2[kAdfMaxCols], rb2[kAdfMaxCols];      // squares of the column's radii for its lower and its higher ligand species
};

// the tables live in device memory and are copied into LDS by every workgroup (they are indexed per lane)
__device__ __forceinline__ void adf_stage_tables(AdfTables& T, const AdfTables* __restrict__ tab)
{
    static_assert(sizeof(AdfTables) % sizeof(int32_t) == 0, "AdfTables is copied word by word");
    const int32_t* src = reinterpret_cast<const int32_t*>(tab);
    int32_t* dst = reinterpret_cast<int32_t*>(&T);
    for (int e = threadIdx.x; e < (int)(sizeof(AdfTables) / sizeof(int32_t)); e += kBlock) dst[e] = src[e];
}

// Neighbour count: the lanes of SliceLane, the candidates of grid_walk.  A neighbour of atom i (species g) is an atom j != i with 0 < r2 < rowMax2[g]
// (grid_sep's r2) whose species is in ligMask[g].  neigh[slot] = the count, -1 where g is central to nothing.
// *summary = max over the central atoms of (count << 32 | atom id)
__global__ __launch_bounds__(kBlock) void k_adf_neigh(RdfGrid G, const AdfTables* __restrict__ tab, int n, int sliceShift, const int32_t* __restrict__ cellStart,
                                                      const double* __restrict__ sx, const double* __restrict__ sy, const double* __restrict__ sz,
                                                      const int32_t* __restrict__ sKind, const int32_t* __restrict__ slotId, int32_t* __restrict__ neigh,
                                                      unsigned long long* __restrict__ summary)
{
    __shared__ AdfTables T;
    adf_stage_tables(T, tab);
    __syncthreads();
    const SliceLane lane(sliceShift);
    const int i = lane.i;
    const int gi = i < n ? sKind[i] & 255 : 0;
    const double rmx = i < n ? T.rowMax2[gi] : -1.0;
    int cnt = 0;
    if (rmx >= 0.0)
    {
        const int mask = T.ligMask[gi];
        grid_walk(G, cellStart, lane, sx[i], sy[i], sz[i], sx, sy, sz, [&](int j, double, double, double, double r2, int& acc) {
            acc += (j != i && r2 > 0.0 && r2 < rmx && ((mask >> (sKind[j] & 255)) & 1)) ? 1 : 0;
        }, cnt);
    }
    cnt = slice_fold(cnt, lane.S);
    const bool writer = i < n && lane.slice == 0;
    if (writer) neigh[i] = rmx >= 0.0 ? cnt : -1;
    // one max per wave
    unsigned long long top = writer && rmx >= 0.0 ? ((unsigned long long)cnt << 32) | (unsigned int)slotId[i] : 0ull;
    for (int m = 1; m < 64; m <<= 1)
    {
        const unsigned long long o = __shfl_xor(top, m);
        top = o > top ? o : top;
    }
    if ((threadIdx.x & 63) == 0 && top) atomicMax(summary, top);
}

// bin = #{ b in [1, nBins - 1] : s <= fl(edges[b] * p) }: the edges decrease and a rounded product is monotone, so the true b are a prefix
__device__ __forceinline__ int adf_bin(const double* __restrict__ edges, int nBins, double s, double p)
{
    int lo = 0, hi = nBins - 1;
    while (lo < hi)
    {
        const int mid = (lo + hi + 1) >> 1;
        if (s <= __dmul_rn(edges[mid], p)) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Triplet walk.  A workgroup serves kBlock >> laneShift central atoms at a time (slot order, grid-stride, the same number of rounds for every thread so that
// the barriers are uniform); an atom has G = 1 << laneShift lanes of one wave.  Per round:
//   1. the atom's lanes walk the neighbour cells and append every neighbour (the rule of k_adf_neigh) to the atom's tile: u, r2, species.  `cap` is the
//      largest count k_adf_neigh found in this very configuration, so the tile holds them all; a slot past it is never written;
//   2. the pairs j < k of the tile are dealt to the lanes, pair number lane, lane + G, ...; the column comes from colOf[c][species j][species k], the lower
//      ligand species is held to ra2 and the higher to rb2; the bin rule of include/aztot.h; one integer add.
// Dynamic LDS: tile doubles [groups][4][cap], then the uint32 sub-histogram [nBins][nCols] (useLds), then tile species [groups][cap].
// OVERFLOW BOUND of a uint32 cell between two flushes: an atom with n <= 256 neighbours adds at most n (n - 1) / 2 <= 32 640 to all cells together; the
// host sizes the grid so that a workgroup serves at most kAdfAtomsPerFlush + 64 atoms: (65 536 + 64) * 32 640 = 2 141 184 000 < 2^32.
__global__ __launch_bounds__(kBlock) void k_adf_triplets(RdfGrid G, const AdfTables* __restrict__ tab, int n, int laneShift, int cap, int nBins, int nCols, int useLds,
                                                         const int32_t* __restrict__ cellStart, const double* __restrict__ sx, const double* __restrict__ sy,
                                                         const double* __restrict__ sz, const int32_t* __restrict__ sKind, const int8_t* __restrict__ colOf,
                                                         const double* __restrict__ edges, unsigned long long* __restrict__ totals)
{
    extern __shared__ double adfLds[];
    __shared__ int8_t sCol[kSpecCap * kSpecCap * kSpecCap];
    __shared__ int sCount[kBlock / 4];      // (4 lanes per atom at the least)
    __shared__ AdfTables T;
    adf_stage_tables(T, tab);
    const int Gl = 1 << laneShift, groups = kBlock >> laneShift;
    const int nEnt = useLds ? nBins * nCols : 0;
    double* tile = adfLds;
    uint32_t* hist = reinterpret_cast<uint32_t*>(tile + (size_t)groups * 4 * cap);
    int32_t* tileSpec = reinterpret_cast<int32_t*>(hist + nEnt);
    for (int e = threadIdx.x; e < kSpecCap * kSpecCap * kSpecCap; e += kBlock) sCol[e] = colOf[e];
    for (int e = threadIdx.x; e < nEnt; e += kBlock) hist[e] = 0u;
    const int grp = threadIdx.x >> laneShift, lane = threadIdx.x & (Gl - 1);
    double* tu = tile + (size_t)grp * 4 * cap;          // [ux | uy | uz | r2][cap]
    int32_t* ts = tileSpec + (size_t)grp * cap;
    for (long long base = (long long)blockIdx.x * groups; base < n; base += (long long)gridDim.x * groups)
    {
        if (lane == 0) sCount[grp] = 0;
        __syncthreads();                                // (also: the tables and the zeroed histogram of the first round; the tile of the round before is free)
        const long long i = base + grp;
        const int gi = i < n ? sKind[i] & 255 : 0;
        const double rmx = i < n ? T.rowMax2[gi] : -1.0;
        if (rmx >= 0.0)
        {
            const double xi = sx[i], yi = sy[i], zi = sz[i];
            const int mask = T.ligMask[gi];
            grid_cells(G, cellStart, cell_coord(xi, G.icsz[0], G.nc[0]), cell_coord(yi, G.icsz[1], G.nc[1]), cell_coord(zi, G.icsz[2], G.nc[2]), [&](int s0, int s1) {
                for (int j = s0 + lane; j < s1; j += Gl)
                {
                    double ux, uy, uz;
                    const double r2 = grid_sep(G, xi, yi, zi, sx[j], sy[j], sz[j], ux, uy, uz);
                    const int gj = sKind[j] & 255;
                    if (j != i && r2 > 0.0 && r2 < rmx && ((mask >> gj) & 1))
                    {
                        const int q = atomicAdd(&sCount[grp], 1);
                        if (q < cap) { tu[q] = ux; tu[cap + q] = uy; tu[2 * cap + q] = uz; tu[3 * cap + q] = r2; ts[q] = gj; }
                    }
                }
            });
        }
        __syncthreads();
        const int m = min(sCount[grp], cap);
        if (rmx >= 0.0 && m >= 2)
        {
            const int8_t* col = sCol + gi * kSpecCap * kSpecCap;
            // pair number `lane` of the rows (0, 1..m-1), (1, 2..m-1), ...: step through the rows
            int j = 0, k = 1 + lane;
            while (j < m - 1 && k >= m) { j++; k = k - m + j + 1; }
            while (j < m - 1)
            {
                const int a = ts[j], b = ts[k];
                const int c = col[a * kSpecCap + b];
                if (c >= 0)
                {
                    const double rj2 = tu[3 * cap + j], rk2 = tu[3 * cap + k];
                    // the lower ligand species is held to R_a, the higher to R_b (equal where the species are)
                    const bool in = a <= b ? (rj2 < T.ra2[c] && rk2 < T.rb2[c]) : (rj2 < T.rb2[c] && rk2 < T.ra2[c]);
                    if (in)
                    {
                        const double dot = __dadd_rn(__dadd_rn(__dmul_rn(tu[j], tu[k]), __dmul_rn(tu[cap + j], tu[cap + k])), __dmul_rn(tu[2 * cap + j], tu[2 * cap + k]));
                        const double s = __dmul_rn(dot, fabs(dot)), p = __dmul_rn(rj2, rk2);
                        const int e = adf_bin(edges, nBins, s, p) * nCols + c;
                        if (useLds) atomicAdd(&hist[e], 1u);
                        else atomicAdd(&totals[e], 1ull);
                    }
                }
                k += Gl;
                while (j < m - 1 && k >= m) { j++; k = k - m + j + 1; }
            }
        }
    }
    if (!useLds) return;
    __syncthreads();
    for (int e = threadIdx.x; e < nEnt; e += kBlock)
        if (hist[e]) atomicAdd(&totals[e], (unsigned long long)hist[e]);
}

}  // namespace aztot
