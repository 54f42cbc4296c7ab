// Coordination numbers (out_cn, out_md.cpp:389-504, and out_ncn, out_md.cpp:196-387) on the RDF sampler's kind of private cell grid.
//
//  reference                                   ours
//  ------------------------------------------  -------------------------------------------------------------------------------
//  out_cn / out_ncn: all N^2 (N^2 / 2) pairs    k_grid_bin + k_scan_* + k_grid_place (grid.hip.h): counting sort of the current positions into cells with an
//  on one host core after md_to_host            edge >= the largest radius; k_grid_slot_ids: the slot -> atom id map of that sort;
//                                               k_cn_pairs: full-neighbour walk (grid_walk), lanes = (atom, slice of the candidates), counters in registers,
//                                               slices folded with lane exchanges, one store per (atom, column), no atomics;
//                                               k_cn_range + k_cn_table: per-atom counts -> min / max and the uint64 table [cn][column] (integer atomics)
//
// A column is (central group, ligand group, R): groups are species (outCN) or nuclei (ncn).  Within one set-up a (central, ligand) pair names at most
// one column, so an atom of group g keeps one counter per ligand group that g is central to ("live" columns of g, at most kCnLive), and a partner of
// group h adds to counter slot[g][h].  Only engine state is READ; everything is integer, so the results do not depend on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>

#include "grid.hip.h"

namespace aztot {

constexpr int kCnMaxBlocks = 1024;          // k_cn_range / k_cn_table walk the atoms grid-stride
constexpr int kCnLdsBudget = 32768;         // bytes of LDS k_cn_table may take for its uint32 sub-table

// Pair walk: the lanes of SliceLane, the candidates of grid_walk (j == i among them: counted where C.countSelf).  NL: counters kept (>= C.maxLive).
//   slotOf[g * kSpecCap + h]: counter of an atom of group g for a partner of group h, -1: no such column;  r2Of: R * R of that column;
//   rowMax[g]: the largest R * R of g's columns (a cheap first test before the table is read), < 0: g is central to nothing
template <int NL>
__global__ __launch_bounds__(kBlock) void k_cn_pairs(RdfGrid G, CnParams C, int n, int sliceShift, const int32_t* __restrict__ cellStart,
                                                     const double* __restrict__ sx, const double* __restrict__ sy, const double* __restrict__ sz,
                                                     const int32_t* __restrict__ sKind, const int32_t* __restrict__ slotOf, const double* __restrict__ r2Of,
                                                     const double* __restrict__ rowMax, int32_t* __restrict__ counts)
{
    __shared__ int32_t sSlot[kSpecCap * kSpecCap];
    __shared__ double sR2[kSpecCap * kSpecCap];
    __shared__ double sRowMax[kSpecCap];
    for (int e = threadIdx.x; e < kSpecCap * kSpecCap; e += kBlock) { sSlot[e] = slotOf[e]; sR2[e] = r2Of[e]; }
    if (threadIdx.x < kSpecCap) sRowMax[threadIdx.x] = rowMax[threadIdx.x];
    __syncthreads();
    const SliceLane lane(sliceShift);
    const int i = lane.i;
    int cnt[NL];
#pragma unroll
    for (int k = 0; k < NL; k++) cnt[k] = 0;
    const int gi = i < n ? (sKind[i] >> C.shift) & 255 : 0;
    const double rmx = i < n ? sRowMax[gi] : -1.0;
    if (rmx >= 0.0)
    {
        const int32_t* rowSlot = sSlot + gi * kSpecCap;
        const double* rowR2 = sR2 + gi * kSpecCap;
        grid_walk(G, cellStart, lane, sx[i], sy[i], sz[i], sx, sy, sz, [&](int j, double, double, double, double r2, int (&acc)[NL]) {
            if (r2 <= rmx && (j != i || C.countSelf))
            {
                const int gj = (sKind[j] >> C.shift) & 255;
                const int k = rowSlot[gj];
                const double R2 = rowR2[gj];
                const bool hit = k >= 0 && (C.inclusive ? R2 >= r2 : r2 < R2);
#pragma unroll
                for (int q = 0; q < NL; q++) acc[q] += (hit && q == k) ? 1 : 0;
            }
        }, cnt);
    }
    slice_fold(cnt, lane.S);
    if (i < n && lane.slice == 0)
    {
#pragma unroll
        for (int q = 0; q < NL; q++)
            if (q < C.maxLive) counts[(size_t)i * C.maxLive + q] = cnt[q];
    }
}

// smallest and largest count over every (atom, live column): range[0] = min, range[1] = max (preset by the host to the reference's starting values)
__global__ __launch_bounds__(kBlock) void k_cn_range(CnParams C, int n, const int32_t* __restrict__ sKind, const int32_t* __restrict__ nLive,
                                                     const int32_t* __restrict__ counts, int32_t* __restrict__ range)
{
    int mn = 0x7fffffff, mx = -1;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
    {
        const int nl = nLive[(sKind[i] >> C.shift) & 255];
        for (int q = 0; q < nl; q++)
        {
            const int v = counts[(size_t)i * C.maxLive + q];
            mn = min(mn, v);
            mx = max(mx, v);
        }
    }
    for (int m = 1; m < 64; m <<= 1)
    {
        mn = min(mn, __shfl_xor(mn, m));
        mx = max(mx, __shfl_xor(mx, m));
    }
    if ((threadIdx.x & 63) == 0 && mx >= 0)
    {
        atomicMin(&range[0], mn);
        atomicMax(&range[1], mx);
    }
}

// table[(cn - cnMin) * nCols + column] += 1 for every (atom, live column); colOf[g * kCnLive + q]: the column of counter q of group g.
// useLds: a uint32 sub-table per workgroup (rows * nCols entries fit kCnLdsBudget), flushed once into the uint64 totals
__global__ __launch_bounds__(kBlock) void k_cn_table(CnParams C, int n, const int32_t* __restrict__ sKind, const int32_t* __restrict__ nLive,
                                                     const int32_t* __restrict__ colOf, const int32_t* __restrict__ counts, int cnMin, int rows, int useLds,
                                                     unsigned long long* __restrict__ table)
{
    extern __shared__ uint32_t cnLds[];
    const int nEnt = rows * C.nCols;
    if (useLds)
    {
        for (int e = threadIdx.x; e < nEnt; e += kBlock) cnLds[e] = 0u;
        __syncthreads();
    }
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
    {
        const int g = (sKind[i] >> C.shift) & 255;
        const int nl = nLive[g];
        for (int q = 0; q < nl; q++)
        {
            const int row = counts[(size_t)i * C.maxLive + q] - cnMin;
            if (row < 0 || row >= rows) continue;           // (cannot happen: the range was taken over the same counts)
            const int e = row * C.nCols + colOf[g * kCnLive + q];
            if (useLds) atomicAdd(&cnLds[e], 1u);
            else atomicAdd(&table[e], 1ull);
        }
    }
    if (!useLds) return;
    __syncthreads();
    for (int e = threadIdx.x; e < nEnt; e += kBlock)
        if (cnLds[e]) atomicAdd(&table[e], (unsigned long long)cnLds[e]);
}

}  // namespace aztot
