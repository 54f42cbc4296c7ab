// Bond-orientational order (Steinhardt q_l and the neighbour-averaged q-bar_l of Lechner and Dellago; aztot_boo_*, include/aztot.h) on the samplers' kind of
// private cell grid.  The reference has no such output: the directive is ours.
//
//  k_boo_bin ... k_boo_place (grid.hip.h) the counting sort in its canonical order (Samplers::grid_fill_canonical), cells with an edge >= R: slot order is a
//                                        function of the state; positions, species and the slot -> id map in that order
//  k_boo_qlm<L>                          lanes = (atom, slice of the candidates), grid_walk; per bond one sqrt and one division, then the 2 (L + 1) sums
//                                        of T_L^m(z) (x + i y)^m in registers; slices folded with lane exchanges; q_lm and n_i by slot
//  k_boo_average<L>                      the same walk over the neighbours' q_lm by slot; q_l and q-bar_l by atom id
//  k_boo_hist                            bins of the per-atom values: a uint32 sub-histogram in LDS flushed into the uint64 totals
//  k_boo_chunks / k_boo_fold             the summation tree over atom ids (kernels.hip.h) over the per-atom values, per species
//
// Harmonics without an angle.  With the unit vector (x, y, z) of a bond, sin^m(theta) e^(i m phi) = (x + i y)^m, and T_l^m(z) = P_l^m(z) / sin^m(theta) is a
// polynomial in z: T_m^m = (-1)^m (2m - 1)!!, T_(m+1)^m = (2m + 1) z T_m^m, (l - m) T_l^m = (2l - 1) z T_(l-1)^m - (l + m - 1) T_(l-2)^m.  Nothing divides by
// sin(theta): a bond along z gives (x + i y)^m = 0 for m > 0 like any other number.  The sums are linear in the bonds, so the normalisation N_lm (host
// table, extended precision) is applied once per atom, after the fold.  Only engine state is READ; no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "grid.hip.h"

namespace aztot {

constexpr int kBooMaxL = 12, kBooMaxOrders = 4, kBooMaxBins = 4096;     // AZTOT_BOO_MAX_* of include/aztot.h
constexpr int kBooMaxBlocks = 1024;         // k_boo_hist walks the ids grid-stride: at most this many LDS histograms are flushed per sample
constexpr int kBooHistBudget = 32768;       // bytes of LDS k_boo_hist may take for its uint32 sub-histogram; beyond it: 64-bit global atomics

// what the kernels need of the set-up; norm and the rest are indexed at compile time only (kernel arguments: scalar registers)
struct BooParams
{
    double r2;                              // R * R
    int32_t centralMask, ligandMask;
};
struct BooOrder
{
    double norm[kBooMaxL + 1];              // N_lm = sqrt((2l + 1) / (4 pi) * (l - m)! / (l + m)!), m = 0 ... l
    double scale;                           // 4 pi / (2l + 1)
    int32_t at, stride;                     // q_lm of this order: qlm[slot * stride + at + 2 m + (0 re, 1 im)]
};

// (-1)^m (2m - 1)!!
__host__ __device__ constexpr double boo_tmm(int m)
{
    double v = 1.0;
    for (int k = 1; k <= m; k++) v *= -(double)(2 * k - 1);
    return v;
}

// acc[2 m], acc[2 m + 1] += T_L^m(z) (x + i y)^m for m = 0 ... L; every index is a compile-time constant once the loops are unrolled
template <int L> __device__ __forceinline__ void boo_add_bond(double (&acc)[2 * (L + 1)], double x, double y, double z)
{
    double cr = 1.0, ci = 0.0;
#pragma unroll
    for (int m = 0; m <= L; m++)
    {
        double p0 = boo_tmm(m), p1 = p0;
        if (m < L) p1 = (double)(2 * m + 1) * z * p0;
#pragma unroll
        for (int l = m + 2; l <= L; l++)
        {
            const double p2 = ((double)(2 * l - 1) * z * p1 - (double)(l + m - 1) * p0) * (1.0 / (double)(l - m));
            p0 = p1; p1 = p2;
        }
        acc[2 * m] += p1 * cr;
        acc[2 * m + 1] += p1 * ci;
        const double nr = cr * x - ci * y, ni = cr * y + ci * x;
        cr = nr; ci = ni;
    }
}

// q_l from the q_lm of one atom: sqrt(scale * (|q_l0|^2 + 2 sum_{m > 0} |q_lm|^2)), m ascending
template <int L> __device__ __forceinline__ double boo_invariant(const double (&q)[2 * (L + 1)], double scale)
{
    const double s0 = q[0] * q[0] + q[1] * q[1];
    double sm = 0.0;
#pragma unroll
    for (int m = 1; m <= L; m++) sm += q[2 * m] * q[2 * m] + q[2 * m + 1] * q[2 * m + 1];
    return sqrt(scale * (s0 + 2.0 * sm));
}

// Bond sums: the lanes of SliceLane, the candidates of grid_walk in its order.  Slot order is canonical and S depends on N alone: the order of every sum is
// a function of the sampled state.  A neighbour of a central atom i: j != i, species in ligandMask, 0 < r2 < R * R (grid_sep's r2).
//   nSlot[slot] = n_i (-1: not central);  qlm[slot * stride + at + 2 m + c] = N_lm * sum / n_i (0 where n_i <= 0)
template <int L>
__global__ __launch_bounds__(kBlock) void k_boo_qlm(RdfGrid G, BooParams P, BooOrder O, int n, int sliceShift, const int32_t* __restrict__ cellStart,
                                                    const double* __restrict__ sx, const double* __restrict__ sy, const double* __restrict__ sz,
                                                    const int32_t* __restrict__ sKind, int32_t* __restrict__ nSlot, double* __restrict__ qlm)
{
    const SliceLane lane(sliceShift);
    const int i = lane.i;
    const bool central = i < n && ((P.centralMask >> (sKind[i] & 255)) & 1);
    double acc[2 * (L + 1)];
#pragma unroll
    for (int k = 0; k < 2 * (L + 1); k++) acc[k] = 0.0;
    int cnt = 0;
    if (central)
        grid_walk(G, cellStart, lane, sx[i], sy[i], sz[i], sx, sy, sz, [&](int j, double ux, double uy, double uz, double r2) {
            if (j != i && r2 > 0.0 && r2 < P.r2 && ((P.ligandMask >> (sKind[j] & 255)) & 1))
            {
                const double inv = 1.0 / sqrt(r2);
                boo_add_bond<L>(acc, ux * inv, uy * inv, uz * inv);
                cnt++;
            }
        });
    slice_fold(acc, lane.S);
    cnt = slice_fold(cnt, lane.S);
    if (i < n && lane.slice == 0)
    {
        nSlot[i] = central ? cnt : -1;
        double* q = qlm + (size_t)i * O.stride + O.at;
        const double dn = (double)(cnt > 0 ? cnt : 1);
#pragma unroll
        for (int m = 0; m <= L; m++)
        {
            q[2 * m] = cnt > 0 ? acc[2 * m] * O.norm[m] / dn : 0.0;
            q[2 * m + 1] = cnt > 0 ? acc[2 * m + 1] * O.norm[m] / dn : 0.0;
        }
    }
}

// Neighbour average, the walk of k_boo_qlm: the q_lm of the central atoms among N(i) are summed by slot, then
//   q-bar_lm(i) = (q_lm(i) + sum) / (1 + |C(i)|);  qCols[(kind * nOrders + order) * nPad + id] = q_l (kind 0), q-bar_l (kind 1);  nById, typeById
template <int L>
__global__ __launch_bounds__(kBlock) void k_boo_average(RdfGrid G, BooParams P, BooOrder O, int n, int sliceShift, int order, int nOrders, size_t nPad,
                                                        const int32_t* __restrict__ cellStart, const double* __restrict__ sx, const double* __restrict__ sy,
                                                        const double* __restrict__ sz, const int32_t* __restrict__ sKind, const int32_t* __restrict__ slotId,
                                                        const int32_t* __restrict__ nSlot, const double* __restrict__ qlm, double* __restrict__ qCols,
                                                        int32_t* __restrict__ nById, int32_t* __restrict__ typeById)
{
    const SliceLane lane(sliceShift);
    const int i = lane.i;
    const bool central = i < n && ((P.centralMask >> (sKind[i] & 255)) & 1);
    double acc[2 * (L + 1)];
#pragma unroll
    for (int k = 0; k < 2 * (L + 1); k++) acc[k] = 0.0;
    int cnt = 0;
    if (central)
        grid_walk(G, cellStart, lane, sx[i], sy[i], sz[i], sx, sy, sz, [&](int j, double, double, double, double r2) {
            const int gj = sKind[j] & 255;
            if (j != i && r2 > 0.0 && r2 < P.r2 && ((P.ligandMask >> gj) & 1) && ((P.centralMask >> gj) & 1))
            {
                const double* q = qlm + (size_t)j * O.stride + O.at;
#pragma unroll
                for (int k = 0; k < 2 * (L + 1); k++) acc[k] += q[k];
                cnt++;
            }
        });
    slice_fold(acc, lane.S);
    cnt = slice_fold(cnt, lane.S);
    if (i < n && lane.slice == 0)
    {
        const int id = slotId[i];
        if ((unsigned)id >= (unsigned)n) return;
        double own[2 * (L + 1)];
        const double* q = qlm + (size_t)i * O.stride + O.at;
        const double dn = (double)(1 + cnt);
#pragma unroll
        for (int k = 0; k < 2 * (L + 1); k++)
        {
            own[k] = central ? q[k] : 0.0;
            acc[k] = (own[k] + acc[k]) / dn;
        }
        qCols[(size_t)order * nPad + id] = central ? boo_invariant<L>(own, O.scale) : 0.0;
        qCols[(size_t)(nOrders + order) * nPad + id] = central ? boo_invariant<L>(acc, O.scale) : 0.0;
        if (order == 0) { nById[id] = nSlot[i]; typeById[id] = sKind[i] & 255; }
    }
}

// Histograms.  Cell ((kind * nOrders + order) * nSpec + species) * nBins + bin, then the nSpec cells of `entered`; an atom with n_i > 0 adds 1 to
// 2 nOrders cells and to its species' entered cell.  bin = min(nBins - 1, (int)fl(q * nBins)).
// OVERFLOW BOUND of a uint32 cell between two flushes: an atom adds at most 1 to a cell, and a workgroup serves fewer than 2^31 atoms.
__global__ __launch_bounds__(kBlock) void k_boo_hist(int n, int nOrders, int nSpec, int nBins, size_t nPad, int useLds, const double* __restrict__ qCols,
                                                     const int32_t* __restrict__ nById, const int32_t* __restrict__ typeById,
                                                     unsigned long long* __restrict__ totals)
{
    extern __shared__ uint32_t booLds[];
    const int nHist = 2 * nOrders * nSpec * nBins, nEnt = nHist + nSpec;
    if (useLds)
    {
        for (int e = threadIdx.x; e < nEnt; e += kBlock) booLds[e] = 0u;
        __syncthreads();
    }
    for (int id = blockIdx.x * kBlock + threadIdx.x; id < n; id += gridDim.x * kBlock)
    {
        if (nById[id] <= 0) continue;
        const int s = typeById[id];
        if ((unsigned)s >= (unsigned)nSpec) continue;
        for (int c = 0; c < 2 * nOrders; c++)
        {
            const int b = min(nBins - 1, (int)__dmul_rn(qCols[(size_t)c * nPad + id], (double)nBins));
            const int e = (c * nSpec + s) * nBins + max(b, 0);
            if (useLds) atomicAdd(&booLds[e], 1u);
            else atomicAdd(&totals[e], 1ull);
        }
        if (useLds) atomicAdd(&booLds[nHist + s], 1u);
        else atomicAdd(&totals[nHist + s], 1ull);
    }
    if (!useLds) return;
    __syncthreads();
    for (int e = threadIdx.x; e < nEnt; e += kBlock)
        if (booLds[e]) atomicAdd(&totals[e], (unsigned long long)booLds[e]);
}

// Steps 1 and 2 of the tree for workgroup b (ids [256 b, 256 b + 256)), every column and species: the term of an id is its value where its species is s,
// +0.0 elsewhere (the padding has species -1).  Step 3 is k_tree_fold's (kernels.hip.h), added to the running sums.
//   partials[(c * nSpec + s) * nChunkPad + b]
__global__ __launch_bounds__(kBlock) void k_boo_chunks(int nCols, int nSpec, size_t nPad, int nChunkPad, const double* __restrict__ qCols,
                                                       const int32_t* __restrict__ typeById, double* __restrict__ partials)
{
    __shared__ double red[2 * kBooMaxOrders * kSpecCap][kBlock / kWave];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t id = (size_t)blockIdx.x * kTreeChunk + t;
    const int ty = typeById[id];
    for (int c = 0; c < nCols; c++)
    {
        const double v = qCols[(size_t)c * nPad + id];
        for (int s = 0; s < nSpec; s++)
        {
            const double w = wave_sum(ty == s ? v : 0.0);
            if (lane == 0) red[c * nSpec + s][wv] = w;
        }
    }
    __syncthreads();
    if (t < nCols * nSpec) partials[(size_t)t * nChunkPad + blockIdx.x] = tree_wave4(red[t]);
}

}  // namespace aztot
