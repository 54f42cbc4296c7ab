// Virial pressure tensor of the pair terms (no counterpart in the reference, whose only pressure is the wall-momentum estimate of main.cpp:143-163).
// The contract (pair set, per-atom virial, kinetic part, the order of every sum) is stated in include/aztot.h, 'pressure tensor'.
//
//  k_stress_bin / _scan      the counting sort of rdf.hip.h over the wrapped positions, cells with an edge >= rMax
//  k_stress_ids + _rank      the arrival rank k_rdf_bin hands out is replaced by the rank of the atom's id among its cell-mates: the slot order is then a
//                            function of the sampled state alone
//  k_stress_place            k_rdf_place on that rank
//  k_stress_gather           slot -> id map and radii in slot order; m v_a v_b by atom id
//  k_stress_pairs            full-neighbour walk of k_cn_pairs; every pair term is pair_visit's; six virial components, two energies and two counters in
//                            registers, slices folded with lane exchanges, one store per (atom, column) by atom id, no atomics
//  k_stress_chunks / _fold   the summation tree of the time correlation functions (tcf.hip.h) over the per-atom columns in id order
//
// Only engine state is READ.  No floating-point atomics: a sample is a function of wrapped positions, velocities, ids, types, radii, N and the box.
#pragma once
#include <hip/hip_runtime.h>

#include "cn.hip.h"

namespace aztot {

// per-atom columns by atom id, each nPad long (ids padded to a multiple of 256; the padding stays zero)
enum StressCol { SC_WXX = 0, SC_WYY, SC_WZZ, SC_WXY, SC_WXZ, SC_WYZ, SC_EVDW, SC_ECOUL, SC_KXX, SC_KYY, SC_KZZ, SC_KXY, SC_KXZ, SC_KYZ, SC_COUNT };
constexpr int kStressPairCols = SC_KXX;     // what k_stress_pairs writes; the kinetic columns are k_stress_gather's
constexpr int kStressChunk = kBlock;

// rank of every atom's id among the ids of its cell: arrivalId is the slot -> id map of the arrival order (k_cn_slot_ids)
__global__ __launch_bounds__(kBlock) void k_stress_rank(AtomArrays A, int n, const int32_t* __restrict__ cellOf, const int32_t* __restrict__ cellStart,
                                                        const int32_t* __restrict__ arrivalId, int32_t* __restrict__ rankOf)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int c = cellOf[i], id = A.id[i];
    int r = 0;
    for (int s = cellStart[c]; s < cellStart[c + 1]; s++) r += arrivalId[s] < id ? 1 : 0;
    rankOf[i] = r;
}

// slot -> id and radius in slot order; the kinetic terms m v_a v_b (each product rounded on its own, (m v_a) v_b) by atom id.  Frozen species: +0.0
__global__ __launch_bounds__(kBlock) void k_stress_gather(SpecTable S, AtomArrays A, int n, int useRadii, size_t nPad, const int32_t* __restrict__ cellOf,
                                                          const int32_t* __restrict__ rankOf, const int32_t* __restrict__ cellStart,
                                                          int32_t* __restrict__ slotId, double* __restrict__ sRad, double* __restrict__ cols)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int id = A.id[i];
    const int s = cellStart[cellOf[i]] + rankOf[i];
    slotId[s] = id;
    if (useRadii) sRad[s] = A.rad[i];
    if ((unsigned)id >= (unsigned)n) return;
    const int t = A.type[i];
    const double m = S.frozen[t] ? 0.0 : S.mass[t];
    const double vx = A.vx[i], vy = A.vy[i], vz = A.vz[i];
    const double mx = __dmul_rn(m, vx), my = __dmul_rn(m, vy), mz = __dmul_rn(m, vz);
    cols[SC_KXX * nPad + id] = __dmul_rn(mx, vx); cols[SC_KYY * nPad + id] = __dmul_rn(my, vy); cols[SC_KZZ * nPad + id] = __dmul_rn(mz, vz);
    cols[SC_KXY * nPad + id] = __dmul_rn(mx, vy); cols[SC_KXZ * nPad + id] = __dmul_rn(mx, vz); cols[SC_KYZ * nPad + id] = __dmul_rn(my, vz);
}

// what pair_visit knows about one pair seen from one end: f = -(1/r) dU/dr (0 where the drop rule fires), half the pair energies, dropped or not.
// A unit vector along x as the separation makes PairAcc::fx the scalar itself (f * 1.0 is exact).
__device__ __forceinline__ void stress_pair_term(const StepParams& P, const SpecTable& S, const DevPot* __restrict__ pots, double r2, int ti, int tj,
                                                 double radi, double radj, double& f, double& eV, double& eC, int& dropped)
{
    PairAcc a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    pair_visit(P, S, pots, 1.0, 0.0, 0.0, r2, ti, tj, radi, radj, a);
    f = a.fx; eV = a.eV; eC = a.eC; dropped = a.dropped != 0.0 ? 1 : 0;
}

// Pair walk, the decomposition of k_cn_pairs: lane t of the launch is (atom t >> sliceShift in slot order, slice t & (S - 1)); every slice visits all the
// neighbour cells and takes the candidates start + slice, + S, ... of each.  Slot order is canonical (cells by position, ids ascending inside a cell) and S
// depends on N alone, so the order of every per-atom sum is a function of the sampled state.
//   cols[c * nPad + id], c < kStressPairCols;  visits[id], drops[id]: half-visits inside rMax and half-visits the drop rule took the force of
__global__ __launch_bounds__(kBlock) void k_stress_pairs(RdfGrid G, StepParams P, SpecTable S, const DevPot* __restrict__ pots, int n, int sliceShift, size_t nPad,
                                                         const int32_t* __restrict__ cellStart, const double* __restrict__ sx, const double* __restrict__ sy,
                                                         const double* __restrict__ sz, const int32_t* __restrict__ sKind, const double* __restrict__ sRad,
                                                         const int32_t* __restrict__ slotId, double* __restrict__ cols, int32_t* __restrict__ visits,
                                                         int32_t* __restrict__ drops)
{
    const int nS = 1 << sliceShift;
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int i = (int)(t >> sliceShift), slice = (int)(t & (nS - 1));
    double w[kStressPairCols];
#pragma unroll
    for (int k = 0; k < kStressPairCols; k++) w[k] = 0.0;
    int nIn = 0, nDrop = 0;
    if (i < n)
    {
        const int lo[3] = {G.nc[0] >= 3 ? -1 : 0, G.nc[1] >= 3 ? -1 : 0, G.nc[2] >= 3 ? -1 : 0};
        const int hi[3] = {G.nc[0] >= 2 ? 1 : 0, G.nc[1] >= 2 ? 1 : 0, G.nc[2] >= 2 ? 1 : 0};
        const double xi = sx[i], yi = sy[i], zi = sz[i];
        const int ti = sKind[i] & 255;
        const double radi = P.use_radii ? sRad[i] : 0.0;
        const int cx = cell_coord(xi, G.icsz[0], G.nc[0]), cy = cell_coord(yi, G.icsz[1], G.nc[1]), cz = cell_coord(zi, G.icsz[2], G.nc[2]);
        for (int dx = lo[0]; dx <= hi[0]; dx++)
            for (int dy = lo[1]; dy <= hi[1]; dy++)
                for (int dz = lo[2]; dz <= hi[2]; dz++)
                {
                    int ex = cx + dx, ey = cy + dy, ez = cz + dz;
                    ex += ex < 0 ? G.nc[0] : (ex >= G.nc[0] ? -G.nc[0] : 0);
                    ey += ey < 0 ? G.nc[1] : (ey >= G.nc[1] ? -G.nc[1] : 0);
                    ez += ez < 0 ? G.nc[2] : (ez >= G.nc[2] ? -G.nc[2] : 0);
                    const int c = (ex * G.nc[1] + ey) * G.nc[2] + ez;
                    const int s1 = cellStart[c + 1];
                    for (int j = cellStart[c] + slice; j < s1; j += nS)
                    {
                        if (j == i) continue;
                        // the pair rule of k_cn_pairs: fp64 without contraction on the delta_periodic differences
                        double ddx = xi - sx[j], ddy = yi - sy[j], ddz = zi - sz[j];
                        min_image(ddx, G.L[0], G.half[0]);
                        min_image(ddy, G.L[1], G.half[1]);
                        min_image(ddz, G.L[2], G.half[2]);
                        const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)), __dmul_rn(ddz, ddz));
                        if (r2 <= P.r2Max)
                        {
                            double f, eV, eC;
                            int dropped;
                            stress_pair_term(P, S, pots, r2, ti, sKind[j] & 255, radi, P.use_radii ? sRad[j] : 0.0, f, eV, eC, dropped);
                            const double h = 0.5 * f;
                            const double hx = h * ddx, hy = h * ddy, hz = h * ddz;
                            w[SC_WXX] += hx * ddx; w[SC_WYY] += hy * ddy; w[SC_WZZ] += hz * ddz;
                            w[SC_WXY] += hx * ddy; w[SC_WXZ] += hx * ddz; w[SC_WYZ] += hy * ddz;
                            w[SC_EVDW] += eV; w[SC_ECOUL] += eC;
                            nIn += 1; nDrop += dropped;
                        }
                    }
                }
    }
    // fold the slices of an atom (neighbouring lanes of one wave) in the fixed order 1, 2, 4, ...; lanes past the last atom take part with zeros
    for (int m = 1; m < nS; m <<= 1)
    {
#pragma unroll
        for (int k = 0; k < kStressPairCols; k++) w[k] += __shfl_xor(w[k], m);
        nIn += __shfl_xor(nIn, m);
        nDrop += __shfl_xor(nDrop, m);
    }
    if (i < n && slice == 0)
    {
        const int id = slotId[i];
        if ((unsigned)id >= (unsigned)n) return;
#pragma unroll
        for (int k = 0; k < kStressPairCols; k++) cols[k * nPad + id] = w[k];
        visits[id] = nIn; drops[id] = nDrop;
    }
}

// Steps 1 and 2 of the tree for workgroup b (ids [256 b, 256 b + 256)), every column: lane l of wave w is id 256 b + 64 w + l, wave_sum (strides 32 ... 1)
// folds a run of 64, (w0 + w2) + (w1 + w3) the four runs.  All the columns' loads are issued before the first reduction.  The integer counters of the chunk
// go into counters[2] (integer atomics, one per wave).
//   partials[q * nChunkPad + b]
__global__ __launch_bounds__(kBlock) void k_stress_chunks(size_t nPad, int nChunkPad, const double* __restrict__ cols, const int32_t* __restrict__ visits,
                                                          const int32_t* __restrict__ drops, double* __restrict__ partials,
                                                          unsigned long long* __restrict__ counters)
{
    __shared__ double red[SC_COUNT][kBlock / kWave];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t id = (size_t)blockIdx.x * kStressChunk + t;
    double v[SC_COUNT];
#pragma unroll
    for (int q = 0; q < SC_COUNT; q++) v[q] = cols[q * nPad + id];
    int a = visits[id], d = drops[id];
#pragma unroll
    for (int q = 0; q < SC_COUNT; q++)
    {
        const double s = wave_sum(v[q]);
        if (lane == 0) red[q][wv] = s;
    }
    __syncthreads();
    if (t < SC_COUNT) partials[(size_t)t * nChunkPad + blockIdx.x] = __dadd_rn(__dadd_rn(red[t][0], red[t][2]), __dadd_rn(red[t][1], red[t][3]));
    for (int m = 1; m < 64; m <<= 1) { a += __shfl_xor(a, m); d += __shfl_xor(d, m); }
    if (lane == 0)
    {
        if (a) atomicAdd(&counters[0], (unsigned long long)a);
        if (d) atomicAdd(&counters[1], (unsigned long long)d);
    }
}

// Step 3 of the tree for column blockIdx.x: the chunk sums (padded with +0.0 to nChunkPad, a power of two; the fold only writes entries below
// nChunkPad / 2, all of which k_stress_chunks rewrites) folded by halving in place
__global__ __launch_bounds__(kBlock) void k_stress_fold(int nChunkPad, double* partials, double* __restrict__ totals)
{
    double* a = partials + (size_t)blockIdx.x * nChunkPad;
    for (int h = nChunkPad >> 1; h > 0; h >>= 1)
    {
        for (int j = threadIdx.x; j < h; j += kBlock) a[j] = __dadd_rn(a[j], a[j + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = a[0];
}

}  // namespace aztot
