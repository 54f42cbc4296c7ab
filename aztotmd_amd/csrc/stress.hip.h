// Virial pressure tensor of the pair terms (no counterpart in the reference, whose only pressure is the wall-momentum estimate of main.cpp:143-163).
// The contract (pair set, per-atom virial, kinetic part, the order of every sum) is stated in include/aztot.h, 'pressure tensor'.
//
//  k_stress_bin ... _place   the counting sort of grid.hip.h over the wrapped positions in its canonical order (Samplers::grid_fill_canonical), cells with an
//                            edge >= rMax
//  k_stress_gather           slot -> id map and radii in slot order; m v_a v_b by atom id
//  k_stress_pairs            full-neighbour walk (grid_walk); every pair term is pair_visit's; six virial components, two energies and two counters in
//                            registers, slices folded with lane exchanges, one store per (atom, column) by atom id, no atomics
//  k_stress_chunks / _fold   the summation tree over atom ids (kernels.hip.h) over the per-atom columns
//
// Only engine state is READ.  No floating-point atomics: a sample is a function of wrapped positions, velocities, ids, types, radii, N and the box.
#pragma once
#include <hip/hip_runtime.h>

#include "grid.hip.h"

namespace aztot {

// per-atom columns by atom id, each nPad long (ids padded to a multiple of 256; the padding stays zero)
enum StressCol { SC_WXX = 0, SC_WYY, SC_WZZ, SC_WXY, SC_WXZ, SC_WYZ, SC_EVDW, SC_ECOUL, SC_KXX, SC_KYY, SC_KZZ, SC_KXY, SC_KXZ, SC_KYZ, SC_COUNT };
constexpr int kStressPairCols = SC_KXX;     // what k_stress_pairs writes; the kinetic columns are k_stress_gather's

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

// Pair walk: the lanes of SliceLane, the candidates of grid_walk but j == i.  Slot order is canonical (cells by position, ids ascending inside a cell) and S
// depends on N alone, so the order of every per-atom sum is a function of the sampled state.  The virial terms h u_a u_b are even in the separation u.
//   cols[c * nPad + id], c < kStressPairCols;  visits[id], drops[id]: half-visits inside rMax and half-visits the drop rule took the force of
__global__ __launch_bounds__(kBlock) void k_stress_pairs(RdfGrid G, StepParams P, SpecTable S, const DevPot* __restrict__ pots, int n, int sliceShift, size_t nPad,
                                                         const int32_t* __restrict__ cellStart, const double* __restrict__ sx, const double* __restrict__ sy,
                                                         const double* __restrict__ sz, const int32_t* __restrict__ sKind, const double* __restrict__ sRad,
                                                         const int32_t* __restrict__ slotId, double* __restrict__ cols, int32_t* __restrict__ visits,
                                                         int32_t* __restrict__ drops)
{
    const SliceLane lane(sliceShift);
    const int i = lane.i;
    double w[kStressPairCols];
#pragma unroll
    for (int k = 0; k < kStressPairCols; k++) w[k] = 0.0;
    int nIn = 0, nDrop = 0;
    if (i < n)
    {
        const int ti = sKind[i] & 255;
        const double radi = P.use_radii ? sRad[i] : 0.0;
        grid_walk(G, cellStart, lane, sx[i], sy[i], sz[i], sx, sy, sz,
                  [&](int j, double ux, double uy, double uz, double r2, double (&w)[kStressPairCols], int& nIn, int& nDrop) {
            if (r2 <= P.r2Max && j != i)
            {
                double f, eV, eC;
                int dropped;
                stress_pair_term(P, S, pots, r2, ti, sKind[j] & 255, radi, P.use_radii ? sRad[j] : 0.0, f, eV, eC, dropped);
                const double h = 0.5 * f;
                const double hx = h * ux, hy = h * uy, hz = h * uz;
                w[SC_WXX] += hx * ux; w[SC_WYY] += hy * uy; w[SC_WZZ] += hz * uz;
                w[SC_WXY] += hx * uy; w[SC_WXZ] += hx * uz; w[SC_WYZ] += hy * uz;
                w[SC_EVDW] += eV; w[SC_ECOUL] += eC;
                nIn += 1; nDrop += dropped;
            }
        }, w, nIn, nDrop);
    }
    slice_fold(w, lane.S);
    nIn = slice_fold(nIn, lane.S);
    nDrop = slice_fold(nDrop, lane.S);
    if (i < n && lane.slice == 0)
    {
        const int id = slotId[i];
        if ((unsigned)id >= (unsigned)n) return;
#pragma unroll
        for (int k = 0; k < kStressPairCols; k++) cols[k * nPad + id] = w[k];
        visits[id] = nIn; drops[id] = nDrop;
    }
}

// Steps 1 and 2 of the tree for workgroup b (ids [256 b, 256 b + 256)), every column: lane l of wave w is id 256 b + 64 w + l, wave_sum folds a run of 64,
// tree_wave4 the four runs.  All the columns' loads are issued before the first reduction.  The integer counters of the chunk go into counters[2] (integer
// atomics, one per wave).  Step 3 is k_tree_fold's (kernels.hip.h; the fold only writes entries below nChunkPad / 2, all of which this kernel rewrites).
//   partials[q * nChunkPad + b]
__global__ __launch_bounds__(kBlock) void k_stress_chunks(size_t nPad, int nChunkPad, const double* __restrict__ cols, const int32_t* __restrict__ visits,
                                                          const int32_t* __restrict__ drops, double* __restrict__ partials,
                                                          unsigned long long* __restrict__ counters)
{
    __shared__ double red[SC_COUNT][kBlock / kWave];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t id = (size_t)blockIdx.x * kTreeChunk + t;
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
    if (t < SC_COUNT) partials[(size_t)t * nChunkPad + blockIdx.x] = tree_wave4(red[t]);
    for (int m = 1; m < 64; m <<= 1) { a += __shfl_xor(a, m); d += __shfl_xor(d, m); }
    if (lane == 0)
    {
        if (a) atomicAdd(&counters[0], (unsigned long long)a);
        if (d) atomicAdd(&counters[1], (unsigned long long)d);
    }
}

}  // namespace aztot
