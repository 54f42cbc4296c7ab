// Time correlation functions: mean-square displacement (out_msd, out_md.cpp:89-124) and velocity autocorrelation (vaf_init / vaf_info, out_md.cpp:535-582)
// per species, over a ring of time origins.  The contract (per-atom terms, the summation tree, the ring) is stated in include/aztot.h.
//
//  reference                                   ours
//  ------------------------------------------  -------------------------------------------------------------------------------
//  x0s / vx0 ...: one origin, host arrays in    k_tcf_gather: the current state from slot order into atom-id order (wrapped positions as
//  atom order; out_msd / vaf_info: one host     aztot_md_to_host hands them out), and into its ring slot when the sample is an origin;
//  loop over the atoms per output row           k_tcf_correlate: one workgroup per 256 ids reads its current state once and streams every live
//                                               origin past it; per origin and species the two chunk sums in the fixed tree;
//                                               k_tcf_fold: the chunk sums of one (origin, quantity, species) folded by halving, added to the
//                                               accumulator of the origin's lag
//
// Only engine state is READ.  Every sum has one fixed order (no floating-point atomics, no dependence on the slot order the cell sort left or on the
// launch shape), every operation is rounded on its own: a sample's sums are a function of the state alone.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hip.h"

namespace aztot {

struct TcfBox { double L[3], invL[3], half[3]; };

// the six arrays of one stored state: x y z vx vy vz, each nPad long (ids padded to a multiple of kTreeChunk; the padding stays zero)
__device__ __forceinline__ void tcf_store(double* __restrict__ s, size_t nPad, int id, double x, double y, double z, double vx, double vy, double vz)
{
    s[id] = x; s[nPad + id] = y; s[2 * nPad + id] = z;
    s[3 * nPad + id] = vx; s[4 * nPad + id] = vy; s[5 * nPad + id] = vz;
}

// slot order -> id order; org != nullptr: the sample is an origin and goes into its ring slot too
__global__ __launch_bounds__(kBlock) void k_tcf_gather(TcfBox B, AtomArrays A, int n, size_t nPad, double* __restrict__ cur, double* __restrict__ org,
                                                       int32_t* __restrict__ typeById)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int id = A.id[i];
    if ((unsigned)id >= (unsigned)n) return;
    double x = A.x[i], y = A.y[i], z = A.z[i];
    wrap_coord(x, B.L[0], B.invL[0]);
    wrap_coord(y, B.L[1], B.invL[1]);
    wrap_coord(z, B.L[2], B.invL[2]);
    const double vx = A.vx[i], vy = A.vy[i], vz = A.vz[i];
    tcf_store(cur, nPad, id, x, y, z, vx, vy, vz);
    if (org) tcf_store(org, nPad, id, x, y, z, vx, vy, vz);
    typeById[id] = A.type[i];
}

struct TcfOrigin { double x, y, z, vx, vy, vz; };
__device__ __forceinline__ TcfOrigin tcf_load(const double* __restrict__ s, size_t nPad, size_t id)
{
    return TcfOrigin{s[id], s[nPad + id], s[2 * nPad + id], s[3 * nPad + id], s[4 * nPad + id], s[5 * nPad + id]};
}

// Workgroup b holds ids [256 b, 256 b + 256): lane l of wave w is id 256 b + 64 w + l, so wave_sum is step 1 of the tree and tree_wave4 is step 2.
// The current state stays in registers while the live origins (ring slots 0 ... nLive - 1) stream past; origin k + 1 is loaded before origin k is
// reduced, so that its six loads are in flight across the reduction and the barrier.  Species are found by ballot: only those that occur in the
// chunk are reduced, the others get their +0.0 written.
//   partials[((k * 2 + quantity) * nSpec + species) * nChunkPad + b], quantity 0 MSD, 1 VAF
__global__ __launch_bounds__(kBlock) void k_tcf_correlate(TcfBox B, int nSpec, size_t nPad, int nChunkPad, int nLive, const double* __restrict__ cur,
                                                          const int32_t* __restrict__ typeById, const double* __restrict__ ring,
                                                          double* __restrict__ partials)
{
    __shared__ double red[2][2][kSpecCap][kBlock / kWave];      // [origin parity][quantity][species][wave]
    __shared__ unsigned sPresent;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const size_t id = (size_t)blockIdx.x * kTreeChunk + t;
    const TcfOrigin c = tcf_load(cur, nPad, id);
    const int ty = typeById[id];                                // -1 in the padding
    if (t == 0) sPresent = 0u;
    __syncthreads();
    unsigned seen = 0u;
    for (int s = 0; s < nSpec; s++)
        if (__ballot(ty == s) != 0ULL) seen |= 1u << s;
    if (lane == 0 && seen) atomicOr(&sPresent, seen);
    __syncthreads();
    const unsigned present = sPresent;
    const size_t slot = 6 * nPad;
    TcfOrigin next = tcf_load(ring, nPad, id);
    for (int k = 0; k < nLive; k++)
    {
        const TcfOrigin o = next;
        if (k + 1 < nLive) next = tcf_load(ring + (size_t)(k + 1) * slot, nPad, id);
        double dx = c.x - o.x, dy = c.y - o.y, dz = c.z - o.z;
        min_image(dx, B.L[0], B.half[0]);
        min_image(dy, B.L[1], B.half[1]);
        min_image(dz, B.L[2], B.half[2]);
        const double msd = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        const double vaf = __dadd_rn(__dadd_rn(__dmul_rn(c.vx, o.vx), __dmul_rn(c.vy, o.vy)), __dmul_rn(c.vz, o.vz));
        double (*r)[kSpecCap][kBlock / kWave] = red[k & 1];
        for (unsigned m = present; m; m &= m - 1)
        {
            const int s = __ffs((int)m) - 1;
            const double a = wave_sum(ty == s ? msd : 0.0), b = wave_sum(ty == s ? vaf : 0.0);
            if (lane == 0) { r[0][s][w] = a; r[1][s][w] = b; }
        }
        // one barrier per origin: origin k + 1 writes the other half of `red`, and origin k + 2 comes after the barrier of k + 1
        __syncthreads();
        if (t < 2 * nSpec)
        {
            const int q = t / nSpec, s = t - q * nSpec;
            double v = 0.0;
            if ((present >> s) & 1u) v = tree_wave4(r[q][s]);
            partials[(((size_t)k * 2 + q) * nSpec + s) * nChunkPad + blockIdx.x] = v;
        }
    }
}

// Step 3 of the tree for workgroup (k, quantity, species): the chunk sums (padded with +0.0 to nChunkPad, a power of two; the padding is never
// written, the fold only touches entries below nChunkPad / 2) folded by tree_fold, then acc = acc + S at the lag of the origin in ring slot k.
// Sample c (counted from 0), origins every E samples in slot (c / E) % M: slot k holds origin number j = the largest j <= c / E with j % M == k.
__global__ __launch_bounds__(kBlock) void k_tcf_fold(int nSpec, int nChunkPad, long long c, int E, int M, double* partials, long long* __restrict__ count,
                                                     double* __restrict__ msdSum, double* __restrict__ vafSum)
{
    const double sum = tree_fold(partials + (size_t)blockIdx.x * nChunkPad, nChunkPad);
    if (threadIdx.x != 0) return;
    const int s = blockIdx.x % nSpec, q = (blockIdx.x / nSpec) & 1, k = blockIdx.x / (2 * nSpec);
    const long long newest = c / E, j = newest - (newest - k) % M;
    const long long lag = c - j * E;
    double* acc = (q ? vafSum : msdSum) + lag * nSpec + s;
    *acc = __dadd_rn(*acc, sum);
    if (q == 0 && s == 0) count[lag] += 1;
}

}  // namespace aztot
