// Radial distribution functions (brute_rdf / brute_nrdf, cuStat.cu:436-700, and get_rdf, rdf.cpp:98-129) on a private cell grid.
//
//  reference                                   ours
//  ------------------------------------------  -------------------------------------------------------------------------------
//  brute_rdf / brute_nrdf: all N^2/2 pairs,     k_grid_bin + k_scan_* + k_grid_place (grid.hip.h): counting sort of the current positions into a
//  float atomics into a float histogram         grid of cells with edge >= rmax (its own, not the engine's: those are stale by up
//                                               to the skin and sized for the force cut-off);
//                                               k_rdf_pairs: half-shell walk over that grid, fp64 distances, uint32 sub-histograms
//                                               in LDS flushed once per workgroup into uint64 totals with integer atomics
//
// Only engine state is READ (positions, species); nothing the step uses is written.  The counts are integers: the totals do not depend
// on the order in which pairs arrive, so they are exactly reproducible.
#pragma once
#include <hip/hip_runtime.h>

#include "grid.hip.h"

namespace aztot {

constexpr int kRdfMaxBlocks = 1024;         // k_rdf_pairs walks the atoms grid-stride: at most this many LDS histograms are flushed per sample
constexpr int kRdfLdsBudget = 65536;        // bytes of LDS k_rdf_pairs may take for its sub-histograms (one per wave where they fit, else one per workgroup)

__device__ __forceinline__ int rdf_pair(int a, int b, int n)
{   // iPair = mn * (n - 1) + mn * (1 - mn) / 2 + mx (cuStat.cu:479-486)
    const int mn = min(a, b), mx = max(a, b);
    return mn * (n - 1) + mn * (1 - mn) / 2 + mx;
}

// Pair walk: one thread per atom i (slot order, so a wave's atoms share their cells and their partners' loads), partners j in the neighbour cells
// counted once per unordered pair.  copies > 0: `copies` uint32 sub-histograms in LDS (wave w adds into copy w % copies), summed and added into the
// uint64 totals once per workgroup; copies == 0: the histogram does not fit the LDS budget, every pair adds straight into the totals.
// Histogram entries: [bin][species pair] (nBins * nPairS), then [bin][nucleus pair] (nBins * nPairN).
__global__ __launch_bounds__(kBlock) void k_rdf_pairs(RdfGrid G, int n, const int32_t* __restrict__ cellStart, const double* __restrict__ sx,
                                                      const double* __restrict__ sy, const double* __restrict__ sz, const int32_t* __restrict__ sKind,
                                                      int copies, unsigned long long* __restrict__ histS, unsigned long long* __restrict__ histN)
{
    extern __shared__ uint32_t rdfLds[];
    const int nEntS = G.nBins * G.nPairS, nEnt = nEntS + G.nBins * G.nPairN;
    uint32_t* mine = copies ? rdfLds + (size_t)((threadIdx.x >> 6) % copies) * nEnt : nullptr;
    if (copies)
    {
        for (int e = threadIdx.x; e < copies * nEnt; e += kBlock) rdfLds[e] = 0u;
        __syncthreads();
    }
    const int lo[3] = {G.nc[0] >= 3 ? -1 : 0, G.nc[1] >= 3 ? -1 : 0, G.nc[2] >= 3 ? -1 : 0};
    const int hi[3] = {G.nc[0] >= 2 ? 1 : 0, G.nc[1] >= 2 ? 1 : 0, G.nc[2] >= 2 ? 1 : 0};
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
    {
        const double xi = sx[i], yi = sy[i], zi = sz[i];
        const int ki = sKind[i], ti = ki & 255, ni = ki >> 8;
        const int cx = cell_coord(xi, G.icsz[0], G.nc[0]), cy = cell_coord(yi, G.icsz[1], G.nc[1]), cz = cell_coord(zi, G.icsz[2], G.nc[2]);
        for (int dx = lo[0]; dx <= hi[0]; dx++)
            for (int dy = lo[1]; dy <= hi[1]; dy++)
                for (int dz = lo[2]; dz <= hi[2]; dz++)
                {
                    const bool self = dx == 0 && dy == 0 && dz == 0;
                    // half shell: the forward half of the 26 neighbours (lexicographically positive offset) + the own cell with j > i
                    if (G.halfShell && (dx < 0 || (dx == 0 && (dy < 0 || (dy == 0 && dz < 0))))) continue;
                    int ex = cx + dx, ey = cy + dy, ez = cz + dz;
                    ex += ex < 0 ? G.nc[0] : (ex >= G.nc[0] ? -G.nc[0] : 0);
                    ey += ey < 0 ? G.nc[1] : (ey >= G.nc[1] ? -G.nc[1] : 0);
                    ez += ez < 0 ? G.nc[2] : (ez >= G.nc[2] ? -G.nc[2] : 0);
                    const int c = (ex * G.nc[1] + ey) * G.nc[2] + ez;
                    const int s1 = cellStart[c + 1];
                    int j = cellStart[c];
                    if (self || !G.halfShell) j = max(j, i + 1);     // without the half shell every distinct cell is visited once: count j > i only
                    for (; j < s1; j++)
                    {
                        // fp64 without contraction: the same rounding as the host's (dx*dx + dy*dy) + dz*dz on the delta_periodic differences
                        double ddx = xi - sx[j], ddy = yi - sy[j], ddz = zi - sz[j];
                        min_image(ddx, G.L[0], G.half[0]);
                        min_image(ddy, G.L[1], G.half[1]);
                        min_image(ddz, G.L[2], G.half[2]);
                        const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)), __dmul_rn(ddz, ddz));
                        if (r2 < G.r2max)
                        {
                            const int bin = (int)__dmul_rn(__dsqrt_rn(r2), G.idr);
                            if (bin < G.nBins)
                            {
                                const int kj = sKind[j];
                                const int eS = bin * G.nPairS + rdf_pair(ti, kj & 255, G.nSpec);
                                const int eN = G.nPairN ? nEntS + bin * G.nPairN + rdf_pair(ni, kj >> 8, G.nNucl) : -1;
                                if (copies)
                                {
                                    atomicAdd(&mine[eS], 1u);
                                    if (eN >= 0) atomicAdd(&mine[eN], 1u);
                                }
                                else
                                {
                                    atomicAdd(&histS[eS], 1ull);
                                    if (eN >= 0) atomicAdd(&histN[eN - nEntS], 1ull);
                                }
                            }
                        }
                    }
                }
    }
    if (!copies) return;
    __syncthreads();
    for (int e = threadIdx.x; e < nEnt; e += kBlock)
    {
        unsigned long long v = 0;
        for (int k = 0; k < copies; k++) v += rdfLds[(size_t)k * nEnt + e];
        if (v) atomicAdd(e < nEntS ? &histS[e] : &histN[e - nEntS], v);
    }
}

}  // namespace aztot
