// Static structure factors (aztot_sk_*, include/aztot.h): per-species amplitudes rho_s(k) = sum_{j of species s} exp(i k r_j) over a set of k-vectors chosen
// by |k|, partial structure factors accumulated over the samples.  The reference computes no structure factor: the directive ('strfac') is ours.
//
//  k_sk_gather       wrapped x, y, z and the species from slot order into atom-id order (the pattern of k_tcf_gather); the padding keeps species -1
//  k_sk_amplitudes   threads <-> k-vectors (kSkPerThread each), one workgroup per (1024 vectors of the batch, row).  Per LDS tile of T <= 64 consecutive ids the
//                    three per-atom harmonic tables are rebuilt in LDS ([atom][harmonic], as k_ewald_sfac: the 64 lanes read the same atom, different
//                    harmonics): one sincospi per atom and axis, higher harmonics by complex multiplication, negative m / n by conjugation.  Nothing per
//                    (atom, vector) touches HBM.  The atoms of a tile are placed species by species (ballots; ascending id inside a species), so the walk over one
//                    species is a dense, wave-uniform loop with ONE accumulator pair per vector however many species the model has.  The running row sum of
//                    (vector, species) is read from `partial` before a tile and written back after it: the sum goes one atom at a time from +0.0 whatever T is
//  k_sk_fold         the 256 zero-padded row sums of one (vector, species, component) folded by halving (tests/tcf_model.py fold) into the amplitudes
//  k_sk_accumulate   acc[vector][pair] = acc + (re_a re_b + im_a im_b), every operation rounded on its own
//
// THE ORDER OF THE SUM is a function of N alone (include/aztot.h): row r of nB = min(256, ceil(N / 64)) adds the ids of the 64-id tiles r, r + nB, ... in
// ascending order, atoms of other species add nothing; it does not depend on the slot order, on T, on the batches or on the launch shape.  Every
// operation of the term and of the sums is written as a single rounded operation (__dmul_rn / __fma_rn / __dadd_rn): nothing is left to contraction.
// Only engine state is READ.  No floating-point atomics, no MFMA: the term is a product of three table entries, not a contraction of stored matrices.
#pragma once
#include <hip/hip_runtime.h>

#include "ewald.hip.h"
#include "tcf.hip.h"

namespace aztot {

constexpr int kSkMaxHarmonic = 48, kSkMaxBins = 4096;   // AZTOT_SK_MAX_HARMONIC (= kEwaldKMax), AZTOT_SK_MAX_BINS
constexpr int kSkIdTile = 64;                           // ids per tile of the summation order
constexpr int kSkRows = 256;                            // rows at the most; the fold is written for exactly this many
constexpr int kSkPerThread = 4;                         // k-vectors per thread of k_sk_amplitudes: the tables of a tile are built once per 1024 vectors
constexpr int kSkChunk = kBlock * kSkPerThread;
constexpr int kSkLdsBudget = 49152;                     // the tile's tables: T = 64 up to 48 harmonic entries per atom, 32 up to 96, 16 beyond (147 at the most)
constexpr size_t kSkPartialBudget = (size_t)64 << 20;   // bytes of `partial`; larger sets go batch by batch (the sums do not depend on the batches)
static_assert(kSkMaxHarmonic == kEwaldKMax, "the harmonic recurrence is held to its tolerance up to kEwaldKMax (tests/test_gpu_ewald.py)");

struct SkGeom
{
    double L[3];
    int h[3];                                           // entries of the per-axis tables: the largest |harmonic| of the set + 1
};

// slot order -> id order (wrapped positions, as aztot_md_to_host hands them out)
__global__ __launch_bounds__(kBlock) void k_sk_gather(TcfBox B, AtomArrays A, int n, double* __restrict__ x, double* __restrict__ y, double* __restrict__ z,
                                                      int32_t* __restrict__ typeById)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int id = A.id[i];
    if ((unsigned)id >= (unsigned)n) return;
    double px = A.x[i], py = A.y[i], pz = A.z[i];
    wrap_coord(px, B.L[0], B.invL[0]);
    wrap_coord(py, B.L[1], B.invL[1]);
    wrap_coord(pz, B.L[2], B.invL[2]);
    x[id] = px; y[id] = py; z[id] = pz;
    typeById[id] = A.type[i];
}

__device__ __forceinline__ cplx sk_cmul(cplx a, cplx b)
{
    return cplx{__fma_rn(a.c, b.c, -__dmul_rn(a.s, b.s)), __fma_rn(a.s, b.c, __dmul_rn(a.c, b.s))};
}

// exp(2 pi i c / L) with the true pi: u = fl(c / L) goes through sincospi (no reduction error), what the division lost (r = c - u L, exact in an fma)
// turns the result by the small angle 2 pi r / L.  The phase is periodic in the box whatever the harmonic it is raised to
__device__ __forceinline__ cplx sk_phase(double c, double L)
{
    const double u = c / L;
    const double r = __fma_rn(-u, L, c);
    cplx e;
    sincospi(2.0 * u, &e.s, &e.c);
    const double eps = 6.283185307179586 * (r / L);
    return cplx{__fma_rn(-e.s, eps, e.c), __fma_rn(e.c, eps, e.s)};
}

// Grid (chunks of kSkChunk vectors of the batch, rows).  lmn: the batch's vectors; partial[row][vector of the batch][species][re, im], rowStride doubles per
// row.  x, y, z, type: by id, padded to a multiple of kSkIdTile (species -1 there).  T divides kSkIdTile; dynamic LDS: T * (h[0] + h[1] + h[2]) * 16 bytes.
__global__ __launch_bounds__(kBlock) void k_sk_amplitudes(SkGeom G, int nSpec, int T, int nIdTiles, int nvb, size_t rowStride, const int32_t* __restrict__ lmn,
                                                          const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                          const int32_t* __restrict__ type, double* __restrict__ partial)
{
    extern __shared__ __align__(16) double skLds[];
    __shared__ int sStart[kSpecCap + 1];                        // where the atoms of each species start in the tile
    cplx* tab = (cplx*)skLds;                                   // [T][nH]
    const int nH = G.h[0] + G.h[1] + G.h[2];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int off[kSkPerThread][3];
    double sm[kSkPerThread], sn[kSkPerThread];
    bool ok[kSkPerThread];
    size_t slot[kSkPerThread];
#pragma unroll
    for (int j = 0; j < kSkPerThread; j++)
    {
        const int v = blockIdx.x * kSkChunk + j * kBlock + threadIdx.x;
        ok[j] = v < nvb;
        const int l = ok[j] ? lmn[3 * v] : 0, m = ok[j] ? lmn[3 * v + 1] : 0, n = ok[j] ? lmn[3 * v + 2] : 0;
        off[j][0] = l; off[j][1] = G.h[0] + abs(m); off[j][2] = G.h[0] + G.h[1] + abs(n);
        sm[j] = m < 0 ? -1.0 : 1.0; sn[j] = n < 0 ? -1.0 : 1.0;
        slot[j] = (size_t)blockIdx.y * rowStride + (size_t)v * nSpec * 2;
    }
    bool first = true;
    for (int it = blockIdx.y; it < nIdTiles; it += gridDim.y)
        for (int base = it * kSkIdTile; base < (it + 1) * kSkIdTile; base += T)
        {
            __syncthreads();                                    // the tile before is done with
            if (w < 3)
            {   // wave w makes the tables of axis w; every one of the three finds the places of the atoms (lanes = atoms)
                const int id = base + lane;
                const int ty = lane < T ? type[id] : -1;
                int pos = -1, o = 0;
                for (int s = 0; s < nSpec; s++)
                {
                    const unsigned long long mask = __ballot(ty == s);
                    if (ty == s) pos = o + __popcll(mask & ((1ull << lane) - 1ull));
                    if (threadIdx.x == 0) sStart[s] = o;
                    o += __popcll(mask);
                }
                if (threadIdx.x == 0) sStart[nSpec] = o;
                if (pos >= 0)
                {
                    const double c = w == 0 ? x[id] : (w == 1 ? y[id] : z[id]);
                    const cplx e1 = sk_phase(c, G.L[w]);
                    cplx* out = tab + (size_t)pos * nH + (w == 0 ? 0 : (w == 1 ? G.h[0] : G.h[0] + G.h[1]));
                    cplx cur = e1;
                    out[0] = cplx{1.0, 0.0};
                    for (int h = 1; h < G.h[w]; h++)
                    {
                        out[h] = cur;
                        cur = sk_cmul(cur, e1);
                    }
                }
            }
            __syncthreads();
            for (int s = 0; s < nSpec; s++)
            {
                const int a0 = sStart[s], a1 = sStart[s + 1];
                if (a0 == a1 && !first) continue;               // (the first tile writes the +0.0 of a species it does not hold)
                double ac[kSkPerThread], as[kSkPerThread];
#pragma unroll
                for (int j = 0; j < kSkPerThread; j++)
                {
                    const bool load = ok[j] && !first;
                    ac[j] = load ? partial[slot[j] + 2 * s] : 0.0;
                    as[j] = load ? partial[slot[j] + 2 * s + 1] : 0.0;
                }
                for (int a = a0; a < a1; a++)
                {
                    const cplx* row = tab + (size_t)a * nH;
#pragma unroll
                    for (int j = 0; j < kSkPerThread; j++)
                    {
                        const cplx ex = row[off[j][0]];
                        cplx em = row[off[j][1]], en = row[off[j][2]];
                        em.s *= sm[j];                          // negative m, negative n: the complex conjugate
                        en.s *= sn[j];
                        const cplx ck = sk_cmul(sk_cmul(ex, em), en);
                        ac[j] = __dadd_rn(ac[j], ck.c);
                        as[j] = __dadd_rn(as[j], ck.s);
                    }
                }
#pragma unroll
                for (int j = 0; j < kSkPerThread; j++)
                    if (ok[j]) { partial[slot[j] + 2 * s] = ac[j]; partial[slot[j] + 2 * s + 1] = as[j]; }
            }
            first = false;
        }
}

// F(j, 256) = row j (+0.0 from row nB on), F(j, h) = F(j, 2h) + F(j + h, 2h): F(0, 1) is what folding the 256 rows by halving leaves in entry 0.
// F(w, 16) is the tree over the 16 rows w, w + 16, ...: one thread's share
template <int H> __device__ __forceinline__ double sk_fold_rows(const double* __restrict__ p, size_t rowStride, int j, int nB)
{
    if constexpr (H == kSkRows) return j < nB ? p[(size_t)j * rowStride] : 0.0;
    else return __dadd_rn(sk_fold_rows<2 * H>(p, rowStride, j, nB), sk_fold_rows<2 * H>(p, rowStride, j + H, nB));
}
constexpr int kSkFoldWaves = 16;
template <int H> __device__ __forceinline__ double sk_fold_waves(const double (*red)[kWave], int j, int lane)
{
    if constexpr (H == kSkFoldWaves) return red[j][lane];
    else return __dadd_rn(sk_fold_waves<2 * H>(red, j, lane), sk_fold_waves<2 * H>(red, j + H, lane));
}

// A workgroup of 16 waves folds 64 consecutive (vector of the batch, species, component) entries: lane <-> entry (coalesced row segments), wave w the
// sub-tree F(w, 16), wave 0 the four levels above it.  rho: the amplitudes of the batch's first vector onwards
__global__ __launch_bounds__(kWave* kSkFoldWaves) void k_sk_fold(int nB, size_t nEnt, size_t rowStride, const double* __restrict__ partial, double* __restrict__ rho)
{
    __shared__ double red[kSkFoldWaves][kWave];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t e = (size_t)blockIdx.x * kWave + lane;
    red[w][lane] = e < nEnt ? sk_fold_rows<kSkFoldWaves>(partial + e, rowStride, w, nB) : 0.0;
    __syncthreads();
    if (w == 0 && e < nEnt) rho[e] = sk_fold_waves<1>(red, 0, lane);
}

// thread <-> (vector, pair a <= b in the RDF's pair order): acc = acc + (re_a re_b + im_a im_b)
__global__ __launch_bounds__(kBlock) void k_sk_accumulate(int nK, int nSpec, int nPairs, const double* __restrict__ rho, double* __restrict__ acc)
{
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (size_t)nK * nPairs) return;
    const size_t v = e / nPairs;
    int p = (int)(e - v * nPairs), a = 0;
    while (p >= nSpec - a) { p -= nSpec - a; a++; }
    const int b = a + p;
    const double* r = rho + v * nSpec * 2;
    const double t = __dadd_rn(__dmul_rn(r[2 * a], r[2 * b]), __dmul_rn(r[2 * a + 1], r[2 * b + 1]));
    acc[e] = __dadd_rn(acc[e], t);
}

}  // namespace aztot
