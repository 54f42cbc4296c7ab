// Reciprocal-space part of the smooth particle-mesh Ewald sum ('elec spme', our directive; Essmann et al., J. Chem. Phys. 103, 8577 (1995)).
//
// The contract (DESIGN.md "Smooth particle-mesh Ewald" states it in full; tests/spme_model.py restates it in numpy):
//   u = K x / L per axis, f = floor(u), w = u - f; theta(j) = M_p(w + j), j = 0 .. p - 1, lands on mesh index (f - j) mod K; M_p the cardinal B-spline
//   Q(g)    = 2^-40 sum_i llrint(((q_i theta_x) theta_y) theta_z 2^40): 64-bit integer sums, the same whatever the order the atoms arrive in
//   FQ      = forward DFT of Q;  E = 1/2 scale sum_m G(m) |FQ(m)|^2;  phi = scale * inverse DFT (unnormalised) of G FQ, real part
//   F_i,a   = -q_i (K_a / L_a) sum_g phi(g) theta'_a theta_b theta_c over the atom's p^3 points
//
//   k_spme_spread      one wave per atom: lane <-> (tx, ty[, tz]) of the atom's p^3 points, 64-bit integer adds to the mesh (device scope)
//   k_spme_to_complex  integer mesh -> complex work mesh; clears the integer mesh for the next evaluation
//   k_spme_fft         batched 1-D transforms of <= 256 points in LDS, Stockham autosort, radix 4 (+ one radix-2 pass where log2 N is odd), twiddles
//                      from a table built on the host in long double; launched along x, y and z.  A workgroup holds a tile of 1024 points: for the
//                      strided axes the lines through adjacent x, so that every global access is a run of LT * 16 contiguous bytes.  The butterfly
//                      order is fixed: two evaluations of the same mesh agree to the bit, and nothing here allocates, synchronises or compiles
//                      at run time (no FFT library is linked)
//   k_spme_convolve    W = scale G FQ; energy partial per 256 points (wave_sum, tree_wave4: the samplers' sum tree)
//   k_spme_energy      tree_fold over the partials -> DevStats::engCoulRec
//   k_spme_gather      one wave per atom as in the spread; lane partial sums in tz order, then wave_sum; lane 0 adds the force to the atom's
// No floating-point atomics anywhere; weights are recomputed in the gather, not stored.
#pragma once
#include <hip/hip_runtime.h>

#include "device_md.h"
#include "kernels.hip.h"

namespace aztot {

constexpr double kSpmeFix = 1099511627776.0;         // 2^40: one unit of the integer mesh is 2^-40 e
constexpr int kSpmeTilePts = 1024;                   // complex points a workgroup of k_spme_fft holds (twice: the autosort ping-pongs)
constexpr int kSpmeAtomsPerBlock = kBlock / kWave;

// th[j] = M_P(w + j), dth[j] = M_{P-1}(w + j) - M_{P-1}(w + j - 1), j = 0 .. P - 1, by the recurrence
// M_n(u) = (u M_{n-1}(u) + (n - u) M_{n-1}(u - 1)) / (n - 1) from M_2(u) = 1 - |u - 1|, in place from the top index down
template <int P>
__device__ __forceinline__ void spme_weights(double w, double (&th)[P], double (&dth)[P])
{
#pragma unroll
    for (int j = 0; j < P; j++) th[j] = 0.0;
    th[0] = w; th[1] = 1.0 - w;
#pragma unroll
    for (int n = 3; n <= P; n++)
    {
        if (n == P)
        {
#pragma unroll
            for (int j = P - 1; j >= 1; j--) dth[j] = th[j] - th[j - 1];
            dth[0] = th[0];
        }
        const double div = 1.0 / (double)(n - 1);
#pragma unroll
        for (int j = P - 1; j >= 1; j--)       // (constant bounds, so that every index is known when the loops are unrolled: the arrays stay in registers)
            if (j <= n - 1) th[j] = div * ((w + (double)j) * th[j] + ((double)(n - j) - w) * th[j - 1]);
        th[0] = div * (w * th[0]);
    }
}

template <int P>
__device__ __forceinline__ double spme_pick(const double (&a)[P], int j)
{
    // a[j] without an indexed read (which would put the array into scratch): the one term with j == k survives, exactly (the weights are finite)
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < P; k++) v += a[k] * (j == k ? 1.0 : 0.0);
    return v;
}

// where an atom sits on one axis: f = floor(K x / L) (any integer: a lazily sorted atom may lie outside [0, L)), w in [0, 1]
__device__ __forceinline__ int spme_cell(double x, int K, double L, double& w)
{
    const double u = ((double)K * x) / L;
    const double fl = floor(u);
    w = u - fl;
    return (int)fl;
}

// lanes of the wave that owns an atom: lane = tx + P ty + P^2 tz0; the wave visits tz = tz0, tz0 + NZ, ... (NZ = 4 for P = 4, else 1)
template <int P>
struct SpmeLanes
{
    static constexpr int NZ = (64 / (P * P)) > 0 ? 64 / (P * P) : 1;
    static constexpr int ITER = P / NZ;
};

template <int P>
__global__ __launch_bounds__(kBlock) void k_spme_spread(StepParams Pm, SpecTable S, AtomArrays A, const Counts* __restrict__ cnt, SpmeTables M)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int i = cnt->ownedBegin + blockIdx.x * kSpmeAtomsPerBlock + (int)(threadIdx.x >> 6);      // wave-uniform
    if (i >= cnt->ownedEnd) return;
    const double q = S.charge[A.type[i]];
    if (q == 0.0) return;
    double thx[P], thy[P], thz[P], dth[P], wx, wy, wz;
    const int fx = spme_cell(A.x[i], M.K[0], Pm.L[0], wx), fy = spme_cell(A.y[i], M.K[1], Pm.L[1], wy), fz = spme_cell(A.z[i], M.K[2], Pm.L[2], wz);
    spme_weights<P>(wx, thx, dth);
    spme_weights<P>(wy, thy, dth);
    spme_weights<P>(wz, thz, dth);
    constexpr int NZ = SpmeLanes<P>::NZ;
    const int txy = lane % (P * P), tz0 = lane / (P * P);
    if (tz0 >= NZ) return;
    const int tx = txy % P, ty = txy / P;
    const double qxy = __dmul_rn(__dmul_rn(q, spme_pick<P>(thx, tx)), spme_pick<P>(thy, ty));
    const int gx = (fx - tx) & (M.K[0] - 1), gy = (fy - ty) & (M.K[1] - 1);
    unsigned long long* mesh = (unsigned long long*)M.Qi;
#pragma unroll
    for (int k = 0; k < SpmeLanes<P>::ITER; k++)
    {
        const int tz = tz0 + k * NZ;
        const double c = __dmul_rn(qxy, NZ == 1 ? thz[k] : spme_pick<P>(thz, tz));
        const long long v = __double2ll_rn(__dmul_rn(c, kSpmeFix));
        const int gz = (fz - tz) & (M.K[2] - 1);
        if (v != 0) atomicAdd(mesh + ((size_t)gz * M.K[1] + gy) * M.K[0] + gx, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kBlock) void k_spme_to_complex(SpmeTables M)
{
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= M.nPts) return;
    const long long v = M.Qi[g];
    M.Qi[g] = 0;
    reinterpret_cast<double2*>(M.W)[g] = make_double2((double)v * (1.0 / kSpmeFix), 0.0);
}

__device__ __forceinline__ double2 spme_cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 spme_csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
// a * w, w the table's forward twiddle (cos, -sin); INV: its conjugate
template <bool INV>
__device__ __forceinline__ double2 spme_ctw(double2 a, double2 w)
{
    const double s = INV ? -w.y : w.y;
    return make_double2(a.x * w.x - a.y * s, a.x * s + a.y * w.x);
}

// Stockham autosort, decimation in frequency: a pass of radix r at sub-length n and stride s (n s = N, or N LT where the tile's lines are interleaved)
// reads x[q + s (p + k n / r)] and writes y[q + s (r p + k)], k = 0 .. r - 1, p < n / r, q < s; a stride s pass is s interleaved transforms, so a tile
// of the strided axes - LT lines, element e of line l at e LT + l - is ONE transform run from s = LT.  The output is in natural order.
template <bool INV>
__global__ __launch_bounds__(kBlock) void k_spme_fft(double* __restrict__ mesh, const double* __restrict__ twiddle, SpmeAxis ax)
{
    __shared__ double2 buf[2][kSpmeTilePts];
    __shared__ double2 tw[256];
    double2* W = reinterpret_cast<double2*>(mesh);
    const int N = ax.N, LT = ax.LT, pts = N * LT;
    const size_t base = (size_t)(blockIdx.x / ax.tilesPerRow) * (size_t)ax.outerStride + (size_t)(blockIdx.x % ax.tilesPerRow) * LT;
    if ((int)threadIdx.x < N) tw[threadIdx.x] = reinterpret_cast<const double2*>(twiddle)[threadIdx.x];
    for (int idx = threadIdx.x; idx < pts; idx += kBlock)
    {
        const size_t g = ax.contiguous ? base + idx : base + (size_t)(idx % LT) + (size_t)(idx / LT) * (size_t)ax.elemStride;
        buf[0][idx] = W[g];
    }
    __syncthreads();
    int cur = 0, n = N, logS = 0, s0 = ax.contiguous ? 1 : LT;       // stride s = s0 << logS
    while (n >= 4)
    {
        const double2* x = buf[cur];
        double2* y = buf[cur ^ 1];
        const int n1 = n >> 2, s = s0 << logS, perLine = N >> 2, tstep = N / n;
        for (int j = threadIdx.x; j < (pts >> 2); j += kBlock)
        {
            const int off = ax.contiguous ? (j / perLine) * N : 0, jj = ax.contiguous ? j % perLine : j;
            const int p = jj / s, q = jj % s;
            const double2 a = x[off + q + s * p], b = x[off + q + s * (p + n1)], c = x[off + q + s * (p + 2 * n1)], d = x[off + q + s * (p + 3 * n1)];
            const double2 apc = spme_cadd(a, c), amc = spme_csub(a, c), bpd = spme_cadd(b, d), bmd = spme_csub(b, d);
            const double2 jbmd = make_double2(-bmd.y, bmd.x);                       // i (b - d)
            const double2 t1 = INV ? spme_cadd(amc, jbmd) : spme_csub(amc, jbmd), t3 = INV ? spme_csub(amc, jbmd) : spme_cadd(amc, jbmd);
            y[off + q + s * (4 * p)] = spme_cadd(apc, bpd);
            y[off + q + s * (4 * p + 1)] = spme_ctw<INV>(t1, tw[p * tstep]);
            y[off + q + s * (4 * p + 2)] = spme_ctw<INV>(spme_csub(apc, bpd), tw[2 * p * tstep]);
            y[off + q + s * (4 * p + 3)] = spme_ctw<INV>(t3, tw[3 * p * tstep]);
        }
        __syncthreads();
        cur ^= 1; n >>= 2; logS += 2;
    }
    if (n == 2)
    {   // the last pass where log2 N is odd: p = 0, no twiddle
        const double2* x = buf[cur];
        double2* y = buf[cur ^ 1];
        const int s = s0 << logS, perLine = N >> 1;
        for (int j = threadIdx.x; j < (pts >> 1); j += kBlock)
        {
            const int off = ax.contiguous ? (j / perLine) * N : 0, q = ax.contiguous ? j % perLine : j;
            const double2 a = x[off + q], b = x[off + q + s];
            y[off + q] = spme_cadd(a, b);
            y[off + q + s] = spme_csub(a, b);
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int idx = threadIdx.x; idx < pts; idx += kBlock)
    {
        const size_t g = ax.contiguous ? base + idx : base + (size_t)(idx % LT) + (size_t)(idx / LT) * (size_t)ax.elemStride;
        W[g] = buf[cur][idx];
    }
}

// W = scale G FQ (the inverse transform then gives phi); workgroup b leaves sum G |FQ|^2 over its 256 points in partial[b]: wave_sum over each
// run of 64 points, tree_wave4 over the four runs
__global__ __launch_bounds__(kBlock) void k_spme_convolve(SpmeTables M)
{
    __shared__ double runs[kBlock / kWave];
    const int g = blockIdx.x * kBlock + threadIdx.x;           // nPts is a multiple of 256
    double2* W = reinterpret_cast<double2*>(M.W);
    const double2 f = W[g];
    const double Gm = M.G[g];
    const double e = __dmul_rn(Gm, __dadd_rn(__dmul_rn(f.x, f.x), __dmul_rn(f.y, f.y)));
    const double t = __dmul_rn(Gm, M.scale);
    W[g] = make_double2(__dmul_rn(t, f.x), __dmul_rn(t, f.y));
    const double r = wave_sum(e);
    if ((threadIdx.x & (kWave - 1)) == 0) runs[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) M.partial[blockIdx.x] = tree_wave4(runs);
}

// engCoulRec = 1/2 scale sum_m G |FQ|^2: tree_fold over the partials (their number is a power of two)
__global__ __launch_bounds__(kBlock) void k_spme_energy(SpmeTables M, DevStats* st)
{
    const double sum = tree_fold(M.partial, M.nPts / kBlock);
    if (threadIdx.x == 0) st->engCoulRec = __dmul_rn(__dmul_rn(0.5, M.scale), sum);
}

template <int P>
__global__ __launch_bounds__(kBlock) void k_spme_gather(StepParams Pm, SpecTable S, AtomArrays A, const Counts* __restrict__ cnt, SpmeTables M)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int i = cnt->ownedBegin + blockIdx.x * kSpmeAtomsPerBlock + (int)(threadIdx.x >> 6);      // wave-uniform
    if (i >= cnt->ownedEnd) return;
    const double q = S.charge[A.type[i]];
    if (q == 0.0) return;
    double thx[P], thy[P], thz[P], dthx[P], dthy[P], dthz[P], wx, wy, wz;
    const int fx = spme_cell(A.x[i], M.K[0], Pm.L[0], wx), fy = spme_cell(A.y[i], M.K[1], Pm.L[1], wy), fz = spme_cell(A.z[i], M.K[2], Pm.L[2], wz);
    spme_weights<P>(wx, thx, dthx);
    spme_weights<P>(wy, thy, dthy);
    spme_weights<P>(wz, thz, dthz);
    constexpr int NZ = SpmeLanes<P>::NZ;
    const int txy = lane % (P * P), tz0 = lane / (P * P);
    const bool live = tz0 < NZ;
    const int tx = txy % P, ty = txy / P;
    const double ax = spme_pick<P>(thx, tx), ay = spme_pick<P>(thy, ty), dax = spme_pick<P>(dthx, tx), day = spme_pick<P>(dthy, ty);
    const double txy_ = ax * ay, dxy = dax * ay, xdy = ax * day;
    const int gx = (fx - tx) & (M.K[0] - 1), gy = (fy - ty) & (M.K[1] - 1);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (live)
    {
#pragma unroll
        for (int k = 0; k < SpmeLanes<P>::ITER; k++)
        {
            const int tz = tz0 + k * NZ;
            const double az = NZ == 1 ? thz[k] : spme_pick<P>(thz, tz), daz = NZ == 1 ? dthz[k] : spme_pick<P>(dthz, tz);
            const int gz = (fz - tz) & (M.K[2] - 1);
            const double phi = M.W[2 * (((size_t)gz * M.K[1] + gy) * M.K[0] + gx)];
            sx += phi * (dxy * az);
            sy += phi * (xdy * az);
            sz += phi * (txy_ * daz);
        }
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    if (lane == 0)
    {
        A.fx[i] += -q * M.KoverL[0] * sx;
        A.fy[i] += -q * M.KoverL[1] * sy;
        A.fz[i] += -q * M.KoverL[2] * sz;
    }
}

}  // namespace aztot
