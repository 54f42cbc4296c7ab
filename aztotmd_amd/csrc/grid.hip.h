// The samplers' private cell grid (RdfGrid; Samplers::grid_setup sizes it): the counting sort of the current positions into it, the canonical in-cell
// order, and the sliced walk over an atom's neighbour cells.  Every sampler that looks at pairs of atoms is built from these pieces, and the documented
// order of its sums (include/aztot.h) is the order written here, once.
//
//  k_grid_bin + k_scan_* + k_grid_place   counting sort: wrapped coordinates and species | nucleus << 8 in slot order (cells by position)
//  k_grid_slot_ids                        the slot -> atom id map of a sort
//  k_grid_canon_rank                      the arrival rank k_grid_bin hands out replaced by the rank of the atom's id among its cell-mates: placed by that
//                                         rank, the slot order is canonical - a function of the sampled state alone
//  SliceLane, grid_walk, slice_fold       lanes = (atom in slot order, slice of the candidates); every candidate of every neighbour cell; the fold of an
//                                         atom's slices
//
// Only engine state is READ (positions, species, ids); nothing the step uses is written.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hip.h"

namespace aztot {

__device__ __forceinline__ int rdf_cell(const RdfGrid& G, double x, double y, double z)
{
    return (cell_coord(x, G.icsz[0], G.nc[0]) * G.nc[1] + cell_coord(y, G.icsz[1], G.nc[1])) * G.nc[2] + cell_coord(z, G.icsz[2], G.nc[2]);
}

// position as aztot_md_to_host hands it out: a lazy run keeps coordinates unwrapped between two sorts (put_periodic, box.cpp:230-295)
__device__ __forceinline__ void rdf_wrapped(const RdfGrid& G, const AtomArrays& A, int i, double& x, double& y, double& z)
{
    x = A.x[i]; y = A.y[i]; z = A.z[i];
    wrap_coord(x, G.L[0], G.invL[0]);
    wrap_coord(y, G.L[1], G.invL[1]);
    wrap_coord(z, G.L[2], G.invL[2]);
}

// pass 1 of the counting sort: cell of every atom and its arrival rank inside the cell
__global__ __launch_bounds__(kBlock) void k_grid_bin(RdfGrid G, AtomArrays A, int n, int32_t* __restrict__ cellOf, int32_t* __restrict__ rankOf,
                                                     int32_t* __restrict__ cellCount)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    rdf_wrapped(G, A, i, x, y, z);
    const int c = rdf_cell(G, x, y, z);
    cellOf[i] = c;
    rankOf[i] = atomicAdd(&cellCount[c], 1);
}

// pass 2: wrapped position and (species | nucleus << 8) of every atom at its slot of the grid
__global__ __launch_bounds__(kBlock) void k_grid_place(RdfGrid G, AtomArrays A, int n, const int32_t* __restrict__ cellOf, const int32_t* __restrict__ rankOf,
                                                       const int32_t* __restrict__ cellStart, double* __restrict__ sx, double* __restrict__ sy,
                                                       double* __restrict__ sz, int32_t* __restrict__ sKind)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    rdf_wrapped(G, A, i, x, y, z);
    const int s = cellStart[cellOf[i]] + rankOf[i];
    const int t = A.type[i];
    sx[s] = x; sy[s] = y; sz[s] = z;
    sKind[s] = t | (G.nucl[t] << 8);
}

// slot of every atom in the sorted order (the inverse is what a reader needs: atom id of each slot)
__global__ __launch_bounds__(kBlock) void k_grid_slot_ids(AtomArrays A, int n, const int32_t* __restrict__ cellOf, const int32_t* __restrict__ rankOf,
                                                          const int32_t* __restrict__ cellStart, int32_t* __restrict__ slotId)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    slotId[cellStart[cellOf[i]] + rankOf[i]] = A.id[i];
}

// rank of every atom's id among the ids of its cell: arrivalId is the slot -> id map of the arrival order (k_grid_slot_ids)
__global__ __launch_bounds__(kBlock) void k_grid_canon_rank(AtomArrays A, int n, const int32_t* __restrict__ cellOf, const int32_t* __restrict__ cellStart,
                                                            const int32_t* __restrict__ arrivalId, int32_t* __restrict__ rankOf)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int c = cellOf[i], id = A.id[i];
    int r = 0;
    for (int s = cellStart[c]; s < cellStart[c + 1]; s++) r += arrivalId[s] < id ? 1 : 0;
    rankOf[i] = r;
}

// u = r_j - r_i after delta_periodic (box.cpp:297-305), and r2 = (ux*ux + uy*uy) + uz*uz with every operation rounded on its own (no contraction): the
// same rounding as the host's
__device__ __forceinline__ double grid_sep(const RdfGrid& G, double xi, double yi, double zi, double xj, double yj, double zj, double& ux, double& uy, double& uz)
{
    ux = xj - xi; uy = yj - yi; uz = zj - zi;
    min_image(ux, G.L[0], G.half[0]);
    min_image(uy, G.L[1], G.half[1]);
    min_image(uz, G.L[2], G.half[2]);
    return __dadd_rn(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)), __dmul_rn(uz, uz));
}

// the neighbour cells of cell (cx, cy, cz): 27, or each distinct one where an axis has fewer than 3; f(first slot, one past the last slot) per cell,
// dx, dy, dz from low to high, dz fastest
template <typename F> __device__ __forceinline__ void grid_cells(const RdfGrid& G, const int32_t* __restrict__ cellStart, int cx, int cy, int cz, F&& f)
{
    const int lo[3] = {G.nc[0] >= 3 ? -1 : 0, G.nc[1] >= 3 ? -1 : 0, G.nc[2] >= 3 ? -1 : 0};
    const int hi[3] = {G.nc[0] >= 2 ? 1 : 0, G.nc[1] >= 2 ? 1 : 0, G.nc[2] >= 2 ? 1 : 0};
    for (int dx = lo[0]; dx <= hi[0]; dx++)
        for (int dy = lo[1]; dy <= hi[1]; dy++)
            for (int dz = lo[2]; dz <= hi[2]; dz++)
            {
                int ex = cx + dx, ey = cy + dy, ez = cz + dz;
                ex += ex < 0 ? G.nc[0] : (ex >= G.nc[0] ? -G.nc[0] : 0);
                ey += ey < 0 ? G.nc[1] : (ey >= G.nc[1] ? -G.nc[1] : 0);
                ez += ez < 0 ? G.nc[2] : (ez >= G.nc[2] ? -G.nc[2] : 0);
                const int c = (ex * G.nc[1] + ey) * G.nc[2] + ez;
                f(cellStart[c], cellStart[c + 1]);
            }
}

// Lane t of a launch of lane_blocks(sliceShift) workgroups is (atom t >> sliceShift in slot order, slice t & (S - 1)), S = 1 << sliceShift <= 64 lanes of
// one wave per atom.  Lanes past the last atom have i >= n: they walk nothing and take part in the fold with zeros.
struct SliceLane
{
    int i, slice, S;
    __device__ __forceinline__ explicit SliceLane(int sliceShift) : S(1 << sliceShift)
    {
        const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
        i = (int)(t >> sliceShift);
        slice = (int)(t & (S - 1));
    }
};

// The walk of one lane of the atom at (xi, yi, zi): every slice visits all the neighbour cells in the order of grid_cells and takes the candidates
// start + slice, + S, ... of each, so S = 1 is the one-thread-per-atom walk and S = 64 reads a cell's atoms as one coalesced row.
// visit(j, ux, uy, uz, r2, acc...) with grid_sep's u = r_j - r_i and r2, for every candidate, j == i included: the self rule is the caller's.
// acc...: what the visitor adds to, handed through to it as arguments, where that serves the kernel: a visitor that captures its register accumulators
// costs k_cn_pairs and k_stress_pairs two to four VGPRs against the loop written out in the kernel, as arguments they cost none; k_boo_* measure the
// other way round (up to 28 VGPRs more with arguments) and capture theirs.  `make resource-usage` is the judge.
template <typename F, typename... Acc>
__device__ __forceinline__ void grid_walk(const RdfGrid& G, const int32_t* __restrict__ cellStart, const SliceLane& lane, double xi, double yi, double zi,
                                          const double* __restrict__ sx, const double* __restrict__ sy, const double* __restrict__ sz, F&& visit, Acc&... acc)
{
    grid_cells(G, cellStart, cell_coord(xi, G.icsz[0], G.nc[0]), cell_coord(yi, G.icsz[1], G.nc[1]), cell_coord(zi, G.icsz[2], G.nc[2]), [&](int s0, int s1) {
        for (int j = s0 + lane.slice; j < s1; j += lane.S)
        {
            double ux, uy, uz;
            const double r2 = grid_sep(G, xi, yi, zi, sx[j], sy[j], sz[j], ux, uy, uz);
            visit(j, ux, uy, uz, r2, acc...);
        }
    });
}

// the slices of an atom (neighbouring lanes of one wave) folded in the fixed order of strides 1, 2, 4, ...; every lane of the wave must call it.  The array
// form folds each element as the scalar form does, with the independent exchanges of a stride issued together
template <typename T> __device__ __forceinline__ T slice_fold(T v, int S)
{
    for (int m = 1; m < S; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
template <typename T, int N> __device__ __forceinline__ void slice_fold(T (&v)[N], int S)
{
    for (int m = 1; m < S; m <<= 1)
    {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] += __shfl_xor(v[k], m);
    }
}

}  // namespace aztot
