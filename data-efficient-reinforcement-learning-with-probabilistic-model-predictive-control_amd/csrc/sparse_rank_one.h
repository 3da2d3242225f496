// sparse_rank_one.h -- the two products with a lower-triangular factor that the rank-one recurrences of a sparse model share:
// gpmpc_sparse_append (sparse_append.hip) and gpmpc_sparse_forget (sparse_forget.hip) run the same chain of vectors with opposite
// signs.  Device code, included by those two files only; the shapes are those of sparse_append_plan.h.
#pragma once
#include "device_common.h"
#include "sparse_append_plan.h"

// every fused multiply-add here is written out as fma(), as in the files that include this: the sums round as gpmpc.h writes them
#pragma clang fp contract(off)

namespace gpmpc_hip {

namespace {

// a row of a lower-triangular matrix times x (LDS): lane-strided partial sums, then the xor tree -- every lane gets the total
__device__ inline double row_dot(const double* __restrict__ row, const double* x, int i, int lane) {
    double s = 0.0;
    for (int k = lane; k <= i; k += 64) s = fma(row[k], x[k], s);
    return wave_xor_sum(s);
}

// out = A^T x for a lower-triangular row-major A (M, M), x in LDS: work item (column tile, row group) per wavefront, lane = column,
// rows ascending inside a group (the first row of column j is j); then the groups' partial sums in group order
__device__ inline void trans_product(const double* __restrict__ A, const double* x, int M, int nct, int groups, int rpg,
                                     double* part, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int it = wave; it < nct * groups; it += kAppendWaves) {
        const int tile = it % nct, grp = it / nct;
        const int j = tile * kAppendTile + lane;
        if (j >= M) continue;
        const int r1 = (grp + 1) * rpg < M ? (grp + 1) * rpg : M;
        int i = grp * rpg > j ? grp * rpg : j;
        double s = 0.0;
#pragma unroll 4
        for (; i < r1; ++i) s = fma(A[(size_t)i * M + j], x[i], s);
        part[(size_t)grp * M + j] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < M; j += kAppendThreads) {
        double s = part[j];
        for (int q = 1; q < groups; ++q) s += part[(size_t)q * M + j];
        out[j] = s;
    }
    __syncthreads();
}

}  // namespace

}  // namespace gpmpc_hip
