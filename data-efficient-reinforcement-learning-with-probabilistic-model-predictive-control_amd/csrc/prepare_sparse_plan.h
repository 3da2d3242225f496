// prepare_sparse_plan.h -- host-side planning of gpmpc_prepare_sparse (prepare_sparse.hip, driver in prepare.hip): how many memory
// points a chunk of the stream holds and how the workspace is laid out.  Plain C++ (no HIP), like moments_linear_plan.h.
#pragma once
#include <cstddef>

namespace gpmpc_hip {

constexpr int kSparseTile = 64;                           // points per column tile of the panel; chunks are multiples of it
constexpr size_t kSparseWsBudget = (size_t)64 << 20;      // bytes of one chunk's Kuf and V (or one 64-point chunk's need if that is more)
constexpr int kSparseLanes = 64;                          // partial sums of w = V y per (output, inducing point): point n adds to n mod 64

struct SparsePlan {
    int chunk;               // points per chunk: a multiple of 64 (the last chunk may hold fewer)
    size_t yu;               // offsets (doubles) into the workspace: Yu = Lu^-1 (D, M, M)
    size_t r;                //   R = (I - Yb^T Yb) Yu (D, M, M)
    size_t wpart;            //   partial sums of w (D, M, 64)
    size_t w;                //   w (D, M)
    size_t jit;              //   jitter_rel * outputscale (D)
    size_t kuf;              //   the chunk's cross-Gram panel (D, M, chunk)
    size_t v;                //   the chunk's whitened panel V = Yu Kuf (D, M, chunk)
    size_t total;            // doubles
};

// opt_chunk: option "sparse_chunk_points" (0 = auto, else a multiple of 64).  Needs N, M, D >= 1.  Nothing here is of size N x N or
// M x N: O(D M^2) plus the two panels of one chunk.
inline void plan_prepare_sparse(int N, int M, int D, int opt_chunk, SparsePlan& p) {
    const size_t per_point = 2 * sizeof(double) * (size_t)D * (size_t)M;
    long long chunk = (long long)(kSparseWsBudget / per_point) / kSparseTile * kSparseTile;
    if (opt_chunk > 0) chunk = opt_chunk;
    if (chunk < kSparseTile) chunk = kSparseTile;
    const long long n64 = ((long long)N + kSparseTile - 1) / kSparseTile * kSparseTile;
    if (chunk > n64) chunk = n64;
    p.chunk = (int)chunk;
    const size_t MM = (size_t)D * M * M, DM = (size_t)D * M;
    p.yu = 0;
    p.r = p.yu + MM;
    p.wpart = p.r + MM;
    p.w = p.wpart + DM * kSparseLanes;
    p.jit = p.w + DM;
    p.kuf = p.jit + (size_t)D;
    p.v = p.kuf + DM * (size_t)chunk;
    p.total = p.v + DM * (size_t)chunk;
}

}  // namespace gpmpc_hip
