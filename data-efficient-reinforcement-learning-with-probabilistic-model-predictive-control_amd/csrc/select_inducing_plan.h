// select_inducing_plan.h -- host-side planning of gpmpc_select_inducing (select_inducing.hip): how the call's workspace is laid out
// and whether it stays under the cap.  Plain C++ (no HIP), like prepare_sparse_plan.h.
#pragma once
#include <cstddef>

#include "prepare_sparse_plan.h"

namespace gpmpc_hip {

constexpr unsigned long long kSelectDefaultMaxMb = 4096;      // cap on the workspace (option "select_inducing_max_mb")
constexpr int kSelectStage = 64;                              // rows of L_a[., p] a workgroup stages in LDS at a time

struct SelectPlan {
    int tiles;               // 64-point tiles: one workgroup each
    size_t L;                // offsets (doubles) into the workspace: the partial Cholesky factors (D, M, N), N contiguous
    size_t d;                //   residual variances, two generations (2, D, N): step m reads (m - 1) & 1, writes m & 1
    size_t tpart;            //   per-(step, tile) partial traces (M, tiles)
    size_t rec_score;        //   tile records, two generations: best score (2, tiles) ...
    size_t rec_index;        //   ... and its point (2, tiles) ints
    size_t picks;            //   the picks p_0 .. p_{M-1} (M) ints
    size_t picked;           //   flags of the points picked so far (N) ints
    size_t total;            // doubles
    unsigned long long bytes;   // total in bytes (saturates at ~0ULL when the product overflows)
};

// Needs 1 <= M <= N, D >= 1.  Returns false when the workspace is beyond max_mb MiB or its size overflows 64 bits (p.bytes then
// holds the size, saturated): the D M N doubles of L are the cost of the method.
inline bool plan_select_inducing(int N, int M, int D, unsigned long long max_mb, SelectPlan& p) {
    typedef unsigned long long u64;
    const u64 n = (u64)N, m = (u64)M, dd = (u64)D;
    const u64 tiles = (n + kSparseTile - 1) / kSparseTile;
    p.tiles = (int)tiles;
    u64 total = 0, term = 0;
    bool over = false;
    auto add = [&](u64 a, u64 b, u64 c) {                     // total += a b c, with the offset before it as the result
        const u64 at = total;
        over = over || __builtin_mul_overflow(a, b, &term) || __builtin_mul_overflow(term, c, &term) ||
               __builtin_add_overflow(total, term, &total);
        return (size_t)at;
    };
    p.L = add(dd, m, n);
    p.d = add(2 * dd, n, 1);
    p.tpart = add(m, tiles, 1);
    p.rec_score = add(2, tiles, 1);
    p.rec_index = add(tiles, 1, 1);                           // 2 tiles ints
    p.picks = add((m + 1) / 2, 1, 1);
    p.picked = add((n + 1) / 2, 1, 1);
    p.total = (size_t)total;
    u64 bytes = 0;
    over = over || __builtin_mul_overflow(total, (u64)sizeof(double), &bytes);
    p.bytes = over ? ~0ULL : bytes;
    u64 cap = 0;
    if (__builtin_mul_overflow(max_mb, (u64)1 << 20, &cap)) cap = ~0ULL;
    return !over && bytes <= cap;
}

}  // namespace gpmpc_hip
