// sparse_append_plan.h -- host-side planning of gpmpc_sparse_append (sparse_append.hip, driver in prepare.hip): the layout of the
// record gpmpc_prepare_sparse leaves for it, of the scratch vectors of the point at hand, and the shape of its two launches per
// point.  Plain C++ (no HIP), like prepare_sparse_plan.h; tools/host_checks/sparse_append_plan_check.cpp walks it under a sanitizer.
#pragma once
#include <cstddef>

namespace gpmpc_hip {

constexpr int kAppendThreads = 1024;                      // vector kernel: one workgroup per output, 16 wavefronts
constexpr int kAppendWaves = kAppendThreads / 64;
constexpr int kAppendTile = 64;                           // columns per wavefront of the transposed products and of the Yb' recurrence
constexpr int kAppendUpdThreads = 256;                    // update kernel: threads per workgroup ...
constexpr int kAppendUpdPerThread = 4;                    // ... and entries of iK_eff per thread of its element-wise workgroups

struct SparseAppendPlan {
    // the record (doubles into Handle::sprec; Yu stays where gpmpc_prepare_sparse keeps it, at the head of its workspace)
    size_t yb;               // Yb = LB^-1 (D, M, M)
    size_t w;                // w = V y (D, M)
    size_t noise;            // noises (D)
    // scratch of the point at hand, (D, M) each
    size_t p, c, d, g;
    size_t tau;              // (D)
    size_t t1, t2;           // the two intermediate vectors of beta_eff (D, M)
    size_t total;            // doubles
    // vector kernel: column tiles, row groups per tile of the transposed products, dynamic LDS
    int nct;                 // ceil(M / 64)
    int groups;              // row groups a column tile's sum is split into (>= 1): groups * nct work items on 16 wavefronts
    int rows_per_group;      // ceil(M / groups)
    size_t lds_part;         // doubles of the partial sums: groups * M
    size_t lds_bytes;
    // update kernel: workgroups of the Yb' recurrence (one per column tile) and of the rank-one update of iK_eff
    int upd_rec_blocks, upd_ik_blocks;
    size_t upd_lds_bytes;    // p, c, d of an output
};

// Needs M, D >= 1.  O(D M^2): nothing here depends on N or on the number of appended points.
inline void plan_sparse_append(int M, int D, SparseAppendPlan& p) {
    const size_t MM = (size_t)D * M * M, DM = (size_t)D * M;
    p.yb = 0;
    p.w = p.yb + MM;
    p.noise = p.w + DM;
    p.p = p.noise + (size_t)D;
    p.c = p.p + DM;
    p.d = p.c + DM;
    p.g = p.d + DM;
    p.tau = p.g + DM;
    p.t1 = p.tau + (size_t)D;
    p.t2 = p.t1 + DM;
    p.total = p.t2 + DM;
    p.nct = (M + kAppendTile - 1) / kAppendTile;
    p.groups = p.nct < kAppendWaves ? kAppendWaves / p.nct : 1;
    p.rows_per_group = (M + p.groups - 1) / p.groups;
    p.lds_part = (size_t)p.groups * M;
    // x / l and 1 / l (2 x 24) | kz, later q (M) | u (M) | p (M) | t (M + 1) | partial sums
    p.lds_bytes = sizeof(double) * (48 + 4 * (size_t)M + 1 + p.lds_part);
    p.upd_rec_blocks = p.nct;
    const size_t per_block = (size_t)kAppendUpdThreads * kAppendUpdPerThread;
    p.upd_ik_blocks = (int)(((size_t)M * M + per_block - 1) / per_block);
    p.upd_lds_bytes = sizeof(double) * 3 * (size_t)M;
}

}  // namespace gpmpc_hip
