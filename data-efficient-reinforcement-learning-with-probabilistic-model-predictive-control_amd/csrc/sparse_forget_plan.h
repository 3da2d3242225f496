// sparse_forget_plan.h -- host-side planning of gpmpc_sparse_forget (sparse_forget.hip, driver in prepare.hip): the layout of the
// scratch vectors of the point at hand and of the failure words, and the shape of its two launches per point.  The record it
// continues from is the append's (sparse_append_plan.h: Yb | w | noises in Handle::sprec), whose layout stays as it is; the launch
// shapes follow the append's rule, so the two calls refuse the same M.  Plain C++ (no HIP);
// tools/host_checks/sparse_forget_plan_check.cpp walks it under a sanitizer.
#pragma once
#include <cstddef>

#include "sparse_append_plan.h"

namespace gpmpc_hip {

constexpr int kForgetFailWords = 16;                      // one failure word per output (GPMPC_MAX_D), ints: 64 bytes

struct SparseForgetPlan {
    // doubles into Handle::spfg.  The failure words come first: the block a call clears starts at the allocation's start and is a
    // multiple of 16 bytes
    size_t fail;             // kForgetFailWords ints: 0, or 1 + the point of the call at which the output lost its pivot
    // scratch of the point at hand, (D, M) each
    size_t v, p, c, d, g;
    size_t tau;              // (D)
    size_t t1, t2;           // the two intermediate vectors of beta_eff (D, M)
    size_t total;            // doubles
    // chain kernel: column tiles, row groups per tile of the transposed products, dynamic LDS
    int nct;                 // ceil(M / 64)
    int groups;              // row groups a column tile's sum is split into (>= 1)
    int rows_per_group;      // ceil(M / groups)
    size_t lds_part;         // doubles of the partial sums: groups * M
    size_t lds_bytes;
    // update kernel: workgroups of the Yb' recurrence (one per column tile; the first also writes w') and of iK_eff
    int upd_rec_blocks, upd_ik_blocks;
    size_t upd_lds_bytes;    // p, c, d of an output
};

// Needs M, D >= 1.  O(D M): nothing here depends on N or on the number of removed points.
inline void plan_sparse_forget(int M, int D, SparseForgetPlan& p) {
    const size_t DM = (size_t)D * M;
    p.fail = 0;
    p.v = p.fail + kForgetFailWords * sizeof(int) / sizeof(double);
    p.p = p.v + DM;
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
    // x / l and 1 / l (2 x 24) | kz, later q (M) | u (M) | p (M) | t (M + 1) | partial sums | the workgroup's verdict (1)
    p.lds_bytes = sizeof(double) * (48 + 4 * (size_t)M + 1 + p.lds_part + 1);
    p.upd_rec_blocks = p.nct;
    const size_t per_block = (size_t)kAppendUpdThreads * kAppendUpdPerThread;
    p.upd_ik_blocks = (int)(((size_t)M * M + per_block - 1) / per_block);
    p.upd_lds_bytes = sizeof(double) * 3 * (size_t)M;
}

}  // namespace gpmpc_hip
