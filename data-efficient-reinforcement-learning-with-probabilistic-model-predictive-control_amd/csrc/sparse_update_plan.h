// sparse_update_plan.h -- host-side planning of gpmpc_sparse_append and gpmpc_sparse_forget (sparse_update.hip, driver in
// prepare.hip): the layout of the record gpmpc_prepare_sparse leaves for them, of the scratch block both calls use (the failure words
// of the forget and the vectors of the point at hand), and the shape of the two launches per point.  One plan for both signs, so the
// two calls refuse the same M.  Plain C++ (no HIP), like prepare_sparse_plan.h; tools/host_checks/sparse_update_plan_check.cpp walks
// it under a sanitizer.
#pragma once
#include <cstddef>

namespace gpmpc_hip {

constexpr int kUpdVecThreads = 1024;                      // vectors kernel: one workgroup per output, 16 wavefronts
constexpr int kUpdVecWaves = kUpdVecThreads / 64;
constexpr int kUpdTile = 64;                              // columns per wavefront of the transposed products and of the Yb' recurrence
constexpr int kUpdThreads = 256;                          // update kernel: threads per workgroup ...
constexpr int kUpdPerThread = 4;                          // ... and entries of iK_eff per thread of its element-wise workgroups
constexpr int kUpdFailWords = 16;                         // one failure word per output (GPMPC_MAX_D), ints: 64 bytes

struct SparseUpdatePlan {
    // the record (doubles into Handle::sprec; Yu stays where gpmpc_prepare_sparse keeps it, at the head of its workspace)
    size_t yb;               // Yb = LB^-1 (D, M, M)
    size_t w;                // w = V y (D, M)
    size_t noise;            // noises (D)
    size_t rec_total;        // doubles
    // the scratch (doubles into Handle::spupd).  The failure words come first: the block a forget clears starts at the allocation's
    // start and is a multiple of 16 bytes
    size_t fail;             // kUpdFailWords ints: 0, or 1 + the point of the call at which the output lost its pivot
    size_t v, p, c, d, g;    // vectors of the point at hand, (D, M) each (v: the forget's alone)
    size_t tau;              // (D)
    size_t t1, t2;           // the two intermediate vectors of beta_eff (D, M)
    size_t ws_total;         // doubles
    // vectors kernel: column tiles, row groups per tile of the transposed products, dynamic LDS
    int nct;                 // ceil(M / 64)
    int groups;              // row groups a column tile's sum is split into (>= 1): groups * nct work items on 16 wavefronts
    int rows_per_group;      // ceil(M / groups)
    size_t lds_part;         // doubles of the partial sums: groups * M
    size_t lds_bytes;        // of both signs: the forget's verdict is the last double, which the append leaves alone
    // update kernel: workgroups of the Yb' recurrence (one per column tile; the forget's first also writes w') and of iK_eff
    int upd_rec_blocks, upd_ik_blocks;
    size_t upd_lds_bytes;    // p, c, d of an output
};

// Needs M, D >= 1.  O(D M^2): nothing here depends on N or on the number of points of a call.
inline void plan_sparse_update(int M, int D, SparseUpdatePlan& p) {
    const size_t MM = (size_t)D * M * M, DM = (size_t)D * M;
    p.yb = 0;
    p.w = p.yb + MM;
    p.noise = p.w + DM;
    p.rec_total = p.noise + (size_t)D;
    p.fail = 0;
    p.v = p.fail + kUpdFailWords * sizeof(int) / sizeof(double);
    p.p = p.v + DM;
    p.c = p.p + DM;
    p.d = p.c + DM;
    p.g = p.d + DM;
    p.tau = p.g + DM;
    p.t1 = p.tau + (size_t)D;
    p.t2 = p.t1 + DM;
    p.ws_total = p.t2 + DM;
    p.nct = (M + kUpdTile - 1) / kUpdTile;
    p.groups = p.nct < kUpdVecWaves ? kUpdVecWaves / p.nct : 1;
    p.rows_per_group = (M + p.groups - 1) / p.groups;
    p.lds_part = (size_t)p.groups * M;
    // x / l and 1 / l (2 x 24) | kz, later q (M) | u (M) | p (M) | t (M + 1) | partial sums | the workgroup's verdict (1)
    p.lds_bytes = sizeof(double) * (48 + 4 * (size_t)M + 1 + p.lds_part + 1);
    p.upd_rec_blocks = p.nct;
    const size_t per_block = (size_t)kUpdThreads * kUpdPerThread;
    p.upd_ik_blocks = (int)(((size_t)M * M + per_block - 1) / per_block);
    p.upd_lds_bytes = sizeof(double) * 3 * (size_t)M;
}

}  // namespace gpmpc_hip
