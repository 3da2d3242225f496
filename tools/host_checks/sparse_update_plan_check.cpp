// Stand-alone host check of plan_sparse_update (csrc/sparse_update_plan.h): lays out the record and the scratch block of
// gpmpc_sparse_append / gpmpc_sparse_forget over a grid of shapes and walks, on the host, every index the two kernels of a point
// may form with either sign -- the global offsets into the record and the scratch buffers, the failure words at the scratch's start
// and the LDS offsets of both kernels -- inside buffers of the planned sizes.  One plan serves both calls, so they refuse the same M:
// the largest accepted one is asserted as a literal.  Build with a host sanitizer and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_checks/sparse_update_plan_check.cpp -o plan_check && ./plan_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd/csrc/sparse_update_plan.h"

using namespace gpmpc_hip;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static void one(int M, int D) {
    SparseUpdatePlan p;
    plan_sparse_update(M, D, p);
    const size_t MM = (size_t)D * M * M, DM = (size_t)D * M;
    // the record: the regions follow each other without gaps or overlap, D M^2 + D M + D doubles with the Yu kept elsewhere
    CHECK(p.yb == 0 && p.w == MM && p.noise == p.w + DM && p.rec_total == p.noise + (size_t)D);
    // the scratch: the same; the failure words are whole ints at the buffer's start, a block of a multiple of 16 bytes
    CHECK(p.fail == 0 && D <= kUpdFailWords && kUpdFailWords * sizeof(int) % 16 == 0);
    CHECK(p.v * sizeof(double) == kUpdFailWords * sizeof(int));
    CHECK(p.p == p.v + DM && p.c == p.p + DM && p.d == p.c + DM && p.g == p.d + DM && p.tau == p.g + DM);
    CHECK(p.t1 == p.tau + (size_t)D && p.t2 == p.t1 + DM && p.ws_total == p.t2 + DM);
    CHECK(p.ws_total == 7 * DM + (size_t)D + kUpdFailWords * sizeof(int) / sizeof(double));
    // the transposed products: every column tile and every row is covered by exactly the planned work items
    CHECK(p.nct == (M + 63) / 64 && p.groups >= 1 && p.rows_per_group >= 1);
    CHECK((long long)p.groups * p.rows_per_group >= M);
    CHECK(p.groups == 1 || p.groups * p.nct <= kUpdVecWaves);
    CHECK(p.lds_part == (size_t)p.groups * M);
    CHECK(p.lds_bytes == sizeof(double) * (48 + 4 * (size_t)M + 1 + p.lds_part + 1));
    CHECK(p.upd_rec_blocks == p.nct);
    CHECK((size_t)p.upd_ik_blocks * kUpdThreads * kUpdPerThread >= (size_t)M * M);
    CHECK(((size_t)p.upd_ik_blocks - 1) * kUpdThreads * kUpdPerThread < (size_t)M * M);
    CHECK(p.upd_lds_bytes == sizeof(double) * 3 * (size_t)M);
    if (p.rec_total > ((size_t)256 << 20) / sizeof(double)) return;
    // the vectors kernel's LDS as it carves it, with what its phases touch (the sanitizer sees an overrun); the verdict is the
    // forget's and the last double
    std::vector<double> lds(p.lds_bytes / sizeof(double), 0.0);
    double* xs = lds.data();
    double* il = xs + 24;
    double* a0 = xs + 48;
    double* u = a0 + M;
    double* pp = u + M;
    double* t = pp + M;
    double* part = t + M + 1;
    double* verdict = part + (size_t)p.groups * M;
    xs[23] += 1.0; il[23] += 1.0;
    verdict[0] += 1.0;
    CHECK(verdict + 1 == lds.data() + lds.size());
    for (int i = 0; i < M; ++i) { a0[i] += 1.0; u[i] += 1.0; pp[i] += 1.0; t[i + 1] += 1.0; }
    std::vector<int> rows_seen((size_t)M * p.nct, 0);
    for (int it = 0; it < p.nct * p.groups; ++it) {
        const int tile = it % p.nct, grp = it / p.nct;
        CHECK(grp < p.groups);
        const int r1 = (grp + 1) * p.rows_per_group < M ? (grp + 1) * p.rows_per_group : M;
        for (int lane = 0; lane < 64; lane += 63) {                    // first and last lane of the tile
            const int j = tile * kUpdTile + lane;
            if (j >= M) continue;
            part[(size_t)grp * M + j] += 1.0;
            for (int i = grp * p.rows_per_group > j ? grp * p.rows_per_group : j; i < r1; ++i) {
                CHECK(i >= j && i < M);
                if (lane == 0) rows_seen[(size_t)tile * M + i] += 1;
            }
        }
    }
    for (int tile = 0; tile < p.nct; ++tile)
        for (int i = tile * kUpdTile; i < M; ++i) CHECK(rows_seen[(size_t)tile * M + i] == 1);     // each row of column j once
    // the record buffer: last entries of every region for the last output
    std::vector<double> rec(p.rec_total, 0.0);
    rec[p.yb + MM - 1] += 1.0;
    rec[p.w + DM - 1] += 1.0;
    rec[p.noise + D - 1] += 1.0;
    // the scratch buffer: the same, and every failure word as the kernels address them
    std::vector<double> ws(p.ws_total, 0.0);
    for (size_t o : {p.v, p.p, p.c, p.d, p.g, p.t1, p.t2}) ws[o + DM - 1] += 1.0;
    ws[p.tau + D - 1] += 1.0;
    {
        std::vector<int> words(kUpdFailWords, 0);
        for (int a = 0; a < D; ++a) words[a] = a + 1;
        std::memcpy(ws.data() + p.fail, words.data(), kUpdFailWords * sizeof(int));         // stays in front of v
        CHECK(ws[p.v + DM - 1] == 1.0);
        std::memcpy(words.data(), ws.data() + p.fail, kUpdFailWords * sizeof(int));
        CHECK(words[D - 1] == D);
    }
    // the update kernel: LDS of a recurrence workgroup, the forget's w' of the first one, and the entries of iK_eff the others reach
    std::vector<double> ulds(p.upd_lds_bytes / sizeof(double), 0.0);
    for (int b = 0; b < p.upd_rec_blocks; ++b)
        for (int i = b * kUpdTile; i < M; ++i) { ulds[i] += 1.0; ulds[(size_t)M + i] += 1.0; ulds[2 * (size_t)M + i] += 1.0; }
    for (int tid = 0; tid < kUpdThreads; ++tid)
        for (int i = tid; i < M; i += kUpdThreads) { ws[p.v + (size_t)(D - 1) * M + i] += 1.0; rec[p.w + (size_t)(D - 1) * M + i] += 1.0; }
    size_t reached = 0;
    for (int b = 0; b < p.upd_ik_blocks; ++b)
        for (int q = 0; q < kUpdPerThread; ++q) {
            const size_t lo = (size_t)b * kUpdThreads * kUpdPerThread + (size_t)q * kUpdThreads;
            const size_t hi = lo + kUpdThreads - 1;
            const size_t n = (size_t)M * M;
            if (lo < n) reached += (hi < n ? hi : n - 1) - lo + 1;
        }
    CHECK(reached == (size_t)M * M);
}

int main() {
    const int Ms[] = {1, 2, 16, 37, 63, 64, 65, 70, 127, 128, 129, 130, 256, 1000, 1023, 1024, 1025, 4000};
    const int Ds[] = {1, 3, 4, 16};
    int n = 0;
    for (int M : Ms)
        for (int D : Ds) { one(M, D); ++n; }
    // The largest M both calls accept on a 160 KiB workgroup (Handle::lds_limit): 4086, where the vectors kernel's LDS with the
    // forget's verdict is exactly 160 KiB.  The two separate plans this one replaced (the append's without the verdict) both
    // stopped at this M, so sharing one lds_bytes has not moved the boundary of either call.
    const size_t limit = 160 * 1024;
    constexpr int kLargestM = 4086;
    SparseUpdatePlan p;
    plan_sparse_update(kLargestM, 1, p);
    CHECK(p.lds_bytes == limit && p.upd_lds_bytes <= limit);
    CHECK(p.lds_bytes - sizeof(double) <= limit);                                           // the append's share of it
    plan_sparse_update(kLargestM + 1, 1, p);
    CHECK(p.lds_bytes - sizeof(double) > limit);                                            // ... which the next M exceeds by itself
    int largest = 0, accepted = 0;                                                          // no gap below it: every smaller M fits
    for (int M = 1; M <= 8192; ++M) {
        plan_sparse_update(M, 16, p);
        if (p.lds_bytes <= limit && p.upd_lds_bytes <= limit) { largest = M; ++accepted; }
    }
    CHECK(largest == kLargestM && accepted == kLargestM);
    std::printf("%d plans checked, largest accepted M %d, %d failures\n", n, largest, fails);
    return fails ? 1 : 0;
}
