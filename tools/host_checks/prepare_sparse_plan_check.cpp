// Stand-alone host check of plan_prepare_sparse (csrc/prepare_sparse_plan.h): walks the chunk loop of run_prepare_sparse over a grid
// of shapes and checks that every index a kernel of the chunk may form stays inside the planned workspace.  Build with a host
// sanitizer and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_checks/prepare_sparse_plan_check.cpp -o plan_check && ./plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd/csrc/prepare_sparse_plan.h"

using namespace gpmpc_hip;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static void one(int N, int M, int D, int opt) {
    SparsePlan p;
    plan_prepare_sparse(N, M, D, opt, p);
    const long long n64 = ((long long)N + 63) / 64 * 64;
    CHECK(p.chunk >= 64 && p.chunk % 64 == 0 && p.chunk <= n64);
    if (opt > 0) CHECK(p.chunk == (opt < n64 ? opt : n64));
    const size_t MM = (size_t)D * M * M, DM = (size_t)D * M, Cs = (size_t)p.chunk;
    CHECK(p.yu == 0 && p.r == MM && p.wpart == 2 * MM && p.w == p.wpart + DM * kSparseLanes && p.jit == p.w + DM);
    CHECK(p.kuf == p.jit + (size_t)D && p.v == p.kuf + DM * Cs && p.total == p.v + DM * Cs);
    // the two panels of a chunk: within the budget, or one 64-point chunk's need
    if (opt == 0) CHECK(2 * DM * Cs * sizeof(double) <= kSparseWsBudget || p.chunk == 64);
    // nothing of size M x N or N x N: O(D M^2) plus the chunk
    CHECK(p.total <= 2 * MM + DM * (kSparseLanes + 1) + (size_t)D + 2 * DM * Cs);
    if (p.total > ((size_t)256 << 20) / sizeof(double)) return;
    // touch what the kernels of every chunk touch, in a buffer of the planned size (the sanitizer sees an overrun)
    std::vector<double> ws(p.total, 0.0);
    long long covered = 0;
    for (long long n0 = 0; n0 < N; n0 += p.chunk) {
        const int cn = (N - n0 < p.chunk) ? (int)(N - n0) : p.chunk;
        const int cn64 = (cn + 63) / 64 * 64;
        CHECK(cn >= 1 && cn64 <= p.chunk);
        // last element the panel kernel and the product write: output D - 1, row M - 1, column cn64 - 1
        const size_t last = ((size_t)(D - 1) * M + (M - 1)) * Cs + (size_t)(cn64 - 1);
        ws[p.kuf + last] += 1.0;
        ws[p.v + last] += 1.0;
        ws[p.kuf] += 1.0;
        ws[p.wpart + ((size_t)(D - 1) * M + (M - 1)) * kSparseLanes + kSparseLanes - 1] += 1.0;
        covered += cn;
    }
    CHECK(covered == N);
    ws[p.yu + MM - 1] += 1.0;
    ws[p.r + MM - 1] += 1.0;
    ws[p.w + DM - 1] += 1.0;
    ws[p.jit + D - 1] += 1.0;
}

int main() {
    const int Ns[] = {1, 37, 63, 64, 65, 257, 1000, 4096, 100000};
    const int Ms[] = {1, 16, 64, 70, 130, 256, 1000};
    const int Ds[] = {1, 3, 16};
    const int opts[] = {0, 64, 128, 256, 4096, 1 << 24};
    int n = 0;
    for (int N : Ns)
        for (int M : Ms)
            for (int D : Ds)
                for (int o : opts) { one(N, M, D, o); ++n; }
    std::printf("%d plans checked, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
