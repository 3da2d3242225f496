// Stand-alone host check of plan_moments_linear_backward (csrc/moments_linear_backward_plan.h): walks the chunk loop of
// run_moments_linear_backward / run_rollout_linear_backward / run_rollout_linear_feedback_backward over a grid of shapes and checks that the arrays of a chunk's
// workspace do not overlap and that every index a kernel of the chunk may form stays inside its array.  Build with a host
// sanitizer and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_checks/moments_linear_backward_plan_check.cpp -o plan_check && ./plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd/csrc/moments_linear_backward_plan.h"

using namespace gpmpc_hip;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

// KA: action rows of V kept per step (0: the open loop; A: the closed loop)
static void one(int N, int D, int E, int A, long long count, int H, long long opt, int KA) {
    LinearBwdPlan p;
    plan_moments_linear_backward(N, D, E, A, count, H, opt, KA, p);
    CHECK(p.nCB >= 1 && (long long)p.nCB * kLinBwdBN >= N && (long long)(p.nCB - 1) * kLinBwdBN < N);
    CHECK(p.NW == E + 2);
    CHECK(p.chunk >= 1 && p.chunk <= count);
    CHECK(p.Mc % kLinBwdBM == 0 && p.Mc >= p.chunk && p.Mc - p.chunk < kLinBwdBM);
    if (opt > 0) CHECK(p.chunk == (opt < count ? opt : count));
    // the arrays follow one another without gaps or overlap
    const size_t offs[] = {p.part, p.coef, p.base, p.xq, p.mu, p.Sig, p.stepM, p.stepV, p.cv, p.adj};
    const size_t lens[] = {p.n_part, p.n_coef, p.n_base, p.n_xq, p.n_mu, p.n_Sig, p.n_stepM, p.n_stepV, p.n_cv, p.n_adj};
    size_t o = 0;
    for (int i = 0; i < 10; ++i) {
        CHECK(offs[i] == o);
        o += lens[i];
    }
    CHECK(p.total == o);
    if (KA == 0 && H > 0) {                            // the open loop: the sizes the plan had before it knew of KA
        const size_t c = (size_t)p.chunk;
        CHECK(p.n_stepV == c * H * D * D && p.n_adj == c * (2 * (size_t)D + (size_t)D * D + (size_t)A));
    }
    if (H == 0) CHECK(p.n_xq + p.n_mu + p.n_Sig + p.n_stepM + p.n_stepV + p.n_cv + p.n_adj == 0);
    // within the budget, or one tile's need
    const long long tile = count < kLinBwdBM ? count : kLinBwdBM;
    LinearBwdPlan one_tile;
    plan_moments_linear_backward(N, D, E, A, tile, H, tile, KA, one_tile);
    if (opt == 0) CHECK(p.total * sizeof(double) <= kLinBwdWsBudget || p.total <= one_tile.total);
    // touch what the kernels of every chunk touch, in a buffer of the planned size (the sanitizer sees an overrun)
    if (p.total > ((size_t)64 << 20) / sizeof(double)) return;
    std::vector<double> ws(p.total, 0.0);
    const size_t Mc = (size_t)p.Mc, DD = (size_t)D * D;
    long long covered = 0;
    for (long long m0 = 0; m0 < count; m0 += p.chunk) {
        const long long rows = (count - m0) < p.chunk ? (count - m0) : p.chunk;
        CHECK((rows + kLinBwdBM - 1) / kLinBwdBM * kLinBwdBM <= p.Mc);
        const size_t r = (size_t)(rows - 1);
        // last element a tile workgroup writes: output D - 1, block nCB - 1, sum NW - 1, row rows - 1
        const size_t last_part = (((size_t)(D - 1) * p.nCB + (p.nCB - 1)) * p.NW + (p.NW - 1)) * Mc + r;
        CHECK(last_part < p.n_part);
        ws[p.part + last_part] += 1.0;
        const size_t last_coef = ((size_t)(D - 1) * p.NW + (p.NW - 1)) * Mc + r;          // ... and reads of the coefficients
        CHECK(last_coef < p.n_coef);
        ws[p.coef + last_coef] += 1.0;
        CHECK(r * E + (E - 1) < p.n_base);
        ws[p.base + r * E + (E - 1)] += 1.0;
        if (H > 0) {
            CHECK(r * E + (E - 1) < p.n_xq);
            ws[p.xq + r * E + (E - 1)] += 1.0;
            CHECK((r * (H + 1) + H) * D + (D - 1) < p.n_mu);
            ws[p.mu + (r * (H + 1) + H) * D + (D - 1)] += 1.0;
            CHECK((r * (H + 1) + H) * DD + DD - 1 < p.n_Sig);
            ws[p.Sig + (r * (H + 1) + H) * DD + DD - 1] += 1.0;
            CHECK((r * H + (H - 1)) * D + (D - 1) < p.n_stepM);
            ws[p.stepM + (r * H + (H - 1)) * D + (D - 1)] += 1.0;
            const size_t VS = DD + (size_t)KA * D;                                             // the kept rows of one step's V
            CHECK((r * H + (H - 1)) * VS + VS - 1 < p.n_stepV);
            ws[p.stepV + (r * H + (H - 1)) * VS + VS - 1] += 1.0;
            CHECK(r * (H + 1) + H < p.n_cv);
            ws[p.cv + r * (H + 1) + H] += 1.0;
            const size_t AS = 2 * (size_t)D + DD + (size_t)A;
            CHECK(r * AS + AS - 1 < p.n_adj);
            ws[p.adj + r * AS + AS - 1] += 1.0;
        }
        covered += rows;
    }
    CHECK(covered == count);
}

int main() {
    const int Ns[] = {1, 50, 255, 256, 257, 300, 513, 1000, 4096};
    const int DEAs[][3] = {{1, 2, 1}, {3, 4, 1}, {3, 5, 1}, {4, 6, 2}, {16, 20, 4}, {16, 24, 8}};
    const long long counts[] = {1, 63, 64, 65, 130, 2048, 100000};
    const long long opts[] = {0, 1, 7, 64, 65, 100, 1 << 24};
    int n = 0;
    for (int N : Ns)
        for (auto& s : DEAs)
            for (long long c : counts)
                for (long long o : opts) {
                    one(N, s[0], s[1], 0, c, 0, o, 0);
                    for (int H : {1, 12, 50}) {
                        one(N, s[0], s[1], s[2], c, H, o, 0);
                        one(N, s[0], s[1], s[2], c, H, o, s[2]);
                        n += 2;
                    }
                    n += 1;
                }
    std::printf("%d plans checked, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
