// Stand-alone host check of plan_lqr_gains (csrc/lqr_gains_plan.h): walks the chunk loop of run_lqr_gains over a grid of shapes,
// the compiled limits included, and checks that the arrays of a chunk's workspace do not overlap and that every index a kernel of
// the chunk may form stays inside its array.  Build with a host sanitizer and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_checks/lqr_gains_plan_check.cpp -o plan_check && ./plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd/csrc/lqr_gains_plan.h"

using namespace gpmpc_hip;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static void one(int D, int E, int A, int H, long long count, long long opt) {
    LqrGainsPlan p;
    plan_lqr_gains(D, E, H, count, opt, p);
    CHECK(p.chunk >= 1 && p.chunk <= count);
    if (opt > 0) CHECK(p.chunk == (opt < count ? opt : count));
    if (opt == 0 && p.chunk < count) CHECK(p.chunk % kLqrRound == 0);
    // the arrays follow one another without gaps or overlap
    const size_t offs[] = {p.xq, p.M, p.V}, lens[] = {p.n_xq, p.n_M, p.n_V};
    size_t o = 0;
    for (int i = 0; i < 3; ++i) {
        CHECK(offs[i] == o);
        o += lens[i];
    }
    CHECK(p.total == o);
    // within the budget, or one 64-candidate chunk's need
    const long long least = count < kLqrRound ? count : kLqrRound;
    LqrGainsPlan small;
    plan_lqr_gains(D, E, H, least, least, small);
    if (opt == 0) CHECK(p.total * sizeof(double) <= kLqrWsBudget || p.total <= small.total);
    // touch what the kernels of every chunk touch, in a buffer of the planned size (the sanitizer sees an overrun)
    if (p.total > ((size_t)64 << 20) / sizeof(double)) return;
    std::vector<double> ws(p.total, 0.0);
    const int DA = D + A;
    CHECK(DA <= E && A <= kLqrMaxA);
    long long covered = 0;
    for (long long b0 = 0; b0 < count; b0 += p.chunk) {
        const long long rows = (count - b0) < p.chunk ? (count - b0) : p.chunk;
        const size_t r = (size_t)(rows - 1);
        // lqr_inputs_kernel: the last model input of the last row, and the mean it advances by
        CHECK(r * E + (E - 1) < p.n_xq);
        ws[p.xq + r * E + (E - 1)] += 1.0;
        CHECK(r * D + (D - 1) < p.n_M);
        ws[p.M + r * D + (D - 1)] += 1.0;
        for (int t = 0; t < H; ++t) {
            // the finish kernel of run_moments_linear writes slot t: (rows, E, D) from t rows E D on
            const size_t slot = (size_t)t * rows * E * D;
            const size_t last_write = slot + (r * E + (E - 1)) * D + (D - 1);
            CHECK(last_write < p.n_V);
            ws[p.V + last_write] += 1.0;
            // lqr_riccati_kernel reads the D + A kept rows of ((t rows + b) E D)
            const size_t last_read = ((size_t)t * rows + r) * E * D + (size_t)DA * D - 1;
            CHECK(last_read <= last_write);
            ws[p.V + last_read] += 1.0;
        }
        covered += rows;
    }
    CHECK(covered == count);
}

int main() {
    // D, E, A: small shapes, with and without time, and the compiled limits (D = 16, A = 8, E = 24)
    const int DEAs[][3] = {{1, 2, 1}, {1, 3, 1}, {3, 4, 1}, {3, 5, 1}, {4, 6, 2}, {6, 9, 2}, {16, 20, 4}, {16, 24, 8}, {15, 24, 8}};
    const int Hs[] = {1, 2, 3, 25, 30, 50, 1000};
    const long long counts[] = {1, 2, 63, 64, 65, 70, 130, 2048, 100000};
    const long long opts[] = {0, 1, 3, 7, 64, 65, 100, 1 << 24};
    int n = 0;
    for (auto& s : DEAs)
        for (int H : Hs)
            for (long long c : counts)
                for (long long o : opts) {
                    one(s[0], s[1], s[2], H, c, o);
                    ++n;
                }
    std::printf("%d plans checked, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
