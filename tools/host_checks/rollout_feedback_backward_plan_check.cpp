// Stand-alone host check of plan_rollout_feedback_backward (csrc/rollout_feedback_backward_plan.h): walks the chunk loop of
// run_rollout_feedback_backward over a grid of shapes, the compiled limits included, and checks that the arrays of a chunk's
// workspace do not overlap and that every index a kernel of the chunk may form stays inside its array -- the step-major keepV
// array in particular, which the moment kernels write per step and the reverse kernel reads per candidate.  The memory size N does
// not enter this plan: the N-dependent workspaces of the moment launches are run_moments' and run_moments_backward's own
// (Handle::momws, Handle::mombws).  Build with a host sanitizer and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_checks/rollout_feedback_backward_plan_check.cpp -o plan_check && ./plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd/csrc/rollout_feedback_backward_plan.h"

using namespace gpmpc_hip;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static void one(int D, int E, int A, int H, long long B, bool no_gains, long long opt) {
    FeedbackBwdPlan p;
    plan_rollout_feedback_backward(D, E, A, B, H, no_gains, opt, p);
    CHECK(p.chunk >= 1 && p.chunk <= B);
    if (opt > 0) CHECK(p.chunk == (opt < B ? opt : B));
    if (opt == 0 && p.chunk < B && p.chunk >= kFbbRound) CHECK(p.chunk % kFbbRound == 0);
    // the arrays follow one another without gaps or overlap
    const size_t c = (size_t)p.chunk, d = (size_t)D, e = (size_t)E, t1 = (size_t)H + 1;
    const size_t n_zero = no_gains ? (size_t)H * A * D : 0;
    const size_t offs[] = {p.xin, p.sin, p.M, p.S, p.mu, p.Sig, p.keepV, p.cv, p.adj, p.Mb, p.Sb, p.Vb, p.xb, p.Pb, p.zero_gains};
    const size_t lens[] = {c * e, c * e * e, c * d, c * d * d, c * t1 * d, c * t1 * d * d, (size_t)H * c * e * d, c * t1,
                           c * (d + d * d), c * d, c * d * d, c * e * d, c * e, c * e * e, n_zero};
    const int n_arrays = (int)(sizeof offs / sizeof offs[0]);
    size_t o = 0;
    for (int i = 0; i < n_arrays; ++i) {
        CHECK(offs[i] == o);
        o += lens[i];
    }
    CHECK(p.total == o);
    CHECK(p.total - n_zero == c * feedback_bwd_per_candidate(D, E, H));
    // within the budget, or one candidate's need (the zero gains are the call's, not a candidate's)
    if (opt == 0) CHECK((p.total - n_zero) * sizeof(double) <= kFbbWsBudget || p.chunk == 1);
    // touch what the kernels of every chunk touch, in a buffer of the planned size (the sanitizer sees an overrun)
    if (p.total > ((size_t)64 << 20) / sizeof(double)) return;
    std::vector<double> ws(p.total, 0.0);
    CHECK(D + A <= E);
    const int n = D + A;
    long long covered = 0;
    auto touch = [&](int array, size_t idx) {           // the last element a kernel forms in `array`
        CHECK(idx < lens[array]);
        CHECK(offs[array] + idx < (array + 1 < n_arrays ? offs[array + 1] : p.total) || lens[array] == 0);
        if (idx < lens[array]) ws[offs[array] + idx] += 1.0;
    };
    for (long long b0 = 0; b0 < B; b0 += p.chunk) {
        const long long rows = (B - b0) < p.chunk ? (B - b0) : p.chunk;
        const size_t r = (size_t)(rows - 1);
        // the forward's init / step kernels and run_moments: the last model input and results of the last row
        touch(0, r * e + (e - 1));
        touch(1, r * e * e + e * e - 1);
        touch(2, r * d + (d - 1));
        touch(3, r * d * d + d * d - 1);
        // the trajectory: index t + 1 <= H of the last row
        touch(4, (r * t1 + H) * d + (d - 1));
        touch(5, (r * t1 + H) * d * d + d * d - 1);
        // keepV: run_moments writes (rows, E, D) at step t's block of p.chunk candidates; the reverse kernel reads the state and
        // action rows of candidate b at ((t * chunk + b) * E * D)
        for (int t : {0, H - 1}) {
            touch(6, (size_t)t * c * e * d + r * e * d + e * d - 1);
            touch(6, ((size_t)t * c + r) * e * d + (size_t)(n * D - 1));
        }
        // the cost variances of the trajectory cost kernel, the adjoints, the cotangents and the moment gradient's results
        touch(7, r * t1 + H);
        touch(8, r * (d + d * d) + d + d * d - 1);
        touch(9, r * d + d - 1);
        touch(10, r * d * d + d * d - 1);
        touch(11, r * e * d + e * d - 1);
        touch(12, r * e + e - 1);
        touch(13, r * e * e + (size_t)(n - 1) * e + (n - 1));        // the reverse kernel reads the n x n corner with pitch E
        touch(13, r * e * e + e * e - 1);
        if (no_gains && A > 0)                // shared zero gains: step H - 1, the last action row, whatever the row
            touch(14, (size_t)(H - 1) * A * D + (size_t)A * D - 1);
        covered += rows;
    }
    CHECK(covered == B);
}

int main() {
    // D, E, A: small shapes, with and without time, and the compiled limits (D = 16, E = 24)
    const int DEAs[][3] = {{1, 2, 1}, {1, 3, 1}, {3, 4, 1}, {3, 5, 1}, {3, 6, 2}, {5, 7, 2}, {6, 9, 2},
                           {16, 20, 4}, {16, 24, 8}, {1, 24, 23}, {15, 24, 8}, {12, 24, 12}};
    const int Hs[] = {1, 2, 5, 25, 50, 1000};
    const long long Bs[] = {1, 2, 7, 8, 9, 63, 64, 65, 130, 2048, 100000};
    const long long opts[] = {0, 1, 3, 7, 8, 64, 65, 100, 1 << 24};
    int n = 0;
    for (auto& s : DEAs)
        for (int H : Hs)
            for (long long B : Bs)
                for (long long o : opts)
                    for (int flags = 0; flags < 2; ++flags) {
                        one(s[0], s[1], s[2], H, B, flags != 0, o);
                        ++n;
                    }
    std::printf("%d plans checked, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
