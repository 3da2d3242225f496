// Stand-alone host check of plan_rollout_feedback (csrc/rollout_feedback_plan.h): walks the chunk loop of run_rollout_feedback over
// a grid of shapes, the compiled limits included, and checks that the arrays of a chunk's workspace do not overlap and that every
// index a kernel of the chunk may form stays inside its array.  The memory size N does not enter this plan: the N-dependent
// workspace of the moment launches is run_moments' own (Handle::momws).  Build with a host sanitizer and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_checks/rollout_feedback_plan_check.cpp -o plan_check && ./plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd/csrc/rollout_feedback_plan.h"

using namespace gpmpc_hip;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static void one(int D, int E, int A, int H, long long B, bool own_traj, bool no_gains, long long opt) {
    FeedbackPlan p;
    plan_rollout_feedback(D, E, A, B, H, own_traj, no_gains, opt, p);
    CHECK(p.chunk >= 1 && p.chunk <= B);
    if (opt > 0) CHECK(p.chunk == (opt < B ? opt : B));
    if (opt == 0 && p.chunk < B && p.chunk >= kFbRound) CHECK(p.chunk % kFbRound == 0);
    // the arrays follow one another without gaps or overlap
    const size_t c = (size_t)p.chunk;
    const size_t n_traj_mu = own_traj ? c * (H + 1) * D : 0, n_traj_Sig = own_traj ? c * (H + 1) * D * D : 0;
    const size_t n_zero = no_gains ? (size_t)H * A * D : 0;
    const size_t offs[] = {p.xin, p.sin, p.M, p.S, p.V, p.traj_mu, p.traj_Sig, p.zero_gains};
    const size_t lens[] = {c * E, c * E * E, c * D, c * D * D, c * E * D, n_traj_mu, n_traj_Sig, n_zero};
    size_t o = 0;
    for (int i = 0; i < 8; ++i) {
        CHECK(offs[i] == o);
        o += lens[i];
    }
    CHECK(p.total == o);
    // within the budget, or one candidate's need (the zero gains are the call's, not a candidate's)
    FeedbackPlan single;
    plan_rollout_feedback(D, E, A, 1, H, own_traj, false, 1, single);
    if (opt == 0) CHECK((p.total - n_zero) * sizeof(double) <= kFbWsBudget || p.chunk == 1);
    if (p.chunk == 1) CHECK(p.total - n_zero == single.total);
    // touch what the kernels of every chunk touch, in a buffer of the planned size (the sanitizer sees an overrun)
    if (p.total > ((size_t)64 << 20) / sizeof(double)) return;
    std::vector<double> ws(p.total, 0.0);
    CHECK(D + A <= E);
    long long covered = 0;
    for (long long b0 = 0; b0 < B; b0 += p.chunk) {
        const long long rows = (B - b0) < p.chunk ? (B - b0) : p.chunk;
        const size_t r = (size_t)(rows - 1);
        // init / step kernels: the last model input of the last row; run_moments: its last results; the step kernel's reads
        ws[p.xin + r * E + (E - 1)] += 1.0;
        CHECK(p.xin + r * E + (E - 1) < p.sin);
        ws[p.sin + r * E * E + (size_t)E * E - 1] += 1.0;
        CHECK(p.sin + r * E * E + (size_t)E * E - 1 < p.M);
        ws[p.M + r * D + (D - 1)] += 1.0;
        CHECK(p.M + r * D + (D - 1) < p.S);
        ws[p.S + r * D * D + (size_t)D * D - 1] += 1.0;
        CHECK(p.S + r * D * D + (size_t)D * D - 1 < p.V);
        ws[p.V + r * E * D + (size_t)E * D - 1] += 1.0;
        CHECK(p.V + r * E * D + (size_t)E * D - 1 < p.traj_mu);
        if (own_traj) {                       // index t + 1 <= H of the last row
            const size_t last_mu = (r * (H + 1) + H) * D + (D - 1), last_Sig = (r * (H + 1) + H) * D * D + (size_t)D * D - 1;
            ws[p.traj_mu + last_mu] += 1.0;
            CHECK(p.traj_mu + last_mu < p.traj_Sig);
            ws[p.traj_Sig + last_Sig] += 1.0;
            CHECK(p.traj_Sig + last_Sig < p.zero_gains);
        }
        if (no_gains && A > 0) {              // shared zero gains: step H - 1, the last action row, whatever the row
            const size_t last_gain = (size_t)(H - 1) * A * D + (size_t)A * D - 1;
            CHECK(p.zero_gains + last_gain < p.total);
            ws[p.zero_gains + last_gain] += 1.0;
        }
        covered += rows;
    }
    CHECK(covered == B);
}

int main() {
    // D, E, A: small shapes, with and without time or actions, and the compiled limits (D = 16, E = 24)
    const int DEAs[][3] = {{1, 1, 0}, {1, 2, 1}, {1, 3, 1}, {3, 3, 0}, {3, 4, 1}, {3, 5, 1}, {3, 6, 2}, {5, 7, 2}, {6, 9, 2},
                           {16, 20, 4}, {16, 24, 8}, {1, 24, 23}, {15, 24, 8}};
    const int Hs[] = {1, 2, 5, 25, 50, 1000};
    const long long Bs[] = {1, 2, 7, 8, 9, 63, 64, 65, 130, 2048, 100000};
    const long long opts[] = {0, 1, 3, 7, 64, 65, 100, 1 << 24};
    int n = 0;
    for (auto& s : DEAs)
        for (int H : Hs)
            for (long long B : Bs)
                for (long long o : opts)
                    for (int flags = 0; flags < 4; ++flags) {
                        one(s[0], s[1], s[2], H, B, (flags & 1) != 0, (flags & 2) != 0, o);
                        ++n;
                    }
    std::printf("%d plans checked, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
