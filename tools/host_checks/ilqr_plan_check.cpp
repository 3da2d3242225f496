// Stand-alone host check of plan_ilqr (csrc/ilqr_plan.h) and of the state layout and argument checks of gpmpc_ilqr_*
// (csrc/ilqr_state.h): walks the chunk loops of ilqr.hip's backward and forward passes over a grid of shapes, the compiled limits
// included, and checks that the arrays of a chunk's workspace do not overlap, that every index a kernel of the chunk may form stays
// inside its array, and that the views of the state buffer tile it.  Build with a host sanitizer and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_checks/ilqr_plan_check.cpp -o plan_check && ./plan_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd/csrc/ilqr_plan.h"
#include "../../data-efficient-reinforcement-learning-with-probabilistic-model-predictive-control_amd/csrc/ilqr_state.h"

using namespace gpmpc_hip;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static void plan(int D, int E, int A, int H, int L, long long count, long long opt) {
    IlqrPlan p;
    plan_ilqr(D, E, H, L, count, opt, p);
    CHECK(p.chunk >= 1 && p.chunk <= count);
    if (opt > 0) CHECK(p.chunk == (opt < count ? opt : count));
    if (opt == 0 && p.chunk < count) CHECK(p.chunk % kIlqrRound == 0);
    const size_t offs[] = {p.xq, p.M, p.V, p.tmu}, lens[] = {p.n_xq, p.n_M, p.n_V, p.n_tmu};
    size_t o = 0;
    for (int i = 0; i < 4; ++i) {
        CHECK(offs[i] == o);
        o += lens[i];
    }
    CHECK(p.total == o);
    const long long least = count < kIlqrRound ? count : kIlqrRound;
    IlqrPlan small;
    plan_ilqr(D, E, H, L, least, least, small);
    if (opt == 0) CHECK(p.total * sizeof(double) <= kIlqrWsBudget || p.total <= small.total);
    CHECK(p.chunk * L <= std::numeric_limits<int>::max() / E);            // rows * E of a launch fits an int
    if (p.total > ((size_t)64 << 20) / sizeof(double)) return;
    std::vector<double> ws(p.total, 0.0);
    CHECK(D + A <= E && A <= kIlqrMaxA && L <= kIlqrMaxL);
    long long covered = 0;
    for (long long b0 = 0; b0 < count; b0 += p.chunk) {
        const long long cands = (count - b0) < p.chunk ? (count - b0) : p.chunk;
        // backward: lqr_inputs_kernel and the slots of V, over the chunk's candidates
        const size_t r = (size_t)(cands - 1);
        CHECK(r * E + (E - 1) < p.n_xq);
        ws[p.xq + r * E + (E - 1)] += 1.0;
        CHECK(r * D + (D - 1) < p.n_M);
        ws[p.M + r * D + (D - 1)] += 1.0;
        for (int t = 0; t < H; ++t) {
            const size_t last = (size_t)t * cands * E * D + (r * E + (E - 1)) * D + (D - 1);
            CHECK(last < p.n_V);
            ws[p.V + last] += 1.0;
        }
        // forward: ilqr_forward_kernel over cands * L rows, steps 0 .. H
        const size_t q = (size_t)(cands * L - 1);
        CHECK(q * E + (E - 1) < p.n_xq);
        ws[p.xq + q * E + (E - 1)] += 1.0;
        CHECK(q * D + (D - 1) < p.n_M);
        ws[p.M + q * D + (D - 1)] += 1.0;
        const size_t last_state = (q * (H + 1) + H) * D + (D - 1);
        CHECK(last_state < p.n_tmu);
        ws[p.tmu + last_state] += 1.0;
        covered += cands;
    }
    CHECK(covered == count);
}

static void state(int B, int H, int A, int D, int L) {
    const IlqrLayout Y = make_ilqr_layout(B, H, A, D, L);
    const size_t b = (size_t)B, ha = (size_t)H * A;
    const size_t offs[] = {Y.actions, Y.cost, Y.reg, Y.status, Y.accepts, Y.chosen, Y.dV, Y.step, Y.flags, Y.J, Y.trial_cost, Y.gains,
                           Y.ff, Y.mu, Y.trial_actions};
    const size_t lens[] = {b * ha, b, b, b, b, b, b, b, b, b, b * L, b * ha * D, b * ha, b * (H + 1) * D, b * L * ha};
    size_t o = 0;
    for (int i = 0; i < 15; ++i) {
        CHECK(offs[i] == o);
        o += lens[i];
    }
    CHECK(Y.total == o);
    if (Y.total > ((size_t)64 << 20) / sizeof(double)) return;
    std::vector<double> st(Y.total, 0.0);
    // what the kernels touch last in each view: the accept kernel's copy, the trial rows, the sweep's outputs
    st[Y.trial_actions + ((size_t)(B - 1) * L + (L - 1)) * ha + ha - 1] += 1.0;
    st[Y.actions + (size_t)(B - 1) * ha + ha - 1] += 1.0;
    st[Y.trial_cost + (size_t)(B - 1) * L + (L - 1)] += 1.0;
    st[Y.gains + ((size_t)(B - 1) * ha + ha - 1) * D + (D - 1)] += 1.0;
    st[Y.mu + ((size_t)(B - 1) * (H + 1) + H) * D + (D - 1)] += 1.0;
    st[Y.J + (B - 1)] += 1.0;
}

int main() {
    const int DEAs[][3] = {{1, 2, 1}, {1, 3, 1}, {3, 4, 1}, {3, 5, 1}, {4, 6, 2}, {6, 9, 2}, {16, 20, 4}, {16, 24, 8}, {15, 24, 8}};
    const int Hs[] = {1, 2, 3, 25, 30, 1000};
    const int Ls[] = {1, 4, 8, 16};
    const long long counts[] = {1, 2, 63, 64, 65, 70, 130, 2048, 4096};
    const long long opts[] = {0, 1, 3, 7, 64, 65, 100, 1 << 24};
    int n = 0;
    for (auto& s : DEAs)
        for (int H : Hs)
            for (int L : Ls) {
                for (long long c : counts) {
                    for (long long o : opts) {
                        plan(s[0], s[1], s[2], H, L, c, o);
                        ++n;
                    }
                    state((int)c, H, s[2], s[0], L);
                    ++n;
                }
            }
    // the argument checks
    bool limit = false;
    CHECK(!ilqr_check_shape(1, 1, 1, 1, limit) && !ilqr_check_shape(4096, 1000, 8, 16, limit));
    CHECK(ilqr_check_shape(0, 1, 1, 1, limit) && !limit);
    CHECK(ilqr_check_shape(4097, 1, 1, 1, limit) && !limit);
    CHECK(ilqr_check_shape(1, 0, 1, 1, limit) && ilqr_check_shape(1, 1, 0, 1, limit) && ilqr_check_shape(1, 1, 1, 0, limit));
    CHECK(ilqr_check_shape(1, 1, 1, 17, limit) && !limit);
    CHECK(ilqr_check_shape(1, 1, 9, 1, limit) && limit);
    CHECK(ilqr_check_shape(-2147483647 - 1, 2147483647, 2147483647, 2147483647, limit));
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    CHECK(!ilqr_check_step(0.0, 10.0, 0.0, 0.0) && !ilqr_check_step(1e-3, 1.5, 1e6, 1e-9) && !ilqr_check_step(1e-3, 2.0, inf, 0.0));
    CHECK(ilqr_check_step(-1e-3, 10.0, 1.0, 0.0) && ilqr_check_step(nan, 10.0, 1.0, 0.0) && ilqr_check_step(inf, 10.0, inf, 0.0));
    CHECK(ilqr_check_step(1e-3, 1.0, 1.0, 0.0) && ilqr_check_step(1e-3, nan, 1.0, 0.0));
    CHECK(ilqr_check_step(1e-3, 10.0, 1e-4, 0.0) && ilqr_check_step(1e-3, 10.0, nan, 0.0));
    CHECK(ilqr_check_step(1e-3, 10.0, 1.0, -1.0) && ilqr_check_step(1e-3, 10.0, 1.0, nan));
    std::printf("%d plans and layouts checked, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
