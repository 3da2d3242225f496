// ilqr_state.h -- the caller-owned state buffer of gpmpc_ilqr_* (include/gpmpc.h documents it) and the argument checks of the entry
// points, as plain C++: ilqr.hip reads them on host and device, tools/host_checks/ilqr_plan_check.cpp walks them on the CPU under
// the sanitizers.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define ILQR_HD __host__ __device__
#else
#define ILQR_HD
#endif

namespace gpmpc_hip {

constexpr int kIlqrMaxB = 4096;
constexpr int kIlqrMaxL = 16;                // line-search ladder: the step sizes ride in the kernel argument block
constexpr int kIlqrMaxA = 8;                 // = kLqrMaxA: the sweep's LDS arrays and solves
constexpr int kIlqrMaxD = 16;                // = GPMPC_MAX_D

// Offsets in doubles: actions (B,H,A) | cost | reg | status | accepts | chosen | dV | step | flags | J (B each) | trial_cost (B,L)
// | gains (B,H,A,D) | ff (B,H,A) | mu (B,H+1,D) | trial_actions (B,L,H,A)
struct IlqrLayout {
    int B, H, A, D, L;
    size_t actions, cost, reg, status, accepts, chosen, dV, step, flags, J, trial_cost, gains, ff, mu, trial_actions, total;
};

ILQR_HD inline IlqrLayout make_ilqr_layout(int B, int H, int A, int D, int L) {
    IlqrLayout Y;
    Y.B = B; Y.H = H; Y.A = A; Y.D = D; Y.L = L;
    const size_t b = (size_t)B, ha = (size_t)H * A;
    size_t o = 0;
    Y.actions = o; o += b * ha;
    Y.cost = o; o += b;
    Y.reg = o; o += b;
    Y.status = o; o += b;
    Y.accepts = o; o += b;
    Y.chosen = o; o += b;
    Y.dV = o; o += b;
    Y.step = o; o += b;
    Y.flags = o; o += b;
    Y.J = o; o += b;
    Y.trial_cost = o; o += b * L;
    Y.gains = o; o += b * ha * D;
    Y.ff = o; o += b * ha;
    Y.mu = o; o += b * (size_t)(H + 1) * D;
    Y.trial_actions = o; o += b * L * ha;
    Y.total = o;
    return Y;
}

// 0: fine; otherwise the message of the first check that fails (`limit` set when it is a compiled limit rather than a bad argument)
inline const char* ilqr_check_shape(long long B, long long H, long long A, long long L, bool& limit) {
    limit = false;
    if (B < 1 || B > kIlqrMaxB) return "ilqr: need 1 <= B <= 4096";
    if (H < 1 || A < 1) return "ilqr: need H >= 1, A >= 1";
    if (H > (1 << 20)) return "ilqr: need H <= 2^20";
    if (L < 1 || L > kIlqrMaxL) return "ilqr: need 1 <= L <= 16 line-search steps";
    if (A > kIlqrMaxA) { limit = true; return "ilqr: A beyond the compiled limit (A <= 8)"; }
    return nullptr;
}

inline bool ilqr_finite(double v) { return v - v == 0.0; }

inline const char* ilqr_check_reg0(double reg0) {
    if (!ilqr_finite(reg0) || reg0 < 0.0) return "ilqr: reg0 must be finite and >= 0";
    return nullptr;
}

inline const char* ilqr_check_step(double reg0, double reg_factor, double reg_max, double tol) {
    if (const char* m = ilqr_check_reg0(reg0)) return m;
    if (!(reg_factor > 1.0)) return "ilqr: need reg_factor > 1";
    if (!(reg_max >= reg0)) return "ilqr: need reg_max >= reg0";
    if (!(tol >= 0.0)) return "ilqr: need tol >= 0";
    return nullptr;
}

}  // namespace gpmpc_hip
