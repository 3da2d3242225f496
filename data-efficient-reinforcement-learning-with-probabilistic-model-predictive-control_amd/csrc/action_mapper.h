// action_mapper.h -- the action mapper of the device searches: optimiser vector in [0, 1]^(H A) -> model actions (H, A), and the
// chain rule back.  Identity, or the reference's DerivativeActionMapper (actions_mappers/derivative_action_mapper.py:28-35):
// deltas scaled to [-max_change, max_change], cumulative sum from the previous action, clamp.  Plain C++: cem_map_kernel
// (search.hip) and lbfgs_init_kernel / lbfgs_step_kernel (lbfgs_search.hip) call it on the device,
// tools/host_checks/lbfgs_state_check.cpp on the CPU under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define GPMPC_HD __host__ __device__
#else
#define GPMPC_HD
#endif

namespace gpmpc_hip {

// A cached model has D + A <= GPMPC_MAX_E = 24 inputs with D >= 1, so its A <= 23 always fits (search.hip asserts the 24); the
// L-BFGS entries take any A and check it (lbfgs_check_mapper)
constexpr int kMaxMapperA = 24;

// the mapper and the derivative mapper's parameters, by value in the kernel argument block (mapper 0, identity: arrays unused)
struct ActionMapper {
    int mapper;
    double max_change[kMaxMapperA];
    double action_prev[kMaxMapperA];
};

// One action dimension `a` over the horizon: x and out point at its entry of step 0, the entry of step t is A doubles further.
// The running sum is not clamped, its output is.
GPMPC_HD inline void map_actions(const ActionMapper& mp, int a, int H, int A, const double* x, double* out) {
    if (mp.mapper == 0) {
        for (int t = 0; t < H; ++t) out[(size_t)t * A] = x[(size_t)t * A];
        return;
    }
    const double m = mp.max_change[a];
    double s = mp.action_prev[a];
    for (int t = 0; t < H; ++t) {
        s += x[(size_t)t * A] * 2.0 * m - m;
        out[(size_t)t * A] = fmin(fmax(s, 0.0), 1.0);
    }
}

// ... and the chain rule back: G = d / d(model actions) -> gx = d / d(optimiser vector), the reverse cumulative sum times
// 2 max_change.  (The clamp's derivative is not applied: the objective's gradient is taken at the clamped actions.)
GPMPC_HD inline void map_actions_backward(const ActionMapper& mp, int a, int H, int A, const double* G, double* gx) {
    if (mp.mapper == 0) {
        for (int t = 0; t < H; ++t) gx[(size_t)t * A] = G[(size_t)t * A];
        return;
    }
    const double two_m = 2.0 * mp.max_change[a];
    double acc = 0.0;
    for (int t = H - 1; t >= 0; --t) {
        acc += G[(size_t)t * A];
        gx[(size_t)t * A] = two_m * acc;
    }
}

}  // namespace gpmpc_hip
