// lbfgs_state.h -- the caller-owned state buffer of gpmpc_lbfgs_* (include/gpmpc.h documents it) and the argument checks of the
// entry points, as plain C++: lbfgs_search.hip reads them on host and device, tools/host_checks/lbfgs_state_check.cpp walks them
// on the CPU under the sanitizers.
#pragma once
#include <cstddef>

#include "action_mapper.h"

namespace gpmpc_hip {

constexpr int kLbfgsMaxB = 4096;
constexpr int kLbfgsMaxN = 4096;
constexpr int kLbfgsMaxHistory = 32;

// Offsets in doubles: x | g | d | xt | actions (B, n each) | J | alpha | status | pushes (B each) | S | Y (B, m, n) | sy | yy (B, m)
struct LbfgsLayout {
    int B, n, m;
    size_t x, g, d, xt, actions, J, alpha, status, pushes, S, Y, sy, yy, total;
};

GPMPC_HD inline LbfgsLayout make_lbfgs_layout(int B, int n, int m) {
    LbfgsLayout L;
    L.B = B; L.n = n; L.m = m;
    const size_t Bn = (size_t)B * n, Bm = (size_t)B * m;
    size_t o = 0;
    L.x = o; o += Bn;
    L.g = o; o += Bn;
    L.d = o; o += Bn;
    L.xt = o; o += Bn;
    L.actions = o; o += Bn;
    L.J = o; o += B;
    L.alpha = o; o += B;
    L.status = o; o += B;
    L.pushes = o; o += B;
    L.S = o; o += Bm * n;
    L.Y = o; o += Bm * n;
    L.sy = o; o += Bm;
    L.yy = o; o += Bm;
    L.total = o;
    return L;
}

// 0: fine; otherwise the message of the first limit that fails (`limit` set when it is a compiled limit rather than a bad argument)
inline const char* lbfgs_check_shape(long long B, long long H, long long A, long long history, bool& limit) {
    limit = false;
    if (B < 1 || H < 1 || A < 1 || history < 1) return "lbfgs: need B >= 1, H >= 1, A >= 1, history >= 1";
    limit = true;
    if (B > kLbfgsMaxB) return "lbfgs: at most 4096 restarts";
    if (history > kLbfgsMaxHistory) return "lbfgs: at most 32 pairs of history";
    if (H > kLbfgsMaxN || A > kLbfgsMaxN || H * A > kLbfgsMaxN) return "lbfgs: at most 4096 coordinates (H * A)";
    limit = false;
    return nullptr;
}

inline const char* lbfgs_check_mapper(int mapper, long long A, bool have_max_change, bool have_action_prev, bool& limit) {
    limit = false;
    if (mapper != 0 && mapper != 1) return "lbfgs: mapper must be 0 (identity) or 1 (derivative)";
    if (mapper == 1 && (!have_max_change || !have_action_prev)) return "lbfgs: the derivative mapper needs max_change and the previous action";
    if (mapper == 1 && A > kMaxMapperA) { limit = true; return "lbfgs: the derivative mapper supports A <= 24"; }
    return nullptr;
}

inline const char* lbfgs_check_step(long long iteration, double c1, double pgtol) {
    if (iteration < 0) return "lbfgs: iteration must be >= 0";
    if (!(c1 > 0.0 && c1 < 1.0)) return "lbfgs: need 0 < c1 < 1";
    if (!(pgtol >= 0.0)) return "lbfgs: need pgtol >= 0";
    return nullptr;
}

}  // namespace gpmpc_hip
