// Prints what plan_rollout decides for a shape and a set of engine options -- among it RolloutPlan::x_in_lds, which the engine does
// not report -- without a GPU: the planner reads nothing but the handle's options, limits and monomial counts.  D = 3, A = 1.
//
//   hipcc -std=c++17 tools/rollout_plan_probe.hip -I <package>/csrc -L <package> -lgpmpc_hip -Wl,-rpath,<package> -o rollout_plan_probe
//   ./rollout_plan_probe N E B threads rows_per_chunk cluster lds_limit_kb [N E B ...]
//
// tests/short_item_cases.py quotes its output for the runs whose X^T has to be in LDS / in global memory.
#include <cstdio>
#include <cstdlib>

#include "gpmpc_internal.h"

int main(int argc, char** argv) {
    using namespace gpmpc_hip;
    if (argc < 8 || (argc - 1) % 7 != 0) {
        std::fprintf(stderr, "usage: %s N E B threads rows_per_chunk cluster lds_limit_kb [...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 6 < argc; i += 7) {
        const int N = std::atoi(argv[i]), E = std::atoi(argv[i + 1]), B = std::atoi(argv[i + 2]);
        Handle h;
        // the monomial counts ensure_monomials (rollout.hip) finds for D = 3: degrees 0 ... 9, 220 monomials
        h.mono_D = 3; h.mono_CM = 220; h.sep_kmax = 9;
        h.opt_threads = std::atoi(argv[i + 3]);
        h.opt_rows_per_chunk = std::atoi(argv[i + 4]);
        h.opt_cluster = std::atoi(argv[i + 5]);
        h.opt_lds_kb = std::atoi(argv[i + 6]);
        h.opt_force_sep = 1;
        RolloutPlan p;
        const int rc = plan_rollout(h, N, 3, 1, E, 3, B, RolloutRequest{false, false}, p);
        std::printf("  N=%d E=%d B=%d threads=%d rows_per_chunk=%d cluster=%d lds_kb=%d -> rc=%d path=%d nt=%d G=%d groups=%d CH=%d x_in_lds=%d "
                    "cluster=%d lds_bytes=%zu\n", N, E, B, h.opt_threads, h.opt_rows_per_chunk, h.opt_cluster, h.opt_lds_kb, rc, p.path, p.nt,
                    p.G, p.G > 0 ? (6 + p.G - 1) / p.G : 0, p.CH, p.x_in_lds, p.cluster, p.lds_bytes);
    }
    return 0;
}
