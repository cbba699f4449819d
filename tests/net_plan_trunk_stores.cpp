// Prints every stage's kernel plan with k_trunk_quad's prefetch and vector-store flags (alphazero_amd/csrc/az_net_plan.h) without a GPU,
// for tests/test_net_plan_trunk_stores.py:
//   net_plan_trunk_stores GAME H W BESIDE B...     GAME 0 Othello, 1 Connect4; switches (AZ_*) come from the environment
// one line per (stage, B), tab-separated: stage, B, kernel, variant (as tests/net_plan_trunk_prefetch.cpp spells it), family name,
// profile slot, prefetch (k_trunk_quad: 0 | 1, else -), stores (k_trunk_quad: 0 | 1, else -).
#include <stdio.h>
#include <stdlib.h>
#include <string>

#include "az_net_plan.h"

static std::string variant(const StagePlan &p) {
    const std::string form = p.wino ? "wino" : "direct";
    switch (p.kernel) {
        case K_TRUNK: return form + " lds_blocks=" + std::to_string(p.lds_blocks);
        case K_TRUNK_QUAD: return form + " form=" + std::to_string(p.quad_form) + " lds_blocks=" + std::to_string(p.lds_blocks);
        case K_TRUNK_Q: case K_TRUNK2: return form + " waves=" + std::to_string(p.waves);
        case K_GEMM: return std::to_string(p.bm) + "x" + std::to_string(p.bn) + " form=" + std::to_string(p.gemm_form);
        default: return "-";
    }
}

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s GAME H W BESIDE B...\n", argv[0]); return 2; }
    const int game = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), beside = atoi(argv[4]);
    // the dims as az_net_create derives them (NCH = 32 channels; the heads' width padded to 16 columns)
    NetDims d = {};
    d.game = game;
    d.A = game == AZ_OTHELLO ? H * W + 1 : W;
    if (game == AZ_OTHELLO) { d.CH = H; d.CW = W; d.F1 = 1024; d.F2 = 512; }
    else { d.CH = W; d.CW = H; d.F1 = 64; d.F2 = 32; }
    d.FIN = 32 * (d.CH - 4) * (d.CW - 4);
    d.NH = ((d.A + 1 + 15) / 16) * 16;
    d.fc1wq = frag_shape(d.F1, d.FIN);
    d.fc2wq = frag_shape(d.F2, d.F1);
    for (int i = 5; i < argc; ++i)
        for (int stage = 0; stage < 4; ++stage) {
            const int B = atoi(argv[i]);
            const StagePlan p = plan_stage(d, net_tuning(), stage, B, beside);
            const bool quad = p.kernel == K_TRUNK_QUAD;
            if (!quad && (p.quad_prefetch || p.quad_stores)) { fprintf(stderr, "a flag of k_trunk_quad on %s\n", net_kernel_name(p.kernel)); return 1; }
            printf("%d\t%d\t%s\t%s\t%s\t%d\t%s\t%s\n", stage, B, net_kernel_name(p.kernel), variant(p).c_str(), plan_family_name(p), plan_slot(p),
                   quad ? std::to_string(p.quad_prefetch).c_str() : "-", quad ? std::to_string(p.quad_stores).c_str() : "-");
        }
    return 0;
}
