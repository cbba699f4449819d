// Prints the dense stages' kernel plan with k_gemm's row rule (alphazero_amd/csrc/az_net_plan.h) without a GPU, for
// tests/test_net_plan_gemm_rows.py:
//   net_plan_gemm_rows plan GAME H W BESIDE B...   GAME 0 Othello, 1 Connect4; switches (AZ_*) come from the environment
//       one line per (stage 1 | 2, B), tab-separated: stage, B, kernel, tile, family name, profile slot, form, rows (k_gemm: 0 | 1, else -)
//   net_plan_gemm_rows rule FOLLOW GY M...         one line per M, tab-separated: GY, M, gemm_rows_per_block(GY, M, FOLLOW)
#include <stdio.h>
#include <string.h>
#include <string>

#include "az_net_plan.h"

int main(int argc, char **argv) {
    if (argc >= 5 && !strcmp(argv[1], "rule")) {
        const int follow = atoi(argv[2]), gy = atoi(argv[3]);
        for (int i = 4; i < argc; ++i) printf("%d\t%d\t%d\n", gy, atoi(argv[i]), gemm_rows_per_block(gy, atoi(argv[i]), follow));
        return 0;
    }
    if (argc < 7 || strcmp(argv[1], "plan")) { fprintf(stderr, "usage: %s plan GAME H W BESIDE B... | rule FOLLOW GY M...\n", argv[0]); return 2; }
    const int game = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]), beside = atoi(argv[5]);
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
    for (int i = 6; i < argc; ++i)
        for (int stage = 1; stage <= 2; ++stage) {
            const int B = atoi(argv[i]);
            const StagePlan p = plan_stage(d, net_tuning(), stage, B, beside);
            const std::string tile = p.kernel == K_GEMM ? std::to_string(p.bm) + "x" + std::to_string(p.bn) : "-";
            const std::string form = p.kernel == K_GEMM ? std::to_string(p.gemm_form) : "-";
            const std::string rows = p.kernel == K_GEMM ? std::to_string(p.gemm_rows) : "-";
            printf("%d\t%d\t%s\t%s\t%s\t%d\t%s\t%s\n", stage, B, net_kernel_name(p.kernel), tile.c_str(), plan_family_name(p), plan_slot(p), form.c_str(), rows.c_str());
        }
    return 0;
}
