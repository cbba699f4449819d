// Prints the forward's kernel plan (alphazero_amd/csrc/az_net_plan.h) without a GPU, for tests/test_net_plan_host.py:
//   net_plan_table GAME H W QD_ON BESIDE B...     GAME 0 Othello, 1 Connect4, 2 TicTacToe; switches (AZ_*) come from the environment
// one line per (stage, B), tab-separated: stage, B, kernel, variant, family name (az_net_stage_kernel's answer), profile slot.
#include <stdio.h>
#include <string>

#include "az_net_plan.h"

static std::string variant(const StagePlan &p) {
    const std::string form = p.wino ? "wino" : "direct";
    switch (p.kernel) {
        case K_TRUNK: return form + " lds_blocks=" + std::to_string(p.lds_blocks);
        case K_TRUNK_QUAD: return form + " form=" + std::to_string(p.quad_form) + " lds_blocks=" + std::to_string(p.lds_blocks);
        case K_TRUNK_Q: case K_TRUNK2: return form + " waves=" + std::to_string(p.waves);
        case K_GEMM: return std::to_string(p.bm) + "x" + std::to_string(p.bn);
        case K_QGEMM: return "<" + std::to_string(p.qg[0]) + "," + std::to_string(p.qg[1]) + "," + std::to_string(p.qg[2]) + "," + std::to_string(p.qg[3]) + ">";
        case K_HEADS: return "nt=" + std::to_string(p.nt);
        case K_HEADS2: return "nt=" + std::to_string(p.nt) + " rh=" + std::to_string(p.rh);
        case K_TAIL_SMALL: return "R=" + std::to_string(p.tail_r);
        default: return "-";
    }
}

int main(int argc, char **argv) {
    if (argc < 7) { fprintf(stderr, "usage: %s GAME H W QD_ON BESIDE B...\n", argv[0]); return 2; }
    const int game = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), beside = atoi(argv[5]);
    // the dims as az_net_create derives them (NCH = 32 channels; the heads' width padded to 16 columns)
    NetDims d = {};
    d.game = game;
    d.A = game == AZ_OTHELLO ? H * W + 1 : (game == AZ_CONNECT4 ? W : 9);
    if (game == AZ_OTHELLO) { d.CH = H; d.CW = W; d.F1 = 1024; d.F2 = 512; }
    else if (game == AZ_CONNECT4) { d.CH = W; d.CW = H; d.F1 = 64; d.F2 = 32; }
    else { d.CH = 3; d.CW = 3; d.F1 = 9; d.F2 = 9; }
    d.FIN = game == AZ_TICTACTOE ? 9 : 32 * (d.CH - 4) * (d.CW - 4);
    d.NH = ((d.A + 1 + 15) / 16) * 16;
    d.qd_on = atoi(argv[4]) != 0;
    d.fc1wq = game != AZ_TICTACTOE && frag_shape(d.F1, d.FIN);
    d.fc2wq = game != AZ_TICTACTOE && frag_shape(d.F2, d.F1);
    for (int i = 6; i < argc; ++i)
        for (int stage = 0; stage < 4; ++stage) {
            const int B = atoi(argv[i]);
            const StagePlan p = plan_stage(d, net_tuning(), stage, B, beside);
            printf("%d\t%d\t%s\t%s\t%s\t%d\n", stage, B, net_kernel_name(p.kernel), variant(p).c_str(), plan_family_name(p), plan_slot(p));
        }
    return 0;
}
