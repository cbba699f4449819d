// Prints a training step's launch plan (alphazero_amd/csrc/az_train_plan.h) without a GPU, for tests/test_train_plan_host.py:
//   train_plan_table GAME H W B...     GAME 0 Othello, 1 Connect4, 2 TicTacToe; switches (AZ_TRAIN_*) come from the environment
// First one line "tuning", graphs_ok, graph_steps.  Then per B a header line "plan", B, S, NB, RB, NRB, F1B, n_launches and one line per
// launch: B, index, kernel with its template configuration, grid x, grid y, threads, LDS bytes, argument, the launch's RB and NRB.
// Tab-separated.
#include <stdio.h>

#include "az_train_plan.h"

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s GAME H W B...\n", argv[0]); return 2; }
    const int game = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]);
    // the shape as az_trainer_create derives it (32 channels; the heads' width padded to 16 columns; Connect4's plane is W x H)
    TrainShape s = {game, 0, 0, 0, 0};
    if (game != AZ_TICTACTOE) {
        const int A = game == AZ_OTHELLO ? H * W + 1 : W;
        s.F1 = game == AZ_OTHELLO ? 1024 : 64; s.F2 = game == AZ_OTHELLO ? 512 : 32;
        s.FIN = 32 * (H - 4) * (W - 4);
        s.NHP = (A + 1 + 15) / 16 * 16;
    }
    const TrainTuning &t = train_tuning();
    printf("tuning\t%d\t%d\n", t.graph ? 1 : 0, t.graph_steps);
    for (int i = 4; i < argc; ++i) {
        const int B = atoi(argv[i]);
        const TrainPlan p = plan_train_step(s, t, B);
        printf("plan\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", B, p.S, p.NB, p.RB, p.NRB, p.F1B, p.n_launches);
        for (int k = 0; k < p.n_launches; ++k) {
            const TrainLaunch &l = p.launches[k];
            printf("%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", B, k, train_kernel_name(p, l).c_str(), l.gx, l.gy, l.threads, l.lds, l.arg, l.RB, l.NRB);
        }
    }
    return 0;
}
