// The launch sequence of one training step, decided once per az_trainer_steps call as a value: which kernels, in which template
// configuration, on which grid, with how much LDS.  az_train.hip fills the kernels' TDims from the plan, sets the dynamic-LDS attributes
// of the kernels it names and enqueues it launch by launch (enqueue_step, launch_one); tests/train_plan_table.cpp prints it without a
// GPU.  With it the switches of the step (TrainTuning) and the LDS sizes the kernels carve from.  Plain C++17, no HIP.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#ifndef AZ_OTHELLO  // the games, as az_device.h numbers them
#define AZ_OTHELLO 0
#define AZ_CONNECT4 1
#define AZ_TICTACTOE 2
#endif

// Every environment switch of az_train.hip: name (default) meaning.  Read once per process (train_tuning).
struct TrainTuning {
    bool graph;       // AZ_TRAIN_GRAPH (on): 0 = every step as plain launches, no captured graph
    int graph_steps;  // AZ_TRAIN_GRAPH_STEPS (8): consecutive steps in the long graph; a value outside 1..64 is ignored
    int split;        // AZ_TRAIN_SPLIT (1): 1 / 2 / 4 workgroups per board in the conv kernels, halved until boards x split <= 256; any other value = 1
    int rb;           // AZ_TRAIN_RB (-1: by batch size, see dense_row_block): 0 = the dense layers never row-split; 64 / 128 = that row block wherever the batch is larger
    bool fold1;       // AZ_TRAIN_FOLD1 (on): 0 = conv1's backward as a launch of its own (k_conv1_bwd) everywhere
    bool wg_late;     // AZ_TRAIN_WG_LATE (on): 0 = fc1's weight gradient stays in k_mix2 on the row-split path too
    bool fc2_rb64;    // AZ_TRAIN_FC2_RB64 (on): 0 = fc2's forward keeps the step's row-block size
};

inline const TrainTuning &train_tuning() {
    static const TrainTuning t = [] {  // initialised exactly once
        const auto env = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
        TrainTuning v;
        v.graph = env("AZ_TRAIN_GRAPH", 1) != 0;
        v.graph_steps = env("AZ_TRAIN_GRAPH_STEPS", 8);
        if (v.graph_steps < 1 || v.graph_steps > 64) v.graph_steps = 8;
        v.split = env("AZ_TRAIN_SPLIT", 1);
        if (v.split != 2 && v.split != 4) v.split = 1;
        v.rb = env("AZ_TRAIN_RB", -1);
        v.fold1 = env("AZ_TRAIN_FOLD1", 1) != 0;
        v.wg_late = env("AZ_TRAIN_WG_LATE", 1) != 0;
        v.fc2_rb64 = env("AZ_TRAIN_FC2_RB64", 1) != 0;
        return v;
    }();
    return t;
}

// ---- sizes the kernels and the host share: each number is written here and nowhere else
#define TPB 256       // threads of every kernel that is not a dense template
#define MAXB 512      // largest batch of a conv net's step
#define TTT_MAXB 256  // largest batch of TicTacToeNet's one-workgroup step
#define NRBMAX 8      // most row blocks of the dense kernels (MAXB / 64)
#define LDP 36        // LDS row stride of a 32-channel row: 36 = 4 mod 32 -> the 16 x 4 (row, k) lanes of an A fragment hit every bank twice
#define TT_LD 12      // LDS row stride of TicTacToeNet's [B][9] activations
// k_conv_fwd, k_conv_bwd / k_mix2 (their layouts: above the kernels), k_conv1_bwd's weight-gradient tiles (four 32 x 32 partial tiles)
#define CONV_FWD_LDS_FLOATS (288 * LDP + 100 * LDP + 64 * LDP + 64 * LDP + 4 * 32 + 64)
#define CONV_FWD_LDS_BYTES (CONV_FWD_LDS_FLOATS * 4 + 8 * 32 * 3 * 8)
#define CONV_BWD_LDS_FLOATS (288 * LDP + 100 * LDP + 100 * LDP + 64 * LDP + 64 * LDP + 10 * 32 + 192 + 64 * LDP + 128 + 64)
#define CONV_BWD_LDS_BYTES (CONV_BWD_LDS_FLOATS * 4 + 2048 * 8)
#define CONV1_WG_LDS_BYTES (4 * 1024 * 4 + 4 * 32 * 4 + 768 * 8)
// k_update's elements: conv1's weights | conv2..4's | the four biases | the four BatchNorm2d weights | their biases
#define UPD_W1 288
#define UPD_W (288 + 3 * 9216)
#define UPD_B (UPD_W + 4 * 32)
#define UPD_G (UPD_B + 4 * 32)
#define UPD_ALL (UPD_G + 4 * 32)

// k_fc_fwd, k_fc_dgrad, k_mix1 with NW waves over `rows` rows: red[NW][rows][16] (<= 128 KB), four BatchNorm vectors, the double scratch
inline int fc_lds_bytes(int NW, int rows) { return (NW * rows * 16 + 4 * 32) * 4 + 768 * 8; }
inline int heads_bwd_lds_bytes(int rows) { return rows * 16 * 4 + 768 * 8; }
inline int ttt_lds_bytes(int B) { return (320 + 8 * B * TT_LD + 320 + 64) * 4 + (512 + 16 * 5) * 8; }
// workgroups of NW waves that cover the 32 x 32 tiles of an [N][K] weight gradient, one tile per wave
inline int fc_wgrad_blocks(int N, int K, int NW) { return ((N / 32) * (K / 32) + NW - 1) / NW; }

// ---- the dense configuration
// Rows per row block of the dense kernels for batch size B: 0 = no split (a workgroup sees all rows of its 16 columns: <= 128 rows,
// where sixteen or eight waves splitting K keep a 16-column workgroup short); above, blocks of 64 rows (the batch-64 configuration:
// sixteen waves split K) up to 368 rows and of 128 rows (eight waves) from 384 on, so that fc1 / fc2 run 4 x 64 / 4 x 32 workgroups at
// batch 512 instead of 64 / 32 (measured, ms per step at 256 / 512: unsplit 0.412 / 0.658, blocks of 64 0.315 / 0.442, of 128
// 0.337 / 0.408).
inline int dense_row_block(const TrainTuning &t, int B) {
    if (t.rb == 0 || ((t.rb == 64 || t.rb == 128) && B > t.rb)) return t.rb;
    return B > 128 ? (B >= 384 ? 128 : 64) : 0;
}

// <RTM, NW, PF, SPLIT> of the dense templates: row tiles a workgroup holds, waves that split K, prefetch depth (0: one buffer), by the
// rows a workgroup holds (az_train.hip, "dense layers: shared pieces").  One of six: four unsplit, two split.
struct DenseConfig { int RTM, NW, PF, SPLIT; };
inline DenseConfig dense_config(int rows, bool split) {
    if (split) return rows == 64 ? DenseConfig{4, 16, 1, 1} : DenseConfig{8, 8, 1, 1};
    if (rows <= 64) return {4, 16, 1, 0};  // (both register buffers two steps deep: 0.219 vs 0.195 ms at batch 64)
    if (rows <= 128) return {8, 8, 1, 0};
    if (rows <= 256) return {16, 4, 1, 0};
    return {32, 4, 0, 0};
}

// ---- the plan
struct TrainShape { int game, F1, F2, FIN, NHP; };  // what a plan depends on besides the batch size (az_trainer_create fills it)

enum TrainKernel {
    TK_CONV1_FWD, TK_CONV_FWD, TK_FC_FWD, TK_FC_FIN, TK_HEADS_FWD, TK_HEADS_BWD, TK_BN1D_BWD_FIN, TK_FC_DGRAD, TK_MIX1, TK_MIX2, TK_CONV_BWD,
    TK_CONV1_BWD, TK_UPDATE, TK_TTT_STEP
};

struct TrainLaunch {
    TrainKernel k;
    int gx, gy, threads, lds;  // grid, block, dynamic LDS bytes
    int arg;                   // the kernel's integer argument: layer l, or the weight-gradient workgroups nw in front (0: it takes none)
    int RB, NRB;               // what this launch's TDims carries: the step's own, except fc2's forward and its k_fc_fin under the 64-row override
};

#define TRAIN_MAX_LAUNCHES 19
struct TrainPlan {
    int B, S, NB, RB, NRB, F1B;  // TDims' fields of the same names
    int RTM, NW, PF, SPLIT;      // the step's dense configuration
    int NT;                      // 16-column tiles of the heads (1 / 3 / 5)
    int n_launches;
    TrainLaunch launches[TRAIN_MAX_LAUNCHES];
};
static_assert(sizeof(TrainPlan) == (12 + 8 * TRAIN_MAX_LAUNCHES) * sizeof(int), "no padding: plans compare as bytes");
inline bool same_plan(const TrainPlan &a, const TrainPlan &b) { return memcmp(&a, &b, sizeof a) == 0; }

// Fourteen launches; fifteen where several workgroups share a board or AZ_TRAIN_FOLD1=0 (k_conv1_bwd on its own); nineteen where the
// dense layers are row-split (four finalize kernels, and k_conv1_bwd).  TicTacToeNet: one.
inline TrainPlan plan_train_step(const TrainShape &s, const TrainTuning &t, int B) {
    TrainPlan p = {};
    const auto add = [&p](TrainKernel k, int gx, int gy, int threads, int lds, int arg, int rb = 0) {  // rb: a row block of the launch's own
        p.launches[p.n_launches++] = TrainLaunch{k, gx, gy, threads, lds, arg, rb ? rb : p.RB, rb ? gy : p.NRB};
    };
    p.B = B; p.S = 1; p.NB = 1; p.RB = B; p.NRB = 1;
    if (s.game == AZ_TICTACTOE) { add(TK_TTT_STEP, 1, 1, TPB, ttt_lds_bytes(B), 0); return p; }
    // workgroups per board in the conv kernels (must divide 256)
    for (p.S = t.split; p.S > 1 && B * p.S > 256;) p.S >>= 1;
    p.NB = B * p.S < 256 ? B * p.S : 256;
    const int rb = dense_row_block(t, B);
    if (rb) { p.RB = rb; p.NRB = (B + rb - 1) / rb; }
    // conv1's backward folded into conv2's (one launch less) where a workgroup holds whole boards and fc1's weight gradient does not
    // need k_conv1_bwd's launch
    p.F1B = (t.fold1 && p.S == 1 && rb == 0) ? 1 : 0;
    const DenseConfig c = dense_config(p.RB, rb != 0);
    p.RTM = c.RTM; p.NW = c.NW; p.PF = c.PF; p.SPLIT = c.SPLIT; p.NT = s.NHP / 16;
    const int tw = c.NW * 64, fcl = fc_lds_bytes(c.NW, p.RB);

    add(TK_CONV1_FWD, p.NB, 1, TPB, 0, 0);
    for (int l = 1; l <= 3; ++l) add(TK_CONV_FWD, p.NB, 1, TPB, CONV_FWD_LDS_BYTES, l);
    add(TK_FC_FWD, s.F1 / 16, p.NRB, tw, fcl, 1);
    if (c.SPLIT) add(TK_FC_FIN, s.F1 / 16, p.NRB, TPB, 0, 1);
    if (c.SPLIT && c.RTM == 8 && t.fc2_rb64) {
        // fc2 has half of fc1's columns: at 128 rows per block its forward would run 32 x NRB = 128 workgroups on 256 CUs.  It takes the
        // 64-row configuration (sixteen waves split K) instead; its statistics partials and its finalize kernel follow that block size
        const DenseConfig c2 = dense_config(64, true);
        const int nrb2 = (B + 63) / 64;
        add(TK_FC_FWD, s.F2 / 16, nrb2, c2.NW * 64, fc_lds_bytes(c2.NW, 64), 2, 64);
        add(TK_FC_FIN, s.F2 / 16, nrb2, TPB, 0, 2, 64);
    } else {
        add(TK_FC_FWD, s.F2 / 16, p.NRB, tw, fcl, 2);
        if (c.SPLIT) add(TK_FC_FIN, s.F2 / 16, p.NRB, TPB, 0, 2);
    }
    add(TK_HEADS_FWD, B / 16, 1, 8 * 64, 0, 0);
    add(TK_HEADS_BWD, s.F2 / 16, p.NRB, TPB, heads_bwd_lds_bytes(p.RB), 0);
    if (c.SPLIT) add(TK_BN1D_BWD_FIN, s.F2 / 16, p.NRB, TPB, 0, 2);
    add(TK_FC_DGRAD, s.F1 / 16, p.NRB, tw, fcl, 0);
    if (c.SPLIT) add(TK_BN1D_BWD_FIN, s.F1 / 16, p.NRB, TPB, 0, 1);
    // weight-gradient workgroups in front of k_mix1's / k_mix2's grid: fc2's tiles (K = the batch rows split over four waves of a tile
    // on the row-split path), fc1's (always the four-wave tile)
    const int nw2 = fc_wgrad_blocks(s.F2, s.F1, c.SPLIT ? c.NW / 4 : c.NW), nw1 = fc_wgrad_blocks(s.F1, s.FIN, 4);
    add(TK_MIX1, nw2 + (s.FIN / 16) * p.NRB, 1, tw, fcl, nw2);
    const bool wg_late = c.SPLIT && t.wg_late;  // fc1's weight gradient beside conv1's backward instead of conv4's
    if (wg_late) add(TK_CONV_BWD, p.NB, 1, TPB, CONV_BWD_LDS_BYTES, 3);
    else add(TK_MIX2, nw1 + p.NB, 1, TPB, CONV_BWD_LDS_BYTES, nw1);
    add(TK_CONV_BWD, p.NB, 1, TPB, CONV_BWD_LDS_BYTES, 2);
    add(TK_CONV_BWD, p.NB, 1, TPB, CONV_BWD_LDS_BYTES, 1);
    if (wg_late) add(TK_CONV1_BWD, p.NB + (s.F1 / 32) * (s.FIN / 32), 1, TPB, CONV1_WG_LDS_BYTES, 0);
    else if (!p.F1B) add(TK_CONV1_BWD, p.NB, 1, TPB, 0, 0);
    add(TK_UPDATE, (UPD_ALL + 63) / 64 + 4 + (p.F1B ? 6 : 0), 1, TPB, 0, 0);
    return p;
}

// the kernel of launch l as rocprofv3 lists it: the dense templates as <RTM,NW,PF,SPLIT>, the heads' as <NT,8> / <RTM,NT,SPLIT>
inline std::string train_kernel_name(const TrainPlan &p, const TrainLaunch &l) {
    static const char *const names[] = {"k_conv1_fwd", "k_conv_fwd", "k_fc_fwd", "k_fc_fin", "k_heads_fwd", "k_heads_bwd", "k_bn1d_bwd_fin", "k_fc_dgrad",
                                        "k_mix1", "k_mix2", "k_conv_bwd", "k_conv1_bwd", "k_update", "k_ttt_step"};
    const DenseConfig c = dense_config(l.RB, p.SPLIT != 0);
    const char *split = c.SPLIT ? "true" : "false";
    char cfg[48] = "";
    if (l.k == TK_FC_FWD || l.k == TK_FC_DGRAD || l.k == TK_MIX1) snprintf(cfg, sizeof cfg, "<%d,%d,%d,%s>", c.RTM, c.NW, c.PF, split);
    if (l.k == TK_HEADS_BWD) snprintf(cfg, sizeof cfg, "<%d,%d,%s>", c.RTM, p.NT, split);
    if (l.k == TK_HEADS_FWD) snprintf(cfg, sizeof cfg, "<%d,8>", p.NT);
    return std::string(names[l.k]) + cfg;
}
