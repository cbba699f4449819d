// Which kernel serves a stage of the network forward, and in which variant: decided here, once per launch, as a value.  az_net.hip
// launches from the plan (run_stage), az_net_stage_kernel reports from it, the profiler books under its slot, and
// tests/net_plan_table.cpp prints it without a GPU.  Plain C++17, no HIP: thresholds and their measurements live with the code below.
#pragma once
#include <limits.h>
#include <stdlib.h>

#ifndef AZ_PLAN_HD  // a rule the kernels apply too (az_search_plan.h has the same)
#if defined(__HIPCC__)
#define AZ_PLAN_HD __host__ __device__ inline
#else
#define AZ_PLAN_HD inline
#endif
#endif

#ifndef AZ_OTHELLO  // the games, as az_device.h numbers them
#define AZ_OTHELLO 0
#define AZ_CONNECT4 1
#define AZ_TICTACTOE 2
#endif

// Every environment switch of az_net.hip: name (default) meaning.  Read once per process (net_tuning); "A/B" marks switches kept
// for comparison runs.
struct NetTuning {
    int winograd;             // AZ_WINOGRAD (on): 0 = conv2 in the direct form everywhere, and with it no k_trunk_quad; the CPU oracle reads the same variable
    bool dense_i8;            // AZ_DENSE_I8 (0): 1 = OthelloNet's fc1 / fc2 in the exact block-fixed-point form (k_q_rows + k_qgemm); the oracle reads it too
    bool trunk_v1;            // AZ_TRUNK_V1 (0): 1 = never k_trunk2 (A/B)
    int trunk_quad;           // AZ_TRUNK_QUAD (-1: by plane and regime): 1 / 0 forces k_trunk_quad / k_trunk on the Winograd 8x8 and 7x6 planes (A/B)
    int trunk_quad_form;      // AZ_TRUNK_QUAD_FORM (-1: 7x6 form 1, 8x8 form 2): 0 / 1 / 2 forces one k_trunk_quad form (A/B)
    int trunk_quad_prefetch;  // AZ_TRUNK_QUAD_PREFETCH (-1: by regime, see plan_trunk): 0 = k_trunk_quad as it was everywhere, 1 = its prefetching form wherever it is built (A/B)
    int trunk_quad_stores;    // AZ_TRUNK_QUAD_STORES (-1: with the prefetching form by the same regime, see plan_trunk): 0 = the prefetching form's scalar stores everywhere, 1 = its vector stores wherever the prefetching form runs (A/B)
    int trunk_q_max;          // AZ_TRUNK_Q_MAX (512): boards up to which the trunk runs several waves per board (k_trunk_q); 0 = never
    int trunk_q_waves;        // AZ_TRUNK_Q_WAVES (0: by size): 8 forces eight waves per board, any other value four
    int trunk_blocks_per_cu;  // AZ_TRUNK_BLOCKS_PER_CU (-1: 3, and the natural size for the four-pass 8x8 forms): blocks per CU the LDS request of k_trunk / k_trunk_quad is padded to on the tuned planes; outside 1..8 = the natural size
    int beside_trunk2_min;    // AZ_BESIDE_TRUNK2_MIN (4096): boards from which a beside launch runs k_trunk2 (A/B)
    int beside_frag_max;      // AZ_BESIDE_FRAG_MAX (1024): rows up to which a beside launch runs k_dense_frag (A/B)
    int beside_tile;          // AZ_BESIDE_TILE (0: by size): AZ_GEMM_TILE's codes, for beside launches only (A/B)
    int gemm_solo;            // AZ_GEMM_SOLO (-1: by size): 0 = never a one-wave-per-SIMD GEMM, 1 / 2 forces k_gemm_solo / k_gemm_solo_t
    int dense_frag_max;       // AZ_DENSE_FRAG_MAX (-1: 1024 rows, 2048 for K >= 1024): rows up to which k_dense_frag runs; 0 = never
    int gemm_tile;            // AZ_GEMM_TILE (0: by size): k_gemm's tile 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 64x128 (A/B)
    int gemm_form;            // AZ_GEMM_FORM (-1: by regime, see plan_dense): 0 = k_gemm's double-buffer form everywhere, 1 = the ring form wherever it exists (A/B)
    int gemm_rows;            // AZ_GEMM_ROWS (-1: by regime, see plan_dense): 0 = 64 rows per block of k_gemm's 64 x 64 tile whatever the device row count, 1 = the count-following row forms wherever they exist (A/B)
    int qd_small_max;         // AZ_QD_SMALL_MAX (512): rows up to which k_qdense_small serves a fixed-point layer; 0 = never
    int qg_cfg;               // AZ_QG_CFG (0: by size): k_qgemm's tile plan 1 .. 5, see plan_dense (A/B; every plan gives the same bits)
    int heads_small_max;      // AZ_HEADS_SMALL_MAX (-1: 128, 0 for OthelloNet): rows up to which k_heads_small runs (A/B)
    bool heads_v1;            // AZ_HEADS_V1 (0): 1 = k_heads, the round-1 kernel, in place of k_heads2 (A/B)
    int heads_rh;             // AZ_HEADS_RH (0): 2 = 32-row blocks in k_heads2, anything else 16-row blocks (tuning)
    bool tail_v1;             // AZ_TAIL_V1 (0): 1 = the fma kernel k_tail_small in place of k_tail_mfma (A/B)
    bool no_fused_tail;       // AZ_NO_FUSED_TAIL (0): 1 = Connect4Net's fc1 / fc2 / heads as three stages
    int tail_r8_from;         // AZ_TAIL_R8_FROM (never): rows from which k_tail_small runs 32 rows per workgroup instead of 16
};

inline int net_env(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }

inline const NetTuning &net_tuning() {
    static const NetTuning t = [] {  // initialised exactly once, also with two host threads forwarding
        NetTuning v;
        v.winograd = net_env("AZ_WINOGRAD", -1); v.dense_i8 = net_env("AZ_DENSE_I8", 0) == 1; v.trunk_v1 = net_env("AZ_TRUNK_V1", 0) != 0;
        v.trunk_quad = getenv("AZ_TRUNK_QUAD") ? (net_env("AZ_TRUNK_QUAD", 0) ? 1 : 0) : -1;
        v.trunk_quad_form = net_env("AZ_TRUNK_QUAD_FORM", -1); v.trunk_q_max = net_env("AZ_TRUNK_Q_MAX", 512); v.trunk_q_waves = net_env("AZ_TRUNK_Q_WAVES", 0);
        v.trunk_blocks_per_cu = net_env("AZ_TRUNK_BLOCKS_PER_CU", -1);
        if (v.trunk_blocks_per_cu < 0 && getenv("AZ_TRUNK_BLOCKS_PER_CU")) v.trunk_blocks_per_cu = 0;  // set to a negative number: as any value outside 1..8
        v.beside_trunk2_min = net_env("AZ_BESIDE_TRUNK2_MIN", 4096); v.beside_frag_max = net_env("AZ_BESIDE_FRAG_MAX", 1024); v.beside_tile = net_env("AZ_BESIDE_TILE", 0);
        v.gemm_solo = net_env("AZ_GEMM_SOLO", -1); v.dense_frag_max = net_env("AZ_DENSE_FRAG_MAX", -1); v.gemm_tile = net_env("AZ_GEMM_TILE", 0);
        v.gemm_form = net_env("AZ_GEMM_FORM", -1); v.trunk_quad_prefetch = net_env("AZ_TRUNK_QUAD_PREFETCH", -1);
        v.trunk_quad_stores = net_env("AZ_TRUNK_QUAD_STORES", -1);
        v.gemm_rows = getenv("AZ_GEMM_ROWS") ? (net_env("AZ_GEMM_ROWS", 0) ? 1 : 0) : -1;
        v.qd_small_max = net_env("AZ_QD_SMALL_MAX", 512); v.qg_cfg = net_env("AZ_QG_CFG", 0);
        v.heads_small_max = net_env("AZ_HEADS_SMALL_MAX", -1); v.heads_v1 = net_env("AZ_HEADS_V1", 0) != 0; v.heads_rh = net_env("AZ_HEADS_RH", 0);
        v.tail_v1 = net_env("AZ_TAIL_V1", 0) != 0; v.no_fused_tail = net_env("AZ_NO_FUSED_TAIL", 0) != 0; v.tail_r8_from = net_env("AZ_TAIL_R8_FROM", INT_MAX);
        return v;
    }();
    return t;
}

// what the choice depends on (az_net.hip: net_dims)
struct NetDims {
    int game, CH, CW, FIN, F1, F2, NH, A;
    bool qd_on, fc1wq, fc2wq;  // the fixed-point dense layers are on; fc1 / fc2 exist in k_dense_frag's fragment order
};

enum NetKernel {
    K_NONE, K_MLP, K_TRUNK, K_TRUNK_QUAD, K_TRUNK_Q, K_TRUNK2, K_TAIL_MFMA, K_TAIL_SMALL, K_DENSE_FRAG, K_DENSE_SMALL, K_GEMM, K_GEMM_SOLO,
    K_GEMM_SOLO_T, K_QDENSE_SMALL, K_QGEMM /* k_q_rows + k_qgemm */, K_HEADS_SMALL, K_HEADS, K_HEADS2
};

struct StagePlan {
    int stage;
    NetKernel kernel;  // K_NONE: the stage launches nothing, it ran inside `family`'s launch (the fused tail's stages 2 and 3)
    NetKernel family;  // the kernel the stage is reported and booked under (= kernel wherever the stage launches)
    bool wino;         // trunk kernels: conv2 in the Winograd form
    int waves;         // k_trunk_q: waves per board (4 / 8); k_trunk2: waves per workgroup (4 / 8)
    int quad_form;     // k_trunk_quad: 0 / 1 / 2
    int quad_prefetch; // k_trunk_quad: 1 = the prefetching form (weights and input requested across the phase boundaries; same bits)
    int quad_stores;   // k_trunk_quad's prefetching form: 1 = conv3's planes and conv4's features stored as vectors (same bits)
    int lds_blocks;    // k_trunk, k_trunk_quad: blocks per CU the LDS request is padded to (outside 1..8: the kernel's natural size)
    int bm, bn;        // k_gemm: the workgroup tile (0: N fits none)
    int gemm_form;     // k_gemm: 0 = LDS double buffer, the chain stops at every K tile; 1 = LDS ring, the chain runs through (k_gemm_ring)
    int gemm_rows;     // k_gemm's 64 x 64 tile: 1 = the rows of a block follow the device row count (gemm_rows_per_block), 0 = 64 whatever the count
    int qg[4];         // k_qgemm: the tile plan <NWM, NWN, WM, WN>
    int nt, rh;        // k_heads, k_heads2: 16-column tiles; k_heads2: 16-row tiles per block
    int tail_r;        // k_tail_small: R (4 R rows per workgroup)
};

// layers k_dense_frag can run: K in whole 128-k groups of fragments (PF = 8 loads of 16 k), the 16 rows of K + 4 floats within the LDS
constexpr bool frag_shape(int N, int K) { return N % 64 == 0 && K % 128 == 0 && K <= 2048; }
// K / 32 of the layers k_gemm's tile loop is unrolled for: 512 / 1024 (Othello 8x8), 128 (Othello 6x6), 192 / 64 (Connect4); 0 = the runtime loop
constexpr int gemm_unrolled_kt(int K) { return (K == 1024 || K == 512 || K == 192 || K == 128 || K == 64) ? K / 32 : 0; }
// k_gemm's ring form exists for the 64 x 64 tile with an unrolled tile loop
constexpr bool gemm_ring_shape(int bm, int bn, int K) { return bm == 64 && bn == 64 && gemm_unrolled_kt(K) >= 2; }
// The count-following row forms of the 64 x 64 tile exist for OthelloNet 8x8's unrolled K: 512 and 1024 in the double-buffer form, 1024
// in the ring form (with them k_gemm_ring<16> would leave the 80 registers of its six waves per SIMD, so it stays as it was).  They
// address the rows and the weights by 32-bit byte offsets: 4 B K and 4 K N below 2^32.
constexpr bool gemm_rows_tile(int bm, int bn, int K, int form) { return bm == 64 && bn == 64 && (K == 1024 || (K == 512 && form == 0)); }
constexpr bool gemm_rows_shape(int bm, int bn, int B, int N, int K, int form) {
    return gemm_rows_tile(bm, bn, K, form) && (long long)K * N < (1LL << 30) && (long long)K * B < (1LL << 30);
}
// Rows per block of a launch of k_gemm's 64 x 64 tile with gy row bands, of which the device count fills m rows (clamped to the
// launch): the narrowest of 16 / 32 / 64 whose bands cover the count.  Kernel and host share it: the kernel maps its blocks by it,
// az_net_gemm_rows reports it.  follow = StagePlan::gemm_rows; a launch without a device count has m = its own rows, and runs 64.
AZ_PLAN_HD int gemm_rows_per_block(int gy, int m, int follow) {
    if (!follow) return 64;
    if ((m + 15) / 16 <= gy) return 16;
    if ((m + 31) / 32 <= gy) return 32;
    return 64;
}
// 8x8, 6x6 and 7x6 planes run the tuned kernels; every other plane between 5x5 and 8x8 -- Connect4Net on the board sizes the engine
// plays -- runs k_trunk (one board per wave, direct form) at any batch size
constexpr bool plane_tuned(int CH, int CW) { return (CH == 8 && CW == 8) || (CH == 6 && CW == 6) || (CH == 7 && CW == 6); }
// conv2 in the Winograd F(2x2,3x3) form (2.25x fewer multiplications; exact to the same 5e-7 as the direct form against the
// reference's torch forward; bit-equal to its restatement in the oracle, which reads the same switch AZ_WINOGRAD):
//   * 8x8 planes: ON.  From 4096 boards up both boards of a wave form one 32-row MFMA tile (conv2_wino32) in the
//     one-wave-per-SIMD variant of k_trunk2: 512 registers hold all 16 frequency accumulators, the LDS the other four waves
//     would use holds the transformed weights.  MI355X: 473 vs 526 us at 32768 boards, 71 vs 80 us at 4096.  Below 4096
//     boards k_trunk runs the 16-row form (conv2_wino; same chains, same bits): 21 vs 23 us at 1024 boards.
//   * 7x6 planes (Connect4): ON, in the same 32-row one-wave-per-SIMD form (12 tiles per board, 24 of the 32 rows of the MFMA tile):
//     100 vs 105.5 us at 8192 boards, 52.9 vs 54.8 at 4096; equal below 4096 boards (16-row form in k_trunk).  The 16-row form in
//     the two-waves-per-SIMD kernel had not paid (103 vs 101 us: with 16-row tiles every 32-cycle MFMA needs an operand transformed
//     by the wave itself and a 256-byte weight fragment -- the instruction stream, not the matrix pipe, is the limit).
//   * 6x6 planes: never (9 tiles per board would leave the MFMA tile 44 % empty).
constexpr bool plane_wino(int CH, int CW) { return (CH == 8 && CW == 8) || (CH == 7 && CW == 6); }
// k_trunk_quad's prefetching form is built for the 8x8 plane's form 2, the kernel it was measured on
constexpr bool quad_prefetch_shape(int CH, int CW, int form) { return CH == 8 && CW == 8 && form == 2; }

// `beside` (az_net_forward_lane): the forward shares the chip with another launch chain.  Thresholds of that regime, measured with two
// 2048-row chains of OthelloNet side by side (games/s of the headline):
//   * dense layers: k_dense_frag up to 1024 rows only, and k_gemm's 64 x 64 tile from ONE block per CU up (fc2 at 2048 rows: 256 blocks
//     instead of 128 of 64 x 128).  4 352 against 3 830 with the lone launch's picks (k_dense_frag for fc2, L2-bound at ~9 TB/s, or the
//     64 x 128 tile: the same 3 830): the other chain's kernels are the second resident block the lone launch needs two of its own for.
//   * trunk: k_trunk stays below 4096 boards (k_trunk2 from 2048: 3 652, its one-wave-per-SIMD blocks leave no room for the neighbour).
inline StagePlan plan_trunk(const NetDims &d, const NetTuning &t, int B, int beside) {
    StagePlan p = {};
    p.kernel = p.family = K_TRUNK;
    p.lds_blocks = 3;
    if (!plane_tuned(d.CH, d.CW)) return p;
    p.wino = t.winograd != 0 && plane_wino(d.CH, d.CW);
    // two boards per wave on 32x32x2 pays from ~4096 boards up (16384: 325 vs 331 us); below that the one-board-per-wave kernel fills
    // the chip better (2048: 45 vs 77 us).  One workgroup per CU: two waves per SIMD -- or, for the Winograd conv2, ONE wave per SIMD
    // with 512 registers (all 16 frequency accumulators live) and the transformed weights in the LDS the other four waves would use.
    if (!t.trunk_v1 && B >= (beside ? t.beside_trunk2_min : 4096)) { p.kernel = p.family = K_TRUNK2; p.waves = p.wino ? 4 : 8; return p; }
    if (B <= t.trunk_q_max) {  // few boards: four waves per board, eight while that leaves a SIMD at most two (11.7 vs 13.2 us; 512 boards: 23.0 vs 18.6)
        p.kernel = p.family = K_TRUNK_Q;
        p.waves = (t.trunk_q_waves ? t.trunk_q_waves : (B <= 256 ? 8 : 4)) == 8 ? 8 : 4;
        return p;
    }
    // resident blocks per CU = 160 KB / LDS request.  Measured on MI355X (4096 boards): 3 or 2 blocks per CU 88 us, 4 blocks 94 us,
    // 1 block 92 us -> pad the request to 3.  The four-pass QUAD forms: 8x8 asks for its natural size, 7x6 for the pad.
    const int want = t.trunk_blocks_per_cu >= 0 ? t.trunk_blocks_per_cu : 3;
    const int want_lean = t.trunk_blocks_per_cu >= 0 ? t.trunk_blocks_per_cu : (d.CH == 8 ? 0 : 3);
    p.lds_blocks = want;
    // k_trunk's workgroup of four boards sharing row tiles (QUAD) or every board its own tiles.  The QUAD form exists for the Winograd
    // 8x8 and 7x6 kernels, the planes it was measured on: 7x6 gains alone (4095 boards: 51.6 vs 55.7 us) and beside
    // another chain; 8x8 gains beside another chain (the headline's two groups) and loses ~1 us alone.
    if (!p.wino || !(t.trunk_quad >= 0 ? t.trunk_quad == 1 : (d.CH == 7 || beside))) return p;
    // Which k_trunk_quad.  0: conv2 in two passes of eight frequencies (256 registers, two waves per SIMD: a 2048-board launch fills the
    // register files and no wave of another chain is resident beside it).  1: four passes of one frequency row, U one k-step ahead
    // (<= 128 registers, four waves per SIMD).  2: four passes, U two k-steps ahead (<= 136 registers, three waves).  Same bits.
    // Default: 7x6 form 1, 8x8 form 2, each with the LDS request it measured best with; the legs are in profiles/r19_trunk_regs.txt.
    p.kernel = K_TRUNK_QUAD;  // reported as k_trunk, the family it belongs to
    p.quad_form = (t.trunk_quad_form >= 0 && t.trunk_quad_form <= 2) ? t.trunk_quad_form : (d.CH == 8 ? 2 : 1);
    if (p.quad_form) p.lds_blocks = want_lean;
    // The prefetching form.  The rule is the measured shape and no more: OthelloNet on the 8x8 plane beside another
    // chain (the headline's 2048-row groups), on every row count that runs k_trunk_quad there.  A lone launch forced onto k_trunk_quad
    // (AZ_TRUNK_QUAD=1) reaches it through AZ_TRUNK_QUAD_PREFETCH=1 only.  Legs: profiles/r24_trunk_prefetch.txt.
    const bool measured = d.game == AZ_OTHELLO && beside;
    p.quad_prefetch = quad_prefetch_shape(d.CH, d.CW, p.quad_form) && (t.trunk_quad_prefetch >= 0 ? t.trunk_quad_prefetch == 1 : measured) ? 1 : 0;
    // Its vector stores: conv3's planes as paired LDS writes, conv4's features as 16-byte stores.  A form OF the
    // prefetching form, under the same rule, on the same measurement (OthelloNet 8x8 beside another chain).  Legs:
    // profiles/r25_beside_fc1_trunk.txt.
    p.quad_stores = p.quad_prefetch && (t.trunk_quad_stores >= 0 ? t.trunk_quad_stores == 1 : measured) ? 1 : 0;
    return p;
}

// fc1 (stage 1) / fc2 (stage 2) of B rows
inline StagePlan plan_dense(const NetDims &d, const NetTuning &t, int stage, int B, int beside) {
    StagePlan p = {};
    const int N = stage == 1 ? d.F1 : d.F2, K = stage == 1 ? d.FIN : d.F1;
    auto is = [&p](NetKernel k) { p.kernel = p.family = k; return p; };
    if (d.qd_on) {  // the exact block-fixed-point form: one launch for few rows, else quantise the rows, then the int8 GEMM
        if (B <= t.qd_small_max && N % 64 == 0 && (K == 128 || K == 512 || K == 1024)) return is(K_QDENSE_SMALL);
        // 1: 64 x 128, four waves, two workgroups per CU; 2: 64 x 64, four waves; 3: 128 x 64, eight waves; 4: 128 x 128, eight waves;
        // 5: 64 x 128, eight waves.  By size: 128 x 128 tiles from one workgroup per CU up, 64 x 128 below.
        static const int plans[6][4] = {{0, 0, 0, 0}, {2, 2, 1, 2}, {2, 2, 1, 1}, {4, 2, 1, 1}, {4, 2, 1, 2}, {2, 4, 1, 1}};
        const int cfg = (t.qg_cfg >= 1 && t.qg_cfg <= 5) ? t.qg_cfg : ((long long)((B + 127) / 128) * (N / 128) >= 256 ? 4 : 5);
        for (int i = 0; i < 4; ++i) p.qg[i] = plans[cfg][i];
        return is(K_QGEMM);
    }
    // rows up to which k_dense_frag runs a layer.  Measured on OthelloNet 8x8 (us, k_dense_frag | what ran before: k_dense_small up to 128 / 256
    // rows, k_gemm above): fc1 (K = 512) 6.6 | 8.7 at 1 row, 7.3 | 21.0 at 256, 9.9 | 20.9 at 512, 16.3 | 21.2 at 1024, 22.3 | 21.0 at 1536;
    // fc2 (K = 1024) 11.2 | 15.9 at 1 row, 11.7 | 24.1 at 256, 11.9 | 39.8 at 512, 17.5 | 39.8 at 1024, 28.2 | 40.0 at 1536, 34.5 | 40.0 at 2048,
    // 65 | 37 at 4096 (every 16 rows stream the whole weight matrix from L2: ~9 TB/s from 1024 rows up, the kernel's bound there).
    const int lone_max = t.dense_frag_max >= 0 ? t.dense_frag_max : (K >= 1024 ? 2048 : 1024);
    const int fmax = (beside && t.beside_frag_max < lone_max) ? t.beside_frag_max : lone_max;
    if ((stage == 1 ? d.fc1wq : d.fc2wq) && B <= fmax && frag_shape(N, K)) return is(K_DENSE_FRAG);  // latency-bound row counts: the shortest accumulation chain
    // measured crossover against the tiled GEMM (MI355X): K = 512 up to 128 rows (15 vs 21 us), K = 1024 up to 256 rows (28 vs 40 us)
    if (B <= (K >= 1024 ? 256 : 128) && K % 32 == 0) return is(K_DENSE_SMALL);  // few rows: latency matters, not throughput
    // large row counts: the one-wave-per-SIMD kernel (256x256 workgroup tiles), from one tile per CU up
    const int solo = t.gemm_solo;
    if (solo != 0 && N % 256 == 0 && (solo == 1 || (long long)((B + 255) / 256) * (N / 256) >= 256)) return is(K_GEMM_SOLO);
    // below that: the same scheme on 128x128 tiles from TWO tiles per CU up (fc1 from 8192 rows, fc2 from 16384).  Measured against
    // k_gemm: 76 vs 80 us (fc1, 8192 rows), 137 vs 144 (fc2, 16384); with ONE tile per CU it loses (4096 rows: 42.6 vs 41.4 us, 64x128
    // tiles 57 vs 42): a 4096-cycle K tile does not carry its barrier and LDS turnaround without a partner wave, and k_gemm's two
    // blocks per CU are exactly that partner.
    if (solo != 0 && solo != 1 && N % 128 == 0 && (solo == 2 || (solo < 0 && (long long)((B + 127) / 128) * (N / 128) >= 512))) return is(K_GEMM_SOLO_T);
    // k_gemm: the largest tile that still gives every CU two resident blocks (512 blocks on 256 CUs): a block's barrier and LDS-fill
    // phases then overlap the other block's MFMAs.  Beside another chain the 64 x 64 tile runs from one block per CU up (above).
    const long long mb128 = (B + 127) / 128, mb64 = (B + 63) / 64;
    const int tile = t.gemm_tile ? t.gemm_tile : (beside ? t.beside_tile : 0);
    // The form.  A wave of the 64 x 64 tile holds one accumulator: 32 k are 16 dependent MFMAs, 1024 cycles, and the double-buffer form
    // stops the chain behind each of them for the staged loads, the LDS stores, the barrier and the first fragment reads.  Its own
    // stamps: fc2, one wave per SIMD, takes 1850 cycles per 32 k, 45 % of its tile loop outside the MFMA chain; fc1, two waves on most
    // SIMDs, takes 2590 for the 2048 of the two chains, 21 % (tools/probe_gemm.py prints the share against ONE chain, 59 % for fc1: the
    // partner's MFMAs counted as a stop).  With two blocks per CU a second wave of the launch fills the stop.  Beside another chain the
    // tile runs from ONE block per CU up, where nothing does -- the other chain's kernels do not -- and there the
    // ring form, whose chain runs through the boundary, is the pick: fc2 of the headline's 2048-row groups, 135.1 against 137.4 us per
    // pair of forwards.  The rule is the measured shape and no more: OthelloNet on the 8x8 plane (the neighbour is k_trunk_quad<8,8,2>,
    // whose 35 KB blocks the LDS figures were taken against), beside, at most one block per CU -- fc2 at 1985 .. 2048 rows.  Other nets
    // and planes reach the ring through AZ_GEMM_FORM=1 only.  Measured and left on the double buffer: beside launches above one block
    // per CU (fc1 at 480 blocks: 141 against 137.4 us per pair, with 25 KB of LDS as with 50), and lone launches (the ring is
    // 0.5 .. 2.5 us faster on every lone 64 x 64 launch measured; not the headline's regime, not made the rule on two runs).
    // Legs: profiles/r23_gemm_form.txt.
    auto tiled = [&](int bm, int bn) {
        p.bm = bm; p.bn = bn;
        const bool measured = d.game == AZ_OTHELLO && d.CH == 8 && d.CW == 8 && beside && bm == 64 && bn == 64 && mb64 * (N / 64) <= 256;
        p.gemm_form = gemm_ring_shape(bm, bn, K) && (t.gemm_form >= 0 ? t.gemm_form == 1 : measured) ? 1 : 0;
        // The rows of a block.  A replayed graph fixes a group's launch at 2048 rows; the lock-steps of a wave's first
        // and last plies fill a few hundred of them, and a block of this tile walks its whole K on ONE 32x32x2 chain however few blocks
        // run.  With the count-following forms a block takes 16 or 32 rows where the launch's bands still cover the count, on 16x16x4
        // chains four times / twice shorter; above that the 64-row path as it was.  The rule is the measured shape and no more:
        // OthelloNet 8x8, beside launches of this tile (either form).  Lone launches, other nets and planes: AZ_GEMM_ROWS=1 only.
        const bool rows_measured = d.game == AZ_OTHELLO && d.CH == 8 && d.CW == 8 && beside && bm == 64 && bn == 64;
        p.gemm_rows = gemm_rows_shape(bm, bn, B, N, K, p.gemm_form) && (t.gemm_rows >= 0 ? t.gemm_rows == 1 : rows_measured) ? 1 : 0;
        return is(K_GEMM);
    };
    if (tile == 1 && N % 128 == 0) return tiled(128, 128);
    if (tile == 2 && N % 64 == 0) return tiled(128, 64);
    if (tile == 3 && N % 64 == 0) return tiled(64, 64);
    if (tile == 4 && N % 128 == 0) return tiled(64, 128);
    if (N % 128 == 0 && mb128 * (N / 128) >= 512) return tiled(128, 128);
    if (N % 64 == 0 && mb128 * (N / 64) >= 512) return tiled(128, 64);
    if (N % 64 == 0 && mb64 * (N / 64) >= (beside ? 256 : 512)) return tiled(64, 64);
    if (N % 128 == 0) return tiled(64, 128);
    if (N % 64 == 0) return tiled(64, 64);
    return N % 32 == 0 ? tiled(128, 32) : tiled(0, 0);
}

inline StagePlan plan_heads(const NetDims &d, const NetTuning &t, int B) {
    StagePlan p = {};
    const bool heads2 = d.F2 == 512 && (d.NH == 80 || d.NH == 48);  // OthelloNet: the shapes k_heads2 is instantiated for
    // rows up to which the row-per-workgroup kernel runs: 128 where k_heads2 has no instantiation; never for OthelloNet, whose k_heads2 is
    // faster at every size (8.6 vs 9.8 us at one row, 9.6 vs 10.3 at 128)
    const int small_max = t.heads_small_max >= 0 ? t.heads_small_max : (heads2 ? 0 : 128);
    p.nt = d.NH / 16;
    // k_heads2, measured (us, 16-row / 32-row blocks; round-1 kernel): 4096 rows 9.9 / 14.5 / 15.5, 8192: 13.6 / 15.0, 16384: 20.3 / 21.4,
    // 32768: 39.0 / 55.7 / 44.4 -> 16-row blocks (more waves in flight) everywhere
    p.rh = t.heads_rh == 2 ? 2 : 1;
    if (B <= small_max && d.NH <= 128 && d.F2 % 32 == 0) p.kernel = K_HEADS_SMALL;  // few rows: latency, not throughput
    else p.kernel = (!t.heads_v1 && heads2) ? K_HEADS2 : K_HEADS;
    p.family = p.kernel;
    return p;
}

// stage 0 trunk, 1 fc1, 2 fc2, 3 heads of a launch of B boards
inline StagePlan plan_stage(const NetDims &d, const NetTuning &t, int stage, int B, int beside) {
    StagePlan p = {};
    if (d.game == AZ_TICTACTOE) { p.family = K_MLP; p.kernel = stage == 0 ? K_MLP : K_NONE; }
    // fc1 + fc2 + heads as ONE launch where the dense layers are small: Connect4 6x7 (8x8: 131 KB of fc1 weights, not worth restaging)
    else if (stage >= 1 && !t.no_fused_tail && d.F1 == 64 && d.F2 == 32 && d.NH == 16 && d.FIN == 192 && d.A == 7) {
        p.family = t.tail_v1 ? K_TAIL_SMALL : K_TAIL_MFMA;
        p.kernel = stage == 1 ? p.family : K_NONE;
        // k_tail_small: 16 rows per workgroup (measured: 9.3 us up to 4096 rows, 12.7 us at 8192; 32 rows per workgroup: 19 us at every size)
        p.tail_r = B >= t.tail_r8_from ? 8 : 4;
    }
    else p = stage == 0 ? plan_trunk(d, t, B, beside) : (stage == 3 ? plan_heads(d, t, B) : plan_dense(d, t, stage, B, beside));
    p.stage = stage;
    return p;
}

inline const char *net_kernel_name(NetKernel k) {
    static const char *const names[] = {"nothing", "k_mlp", "k_trunk", "k_trunk_quad", "k_trunk_q", "k_trunk2", "k_tail_mfma", "k_tail_small", "k_dense_frag",
                                        "k_dense_small", "k_gemm", "k_gemm_solo", "k_gemm_solo_t", "k_qdense_small", "k_q_rows + k_qgemm", "k_heads_small", "k_heads", "k_heads2"};
    return names[k];
}
// the kernel family a stage is listed under by rocprofv3 (template arguments abbreviated): what az_net_stage_kernel returns
inline const char *plan_family_name(const StagePlan &p) {
    if (p.family == K_TRUNK2 && p.wino) return "k_trunk2<Winograd conv2>";
    return net_kernel_name(p.family == K_TRUNK_QUAD ? K_TRUNK : p.family);
}
// the az_net_profile slot: k_trunk2, fc1 / fc2 on the tiled GEMMs (Connect4Net: the fused tail in the fc1 slot), heads, the k_trunk
// family | fc1 / fc2 on the small-batch kernels, k_trunk_q -- a slot per KERNEL family, so that a slot's mean is the figure rocprofv3
// lists for that kernel
inline int plan_slot(const StagePlan &p) {
    switch (p.family) {
        case K_TRUNK2: return 0;
        case K_TRUNK: case K_TRUNK_QUAD: return 4;
        case K_TRUNK_Q: return 7;
        case K_TAIL_MFMA: case K_TAIL_SMALL: return 1;
        case K_DENSE_FRAG: case K_DENSE_SMALL: case K_QDENSE_SMALL: return p.stage == 1 ? 5 : 6;
        default: return p.stage;
    }
}
