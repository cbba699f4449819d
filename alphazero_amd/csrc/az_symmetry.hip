// az_symmetry.hip -- leaf evaluation averaged over the board's symmetries (ensemble inference).
//
// The networks are not equivariant; Othello and TicTacToe positions have eight symmetries, Connect4 two.  The trainer uses them to
// augment samples (az_augment.hip); here the search does: every pending row is expanded into its n twins (k_sym_expand, the state
// twin k_augment emits), the ordinary network runs on the n * rows boards, and k_sym_reduce maps each member's policy back to the
// original orientation and averages policy and value.  Transform codes are aug_source's (az_device.h), 0 = identity.
// Both kernels are pure permutations plus n - 1 additions per output: a wave per row, plain vector loads and stores.
//
// One member per row (random mode): every row carries a transform code of its own (one byte).  k_sym_twin writes the
// row's twin under that code, the ordinary network runs on as many rows as came in, and k_sym_unpick gathers the twin's policy back
// through the inverse code and copies its value -- copies only, no sum, no division.  The engine draws the codes per game
// (k_sym_pick, az_engine.hip: only a slot knows its game id and ply); az_net_forward_sym_codes takes them from the caller.
#include "az_device.h"
#include "az_host.h"

#define SYM_WAVES 4  // rows per 256-thread workgroup

// rows really present: the device count (clamped like az_net_forward_dyn clamps it) or the host's B
AZ_D int sym_rows(const int *cnt, int B) {
    if (!cnt) return B;
    const int c = *cnt;
    return c < B ? (c < 0 ? 0 : c) : B;
}

// lane = cell of the twin; one gather per member, stores coalesced
__global__ __launch_bounds__(64 * SYM_WAVES) void k_sym_expand(GameDesc gd, int mask, int n, const float *__restrict__ in, const int *cnt, int B,
                                                               float *__restrict__ out, int *cnt_out) {
    const int rows = sym_rows(cnt, B);
    if (cnt_out && blockIdx.x == 0 && threadIdx.x == 0) *cnt_out = n * rows;
    const int r = blockIdx.x * SYM_WAVES + (threadIdx.x >> 6), x = threadIdx.x & 63;
    if (r >= rows || x >= gd.cells) return;
    const float *src = in + (size_t)r * gd.cells;
    const int i = x / gd.W, c0 = x % gd.W;
    int j = 0;
    for (int t = 0; t < 8; ++t) {
        if (!(mask & (1 << t))) continue;
        int rr, cc;
        aug_source(t, gd.H, gd.W, i, c0, &rr, &cc);
        out[((size_t)r * n + j) * gd.cells + x] = src[rr * gd.W + cc];
        ++j;
    }
}

// lane = action of the original orientation (Othello 8x8 has 65: the loop's second trip is the pass entry alone, kept in place).
// Sums are float32, sequential in member order starting from member 0, no fma (the library is built with -ffp-contract=off).
__global__ __launch_bounds__(64 * SYM_WAVES) void k_sym_reduce(GameDesc gd, int mask, int n, const float *__restrict__ p, const float *__restrict__ v,
                                                               const int *cnt, int B, float *__restrict__ probs, float *__restrict__ value) {
    const int rows = sym_rows(cnt, B);
    const int r = blockIdx.x * SYM_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const int A = gd.A;
    const float fn = (float)n;
    for (int a = lane; a < A; a += 64) {
        float s = 0.0f;
        int j = 0;
        for (int t = 0; t < 8; ++t) {
            if (!(mask & (1 << t))) continue;
            int f;  // the twin's entry that holds original action a: the pi mapping of the inverse code
            if (gd.game == AZ_CONNECT4) f = (t & 1) ? A - 1 - a : a;
            else if (a >= gd.cells) f = a;
            else { int rr, cc; aug_source(aug_inverse(t), gd.H, gd.W, a / gd.W, a % gd.W, &rr, &cc); f = rr * gd.W + cc; }
            const float q = p[((size_t)r * n + j) * A + f];
            s = j == 0 ? q : s + q;
            ++j;
        }
        probs[(size_t)r * A + a] = s / fn;
    }
    if (lane == 0) {
        float s = v[(size_t)r * n];
        for (int j = 1; j < n; ++j) s = s + v[(size_t)r * n + j];
        value[r] = s / fn;
    }
}

// the codes a board has as a mask (az_sym_resolve's rule); a code outside it -- codes from a caller are trusted, the engine's are
// drawn from a valid mask -- is read as the identity, so that no gather can leave the row
AZ_D int sym_code_of(const GameDesc &gd, const uint8_t *codes, int r) {
    const int valid = (gd.game != AZ_CONNECT4 && gd.H == gd.W) ? 0xFF : 0x3;
    const int t = codes[r];
    return (t < 8 && ((valid >> t) & 1)) ? t : 0;
}

// lane = cell of the twin, one gather under the row's own code
__global__ __launch_bounds__(64 * SYM_WAVES) void k_sym_twin(GameDesc gd, const uint8_t *__restrict__ codes, const float *__restrict__ in, const int *cnt,
                                                             int B, float *__restrict__ out) {
    const int rows = sym_rows(cnt, B);
    const int r = blockIdx.x * SYM_WAVES + (threadIdx.x >> 6), x = threadIdx.x & 63;
    if (r >= rows || x >= gd.cells) return;
    int rr, cc;
    aug_source(sym_code_of(gd, codes, r), gd.H, gd.W, x / gd.W, x % gd.W, &rr, &cc);
    out[(size_t)r * gd.cells + x] = in[(size_t)r * gd.cells + rr * gd.W + cc];
}

// lane = action of the original orientation, as in k_sym_reduce (second trip: Othello 8x8's pass entry, kept in place)
__global__ __launch_bounds__(64 * SYM_WAVES) void k_sym_unpick(GameDesc gd, const uint8_t *__restrict__ codes, const float *__restrict__ p,
                                                               const float *__restrict__ v, const int *cnt, int B, float *__restrict__ probs,
                                                               float *__restrict__ value) {
    const int rows = sym_rows(cnt, B);
    const int r = blockIdx.x * SYM_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const int A = gd.A, t = sym_code_of(gd, codes, r);
    for (int a = lane; a < A; a += 64) {
        int f;  // the twin's entry that holds original action a
        if (gd.game == AZ_CONNECT4) f = (t & 1) ? A - 1 - a : a;
        else if (a >= gd.cells) f = a;
        else { int rr, cc; aug_source(aug_inverse(t), gd.H, gd.W, a / gd.W, a % gd.W, &rr, &cc); f = rr * gd.W + cc; }
        probs[(size_t)r * A + a] = p[(size_t)r * A + f];
    }
    if (lane == 0) value[r] = v[r];
}

#define AZ_TRY(x) do { int _rc = (x); if (_rc != AZ_OK) return _rc; } while (0)

int az_sym_resolve(const GameDesc *gd, int32_t mask, int32_t *mask_out, int *n_out) {
    const bool rotations = gd->game != AZ_CONNECT4 && gd->H == gd->W;  // gravity rules rotations out even on a square Connect4 board
    const int32_t valid = rotations ? 0xFF : 0x3;
    if (mask == AZ_SYM_ALL) mask = valid;
    AZ_REQUIRE(mask >= 0 && mask <= 0xFF, AZ_EINVAL, "symmetry mask 0x%x: a mask is a set of the transform codes 0..7 (or AZ_SYM_ALL)", (unsigned)mask);
    AZ_REQUIRE((mask & ~valid) == 0, AZ_EINVAL, "symmetry mask 0x%x holds rotation codes: %s has the identity and the horizontal reflection only (valid mask 0x%x)",
               (unsigned)mask, gd->game == AZ_CONNECT4 ? "Connect4" : "a board that is not square", (unsigned)valid);
    *mask_out = mask;
    *n_out = __builtin_popcount((unsigned)mask);
    return AZ_OK;
}

int az_sym_expand(const GameDesc *gd, int32_t mask, const float *d_in, const int32_t *d_count, int B, float *d_out, int32_t *d_count_out,
                  hipStream_t st) {
    const int n = __builtin_popcount((unsigned)mask);
    hipLaunchKernelGGL(k_sym_expand, dim3((unsigned)((B + SYM_WAVES - 1) / SYM_WAVES)), dim3(64 * SYM_WAVES), 0, st, *gd, (int)mask, n, d_in, d_count, B,
                       d_out, d_count_out);
    AZ_HIP(hipGetLastError());
    return AZ_OK;
}

int az_sym_reduce(const GameDesc *gd, int32_t mask, const float *d_p, const float *d_v, const int32_t *d_count, int B, float *d_probs,
                  float *d_value, hipStream_t st) {
    const int n = __builtin_popcount((unsigned)mask);
    hipLaunchKernelGGL(k_sym_reduce, dim3((unsigned)((B + SYM_WAVES - 1) / SYM_WAVES)), dim3(64 * SYM_WAVES), 0, st, *gd, (int)mask, n, d_p, d_v, d_count, B,
                       d_probs, d_value);
    AZ_HIP(hipGetLastError());
    return AZ_OK;
}

extern "C" int az_net_forward_sym(az_net *net, const float *d_input, int B, int32_t mask, float *d_probs, float *d_value, void *stream) {
    AZ_REQUIRE(net && d_input && d_probs && d_value, AZ_EINVAL, "null argument");
    AZ_REQUIRE(B > 0, AZ_EINVAL, "batch %d must be positive", B);
    GameDesc gd;
    int game, H, W, n = 0;
    az_net_shape(net, &game, &H, &W);
    AZ_TRY(az_make_game_desc(game, H, W, &gd));
    AZ_TRY(az_sym_resolve(&gd, mask, &mask, &n));
    if (n == 0) return az_net_forward(net, d_input, B, d_probs, d_value, stream);  // mask 0: off
    AZ_REQUIRE((long long)n * B <= az_net_max_batch(net), AZ_EINVAL, "%d symmetries of %d boards are %lld rows, the network's max_batch is %d", n, B,
               (long long)n * B, az_net_max_batch(net));
    float *in = nullptr, *p = nullptr, *v = nullptr;
    AZ_TRY(az_net_sym_scratch(net, &in, &p, &v));
    hipStream_t st = (hipStream_t)stream;
    AZ_TRY(az_sym_expand(&gd, mask, d_input, nullptr, B, in, nullptr, st));
    AZ_TRY(az_net_forward(net, in, n * B, p, v, stream));
    return az_sym_reduce(&gd, mask, p, v, nullptr, B, d_probs, d_value, st);
}

int az_sym_twin(const GameDesc *gd, const uint8_t *d_codes, const float *d_in, const int32_t *d_count, int B, float *d_out, hipStream_t st) {
    hipLaunchKernelGGL(k_sym_twin, dim3((unsigned)((B + SYM_WAVES - 1) / SYM_WAVES)), dim3(64 * SYM_WAVES), 0, st, *gd, d_codes, d_in, d_count, B, d_out);
    AZ_HIP(hipGetLastError());
    return AZ_OK;
}

int az_sym_unpick(const GameDesc *gd, const uint8_t *d_codes, const float *d_p, const float *d_v, const int32_t *d_count, int B, float *d_probs,
                  float *d_value, hipStream_t st) {
    hipLaunchKernelGGL(k_sym_unpick, dim3((unsigned)((B + SYM_WAVES - 1) / SYM_WAVES)), dim3(64 * SYM_WAVES), 0, st, *gd, d_codes, d_p, d_v, d_count, B,
                       d_probs, d_value);
    AZ_HIP(hipGetLastError());
    return AZ_OK;
}

extern "C" int az_net_forward_sym_codes(az_net *net, const float *d_input, int B, const uint8_t *d_codes, float *d_probs, float *d_value, void *stream) {
    AZ_REQUIRE(net && d_input && d_codes && d_probs && d_value, AZ_EINVAL, "null argument");
    AZ_REQUIRE(B > 0, AZ_EINVAL, "batch %d must be positive", B);
    AZ_REQUIRE(B <= az_net_max_batch(net), AZ_EINVAL, "batch %d exceeds the network's max_batch %d", B, az_net_max_batch(net));
    GameDesc gd;
    int game, H, W;
    az_net_shape(net, &game, &H, &W);
    AZ_TRY(az_make_game_desc(game, H, W, &gd));
    float *in = nullptr, *p = nullptr, *v = nullptr;
    AZ_TRY(az_net_sym_scratch(net, &in, &p, &v));
    hipStream_t st = (hipStream_t)stream;
    AZ_TRY(az_sym_twin(&gd, d_codes, d_input, nullptr, B, in, st));
    AZ_TRY(az_net_forward(net, in, B, p, v, stream));
    return az_sym_unpick(&gd, d_codes, p, v, nullptr, B, d_probs, d_value, st);
}
