// az_host.h -- host-side helpers shared by the translation units of libaz_amd.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/az_amd.h"

void az_set_error(const char *fmt, ...);

#define AZ_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            az_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return AZ_EHIP;                                                                   \
        }                                                                                     \
    } while (0)

#define AZ_REQUIRE(cond, code, ...)     \
    do {                                \
        if (!(cond)) {                  \
            az_set_error(__VA_ARGS__);  \
            return (code);              \
        }                               \
    } while (0)

struct GameDesc;
// fills gd for (game,H,W); returns AZ_OK or AZ_EINVAL with the reference's constructor conditions
// (othello.py:87-88 odd size, connect4.py:90-91 smaller than 4x4)
int az_make_game_desc(int game, int H, int W, GameDesc *gd);

// ---- evaluation over the board's symmetries (az_symmetry.hip) ----
// mask: bit t = transform code t of aug_source (0 identity); AZ_SYM_ALL = every code valid for the board.  Writes the explicit
// mask and its member count; AZ_EINVAL (message set) for a code the game or board does not have.
int az_sym_resolve(const GameDesc *gd, int32_t mask, int32_t *mask_out, int *n_out);
// rows [0, min(*d_count, B)) (d_count NULL: B rows) of d_in -> n twins each, rows r*n+j of d_out; *d_count_out = n * rows (may be NULL)
int az_sym_expand(const GameDesc *gd, int32_t mask, const float *d_in, const int32_t *d_count, int B, float *d_out, int32_t *d_count_out,
                  hipStream_t st);
// the n member outputs of every row, mapped back and averaged (float32, member order) into d_probs / d_value rows [0, rows)
int az_sym_reduce(const GameDesc *gd, int32_t mask, const float *d_p, const float *d_v, const int32_t *d_count, int B, float *d_probs,
                  float *d_value, hipStream_t st);
// one member per row, d_codes[r] its transform code (trusted: a code the board does not have is read as the identity): the twin of
// rows [0, min(*d_count, B)) of d_in, and the twins' outputs gathered back through the inverse code (copies only)
int az_sym_twin(const GameDesc *gd, const uint8_t *d_codes, const float *d_in, const int32_t *d_count, int B, float *d_out, hipStream_t st);
int az_sym_unpick(const GameDesc *gd, const uint8_t *d_codes, const float *d_p, const float *d_v, const int32_t *d_count, int B, float *d_probs,
                  float *d_value, hipStream_t st);
// az_net.hip: what az_symmetry.hip needs of a network
struct az_net;
int az_net_max_batch(const az_net *net);
void az_net_shape(const az_net *net, int *game, int *H, int *W);
int az_net_sym_scratch(az_net *net, float **d_in, float **d_p, float **d_v);  // [max_batch] rows each, allocated at the first call
