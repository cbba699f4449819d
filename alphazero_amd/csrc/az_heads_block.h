// az_heads_block.h -- the policy + value heads of OthelloNet as a routine of ONE 256-thread workgroup, for a kernel that needs the heads
// of 16 rows of h2 and of no others (the fused search step).  The arithmetic is k_heads2's (az_net.hip) to the letter
// -- per output: bias, then k ascending on v_mfma_f32_16x16x4_f32; softmax with the exact maximum, az_det_expf, the row sum by one lane
// in ascending action order, e / S; az_det_tanhf on logit A -- so the priors and values carry the bits k_heads2 would have stored.
//   * rows: slot j of the block (threads 16 j .. 16 j + 15) brings row index `row` of X, or -1 for none; its own 16 lanes stage the row
//     into LDS (k_heads2's layout: K + 2 floats per row).  A slot without a row leaves its LDS row as it was: its logits are never read.
//   * weights: the head matrix in k_heads2's fragment order [K/16][NT][64 lanes][4], streamed from L2 PF loads ahead, requested before
//     the rows are staged.  NT column tiles on four waves: wave w takes tile w, and tile w + 4 where there is one, on a second
//     accumulator interleaved with the first (two independent chains: neither stops behind the other).
//   * outputs stay in LDS: *pr = the slot's A priors, *v its value.
// Barriers: one block-wide vote, then five barriers; EVERY thread of the block calls the routine, whatever its slot holds.  A block none
// of whose slots brings a row leaves behind the vote -- block-uniform.
#pragma once
#include "az_device.h"

typedef float hb_f32x4 __attribute__((ext_vector_type(4)));
#define AZ_HB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define AZ_HB_K 512  // F2 of the nets k_heads2 is instantiated for

template <int NT>
struct HeadsBlockLds {
    float X[16 * (AZ_HB_K + 2)];   // [16][K + 2]
    float L[16 * (NT * 16 + 1)];   // [16][NH + 1]: logits, then exponentials, then priors
    float rsum[16], val[16];
};

// the MFMA chains of one wave: NTW tiles (t0, t0 + 4) of the block's 16 rows
template <int NT, int NTW>
AZ_D void heads_block_chain(const float *Xs, float *Ls, const float4 *wq, float4 (&bq)[2][4], const float *bh, int t0, int lane) {
    constexpr int K = AZ_HB_K, NH = NT * 16, XSTR = K + 2, NKB = K / 16, PF = 4;
    const int m = lane & 15, kq = lane >> 4;
    hb_f32x4 acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) { const float bv = bh[(t0 + 4 * j) * 16 + m]; acc[j] = (hb_f32x4){bv, bv, bv, bv}; }
    const float *xa = Xs + m * XSTR + kq;  // A fragment of k-step ks: xa[4 * ks]
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        float4 b[NTW];
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            b[j] = bq[j][kb % PF];
            if (kb + PF < NKB) bq[j][kb % PF] = wq[(size_t)(kb + PF) * NT * 64 + (size_t)j * 4 * 64];
        }
        float a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = xa[16 * kb + 4 * i];
        __builtin_amdgcn_sched_barrier(0);  // loads stay issued ahead of this block's MFMAs
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[j] = AZ_HB_MFMA(a[0], b[j].x, acc[j]);
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[j] = AZ_HB_MFMA(a[1], b[j].y, acc[j]);
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[j] = AZ_HB_MFMA(a[2], b[j].z, acc[j]);
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[j] = AZ_HB_MFMA(a[3], b[j].w, acc[j]);
        __builtin_amdgcn_sched_barrier(0);
    }
    // C layout of 16x16x4: column lane & 15, rows 4 (lane >> 4) + r
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ls[(4 * kq + r) * (NH + 1) + (t0 + 4 * j) * 16 + m] = acc[j][r];
}

// Returns false where no slot of the block brought a row (nothing computed, *pr and *v untouched); else true with *pr / *v = the priors
// and the value of this thread's slot (meaningless for a slot that brought none).
template <int NT>
AZ_D bool heads_block16(const float *__restrict__ X, int row, const float *__restrict__ Wq, const float *__restrict__ bh, int A,
                        const float **pr, float *v) {
    constexpr int K = AZ_HB_K, NH = NT * 16, XSTR = K + 2, PF = 4, LSTR = NH + 1, C = K / 4 / 16;
    static_assert(NT >= 1 && NT <= 8, "tiles of four waves, two each at most");
    __shared__ __attribute__((aligned(16))) HeadsBlockLds<NT> s;
    if (!__syncthreads_or(row >= 0)) return false;  // block-uniform
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, slot = tid >> 4, sub16 = tid & 15;
    // the slot's row of X: every 16-byte load of the block in flight together
    float4 rx[C];
    if (row >= 0) {
        const float4 *src = reinterpret_cast<const float4 *>(X + (size_t)row * K);
#pragma unroll
        for (int i = 0; i < C; ++i) rx[i] = src[sub16 + 16 * i];
    }
    // this wave's fragments: Wq[kb][tile][lane]; the first PF of either tile are requested before the rows are staged
    const int t0 = wave;
    const bool has0 = t0 < NT, has1 = t0 + 4 < NT;  // wave-uniform
    const float4 *wq = reinterpret_cast<const float4 *>(Wq) + (size_t)(has0 ? t0 : 0) * 64 + lane;
    float4 bq[2][4];
#pragma unroll
    for (int p = 0; p < PF; ++p) {
        bq[0][p] = has0 ? wq[(size_t)p * NT * 64] : make_float4(0, 0, 0, 0);
        bq[1][p] = has1 ? wq[(size_t)p * NT * 64 + 4 * 64] : make_float4(0, 0, 0, 0);
    }
    if (row >= 0) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
            float *d = s.X + slot * XSTR + 4 * (sub16 + 16 * i);  // 8-byte aligned (XSTR is even)
            *reinterpret_cast<float2 *>(d) = make_float2(rx[i].x, rx[i].y);
            *reinterpret_cast<float2 *>(d + 2) = make_float2(rx[i].z, rx[i].w);
        }
    }
    __syncthreads();
    if (NT > 4 && has1) heads_block_chain<NT, 2>(s.X, s.L, wq, bq, bh, t0, lane);
    else if (has0) heads_block_chain<NT, 1>(s.X, s.L, wq, bq, bh, t0, lane);
    __syncthreads();
    // softmax (base.py:355 exp(log_softmax)), 8 lanes per row: max and exp in parallel, the row sum by one lane in ascending action order
    const int sub = tid & 7;
    for (int row_l = tid >> 3; row_l < 16; row_l += 256 / 8) {
        float *lrow = s.L + row_l * LSTR;
        float mx = -__builtin_inff();
        for (int a = sub; a < A; a += 8) mx = fmaxf(mx, lrow[a]);
#pragma unroll
        for (int o = 4; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 8));
        if (sub == 0) s.val[row_l] = az_det_tanhf(lrow[A]);
        for (int a = sub; a < A; a += 8) lrow[a] = az_det_expf(lrow[a] - mx);
    }
    __syncthreads();
    if (tid < 16) {
        const float *l = s.L + tid * LSTR;
        float sum = 0.0f;
        int a = 0;
        for (; a + 8 <= A; a += 8) {
            float t0 = l[a], t1 = l[a + 1], t2 = l[a + 2], t3 = l[a + 3], t4 = l[a + 4], t5 = l[a + 5], t6 = l[a + 6], t7 = l[a + 7];
            sum += t0; sum += t1; sum += t2; sum += t3; sum += t4; sum += t5; sum += t6; sum += t7;
        }
        for (; a < A; ++a) sum += l[a];
        s.rsum[tid] = sum;
    }
    __syncthreads();
    {   // p = e / S, in place, by the slot's own lanes
        float *lrow = s.L + slot * LSTR;
        const float S = s.rsum[slot];
        for (int a = sub16; a < A; a += 16) lrow[a] = lrow[a] / S;
    }
    __syncthreads();
    *pr = s.L + slot * LSTR;
    *v = s.val[slot];
    return true;
}
