// The layer code of the fused EqualLinear stacks: one workgroup of NT threads holds a tile of BT samples in two LDS images and walks a layer
// with layer_vec / layer_scalar.  Shared by csrc/fc_stack.hip (inference: gc_fc_stacks_fwd_f32) and csrc/fc_train.hip (the training forward
// that also stores every layer's output: gc_fc_stack_fwd_save_f32), so that both give the same bits for the same stack and input.
#pragma once
#include <cstdint>

#include "common.h"

namespace gcfc {

constexpr int MAXL = 8;            // layers per stack
constexpr int MAXW = 512;          // widest layer (input or output)
constexpr int BT = 8;              // samples per workgroup
constexpr int LDW = MAXW + 4;      // LDS row stride in floats (16-byte aligned rows; the padding is explained in fc_stack.hip)
constexpr int NT = 512, NW = NT / 64;
static_assert(NW == BT, "PixelNorm gives one wave to every sample of the tile");

__device__ __forceinline__ float dot4(float4 a, float4 b, float s) {
    s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); return fmaf(a.w, b.w, s);
}

// The sums over the 64 lanes of v[0 .. 7]: lane 8 b (and the 7 lanes after it) return the sum of v[b].  The steps over lane bits 5, 4, 3
// each send one half of the values to the partner lane and keep the other half; bits 2, 1, 0 are a plain butterfly.
__device__ __forceinline__ float reduce8(const float (&v)[BT], int lane) {
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
    float a[4], c[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float keep = h5 ? v[i + 4] : v[i], send = h5 ? v[i] : v[i + 4];
        a[i] = keep + __shfl_xor(send, 32, 64);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float keep = h4 ? a[i + 2] : a[i], send = h4 ? a[i] : a[i + 2];
        c[i] = keep + __shfl_xor(send, 16, 64);
    }
    const float keep = h3 ? c[1] : c[0], send = h3 ? c[0] : c[1];
    float d = keep + __shfl_xor(send, 8, 64);
    d += __shfl_xor(d, 4, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 1, 64);
    return d;
}

// leaky_relu(alpha * sum + beta_bias, 0.2) * sqrt(2) into column j of the next activations (lanes 8 b hold sample b)
__device__ __forceinline__ void finish_row(float sum, int j, int n, int nb, int lane, float alpha, float beta_bias, float* nxt) {
    const int b = lane >> 3;
    if (j < n && (lane & 7) == 0 && b < nb) {
        const float t = fmaf(alpha, sum, beta_bias);
        nxt[b * LDW + j] = (t > 0.f ? t : 0.2f * t) * 1.41421356237309515f;
    }
}

// rows j0 .. j0 + RU - 1 of w, float4 columns lane (and lane + 64).  Rows and columns past the end read the last one (an address inside w: the
// load stays one unconditional 16-byte load); the column's value is replaced by zero and such a row is never stored.
template <int QPL, int RU>
__device__ __forceinline__ void load_rows(float4 (&w4)[RU][QPL], const float* __restrict__ w, int j0, int n, int k, int lane) {
    const int k4 = k >> 2;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < RU; ++r) {
#pragma unroll
        for (int i = 0; i < QPL; ++i) {
            const int q = lane + 64 * i;
            const float4 v = reinterpret_cast<const float4*>(w + (long long)min(j0 + r, n - 1) * k)[min(q, k4 - 1)];
            w4[r][i] = q < k4 ? v : zero;
        }
    }
}

// k % 4 == 0, w 16-byte aligned, k <= 256 * QPL; RU weight rows in flight per wave (32 registers of weights either way)
template <int QPL, int RU>
__device__ __forceinline__ void layer_vec(const float* __restrict__ w, const float* __restrict__ bias, int n, int k, float alpha, float beta,
                                          const float* cur, float* nxt, int nb, int lane, int wave) {
    const int k4 = k >> 2;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xr[QPL][BT];
#pragma unroll
    for (int i = 0; i < QPL; ++i) {
        const int q = lane + 64 * i;
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const float4 v = reinterpret_cast<const float4*>(cur + b * LDW)[min(q, k4 - 1)];
            xr[i][b] = q < k4 ? v : zero;
        }
    }
    for (int j0 = wave * RU; j0 < n; j0 += NW * RU) {
        // the biases of the rows are requested with their weights: one round trip to memory per pass, not two
        float4 w4[RU][QPL];
        float bj[RU];
        load_rows<QPL, RU>(w4, w, j0, n, k, lane);
#pragma unroll
        for (int r = 0; r < RU; ++r) bj[r] = bias ? bias[min(j0 + r, n - 1)] : 0.f;
#pragma unroll
        for (int r = 0; r < RU; ++r) {
            float acc[BT];
#pragma unroll
            for (int b = 0; b < BT; ++b) {
                acc[b] = 0.f;
                if (b < nb) {
#pragma unroll
                    for (int i = 0; i < QPL; ++i) acc[b] = dot4(w4[r][i], xr[i][b], acc[b]);
                }
            }
            finish_row(reduce8(acc, lane), j0 + r, n, nb, lane, alpha, beta * bj[r], nxt);
        }
    }
}

// any k, any alignment of w: 4-byte loads, the activations read from LDS
__device__ __forceinline__ void layer_scalar(const float* __restrict__ w, const float* __restrict__ bias, int n, int k, float alpha, float beta,
                                             const float* cur, float* nxt, int nb, int lane, int wave) {
    for (int j = wave; j < n; j += NW) {
        const float* row = w + (long long)j * k;
        const float bj = bias ? bias[j] : 0.f;
        float acc[BT];
#pragma unroll
        for (int b = 0; b < BT; ++b) acc[b] = 0.f;
        for (int kk = lane; kk < k; kk += 64) {
            const float wv = row[kk];
#pragma unroll
            for (int b = 0; b < BT; ++b)
                if (b < nb) acc[b] = fmaf(wv, cur[b * LDW + kk], acc[b]);
        }
        finish_row(reduce8(acc, lane), j, n, nb, lane, alpha, beta * bj, nxt);
    }
}

}  // namespace gcfc
