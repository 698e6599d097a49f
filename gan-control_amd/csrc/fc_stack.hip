// Whole stacks of EqualLinear(activation='fused_lrelu') layers -- the mapping networks of the generator and the attribute controllers -- in ONE
// launch.  See gc_fc_stacks_fwd_f32 in include/gancontrol_hip.h.
//
// The split mapping network of the controllable generator is 7 stacks of PixelNorm + 8 x (GEMM + bias/leaky-ReLU launch) on [B, 64..256]
// operands (gan_model.py:171-202, :489-502), every driven controller 4 more layers (controller_model.py:13-53): ~175 launches per
// generated batch whatever B is, and interactive control is a batch-1 workload.  csrc/style.hip runs ONE layer of many groups per launch;
// here a workgroup owns (stack, tile of <= 8 samples) and walks ALL layers of its stack:
//   - the activations of the tile ping-pong between two LDS images [8][516] (rows padded by 4 floats: the 8 lanes that store one output
//     column of the 8 samples land on different banks); one __syncthreads() between layers;
//   - the waves split the output rows of a layer (8 rows in flight per wave, 4 where k > 256), the 64 lanes of a wave split k: lane c owns
//     the float4 columns c and c + 64 of every row, so its slice of the tile's activations sits in registers for the whole layer and a
//     weight row is ONE 16-byte load per lane, consecutive lanes on consecutive addresses; the rows' biases are requested with them;
//   - the 8 per-sample partial sums of a row meet in a fixed-order butterfly that halves the number of values at each of its first three
//     steps (10 exchanges, not 48); lane 8 b ends up with sample b;
//   - a layer whose k is no multiple of 4, or whose weight is not 16-byte aligned (the controllers' first layer: in_dim 1, 3, 27), takes
//     4-byte loads; the input rows and the output rows are read and written with 4-byte accesses at any alignment and any row stride.
// fp32 FMA only and every sum in an order fixed by the shapes: the same inputs give the same bits.  No workgroup waits for another one: no
// atomics, no flags, no grid barrier -- which is why one stack is NOT split over several workgroups.  The tables (pointers, strides, widths,
// alpha / beta per layer) travel BY VALUE in the kernel arguments: nothing is uploaded and nothing on the device has a lifetime.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "fc_stack_layers.h"

namespace {

using namespace gcfc;
constexpr int MAXS = 8;            // stacks per launch (a longer list is cut into launches)

struct Stack {
    const float* x; float* y;
    long long x_stride, y_stride;
    int in_dim, n_layers, pixel_norm, layer0;          // layer0: index of the stack's first layer in the per-layer tables
};

struct Args {
    Stack s[MAXS];
    const float* w[MAXS * MAXL];
    const float* bias[MAXS * MAXL];
    int n[MAXS * MAXL];
    float alpha[MAXS * MAXL], beta[MAXS * MAXL];
    int batch;
};
static_assert(sizeof(Args) <= 4096, "the tables travel in the kernel arguments");

// grid: (tile of BT samples, stack)
__global__ __launch_bounds__(NT) void fc_stacks_fwd_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) float lds[2][BT * LDW];
    const Stack& S = a.s[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b0 = (long long)blockIdx.x * BT;
    const int nb = (int)min((long long)BT, a.batch - b0);
    const int in_dim = S.in_dim;
    // the tile's input rows; every other word of both images is zero (rows past the batch stay zero through all layers)
    for (int i = threadIdx.x; i < BT * LDW; i += NT) {
        const int b = i / LDW, kk = i - b * LDW;
        lds[0][i] = (b < nb && kk < in_dim) ? S.x[(b0 + b) * S.x_stride + kk] : 0.f;
        lds[1][i] = 0.f;
    }
    __syncthreads();
    if (S.pixel_norm) {
        // wave b normalises sample b: x * rsqrt(mean_k x^2 + 1e-8)
        float* row = lds[0] + wave * LDW;
        float s = 0.f;
        for (int kk = lane; kk < in_dim; kk += 64) s = fmaf(row[kk], row[kk], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const float scale = 1.f / sqrtf(s / (float)in_dim + 1e-8f);
        for (int kk = lane; kk < in_dim; kk += 64) row[kk] *= scale;
        __syncthreads();
    }
    float* cur = lds[0];
    float* nxt = lds[1];
    int k = in_dim;
    for (int l = 0; l < S.n_layers; ++l) {
        const int L = S.layer0 + l;
        const float* w = a.w[L];
        const float* bias = a.bias[L];
        const int n = a.n[L];
        const float alpha = a.alpha[L], beta = a.beta[L];
        if ((k & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0) {
            if (k <= 256) layer_vec<1, 8>(w, bias, n, k, alpha, beta, cur, nxt, nb, lane, wave);
            else          layer_vec<2, 4>(w, bias, n, k, alpha, beta, cur, nxt, nb, lane, wave);
        } else {
            layer_scalar(w, bias, n, k, alpha, beta, cur, nxt, nb, lane, wave);
        }
        __syncthreads();
        float* t = cur; cur = nxt; nxt = t;
        k = n;
    }
    // the last layer's rows: y + b * y_stride, any alignment
    for (int i = threadIdx.x; i < nb * k; i += NT) {
        const int b = i / k, j = i - b * k;
        S.y[(b0 + b) * S.y_stride + j] = cur[b * LDW + j];
    }
}

}  // namespace

extern "C" int gc_fc_stacks_fwd_f32(const float* const* x, const int64_t* x_stride, float* const* y, const int64_t* y_stride,
                                    const int32_t* in_dim, const int32_t* n_layers, const int32_t* pixel_norm,
                                    const float* const* w, const float* const* bias, const int32_t* out_dim, const float* alpha, const float* beta,
                                    int n_stacks, int batch, gc_stream_t stream) {
    const char* what = "gc_fc_stacks_fwd_f32";
    if (n_stacks < 0) return gc::fail(GC_ERR_BAD_ARG, "%s: n_stacks %d", what, n_stacks);
    if (batch < 1) return gc::fail(GC_ERR_UNSUPPORTED, "%s: batch %d: at least one row is expected", what, batch);
    if (n_stacks == 0) return GC_OK;
    if (!x || !x_stride || !y || !y_stride || !in_dim || !n_layers || !pixel_norm || !w || !bias || !out_dim || !alpha || !beta)
        return gc::fail(GC_ERR_BAD_ARG, "%s: null table", what);
    // everything is checked before the first launch
    int layer = 0;
    for (int s = 0; s < n_stacks; ++s) {
        if (n_layers[s] < 1 || n_layers[s] > MAXL)
            return gc::fail(GC_ERR_UNSUPPORTED, "%s: stack %d has %d layers; 1 .. %d are built", what, s, n_layers[s], MAXL);
        if (in_dim[s] < 1 || in_dim[s] > MAXW)
            return gc::fail(GC_ERR_UNSUPPORTED, "%s: stack %d has input width %d; 1 .. %d are built", what, s, in_dim[s], MAXW);
        if (!x[s] || !y[s]) return gc::fail(GC_ERR_BAD_ARG, "%s: stack %d has a null operand", what, s);
        for (int l = 0; l < n_layers[s]; ++l, ++layer) {
            if (out_dim[layer] < 1 || out_dim[layer] > MAXW)
                return gc::fail(GC_ERR_UNSUPPORTED, "%s: stack %d layer %d has output width %d; 1 .. %d are built", what, s, l, out_dim[layer], MAXW);
            if (!w[layer]) return gc::fail(GC_ERR_BAD_ARG, "%s: stack %d layer %d has a null weight", what, s, l);
        }
        if (x_stride[s] < in_dim[s] || y_stride[s] < out_dim[layer - 1])
            return gc::fail(GC_ERR_BAD_ARG, "%s: stack %d: row strides %lld / %lld are shorter than the rows (%d / %d)", what, s,
                            (long long)x_stride[s], (long long)y_stride[s], in_dim[s], out_dim[layer - 1]);
    }
    const int tiles = gc::ceil_div(batch, BT);
    layer = 0;
    for (int first = 0; first < n_stacks; first += MAXS) {
        Args a;
        const int count = std::min(MAXS, n_stacks - first);
        int at = 0;
        for (int i = 0; i < count; ++i) {
            const int s = first + i;
            a.s[i] = Stack{x[s], y[s], (long long)x_stride[s], (long long)y_stride[s], in_dim[s], n_layers[s], pixel_norm[s] != 0, at};
            for (int l = 0; l < n_layers[s]; ++l, ++layer, ++at) {
                a.w[at] = w[layer]; a.bias[at] = bias[layer]; a.n[at] = out_dim[layer]; a.alpha[at] = alpha[layer]; a.beta[at] = beta[layer];
            }
        }
        a.batch = batch;
        hipLaunchKernelGGL(fc_stacks_fwd_kernel, dim3(tiles, count), dim3(NT), 0, (hipStream_t)stream, a);
        if (int rc = gc::check_launch(what)) return rc;
    }
    return GC_OK;
}
