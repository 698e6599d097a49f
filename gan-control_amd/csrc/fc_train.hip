// One optimisation step of ONE stack of EqualLinear(activation='fused_lrelu') layers -- an attribute controller (controller_model.py:13-53)
// trained with L1 / MSE against a slice of the w latents (controller_trainer.py:202-229) -- in n_layers + 2 launches.  See
// gc_fc_stack_fwd_save_f32, gc_rec_loss_grad_f32 and gc_fc_stack_bwd_adam_f32 in include/gancontrol_hip.h.
//
//   forward   the kernel of csrc/fc_stack.hip for one stack without PixelNorm (the layer code is fc_stack_layers.h: the same bits), which also
//             stores every layer's output [batch, out_dim[l]]; the last one is the prediction.
//   loss      one workgroup: dy = d(mean loss) / d(pred) and the mean loss, summed in an order fixed by (batch, n).
//   backward  one launch per layer, last to first.  With g = dY * (A_l > 0 ? 1 : 0.2) * sqrt(2) the layer needs db = beta sum_b g,
//             dW = alpha g^T A_(l-1) and dX = alpha g W.  A workgroup owns KC columns of W: it needs g (recomputed by every workgroup from dY
//             and A_l, JC rows of W at a time through LDS), A_(l-1)[:, slab] and W[:, slab] and nothing of any other workgroup, and it
//             produces dX[:, slab] and dW[:, slab] completely -- so it applies Adam to W[:, slab] itself, from the chunk of the slab it holds
//             in LDS for dX: the gradient never reaches memory and nothing is reduced across workgroups.  One more workgroup does the bias.
//             The three sums are carried in twice the working precision by float32 operations (Sum2 below).
// fp32 FMA only, every sum in an order fixed by the shapes, no atomics, no flags, no grid barrier: the same inputs give the same bits.
#include <atomic>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "fc_stack_layers.h"

namespace {

using namespace gcfc;
constexpr int MAXB = 64;           // rows per step
constexpr float SQRT2 = 1.41421356237309515f;

struct Layers {
    float* w[MAXL];
    float* bias[MAXL];
    int n[MAXL];
    float alpha[MAXL], beta[MAXL];
};

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    Layers l;
    const float* x; float* acts;
    long long x_stride;
    int in_dim, n_layers, batch;
};

// grid: tile of BT samples.  fc_stacks_fwd_kernel (fc_stack.hip) for one stack without PixelNorm; every layer's rows also go to acts.
__global__ __launch_bounds__(NT) void fc_stack_fwd_save_kernel(FwdArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][BT * LDW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b0 = (long long)blockIdx.x * BT;
    const int nb = (int)min((long long)BT, a.batch - b0);
    const int in_dim = a.in_dim;
    for (int i = threadIdx.x; i < BT * LDW; i += NT) {
        const int b = i / LDW, kk = i - b * LDW;
        lds[0][i] = (b < nb && kk < in_dim) ? a.x[(b0 + b) * a.x_stride + kk] : 0.f;
        lds[1][i] = 0.f;
    }
    __syncthreads();
    float* cur = lds[0];
    float* nxt = lds[1];
    float* out = a.acts;
    int k = in_dim;
    for (int l = 0; l < a.n_layers; ++l) {
        const float* w = a.l.w[l];
        const float* bias = a.l.bias[l];
        const int n = a.l.n[l];
        const float alpha = a.l.alpha[l], beta = a.l.beta[l];
        if ((k & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0) {
            if (k <= 256) layer_vec<1, 8>(w, bias, n, k, alpha, beta, cur, nxt, nb, lane, wave);
            else          layer_vec<2, 4>(w, bias, n, k, alpha, beta, cur, nxt, nb, lane, wave);
        } else {
            layer_scalar(w, bias, n, k, alpha, beta, cur, nxt, nb, lane, wave);
        }
        __syncthreads();
        float* t = cur; cur = nxt; nxt = t;
        k = n;
        // layer l's output: dense [batch, n] behind the outputs of the layers before it
        for (int i = threadIdx.x; i < nb * n; i += NT) {
            const int b = i / n, j = i - b * n;
            out[(b0 + b) * n + j] = cur[b * LDW + j];
        }
        out += (long long)a.batch * n;
    }
}

// ---- loss -------------------------------------------------------------------------------------------------------------------------------
constexpr int LT = 1024;

// one workgroup.  Thread t takes the elements t, t + LT, ...; its partial sum, the butterfly over a wave and the 16 wave sums added by thread 0
// in ascending order: an order fixed by (batch, n).
__global__ __launch_bounds__(LT) void rec_loss_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target, long long target_stride,
                                                           int batch, int n, int kind, float* __restrict__ dy, float* __restrict__ loss) {
    __shared__ float part[LT / 64];
    const int total = batch * n;
    const float inv = 1.f / (float)total;
    float s = 0.f;
    for (int i = threadIdx.x; i < total; i += LT) {
        const int b = i / n, j = i - b * n;
        const float d = pred[i] - target[b * target_stride + j];
        if (kind == GC_REC_LOSS_L1) {
            s += fabsf(d);
            dy[i] = d > 0.f ? inv : (d < 0.f ? -inv : 0.f);
        } else {
            s = fmaf(d, d, s);
            dy[i] = 2.f * d * inv;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < LT / 64; ++i) t += part[i];
        *loss = t * inv;
    }
}

// ---- backward + Adam ----------------------------------------------------------------------------------------------------------------------
constexpr int KC = 8;              // columns of W per workgroup
constexpr int JC = 128;            // rows of W (columns of g) per pass through LDS
constexpr int BN = 512;            // threads: one per (row b, column kk) of dX[:, slab] (MAXB * KC)
static_assert(BN == MAXB * KC && JC * KC % BN == 0 && BN >= MAXW, "thread mappings of fc_stack_bwd_adam_kernel");

// the scalars of one Adam step, each computed in float64 on the host and rounded once (as torch.optim.Adam passes them to its kernels:
// 1 - beta2 formed from the float32 beta2 would be off by up to 4e-6 of its value)
struct Adam {
    float beta1, beta2, omb1, omb2;          // omb = 1 - beta
    float step_size;                         // lr / (1 - beta1^t)
    float bc2_sqrt, eps;                     // sqrt(1 - beta2^t)
};

struct BwdArgs {
    float* w; float* bias; float* w_m; float* w_v; float* b_m; float* b_v;
    const float* dy;               // [batch, n] gradient of the layer's output
    const float* a_out;            // [batch, n] the layer's stored output
    const float* a_in;             // [batch, k] the layer's input, rows a_in_stride apart
    float* dx;                     // [batch, k] or null (the first layer)
    long long a_in_stride;
    int n, k, batch;
    float alpha, beta;
    Adam adam;
};

// torch.optim.Adam (weight_decay 0, no amsgrad, no maximize) on one element
__device__ __forceinline__ void adam_update(float* p, float* m, float* v, float g, const Adam& o) {
    // exp_avg.lerp_(grad, 1 - beta1) in ATen's form: the rounding of the weight touches only the smaller share of the result, and
    // beta1 = 0 (the controllers') gives grad itself
    const float diff = g - *m;
    const float mm = o.omb1 < 0.5f ? fmaf(o.omb1, diff, *m) : fmaf(-o.beta1, diff, g);
    const float vv = fmaf(o.beta2, *v, o.omb2 * g * g);
    *m = mm;
    *v = vv;
    *p -= o.step_size * (mm / (sqrtf(vv) / o.bc2_sqrt + o.eps));
}

// one rounding: the slope and the gain are one constant
__device__ __forceinline__ float act_grad(float dy, float a) { return dy * (a > 0.f ? SQRT2 : 0.2f * SQRT2); }

// A sum of products carried as the unevaluated pair s + c (Dot2 of Ogita, Rump and Oishi): the rounding error of every product (one FMA) and
// of every addition (TwoSum) is itself a float and goes to c, so s + c is the sum as if taken in twice the precision -- with float32
// operations alone and in a fixed order.  dX passes its rounding errors on to every layer in front of it; with plain FMA chains the first
// layer's gradient was 2 - 4 ulp off, with this the errors left are the single roundings of the stored values.  Nothing below may be
// contracted or reassociated: a fused s + x * y is not the float sum TwoSum corrects.
struct Sum2 { float s, c; };

__device__ __forceinline__ void add_value(Sum2& a, float p) {
#pragma clang fp contract(off)
    const float t = a.s + p;
    const float z = t - a.s;
    const float f = (a.s - (t - z)) + (p - z);
    a.s = t;
    a.c = a.c + f;
}

__device__ __forceinline__ void add_product(Sum2& a, float x, float y) {
#pragma clang fp contract(off)
    const float p = x * y;
    const float e = fmaf(x, y, -p);
    add_value(a, p);
    a.c = a.c + e;
}

__device__ __forceinline__ float total(const Sum2& a, Sum2 b) {
    Sum2 r = a;
    add_value(r, b.s);
    return r.s + (r.c + b.c);
}

// grid: ceil(k / KC) slab workgroups + one bias workgroup
__global__ __launch_bounds__(BN) void fc_stack_bwd_adam_kernel(BwdArgs a) {
    __shared__ float gs[MAXB][JC + 1];          // g[:, chunk]; rows one word longer: the threads of dX walk b at a stride of JC + 1 banks
    __shared__ float ws[JC][KC];                // W[chunk, slab] as it was before this step
    __shared__ float ap[MAXB][KC];              // A_(l-1)[:, slab]
    const int n = a.n, k = a.k, batch = a.batch;
    const int t = threadIdx.x;
    const int slabs = (k + KC - 1) / KC;
    if ((int)blockIdx.x == slabs) {
        // the bias: thread j sums g[:, j] over the rows in ascending order
        if (t < n) {
            Sum2 s{0.f, 0.f};
            for (int b = 0; b < batch; ++b) add_value(s, act_grad(a.dy[b * n + t], a.a_out[b * n + t]));
            adam_update(a.bias + t, a.b_m + t, a.b_v + t, a.beta * (s.s + s.c), a.adam);
        }
        return;
    }
    const int kk0 = blockIdx.x * KC;
    const int kc = min(KC, k - kk0);
    {
        const int b = t / KC, kk = t - b * KC;
        ap[b][kk] = (b < batch && kk < kc) ? a.a_in[b * a.a_in_stride + kk0 + kk] : 0.f;
    }
    const int xb = t / KC, xk = t - xb * KC;          // this thread's element of dX[:, slab]
    const int bpairs = (batch + 1) & ~1;              // rows past the batch are zero in gs and ap
    Sum2 dx0{0.f, 0.f}, dx1{0.f, 0.f};                // over the even and the odd rows of W, the chunks in ascending order
    for (int j0 = 0; j0 < n; j0 += JC) {
        const int jc = min(JC, n - j0);
        __syncthreads();          // the chunk before is consumed (and ap is complete)
        for (int i = t; i < MAXB * JC; i += BN) {
            const int b = i / JC, j = i - b * JC;
            gs[b][j] = (b < batch && j < jc) ? act_grad(a.dy[b * n + j0 + j], a.a_out[b * n + j0 + j]) : 0.f;
        }
        for (int i = t; i < JC * KC; i += BN) {
            const int j = i / KC, kk = i - j * KC;
            ws[j][kk] = (j < jc && kk < kc) ? a.w[(long long)(j0 + j) * k + kk0 + kk] : 0.f;
        }
        __syncthreads();
        // dX[b, slab] += g[b, chunk] W[chunk, slab]
        if (a.dx) {
            const int jpairs = (jc + 1) & ~1;          // (a row past the chunk is zero in ws)
            for (int j = 0; j < jpairs; j += 2) {
                add_product(dx0, gs[xb][j], ws[j][xk]);
                add_product(dx1, gs[xb][j + 1], ws[j + 1][xk]);
            }
        }
        // dW[chunk, slab] = alpha g[:, chunk]^T A_(l-1)[:, slab], and Adam on these elements of W: every thread of the workgroup has the
        // chunk's old values in ws by now (the barrier above), and no other workgroup reads these columns
        for (int i = t; i < JC * KC; i += BN) {
            const int j = i / KC, kk = i - j * KC;
            if (j < jc && kk < kc) {
                Sum2 s0{0.f, 0.f}, s1{0.f, 0.f};
                for (int b = 0; b < bpairs; b += 2) {
                    add_product(s0, gs[b][j], ap[b][kk]);
                    add_product(s1, gs[b + 1][j], ap[b + 1][kk]);
                }
                const long long at = (long long)(j0 + j) * k + kk0 + kk;
                adam_update(a.w + at, a.w_m + at, a.w_v + at, a.alpha * total(s0, s1), a.adam);
            }
        }
    }
    if (a.dx && xb < batch && xk < kc) a.dx[xb * k + kk0 + xk] = a.alpha * total(dx0, dx1);
}

// kernel launches issued by the three entries in this process (gc_fc_train_launches): how a test SEES n_layers + 2 launches per step
std::atomic<long long> launches{0};

// the checks the three entries share: GC_OK, or the code after gc::fail
int check_stack(const char* what, const void* x, int64_t x_stride, int in_dim, int n_layers, const void* const* w, const void* const* bias,
                const int32_t* out_dim, const float* alpha, const float* beta, int batch) {
    if (!w || !bias || !out_dim || !alpha || !beta) return gc::fail(GC_ERR_BAD_ARG, "%s: null table", what);
    if (batch < 1 || batch > MAXB) return gc::fail(GC_ERR_UNSUPPORTED, "%s: batch %d; 1 .. %d are built", what, batch, MAXB);
    if (n_layers < 1 || n_layers > MAXL) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d layers; 1 .. %d are built", what, n_layers, MAXL);
    if (in_dim < 1 || in_dim > MAXW) return gc::fail(GC_ERR_UNSUPPORTED, "%s: input width %d; 1 .. %d are built", what, in_dim, MAXW);
    for (int l = 0; l < n_layers; ++l) {
        if (out_dim[l] < 1 || out_dim[l] > MAXW)
            return gc::fail(GC_ERR_UNSUPPORTED, "%s: layer %d has output width %d; 1 .. %d are built", what, l, out_dim[l], MAXW);
        if (!w[l] || !bias[l]) return gc::fail(GC_ERR_BAD_ARG, "%s: layer %d has a null weight or bias", what, l);
    }
    if (!x) return gc::fail(GC_ERR_BAD_ARG, "%s: null input", what);
    if (x_stride < in_dim) return gc::fail(GC_ERR_BAD_ARG, "%s: row stride %lld is shorter than the rows (%d)", what, (long long)x_stride, in_dim);
    return GC_OK;
}

}  // namespace

extern "C" int gc_fc_stack_fwd_save_f32(const float* x, int64_t x_stride, int in_dim, int n_layers, const float* const* w, const float* const* bias,
                                        const int32_t* out_dim, const float* alpha, const float* beta, float* acts, int batch, gc_stream_t stream) {
    const char* what = "gc_fc_stack_fwd_save_f32";
    if (int rc = check_stack(what, x, x_stride, in_dim, n_layers, (const void* const*)w, (const void* const*)bias, out_dim, alpha, beta, batch)) return rc;
    if (!acts) return gc::fail(GC_ERR_BAD_ARG, "%s: null workspace", what);
    FwdArgs a;
    for (int l = 0; l < n_layers; ++l) {
        a.l.w[l] = const_cast<float*>(w[l]); a.l.bias[l] = const_cast<float*>(bias[l]);
        a.l.n[l] = out_dim[l]; a.l.alpha[l] = alpha[l]; a.l.beta[l] = beta[l];
    }
    a.x = x; a.acts = acts; a.x_stride = x_stride; a.in_dim = in_dim; a.n_layers = n_layers; a.batch = batch;
    hipLaunchKernelGGL(fc_stack_fwd_save_kernel, dim3(gc::ceil_div(batch, BT)), dim3(NT), 0, (hipStream_t)stream, a);
    ++launches;
    return gc::check_launch(what);
}

extern "C" int gc_rec_loss_grad_f32(const float* pred, const float* target, int64_t target_stride, int batch, int n, int kind, float* dy, float* loss,
                                    gc_stream_t stream) {
    const char* what = "gc_rec_loss_grad_f32";
    if (!pred || !target || !dy || !loss) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (kind != GC_REC_LOSS_L1 && kind != GC_REC_LOSS_MSE) return gc::fail(GC_ERR_BAD_ARG, "%s: kind %d", what, kind);
    if (batch < 1 || batch > MAXB) return gc::fail(GC_ERR_UNSUPPORTED, "%s: batch %d; 1 .. %d are built", what, batch, MAXB);
    if (n < 1 || n > MAXW) return gc::fail(GC_ERR_UNSUPPORTED, "%s: width %d; 1 .. %d are built", what, n, MAXW);
    if (target_stride < n) return gc::fail(GC_ERR_BAD_ARG, "%s: row stride %lld is shorter than the rows (%d)", what, (long long)target_stride, n);
    hipLaunchKernelGGL(rec_loss_grad_kernel, dim3(1), dim3(LT), 0, (hipStream_t)stream, pred, target, (long long)target_stride, batch, n, kind, dy, loss);
    ++launches;
    return gc::check_launch(what);
}

extern "C" int gc_fc_stack_bwd_adam_f32(const float* x, int64_t x_stride, int in_dim, int n_layers, float* const* w, float* const* bias,
                                        const int32_t* out_dim, const float* alpha, const float* beta, float* const* w_m, float* const* w_v,
                                        float* const* b_m, float* const* b_v, const float* acts, float* grads, int batch, double lr, double beta1,
                                        double beta2, double eps, double bias_correction1, double bias_correction2_sqrt, gc_stream_t stream) {
    const char* what = "gc_fc_stack_bwd_adam_f32";
    if (!w_m || !w_v || !b_m || !b_v) return gc::fail(GC_ERR_BAD_ARG, "%s: null table", what);
    if (int rc = check_stack(what, x, x_stride, in_dim, n_layers, (const void* const*)w, (const void* const*)bias, out_dim, alpha, beta, batch)) return rc;
    for (int l = 0; l < n_layers; ++l)
        if (!w_m[l] || !w_v[l] || !b_m[l] || !b_v[l]) return gc::fail(GC_ERR_BAD_ARG, "%s: layer %d has a null optimiser state", what, l);
    if (!acts || !grads) return gc::fail(GC_ERR_BAD_ARG, "%s: null workspace", what);
    if (!(bias_correction1 > 0.) || !(bias_correction2_sqrt > 0.))
        return gc::fail(GC_ERR_BAD_ARG, "%s: bias corrections %g / %g", what, bias_correction1, bias_correction2_sqrt);
    const Adam adam{(float)beta1, (float)beta2, (float)(1. - beta1), (float)(1. - beta2), (float)(lr / bias_correction1),
                    (float)bias_correction2_sqrt, (float)eps};
    // layer l's output and its gradient live at the same offset of acts and grads
    long long at[MAXL + 1];
    at[0] = 0;
    for (int l = 0; l < n_layers; ++l) at[l + 1] = at[l] + (long long)batch * out_dim[l];
    for (int l = n_layers - 1; l >= 0; --l) {
        BwdArgs a;
        a.w = w[l]; a.bias = bias[l]; a.w_m = w_m[l]; a.w_v = w_v[l]; a.b_m = b_m[l]; a.b_v = b_v[l];
        a.dy = grads + at[l];
        a.a_out = acts + at[l];
        a.a_in = l ? acts + at[l - 1] : x;
        a.a_in_stride = l ? out_dim[l - 1] : x_stride;
        a.dx = l ? grads + at[l - 1] : nullptr;
        a.n = out_dim[l]; a.k = l ? out_dim[l - 1] : in_dim; a.batch = batch;
        a.alpha = alpha[l]; a.beta = beta[l];
        a.adam = adam;
        hipLaunchKernelGGL(fc_stack_bwd_adam_kernel, dim3(gc::ceil_div(a.k, KC) + 1), dim3(BN), 0, (hipStream_t)stream, a);
        ++launches;
        if (int rc = gc::check_launch(what)) return rc;
    }
    return GC_OK;
}

extern "C" int64_t gc_fc_train_launches(void) { return launches.load(); }
