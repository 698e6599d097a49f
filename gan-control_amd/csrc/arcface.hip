// The identity predictor of the embedding loss (losses/arc_face.py: ArcFace IR-SE, the reference's arc_face_model.py architecture) --
// forward and INPUT gradient, fp32.  The convolutions run on the generalised convolution kernels (gc_conv2d_fused_*, BatchNorm folded
// into the weights and the epilogue bias); what is left between them is here:
//   gc_crop_resize_ac_f32      centre crop (an offset and the row pitch of the full image: no copy) + F.interpolate(mode='bilinear',
//                              align_corners=True), and its adjoint: the full-size input gradient, zero outside the crop, one gather pass
//   gc_affine_prelu_f32        y = prelu(x * scale[c] + shift[c], alpha[c]) -- the BatchNorm in front of each block's first convolution
//                              (zero padding follows it, so it does not fold) and the PReLUs
//   gc_affine_prelu_bwd_f32    its input gradient, optionally plus a second incoming gradient: dense (identity shortcut) or scattered to
//                              the even pixels (the MaxPool2d(1, 2) shortcut) -- no separate full-plane add
//   gc_plane_reduce_f32        out[p] = mul * sum_hw a[p,:] (* b[p,:]): the squeeze mean and sum_hw g * r of its backward (deterministic)
//   gc_se_mlp_f32 / _bwd_f32   the squeeze-excitation MLP (fc1 -> ReLU -> fc2 -> sigmoid) per sample, and its backward down to the mean
//   gc_se_apply_f32            out = r * s[b,c] + shortcut, the shortcut read with a stride (the MaxPool2d(1, 2) subsample is never written)
// The SE backward's g_r = g * s + g_mean / HW is gc_affine_prelu_f32 over B*C planes of one sample (per-plane scale and shift).
#include "common.h"

#include <cstdint>

namespace {

using gc::f32x4_t;

constexpr int NT = 256;

// align_corners=True: src = o * (in - 1) / (out - 1), taken apart EXACTLY in integers: the lower neighbour i0 = floor(src), the upper one
// (clamped at the last pixel) and the weight of i1, rem / (out - 1) rounded once.  The fp32 product scale * o of the usual formulation is
// off by up to ~3e-5 px at a 480-pixel crop; the input gradient of the predictor is the resize adjoint applied to a gradient that alternates
// in sign between neighbouring 112-pixel samples (the stride-2 adjoints), whose near-cancelling weighted pairs turn that into ~2e-3 of its norm.
__device__ __forceinline__ float ac_source(int o, int in, int out, int& i0, int& i1) {
    if (out <= 1) {
        i0 = 0; i1 = in > 1 ? 1 : 0;
        return 0.f;
    }
    const int num = o * (in - 1), den = out - 1;
    i0 = num / den;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    return (float)(num - i0 * den) / (float)den;
}

__global__ __launch_bounds__(NT) void crop_resize_kernel(const float* __restrict__ x, float* __restrict__ y, int planes, int in_h, int in_w,
                                                         int top, int left, int crop_h, int crop_w, int out_h, int out_w) {
    const size_t total = (size_t)planes * out_h * out_w;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int ox = (int)(i % out_w), oy = (int)((i / out_w) % out_h);
        const size_t p = i / ((size_t)out_w * out_h);
        int y0, y1, x0, x1;
        const float ly = ac_source(oy, crop_h, out_h, y0, y1), lx = ac_source(ox, crop_w, out_w, x0, x1);
        const float* xp = x + p * in_h * in_w + (size_t)top * in_w + left;
        const float a = xp[(size_t)y0 * in_w + x0] * (1.f - lx) + xp[(size_t)y0 * in_w + x1] * lx;
        const float b = xp[(size_t)y1 * in_w + x0] * (1.f - lx) + xp[(size_t)y1 * in_w + x1] * lx;
        y[i] = a * (1.f - ly) + b * ly;
    }
}

// weight of crop pixel c in output sample o (the forward's own arithmetic, so the adjoint is its exact transpose)
__device__ __forceinline__ float ac_weight(int o, int c, int in, int out) {
    int i0, i1;
    const float l = ac_source(o, in, out, i0, i1);
    return (i0 == c ? 1.f - l : 0.f) + (i1 == c ? l : 0.f);
}

// the output samples that can read crop pixel c: floor(o * (in - 1) / (out - 1)) in {c - 1, c}, with a margin of one on either side
__device__ __forceinline__ void ac_range(int c, int in, int out, int& lo, int& hi) {
    if (in > 1 && out > 1) {
        lo = max(0, (max(c - 1, 0) * (out - 1)) / (in - 1) - 1);
        hi = min(out - 1, ((c + 1) * (out - 1)) / (in - 1) + 1);
    } else {
        lo = 0; hi = out - 1;
    }
}

// adjoint: one thread per pixel of the FULL input plane gathers the output samples that read it; fixed order, no atomics
__global__ __launch_bounds__(NT) void crop_resize_adj_kernel(const float* __restrict__ g, float* __restrict__ gx, int planes, int in_h, int in_w,
                                                             int top, int left, int crop_h, int crop_w, int out_h, int out_w) {
    const size_t total = (size_t)planes * in_h * in_w;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int ix = (int)(i % in_w), iy = (int)((i / in_w) % in_h);
        const size_t p = i / ((size_t)in_w * in_h);
        const int cy = iy - top, cx = ix - left;
        float acc = 0.f;
        if (cy >= 0 && cy < crop_h && cx >= 0 && cx < crop_w) {
            int ylo, yhi, xlo, xhi;
            ac_range(cy, crop_h, out_h, ylo, yhi);
            ac_range(cx, crop_w, out_w, xlo, xhi);
            const float* gp = g + p * out_h * out_w;
            for (int oy = ylo; oy <= yhi; ++oy) {
                const float wy = ac_weight(oy, cy, crop_h, out_h);
                if (wy == 0.f) continue;
                float row = 0.f;
                for (int ox = xlo; ox <= xhi; ++ox) {
                    const float wx = ac_weight(ox, cx, crop_w, out_w);
                    if (wx != 0.f) row = fmaf(wx, gp[(size_t)oy * out_w + ox], row);
                }
                acc = fmaf(wy, row, acc);
            }
        }
        gx[i] = acc;
    }
}

__device__ __forceinline__ float affine_prelu(float v, int c, const float* scale, const float* shift, const float* alpha) {
    v = fmaf(v, scale ? scale[c] : 1.f, shift ? shift[c] : 0.f);          // the backward rebuilds the same pre-activation
    if (alpha) v = v > 0.f ? v : alpha[c] * v;
    return v;
}

// grid: x over the plane in chunks of NT * VW elements, y = plane (b * C + c)
template <int VW>
__global__ __launch_bounds__(NT) void affine_prelu_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                          const float* __restrict__ alpha, float* __restrict__ y, int ch, int hw) {
    const int plane = blockIdx.y, c = plane % ch;
    const int e = (blockIdx.x * NT + threadIdx.x) * VW;
    if (e >= hw) return;
    const size_t base = (size_t)plane * hw + e;
    if (VW == 4) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + base);
        *reinterpret_cast<f32x4_t*>(y + base) = f32x4_t{affine_prelu(v[0], c, scale, shift, alpha), affine_prelu(v[1], c, scale, shift, alpha),
                                                        affine_prelu(v[2], c, scale, shift, alpha), affine_prelu(v[3], c, scale, shift, alpha)};
    } else {
        y[base] = affine_prelu(x[base], c, scale, shift, alpha);
    }
}

__device__ __forceinline__ float affine_prelu_grad(float g, float xv, int c, const float* scale, const float* shift, const float* alpha) {
    const float s = scale ? scale[c] : 1.f;
    if (alpha) {
        const float pre = fmaf(xv, s, shift ? shift[c] : 0.f);
        if (!(pre > 0.f)) g *= alpha[c];
    }
    return g * s;
}

// g2_mode: 0 none, 1 dense [B,C,h,w], 2 [B,C,ceil(h/2),ceil(w/2)] added at the even pixels (the adjoint of x[:, :, ::2, ::2])
template <int VW>
__global__ __launch_bounds__(NT) void affine_prelu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, const float* __restrict__ alpha, const float* __restrict__ g2,
                                                              int g2_mode, float* __restrict__ gx, int ch, int h, int w) {
    const int plane = blockIdx.y, c = plane % ch, hw = h * w;
    const int e = (blockIdx.x * NT + threadIdx.x) * VW;
    if (e >= hw) return;
    const size_t base = (size_t)plane * hw + e;
    if (VW == 4) {
        const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(g + base);
        f32x4_t xv = gv;
        if (alpha) xv = *reinterpret_cast<const f32x4_t*>(x + base);
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = affine_prelu_grad(gv[j], xv[j], c, scale, shift, alpha);
        if (g2_mode == 1) {
            const f32x4_t sv = *reinterpret_cast<const f32x4_t*>(g2 + base);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += sv[j];
        }
        *reinterpret_cast<f32x4_t*>(gx + base) = o;
    } else {
        float o = affine_prelu_grad(g[base], alpha ? x[base] : 0.f, c, scale, shift, alpha);
        if (g2_mode == 1) {
            o += g2[base];
        } else if (g2_mode == 2) {
            const int yy = e / w, xx = e % w;
            if (!(yy & 1) && !(xx & 1)) {
                const int h2 = (h + 1) >> 1, w2 = (w + 1) >> 1;
                o += g2[(size_t)plane * h2 * w2 + (size_t)(yy >> 1) * w2 + (xx >> 1)];
            }
        }
        gx[base] = o;
    }
}

// one workgroup per plane, fixed summation order (per-thread strided partials, then a fixed tree)
__global__ __launch_bounds__(NT) void plane_reduce_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int inner, float mul) {
    __shared__ float red[NT];
    const size_t base = (size_t)blockIdx.x * inner;
    float acc = 0.f;
    if (b) {
        for (int i = threadIdx.x; i < inner; i += NT) acc = fmaf(a[base + i], b[base + i], acc);
    } else {
        for (int i = threadIdx.x; i < inner; i += NT) acc += a[base + i];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] * mul;
}

constexpr int SE_MAX_CH = 2048, SE_MAX_RED = 256;

// sum over a wavefront in a fixed butterfly order (every lane ends with the same value)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one workgroup per sample: z = relu(fc1 @ m), s = sigmoid(fc2 @ z); fc1 [red, ch], fc2 [ch, red]
__global__ __launch_bounds__(NT) void se_mlp_kernel(const float* __restrict__ m, const float* __restrict__ fc1, const float* __restrict__ fc2,
                                                    float* __restrict__ z_out, float* __restrict__ s_out, int ch, int red) {
    __shared__ float ms[SE_MAX_CH];
    __shared__ float zs[SE_MAX_RED];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < ch; c += NT) ms[c] = m[(size_t)b * ch + c];
    __syncthreads();
    for (int j = wave; j < red; j += NT / 64) {
        float acc = 0.f;
        for (int c = lane; c < ch; c += 64) acc = fmaf(fc1[(size_t)j * ch + c], ms[c], acc);
        acc = fmaxf(wave_sum(acc), 0.f);
        if (lane == 0) {
            zs[j] = acc;
            z_out[(size_t)b * red + j] = acc;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < ch; c += NT) {
        float acc = 0.f;
        for (int j = 0; j < red; ++j) acc = fmaf(fc2[(size_t)c * red + j], zs[j], acc);
        s_out[(size_t)b * ch + c] = 1.f / (1.f + expf(-acc));
    }
}

// backward of se_mlp_kernel from t = dL/ds: gm = mul * fc1^T (relu'(z) * fc2^T (t * s * (1 - s)))
__global__ __launch_bounds__(NT) void se_mlp_bwd_kernel(const float* __restrict__ t, const float* __restrict__ s, const float* __restrict__ z,
                                                        const float* __restrict__ fc1, const float* __restrict__ fc2, float* __restrict__ gm,
                                                        int ch, int red, float mul) {
    __shared__ float gp[SE_MAX_CH];
    __shared__ float gz[SE_MAX_RED];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < ch; c += NT) {
        const float sv = s[(size_t)b * ch + c];
        gp[c] = t[(size_t)b * ch + c] * sv * (1.f - sv);
    }
    __syncthreads();
    for (int j = wave; j < red; j += NT / 64) {
        float acc = 0.f;
        for (int c = lane; c < ch; c += 64) acc = fmaf(fc2[(size_t)c * red + j], gp[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) gz[j] = z[(size_t)b * red + j] > 0.f ? acc : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < ch; c += NT) {
        float acc = 0.f;
        for (int j = 0; j < red; ++j) acc = fmaf(fc1[(size_t)j * ch + c], gz[j], acc);
        gm[(size_t)b * ch + c] = acc * mul;
    }
}

// out = r * s[plane] + sc[plane, y * st, x * st] (sc optional); grid: x over the plane, y = plane
__global__ __launch_bounds__(NT) void se_apply_kernel(const float* __restrict__ r, const float* __restrict__ s, const float* __restrict__ sc,
                                                      float* __restrict__ out, int h, int w, int sc_h, int sc_w, int st) {
    const int plane = blockIdx.y, hw = h * w;
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= hw) return;
    const size_t base = (size_t)plane * hw + e;
    float v = r[base] * s[plane];
    if (sc) {
        const int yy = e / w, xx = e % w;
        v += sc[(size_t)plane * sc_h * sc_w + (size_t)(yy * st) * sc_w + xx * st];
    }
    out[base] = v;
}

bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int gc_crop_resize_ac_f32(const float* x, float* y, int planes, int in_h, int in_w, int top, int left, int crop_h, int crop_w,
                                     int out_h, int out_w, int adjoint, gc_stream_t stream) {
    if (!x || !y) return gc::fail(GC_ERR_BAD_ARG, "gc_crop_resize_ac_f32: null pointer");
    if (planes < 0 || in_h <= 0 || in_w <= 0 || crop_h <= 0 || crop_w <= 0 || out_h <= 0 || out_w <= 0 || top < 0 || left < 0 ||
        top + crop_h > in_h || left + crop_w > in_w)
        return gc::fail(GC_ERR_BAD_ARG, "gc_crop_resize_ac_f32: bad extents (the crop must lie inside the image)");
    if ((int64_t)(crop_h + 1) * out_h >= INT32_MAX || (int64_t)(crop_w + 1) * out_w >= INT32_MAX)
        return gc::fail(GC_ERR_UNSUPPORTED, "gc_crop_resize_ac_f32: crop x output extent beyond 32-bit source arithmetic");
    if (planes == 0) return GC_OK;
    const size_t total = (size_t)planes * (adjoint ? (size_t)in_h * in_w : (size_t)out_h * out_w);
    const dim3 grid((unsigned)std::min<size_t>((total + NT - 1) / NT, 65535 * 4));
    if (adjoint)
        hipLaunchKernelGGL(crop_resize_adj_kernel, grid, dim3(NT), 0, (hipStream_t)stream, x, y, planes, in_h, in_w, top, left, crop_h, crop_w, out_h, out_w);
    else
        hipLaunchKernelGGL(crop_resize_kernel, grid, dim3(NT), 0, (hipStream_t)stream, x, y, planes, in_h, in_w, top, left, crop_h, crop_w, out_h, out_w);
    return gc::check_launch("gc_crop_resize_ac_f32");
}

extern "C" int gc_affine_prelu_f32(const float* x, const float* scale, const float* shift, const float* alpha, float* y, int batch, int channels,
                                   int hw, gc_stream_t stream) {
    if (!x || !y) return gc::fail(GC_ERR_BAD_ARG, "gc_affine_prelu_f32: null pointer");
    if (batch < 0 || channels <= 0 || hw <= 0) return gc::fail(GC_ERR_BAD_ARG, "gc_affine_prelu_f32: bad extents");
    if (batch == 0) return GC_OK;
    const int64_t planes = (int64_t)batch * channels;
    if (planes > 65535) return gc::fail(GC_ERR_UNSUPPORTED, "gc_affine_prelu_f32: more than 65535 planes");
    if (hw % 4 == 0 && aligned16(x) && aligned16(y)) {
        hipLaunchKernelGGL(affine_prelu_kernel<4>, dim3((unsigned)gc::ceil_div(hw, NT * 4), (unsigned)planes), dim3(NT), 0, (hipStream_t)stream,
                           x, scale, shift, alpha, y, channels, hw);
    } else {
        hipLaunchKernelGGL(affine_prelu_kernel<1>, dim3((unsigned)gc::ceil_div(hw, NT), (unsigned)planes), dim3(NT), 0, (hipStream_t)stream,
                           x, scale, shift, alpha, y, channels, hw);
    }
    return gc::check_launch("gc_affine_prelu_f32");
}

extern "C" int gc_affine_prelu_bwd_f32(const float* g, const float* x, const float* scale, const float* shift, const float* alpha, const float* g2,
                                       int g2_mode, float* gx, int batch, int channels, int h, int w, gc_stream_t stream) {
    if (!g || !gx || (alpha && !x) || (g2_mode != 0 && !g2)) return gc::fail(GC_ERR_BAD_ARG, "gc_affine_prelu_bwd_f32: null pointer");
    if (batch < 0 || channels <= 0 || h <= 0 || w <= 0 || g2_mode < 0 || g2_mode > 2) return gc::fail(GC_ERR_BAD_ARG, "gc_affine_prelu_bwd_f32: bad extents");
    if (batch == 0) return GC_OK;
    const int64_t planes = (int64_t)batch * channels;
    if (planes > 65535) return gc::fail(GC_ERR_UNSUPPORTED, "gc_affine_prelu_bwd_f32: more than 65535 planes");
    const int hw = h * w;
    if (g2_mode != 2 && hw % 4 == 0 && aligned16(g) && aligned16(x) && aligned16(g2) && aligned16(gx)) {
        hipLaunchKernelGGL(affine_prelu_bwd_kernel<4>, dim3((unsigned)gc::ceil_div(hw, NT * 4), (unsigned)planes), dim3(NT), 0, (hipStream_t)stream,
                           g, x, scale, shift, alpha, g2, g2_mode, gx, channels, h, w);
    } else {
        hipLaunchKernelGGL(affine_prelu_bwd_kernel<1>, dim3((unsigned)gc::ceil_div(hw, NT), (unsigned)planes), dim3(NT), 0, (hipStream_t)stream,
                           g, x, scale, shift, alpha, g2, g2_mode, gx, channels, h, w);
    }
    return gc::check_launch("gc_affine_prelu_bwd_f32");
}

extern "C" int gc_plane_reduce_f32(const float* a, const float* b, float* out, int planes, int inner, float mul, gc_stream_t stream) {
    if (!a || !out) return gc::fail(GC_ERR_BAD_ARG, "gc_plane_reduce_f32: null pointer");
    if (planes < 0 || inner <= 0) return gc::fail(GC_ERR_BAD_ARG, "gc_plane_reduce_f32: bad extents");
    if (planes == 0) return GC_OK;
    hipLaunchKernelGGL(plane_reduce_kernel, dim3((unsigned)planes), dim3(NT), 0, (hipStream_t)stream, a, b, out, inner, mul);
    return gc::check_launch("gc_plane_reduce_f32");
}

extern "C" int gc_se_mlp_f32(const float* m, const float* fc1, const float* fc2, float* z, float* s, int batch, int channels, int red, gc_stream_t stream) {
    if (!m || !fc1 || !fc2 || !z || !s) return gc::fail(GC_ERR_BAD_ARG, "gc_se_mlp_f32: null pointer");
    if (batch < 0 || channels <= 0 || red <= 0) return gc::fail(GC_ERR_BAD_ARG, "gc_se_mlp_f32: bad extents");
    if (channels > SE_MAX_CH || red > SE_MAX_RED) return gc::fail(GC_ERR_UNSUPPORTED, "gc_se_mlp_f32: at most %d channels, %d reduced", SE_MAX_CH, SE_MAX_RED);
    if (batch == 0) return GC_OK;
    hipLaunchKernelGGL(se_mlp_kernel, dim3((unsigned)batch), dim3(NT), 0, (hipStream_t)stream, m, fc1, fc2, z, s, channels, red);
    return gc::check_launch("gc_se_mlp_f32");
}

extern "C" int gc_se_mlp_bwd_f32(const float* t, const float* s, const float* z, const float* fc1, const float* fc2, float* gm, int batch, int channels,
                                 int red, float mul, gc_stream_t stream) {
    if (!t || !s || !z || !fc1 || !fc2 || !gm) return gc::fail(GC_ERR_BAD_ARG, "gc_se_mlp_bwd_f32: null pointer");
    if (batch < 0 || channels <= 0 || red <= 0) return gc::fail(GC_ERR_BAD_ARG, "gc_se_mlp_bwd_f32: bad extents");
    if (channels > SE_MAX_CH || red > SE_MAX_RED) return gc::fail(GC_ERR_UNSUPPORTED, "gc_se_mlp_bwd_f32: at most %d channels, %d reduced", SE_MAX_CH, SE_MAX_RED);
    if (batch == 0) return GC_OK;
    hipLaunchKernelGGL(se_mlp_bwd_kernel, dim3((unsigned)batch), dim3(NT), 0, (hipStream_t)stream, t, s, z, fc1, fc2, gm, channels, red, mul);
    return gc::check_launch("gc_se_mlp_bwd_f32");
}

extern "C" int gc_se_apply_f32(const float* r, const float* s, const float* sc, float* out, int planes, int h, int w, int sc_h, int sc_w, int sc_stride,
                               gc_stream_t stream) {
    if (!r || !s || !out) return gc::fail(GC_ERR_BAD_ARG, "gc_se_apply_f32: null pointer");
    if (planes < 0 || h <= 0 || w <= 0) return gc::fail(GC_ERR_BAD_ARG, "gc_se_apply_f32: bad extents");
    if (sc && (sc_stride <= 0 || (int64_t)(h - 1) * sc_stride >= sc_h || (int64_t)(w - 1) * sc_stride >= sc_w))
        return gc::fail(GC_ERR_BAD_ARG, "gc_se_apply_f32: the strided shortcut does not cover the output");
    if (planes == 0) return GC_OK;
    if (planes > 65535) return gc::fail(GC_ERR_UNSUPPORTED, "gc_se_apply_f32: more than 65535 planes");
    hipLaunchKernelGGL(se_apply_kernel, dim3((unsigned)gc::ceil_div(h * w, NT), (unsigned)planes), dim3(NT), 0, (hipStream_t)stream,
                       r, s, sc, out, h, w, sc_h, sc_w, sc_stride);
    return gc::check_launch("gc_se_apply_f32");
}
