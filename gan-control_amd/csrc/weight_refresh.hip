// Everything that happens to a network's parameters between Optimizer.step() and the next forward pass, in one pass per parameter:
// gc_weight_refresh_grouped_f32 (include/gancontrol_hip.h).
//
// The level-by-level refill (weight_layout.hip, the pack of conv_bf16x3.hip, style_wsq_kernel) reads a convolution weight up to five
// times per optimiser step -- parameter -> w_t, w_t -> adj(w_t), w_t -> pack, adj -> pack, parameter -> wsq -- one tap per block on the
// parameter side (4 of every 36 bytes of a fetched line used), and the EMA of the generator reads it once more in two ATen passes.  Here a
// workgroup owns a 32(k) x 32(n) tile with ALL taps: it reads the tile once in the parameter's memory order (runs of 32 * taps floats per
// n), updates the EMA copy at the same positions, keeps the tile in LDS and writes every derived form the item asks for.  The arithmetic
// of each form is the expression of the kernel that made it before (layout_tile, pack_weights_kernel, style_wsq_kernel<false>, the two
// foreach kernels of the EMA): bit-identical values.  Parameters that are no convolution weights ("flat" items) get the EMA only.
#include <algorithm>
#include <atomic>
#include <cstdint>

#include "common.h"

// Every product and sum below is rounded on its own unless it is written as fmaf: `scale * w - hi` must not become one fused operation
#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32;
constexpr int MAXRW = 16;        // weight items per launch
constexpr int MAXRF = 76;        // flat items per launch
constexpr int FLAT_BLOCK = 1024; // elements of a flat item per workgroup: one 16-byte access per lane

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct RefreshWeight {
    const float* src; float* ema; float* w_t; float* adj; float* adj2; uint4* pack_w; uint4* pack_adj; float* wsq;
    int N, K, taps, flip; float scale, decay, alpha; int first;
};
struct RefreshFlat { const float* src; float* ema; int count, first; float decay, alpha; };
struct RefreshArgs {
    RefreshWeight w[MAXRW];
    RefreshFlat f[MAXRF];
    int n_w, n_f, w_blocks;      // blocks [0, w_blocks) are weight tiles, the rest belong to the flat items
};
static_assert(sizeof(RefreshArgs) <= 4096, "the tables travel by value in the kernel arguments");

// ema <- decay * ema + alpha * p as torch._foreach_mul_(ema, decay) followed by torch._foreach_add_(ema, p, alpha=alpha) computes it: the
// product with decay is rounded to float (it is stored between the two ATen kernels); ATen's `a + alpha * b` is one fused multiply-add
// in this build of the foreach kernels (tests/test_weight_refresh_gpu.py compares the bits)
__device__ __forceinline__ float ema_value(float e, float p, float decay, float alpha) {
    return __fmaf_rn(alpha, p, __fmul_rn(e, decay));
}

// hi = bf16(v), lo = bf16(v - hi) of eight values: one 16-byte unit each (pack_weights_kernel, conv_bf16x3.hip)
__device__ __forceinline__ void split8(const float (&v)[8], uint4* hi, uint4* lo) {
    bf16x8 h, l;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const __bf16 hh = (__bf16)v[q];
        h[q] = hh;
        l[q] = (__bf16)(v[q] - (float)hh);
    }
    *hi = *reinterpret_cast<uint4*>(&h);
    *lo = *reinterpret_cast<uint4*>(&l);
}

// One 32(k) x 32(n) x TT tile of a parameter [N, K, TT].  The tile sits in LDS in the read order with the strides of TileLds<NKT, TT>
// (weight_layout.hip): odd strides along k and n, so that lanes running along either axis in the write phases hit distinct banks.
template <int TT>
__device__ __forceinline__ void refresh_tile(const RefreshWeight& W, int r, float* tile) {
    constexpr int MIDS = TT | 1, SLOWS = (TILE * MIDS) | 1;
    static_assert(MIDS == TT, "odd tap counts: a run of k * TT + t floats of one n lands in LDS as it is");
    constexpr int RUN = TILE * TT, TOTAL = TILE * RUN, PER = TOTAL / 256;
    const int K = W.K, N = W.N;
    const int kb = (K + TILE - 1) / TILE;
    const int k0 = (r % kb) * TILE, n0 = (r / kb) * TILE;
    const int ke = min(TILE, K - k0), ne = min(TILE, N - n0);
    const int run = ke * TT;                 // floats of one n of this tile that exist: contiguous in the parameter
    const int tid = threadIdx.x;
    // all loads of the lane first (36 in flight for 3x3 taps), as layout_tile does
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = tid + 256 * i, n = e / RUN, q = e % RUN;
        v[i] = (n < ne && q < run) ? W.src[((long long)(n0 + n) * K + k0) * TT + q] : 0.f;
    }
    if (W.ema) {
        // the EMA copy at the same positions: every load before the first store (the compiler cannot tell the addresses apart and would
        // otherwise wait for each load before it issues the next)
        float ev[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + 256 * i, n = e / RUN, q = e % RUN;
            ev[i] = (n < ne && q < run) ? W.ema[((long long)(n0 + n) * K + k0) * TT + q] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + 256 * i, n = e / RUN, q = e % RUN;
            if (n < ne && q < run) W.ema[((long long)(n0 + n) * K + k0) * TT + q] = ema_value(ev[i], v[i], W.decay, W.alpha);
        }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = tid + 256 * i;
        tile[(e / RUN) * SLOWS + e % RUN] = v[i];
    }
    __syncthreads();
    const float scale = W.scale;
    if (W.w_t || W.adj || W.adj2) {
        // w_t [TT, K, N] = scale * parameter, taps mirrored if flip (layout_tile's expression); lanes along n
        // adj(w_t) [TT, N, K]: adj[TT - 1 - t'][n][k] = w_t[t'][k][n]; lanes along k
        // adj(adj(w_t)) [TT, K, N]: the values of w_t once more, in a tensor of its own (the weights of a double-backward convolution)
#pragma unroll 4
        for (int e = tid; e < TOTAL; e += 256) {
            const int a = e % TILE, b = (e / TILE) % TILE, t = e / (TILE * TILE);
            const int td = W.flip ? TT - 1 - t : t;
            if ((W.w_t || W.adj2) && b < ke && a < ne) {          // a = n, b = k
                const float x = scale * tile[a * SLOWS + b * MIDS + t];
                const long long at = ((long long)td * K + k0 + b) * N + n0 + a;
                if (W.w_t) W.w_t[at] = x;
                if (W.adj2) W.adj2[at] = x;
            }
            if (W.adj && a < ke && b < ne)            // a = k, b = n
                W.adj[((long long)(TT - 1 - td) * N + n0 + b) * K + k0 + a] = scale * tile[b * SLOWS + a * MIDS + t];
        }
    }
    constexpr int UNITS = TT * (TILE / 8) * TILE;
    if (W.pack_w) {
        // units [t'][kg][n] of 8 consecutive k of w_t, zeros beyond K; lanes along n
        const int groups = (K + 7) / 8;
        uint4* lo = W.pack_w + (long long)TT * groups * N;
        for (int e = tid; e < UNITS; e += 256) {
            const int n = e % TILE, gl = (e / TILE) % (TILE / 8), t = e / (TILE * TILE / 8);
            const int g = k0 / 8 + gl;
            if (n >= ne || g >= groups) continue;
            float x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = (gl * 8 + q < ke) ? scale * tile[n * SLOWS + (gl * 8 + q) * MIDS + t] : 0.f;
            const long long u = ((long long)(W.flip ? TT - 1 - t : t) * groups + g) * N + n0 + n;
            split8(x, W.pack_w + u, lo + u);
        }
    }
    if (W.pack_adj) {
        // units [t''][ng][k] of 8 consecutive n of adj(w_t), zeros beyond N; lanes along k
        const int groups = (N + 7) / 8;
        uint4* lo = W.pack_adj + (long long)TT * groups * K;
        for (int e = tid; e < UNITS; e += 256) {
            const int k = e % TILE, gl = (e / TILE) % (TILE / 8), t = e / (TILE * TILE / 8);
            const int g = n0 / 8 + gl;
            if (k >= ke || g >= groups) continue;
            float x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = (gl * 8 + q < ne) ? scale * tile[(gl * 8 + q) * SLOWS + k * MIDS + t] : 0.f;
            const int td = W.flip ? TT - 1 - t : t;
            const long long u = ((long long)(TT - 1 - td) * groups + g) * K + k0 + k;
            split8(x, W.pack_adj + u, lo + u);
        }
    }
    if (W.wsq) {
        // wsq[n][k] = sum over ascending t of the RAW parameter squared, the fmaf chain of style_wsq_kernel<false>; lanes along k
        for (int e = tid; e < TILE * TILE; e += 256) {
            const int k = e % TILE, n = e / TILE;
            if (k >= ke || n >= ne) continue;
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                const float x = tile[n * SLOWS + k * MIDS + t];
                s = fmaf(x, x, s);
            }
            W.wsq[(long long)(n0 + n) * K + k0 + k] = s;
        }
    }
}

__device__ __forceinline__ void refresh_flat(const RefreshFlat& F, int r) {
    const long long base = (long long)r * FLAT_BLOCK;
    const bool aligned = ((reinterpret_cast<uintptr_t>(F.src) | reinterpret_cast<uintptr_t>(F.ema)) & 15) == 0;
    if (aligned && base + FLAT_BLOCK <= F.count) {
        const long long at = base + 4 * threadIdx.x;
        const float4 p = *reinterpret_cast<const float4*>(F.src + at);
        float4 e = *reinterpret_cast<float4*>(F.ema + at);
        e.x = ema_value(e.x, p.x, F.decay, F.alpha); e.y = ema_value(e.y, p.y, F.decay, F.alpha);
        e.z = ema_value(e.z, p.z, F.decay, F.alpha); e.w = ema_value(e.w, p.w, F.decay, F.alpha);
        *reinterpret_cast<float4*>(F.ema + at) = e;
        return;
    }
    // the tail of an item, or an item that is not 16-byte aligned
    float p[FLAT_BLOCK / 256], e[FLAT_BLOCK / 256];
#pragma unroll
    for (int i = 0; i < FLAT_BLOCK / 256; ++i) {
        const long long at = base + 256 * i + threadIdx.x;
        p[i] = at < F.count ? F.src[at] : 0.f;
        e[i] = at < F.count ? F.ema[at] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < FLAT_BLOCK / 256; ++i) {
        const long long at = base + 256 * i + threadIdx.x;
        if (at < F.count) F.ema[at] = ema_value(e[i], p[i], F.decay, F.alpha);
    }
}

// (the name files the kernel under bench.py's `weights` family)
__global__ __launch_bounds__(256) void weight_layout_refresh_kernel(RefreshArgs a) {
    __shared__ float tile[TILE * ((TILE * 9) | 1)];
    const int b = blockIdx.x;
    if (b < a.w_blocks) {
        int gi = 0;
#pragma unroll 1
        for (int i = 1; i < a.n_w; ++i) gi = (b >= a.w[i].first) ? i : gi;
        const RefreshWeight& W = a.w[gi];
        if (W.taps == 9) refresh_tile<9>(W, b - W.first, tile);
        else             refresh_tile<1>(W, b - W.first, tile);
        return;
    }
    int gi = 0;
#pragma unroll 1
    for (int i = 1; i < a.n_f; ++i) gi = (b >= a.f[i].first) ? i : gi;
    refresh_flat(a.f[gi], b - a.f[gi].first);
}

// kernel launches issued by the entry in this process (gc_weight_refresh_launches): how a test SEES the launches of a refresh
std::atomic<long long> launches{0};

}  // namespace

extern "C" int gc_weight_refresh_grouped_f32(const gc_wrefresh_item* items, int n_items, gc_stream_t stream) {
    const char* what = "gc_weight_refresh_grouped_f32";
    if (n_items < 0 || (n_items > 0 && !items)) return gc::fail(GC_ERR_BAD_ARG, "%s: bad item table", what);
    // everything is checked before the first launch
    int n_w = 0, n_f = 0;
    for (int i = 0; i < n_items; ++i) {
        const gc_wrefresh_item& it = items[i];
        if (!it.src) return gc::fail(GC_ERR_BAD_ARG, "%s: item %d has no source", what, i);
        if (it.taps == 0) {          // flat: the EMA only
            if (!it.ema || it.count <= 0) return gc::fail(GC_ERR_BAD_ARG, "%s: flat item %d needs an EMA destination and a positive count", what, i);
            if (it.w_t || it.adj || it.adj2 || it.pack_w || it.pack_adj || it.wsq) return gc::fail(GC_ERR_BAD_ARG, "%s: flat item %d asks for a weight form", what, i);
            if (it.count > 2147483647LL - FLAT_BLOCK) return gc::fail(GC_ERR_UNSUPPORTED, "%s: flat item %d has %lld elements", what, i, (long long)it.count);
            ++n_f;
            continue;
        }
        if (it.n <= 0 || it.k <= 0 || it.taps < 0) return gc::fail(GC_ERR_BAD_ARG, "%s: item %d has a non-positive extent", what, i);
        if (it.taps != 1 && it.taps != 9) return gc::fail(GC_ERR_UNSUPPORTED, "%s: item %d has %d taps; 1 and 9 are built", what, i, it.taps);
        if ((long long)it.n * it.k * it.taps > 2147483647LL) return gc::fail(GC_ERR_UNSUPPORTED, "%s: item %d is too large", what, i);
        if ((reinterpret_cast<uintptr_t>(it.pack_w) | reinterpret_cast<uintptr_t>(it.pack_adj)) & 15)
            return gc::fail(GC_ERR_BAD_ARG, "%s: item %d: packs must be 16-byte aligned", what, i);
        ++n_w;
    }
    const int n_launches = std::max(gc::ceil_div(n_w, MAXRW), gc::ceil_div(n_f, MAXRF));
    if (n_launches == 0) return GC_OK;
    int iw = 0, jf = 0;          // next unread item of each kind
    for (int l = 0; l < n_launches; ++l) {
        RefreshArgs a;
        a.n_w = a.n_f = 0;
        long long blocks = 0;
        for (; iw < n_items && a.n_w < MAXRW; ++iw) {
            const gc_wrefresh_item& it = items[iw];
            if (it.taps == 0) continue;
            RefreshWeight& W = a.w[a.n_w++];
            W.src = it.src; W.ema = it.ema; W.w_t = it.w_t; W.adj = it.adj; W.adj2 = it.adj2;
            W.pack_w = static_cast<uint4*>(it.pack_w); W.pack_adj = static_cast<uint4*>(it.pack_adj); W.wsq = it.wsq;
            W.N = it.n; W.K = it.k; W.taps = it.taps; W.flip = it.flip_taps ? 1 : 0;
            W.scale = it.scale; W.decay = it.decay; W.alpha = it.alpha; W.first = (int)blocks;
            blocks += (long long)gc::ceil_div(it.k, TILE) * gc::ceil_div(it.n, TILE);
        }
        a.w_blocks = (int)blocks;
        for (; jf < n_items && a.n_f < MAXRF; ++jf) {
            const gc_wrefresh_item& it = items[jf];
            if (it.taps != 0) continue;
            a.f[a.n_f++] = RefreshFlat{it.src, it.ema, (int)it.count, (int)blocks, it.decay, it.alpha};
            blocks += gc::ceil_div64(it.count, FLAT_BLOCK);
        }
        if (blocks > 2147483647LL) return gc::fail(GC_ERR_UNSUPPORTED, "%s: too many blocks", what);
        if (!blocks) continue;
        hipLaunchKernelGGL(weight_layout_refresh_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        ++launches;
    }
    return gc::check_launch(what);
}

extern "C" int64_t gc_weight_refresh_launches(void) { return launches.load(); }

extern "C" size_t gc_weight_refresh_item_bytes(void) { return sizeof(gc_wrefresh_item); }
