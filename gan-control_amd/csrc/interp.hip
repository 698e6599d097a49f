// The two blends of group interpolation (reference: evaluation/inference_class.py:125-185), each over everything that is known up front:
//   latent_interp_kernel   every frame of one interpolation segment, both films: out [2, frames, batch, latent] from the rows `fixed`, `from`
//                          and `to`.  One workgroup per row b: the three row sums (x.x, y.y, x.y) of each slice S | G | E are taken ONCE
//                          (slerp only), the 3 x frames coefficient pairs go to LDS, and every thread then keeps its columns of the three rows
//                          in registers and walks the frames: one blend and two stores per (column, frame).
//   noise_blend_kernel     out[m] = wa * a[m] + wb * b[m] for a whole LIST of noise maps in one launch: a workgroup per 4096 elements of a
//                          map, 16-byte accesses where the three pointers of the map allow, 4-byte ones elsewhere and for the last count % 4.
// Both are bandwidth- and latency-bound; nothing here is for the matrix pipes.  Pointers, weights and extents travel BY VALUE in the kernel
// arguments (at most 64 frames, 32 maps): nothing is uploaded.
//
// Rounding.  A blend is fl(fl(ca * x) + fl(cb * y)): two rounded products and a rounded sum, what ATen computes for a * x + b * y with float32
// scalars.  hipcc contracts a * x + b * y into an FMA by default -- also through __fmul_rn / __fadd_rn, which are plain operators compiled
// under the header's own contraction mode (v_pk_fma_f32 in the listing) -- so blend() spells the expression under `fp contract(off)`.
// The slerp coefficients sin(w omega) / sin(omega), omega = acos(x.y / (|x| |y|)), are scalars per (row, slice, frame): 3 x frames of them per
// row, off the bandwidth path.  They are computed in float64 from float64 row sums (a product of two floats is exact there) and rounded to
// float32 once, so what the result owes the kernel is the three roundings of the blend alone.  The sums are wave shuffles and a four-term
// LDS sum in an order fixed by the extents: no atomics, the same bits every time.  Nothing is clamped: parallel slices are as undefined as
// in the reference.
#include <cstdint>

#include "common.h"

namespace {

constexpr int MAX_FRAMES = 64, MAX_MAPS = 32, NT = 256;
constexpr int VEC_PER_THREAD = 4, CHUNK = NT * 4 * VEC_PER_THREAD;          // elements of a map per workgroup of the noise kernel

struct Weights { float a[MAX_FRAMES], b[MAX_FRAMES]; };

__device__ __forceinline__ float blend(float ca, float x, float cb, float y) {
#pragma clang fp contract(off)
    const float p = ca * x, q = cb * y;
    return p + q;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// grid: batch workgroups.  Slice s of a row: columns [edge[s], edge[s + 1]) with edge = {0, lo, hi, latent}; s == 1 is the group.
__global__ __launch_bounds__(NT) void latent_interp_kernel(const float* __restrict__ fixed, long long fixed_stride, const float* __restrict__ from,
                                                           long long from_stride, const float* __restrict__ to, long long to_stride, int batch,
                                                           int latent, int lo, int hi, Weights w, int frames, int slerp, float* __restrict__ out) {
    __shared__ double part[NT / 64][9];
    __shared__ float ca[3][MAX_FRAMES], cb[3][MAX_FRAMES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* x = from + (long long)b * from_stride;
    const float* y = to + (long long)b * to_stride;
    const float* z = fixed + (long long)b * fixed_stride;
    const int edge[4] = {0, lo, hi, latent};
    if (slerp) {
        double acc[9];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            double xx = 0.0, yy = 0.0, xy = 0.0;
            for (int i = edge[s] + tid; i < edge[s + 1]; i += NT) {          // an empty slice: no trip, nothing is read
                const double xv = (double)x[i], yv = (double)y[i];
                xx += xv * xv; yy += yv * yv; xy += xv * yv;
            }
            acc[3 * s] = xx; acc[3 * s + 1] = yy; acc[3 * s + 2] = xy;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double v = wave_sum(acc[k]);
            if ((tid & 63) == 0) part[tid >> 6][k] = v;
        }
        __syncthreads();
        for (int j = tid; j < 3 * frames; j += NT) {
            const int s = j / frames, f = j - s * frames;
            if (s == 0 ? lo == 0 : s == 2 && hi == latent) continue;        // no 0 / 0 is formed for a slice that does not exist
            const double xx = (part[0][3 * s] + part[1][3 * s]) + (part[2][3 * s] + part[3][3 * s]);
            const double yy = (part[0][3 * s + 1] + part[1][3 * s + 1]) + (part[2][3 * s + 1] + part[3][3 * s + 1]);
            const double xy = (part[0][3 * s + 2] + part[1][3 * s + 2]) + (part[2][3 * s + 2] + part[3][3 * s + 2]);
            const double omega = acos(xy / (sqrt(xx) * sqrt(yy))), so = sin(omega);
            ca[s][f] = (float)(sin((double)w.a[f] * omega) / so);
            cb[s][f] = (float)(sin((double)w.b[f] * omega) / so);
        }
    } else {
        for (int j = tid; j < 3 * frames; j += NT) {
            const int s = j / frames, f = j - s * frames;
            ca[s][f] = w.a[f];
            cb[s][f] = w.b[f];
        }
    }
    __syncthreads();
    const long long film = (long long)frames * batch * latent;          // out[1] - out[0]
    for (int i = tid; i < latent; i += NT) {
        const int s = (i >= lo) + (i >= hi);
        const float xv = x[i], yv = y[i], zv = z[i];
        float* dst = out + (long long)b * latent + i;
        for (int f = 0; f < frames; ++f) {
            const float v = blend(ca[s][f], xv, cb[s][f], yv);
            dst[0] = s == 1 ? zv : v;             // the group is frozen
            dst[film] = s == 1 ? v : zv;          // only the group moves
            dst += (long long)batch * latent;
        }
    }
}

struct NoiseTable {
    const float* a[MAX_MAPS];
    const float* b[MAX_MAPS];
    float* out[MAX_MAPS];
    long long count[MAX_MAPS];
    int blk0[MAX_MAPS + 1];          // first workgroup of the map
    int n;
};

__global__ __launch_bounds__(NT) void noise_blend_kernel(NoiseTable t, float wa, float wb) {
    int m = 0;
    while (m + 1 < t.n && (int)blockIdx.x >= t.blk0[m + 1]) ++m;
    const float* __restrict__ a = t.a[m];
    const float* __restrict__ b = t.b[m];
    float* __restrict__ o = t.out[m];
    const long long count = t.count[m], begin = (long long)((int)blockIdx.x - t.blk0[m]) * CHUNK;
    const long long end = begin + CHUNK < count ? begin + CHUNK : count;
    const bool vec = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(o)) & 15) == 0;
    long long tail = begin;          // first element the 4-byte loop takes
    if (vec) {                       // (begin is a multiple of 4: words stay 16-byte aligned)
        const long long words = (end - begin) >> 2;
        gc::f32x4_t va[VEC_PER_THREAD], vb[VEC_PER_THREAD];
#pragma unroll
        for (int u = 0; u < VEC_PER_THREAD; ++u) {
            const long long wd = threadIdx.x + u * NT;
            if (wd < words) {
                va[u] = *reinterpret_cast<const gc::f32x4_t*>(a + begin + 4 * wd);
                vb[u] = *reinterpret_cast<const gc::f32x4_t*>(b + begin + 4 * wd);
            }
        }
#pragma unroll
        for (int u = 0; u < VEC_PER_THREAD; ++u) {
            const long long wd = threadIdx.x + u * NT;
            if (wd < words) {
                gc::f32x4_t r;
                r.x = blend(wa, va[u].x, wb, vb[u].x); r.y = blend(wa, va[u].y, wb, vb[u].y);
                r.z = blend(wa, va[u].z, wb, vb[u].z); r.w = blend(wa, va[u].w, wb, vb[u].w);
                *reinterpret_cast<gc::f32x4_t*>(o + begin + 4 * wd) = r;
            }
        }
        tail = begin + 4 * words;
    }
    for (long long i = tail + threadIdx.x; i < end; i += NT) o[i] = blend(wa, a[i], wb, b[i]);
}

inline bool overlap(const float* p, long long pn, const float* q, long long qn) {
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(p), q0 = reinterpret_cast<uintptr_t>(q);
    return p0 < q0 + 4ull * (uintptr_t)qn && q0 < p0 + 4ull * (uintptr_t)pn;
}

}  // namespace

extern "C" int gc_latent_interp_f32(const float* fixed, int64_t fixed_stride, const float* from, int64_t from_stride, const float* to,
                                    int64_t to_stride, int batch, int latent, int lo, int hi, const float* wa, const float* wb, int frames,
                                    int mode, float* out, gc_stream_t stream) {
    const char* what = "gc_latent_interp_f32";
    if (!fixed || !from || !to || !wa || !wb || !out) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (batch < 1 || latent < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: extents batch %d, latent %d: at least 1 each", what, batch, latent);
    if (lo < 0 || lo >= hi || hi > latent) return gc::fail(GC_ERR_BAD_ARG, "%s: group [%d, %d) of a latent of %d: 0 <= lo < hi <= latent", what, lo, hi, latent);
    if (frames < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: %d frames: at least 1", what, frames);
    if (frames > MAX_FRAMES) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d frames, at most %d", what, frames, MAX_FRAMES);
    if (mode != GC_INTERP_LINEAR && mode != GC_INTERP_SLERP && mode != GC_INTERP_SQRT) return gc::fail(GC_ERR_BAD_ARG, "%s: unknown mode %d", what, mode);
    const int64_t strides[3] = {fixed_stride, from_stride, to_stride};
    for (int k = 0; k < 3; ++k)          // 0: one row read for every b (an expanded row); anything else holds a whole row
        if (strides[k] < 0 || (strides[k] > 0 && strides[k] < latent))
            return gc::fail(GC_ERR_BAD_ARG, "%s: row stride %lld: 0 or at least the row (%d); a negative stride is not read", what, (long long)strides[k], latent);
    if (2LL * frames * batch * latent > INT32_MAX) return gc::fail(GC_ERR_UNSUPPORTED, "%s: more than 2^31 output elements", what);
    Weights w;
    for (int f = 0; f < MAX_FRAMES; ++f) { w.a[f] = f < frames ? wa[f] : 0.f; w.b[f] = f < frames ? wb[f] : 0.f; }
    hipLaunchKernelGGL(latent_interp_kernel, dim3(batch), dim3(NT), 0, (hipStream_t)stream, fixed, (long long)fixed_stride, from, (long long)from_stride, to,
                       (long long)to_stride, batch, latent, lo, hi, w, frames, mode == GC_INTERP_SLERP ? 1 : 0, out);
    return gc::check_launch(what);
}

extern "C" int gc_noise_blend_f32(const float* const* a, const float* const* b, float* const* out, const int64_t* counts, int n, float wa, float wb,
                                  gc_stream_t stream) {
    const char* what = "gc_noise_blend_f32";
    if (!a || !b || !out || !counts) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (n < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: empty list", what);
    if (n > MAX_MAPS) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d maps, at most %d", what, n, MAX_MAPS);
    NoiseTable t;
    long long blocks = 0;
    for (int m = 0; m < n; ++m) {
        if (!a[m] || !b[m] || !out[m]) return gc::fail(GC_ERR_BAD_ARG, "%s: map %d has a null pointer", what, m);
        if (counts[m] < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: map %d has %lld elements: at least 1", what, m, (long long)counts[m]);
        t.a[m] = a[m]; t.b[m] = b[m]; t.out[m] = out[m]; t.count[m] = counts[m];
        t.blk0[m] = (int)blocks;
        blocks += (counts[m] + CHUNK - 1) / CHUNK;
        if (blocks > INT32_MAX) return gc::fail(GC_ERR_UNSUPPORTED, "%s: more than 2^31 workgroups", what);
    }
    for (int m = n; m < MAX_MAPS; ++m) { t.a[m] = t.b[m] = nullptr; t.out[m] = nullptr; t.count[m] = 0; t.blk0[m] = (int)blocks; }
    t.blk0[n] = t.blk0[MAX_MAPS] = (int)blocks;
    t.n = n;
    for (int m = 0; m < n; ++m)
        for (int k = 0; k < n; ++k) {
            if (overlap(out[m], counts[m], a[k], counts[k]) || overlap(out[m], counts[m], b[k], counts[k]))
                return gc::fail(GC_ERR_BAD_ARG, "%s: output %d overlaps input %d", what, m, k);
            if (k != m && overlap(out[m], counts[m], out[k], counts[k])) return gc::fail(GC_ERR_BAD_ARG, "%s: outputs %d and %d overlap", what, m, k);
        }
    hipLaunchKernelGGL(noise_blend_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, t, wa, wb);
    return gc::check_launch(what);
}
