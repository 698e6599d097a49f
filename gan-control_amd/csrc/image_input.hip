// The real-image input path after the decode: uint8 [B, H, W, 3] (what PIL hands over) -> float32 [B, 3, size, size] in [-1, 1], with the
// 8-bit bilinear resize, the per-sample crop and the horizontal flip of the reference's transform chains (ffhq_dataset.py:56-64,
// afhq_dataset.py:50-59) -- bit for bit what Resize / RandomResizedCrop / RandomHorizontalFlip / ToTensor / Normalize give on the host.
//   image_u8_to_f32_kernel     y[b,c,i,j] = lut[x[b,i,jj,c]], jj = flip[b] ? W-1-j : j                                 (HBM stream: 3 B in, 12 B out per pixel)
//   image_resample_h_kernel    one horizontal pass of the fixed-point resample, uint8 -> uint8 (its rows may start at a per-sample offset)
//   image_resample_v_kernel    one vertical pass; <true> ends in the table lookup, the flip and the planar float store, <false> in uint8
// Arithmetic of a pass: acc = 2^21 + sum_k pixel[first + k] * coeff[k] in int32 (255 * 2^22 fits), out = clamp(acc >> 22, 0, 255); the
// coefficient tables come from the host (datasets/image_ops.py: resample_tables), as does the 256-entry byte -> float table, so no float
// arithmetic happens here at all.
// Memory access: one lane owns 4 consecutive pixels of a row = 12 interleaved bytes in, one 16-byte store to each of the three planes out,
// so that every load and every store instruction of a wave covers one contiguous run (768 B / 1 KiB).  The bytes are fetched as ALIGNED
// dwords -- the row may start at any byte -- and realigned with a funnel shift; only dwords that hold at least one wanted byte are
// loaded, so nothing past the page of the last logical byte is touched.  A flipped sample reads the mirrored group and reverses it in
// registers: same loads, same stores.  Byte loads / scalar stores serve only the ragged last group of a row.
// (16 pixels per lane -- three 16-byte loads, four 16-byte stores per plane 64 B apart across lanes -- measured 2.6 x SLOWER on the
// [4, 1024, 1024, 3] batch, 34.9 vs 13.2 us: profiles/image_input_r08.md.  The stores are 4/5 of the traffic and want to be contiguous.)
#include <algorithm>

#include "common.h"

namespace {

typedef uint32_t u32;
typedef u32 u32x2u_t __attribute__((ext_vector_type(2), aligned(4)));           // gfx9 takes multi-dword accesses at 4-byte alignment

constexpr int HALF = 1 << 21, SHIFT = 22;           // the rounding term and the scale of the fixed-point coefficients

// ND dwords starting at byte address a (any alignment), in memory order
template <int ND>
__device__ __forceinline__ void load_bytes(const uint8_t* a, u32 (&r)[ND]) {
    const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(a) & 3);
    const u32* p = reinterpret_cast<const u32*>(a - sh);
    static_assert(ND == 3, "4 pixels");
    u32 w[ND + 1];
    const u32x2u_t v = *reinterpret_cast<const u32x2u_t*>(p);          // 12 bytes as 8 + 4 (a 3-vector type is loaded and stored as 4 elements)
    w[0] = v.x; w[1] = v.y; w[2] = p[2];
    w[ND] = sh ? p[ND] : 0u;                        // with sh == 0 dword ND holds none of the wanted bytes: not read
#pragma unroll
    for (int d = 0; d < ND; ++d) r[d] = __funnelshift_r(w[d], w[d + 1], sh * 8);
}

// the ragged last group of a row: n < PX pixels, byte by byte, already in OUTPUT order (reversed when the sample is flipped)
template <int ND>
__device__ __forceinline__ void load_tail(const uint8_t* a, int n, bool reversed, u32 (&r)[ND]) {
#pragma unroll
    for (int d = 0; d < ND; ++d) r[d] = 0u;
#pragma unroll
    for (int q = 0; q < ND * 4 / 3; ++q)
        if (q < n) {
            const uint8_t* px = a + 3 * (reversed ? n - 1 - q : q);
#pragma unroll
            for (int c = 0; c < 3; ++c) r[(3 * q + c) >> 2] |= (u32)px[c] << (((3 * q + c) & 3) * 8);
        }
}

template <int ND>
__device__ __forceinline__ u32 byte_of(const u32 (&r)[ND], int k) { return (r[k >> 2] >> ((k & 3) * 8)) & 255u; }

struct CvtArgs {
    const uint8_t* x; long long row_stride, sample_stride;
    const float* lut; const int* flip; float* y;
    int h, w, groups;            // groups of 4 pixels per row
    int vst;                     // rows of y are 16-byte aligned: float4 stores
};

// grid: (row x group, batch)
__global__ __launch_bounds__(256) void image_u8_to_f32_kernel(CvtArgs a) {
    constexpr int PX = 4, ND = 3;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.h * a.groups) return;
    const int i = (int)(idx / a.groups), g = (int)(idx - (long long)i * a.groups), b = blockIdx.y;
    const int j0 = g * PX, n = min(PX, a.w - j0);
    const bool fl = a.flip[b] != 0, full = n == PX;
    const uint8_t* src = a.x + (long long)b * a.sample_stride + (long long)i * a.row_stride + 3LL * (fl ? a.w - j0 - n : j0);
    u32 r[ND];
    if (full) load_bytes<ND>(src, r);
    else      load_tail<ND>(src, n, fl, r);
    const bool rev = fl && full;                    // a tail arrives in output order
    const size_t plane = (size_t)a.h * a.w;
    float* dst = a.y + (size_t)b * 3 * plane + (size_t)i * a.w + j0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float u[PX], v[PX];
#pragma unroll
        for (int q = 0; q < PX; ++q) u[q] = a.lut[byte_of<ND>(r, 3 * q + c)];        // (a tail's unused slots hold byte 0: a valid index)
#pragma unroll
        for (int q = 0; q < PX; ++q) v[q] = rev ? u[PX - 1 - q] : u[q];
        float* d = dst + c * plane;
        if (full && a.vst) {
#pragma unroll
            for (int t = 0; t < PX / 4; ++t) gc::stream_store4(d + 4 * t, v[4 * t], v[4 * t + 1], v[4 * t + 2], v[4 * t + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < PX; ++q)
                if (q < n) d[q] = v[q];
        }
    }
}

struct RsArgs {
    const uint8_t* x; long long row_stride, sample_stride; int in_h, in_w;
    const int* coeff; const int* bounds; int kmax, table_stride;         // table_stride: 0 = one table for every sample, 1 = one per sample
    const int* other;                                                    // [S, 2] (offset, count) along the axis that is NOT resampled, or null
    const float* lut; const int* flip; float* yf; uint8_t* yu;
    int out_h, out_w, groups;
    int vst;                     // the output rows allow vector stores (16-byte aligned floats / 4-byte aligned bytes)
};

__device__ __forceinline__ u32 to_byte(int acc) { return (u32)min(max(acc >> SHIFT, 0), 255); }

// 12 packed bytes (4 pixels) to y; n pixels are real
__device__ __forceinline__ void store_u8_group(uint8_t* d, const u32 (&o)[3], int n, bool vec) {
    if (vec && n == 4) {
        *reinterpret_cast<u32x2u_t*>(d) = u32x2u_t{o[0], o[1]};
        reinterpret_cast<u32*>(d)[2] = o[2];
        return;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k)
        if (k < 3 * n) d[k] = (uint8_t)byte_of<3>(o, k);
}

// the (offset, count) of sample b along the other axis, clamped to the input and the output extents
__device__ __forceinline__ void other_window(const RsArgs& a, int b, int in_extent, int out_extent, int& off, int& cnt) {
    off = 0; cnt = min(out_extent, in_extent);
    if (a.other) {
        off = max(a.other[(size_t)b * a.table_stride * 2], 0);
        cnt = min(min(a.other[(size_t)b * a.table_stride * 2 + 1], out_extent), in_extent - off);
    }
}

// Horizontal pass.  grid: (output row x group of 4 output pixels, batch); y dense uint8 [B, out_h, out_w, 3]; row r of y comes from row
// offset + r of x and exists for r < count.
__global__ __launch_bounds__(256) void image_resample_h_kernel(RsArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.out_h * a.groups) return;
    const int r = (int)(idx / a.groups), g = (int)(idx - (long long)r * a.groups), b = blockIdx.y;
    int off, rows;
    other_window(a, b, a.in_h, a.out_h, off, rows);
    if (r >= rows) return;
    const int j0 = g * 4, n = min(4, a.out_w - j0);
    const uint8_t* row = a.x + (long long)b * a.sample_stride + (long long)(off + r) * a.row_stride;
    const size_t tab = (size_t)b * a.table_stride * a.out_w + j0;
    u32 o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q >= n) break;
        const int* bd = a.bounds + (tab + q) * 2;
        const int x0 = min(max(bd[0], 0), a.in_w);
        const int cnt = max(min(min(bd[1], a.kmax), a.in_w - x0), 0);            // a table slot past the count is never read
        const int* cf = a.coeff + (tab + q) * a.kmax;
        int acc0 = HALF, acc1 = HALF, acc2 = HALF;
        if (cnt > 0) {
            // a 64-bit window of aligned dwords slides over the 3 * cnt bytes
            const uint8_t* pa = row + 3LL * x0;
            const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(pa) & 3);
            const u32* p = reinterpret_cast<const u32*>(pa - sh);
            const int last = (int)(sh + 3 * cnt - 1) >> 2;                        // the last dword that holds a wanted byte
            u32 lo = p[0], hi = last >= 1 ? p[1] : 0u;
            int at = 1;
            unsigned bit = sh * 8;
            for (int k = 0; k < cnt; ++k) {
                const u32 px = (u32)((((unsigned long long)hi << 32) | lo) >> bit);
                const int c = cf[k];
                acc0 += (int)(px & 255u) * c; acc1 += (int)((px >> 8) & 255u) * c; acc2 += (int)((px >> 16) & 255u) * c;
                bit += 24;
                if (bit >= 32) { bit -= 32; lo = hi; ++at; hi = at <= last ? p[at] : 0u; }
            }
        }
        o[(3 * q) >> 2] |= to_byte(acc0) << (((3 * q) & 3) * 8);
        o[(3 * q + 1) >> 2] |= to_byte(acc1) << (((3 * q + 1) & 3) * 8);
        o[(3 * q + 2) >> 2] |= to_byte(acc2) << (((3 * q + 2) & 3) * 8);
    }
    store_u8_group(a.yu + (((size_t)b * a.out_h + r) * a.out_w + j0) * 3, o, n, a.vst != 0);
}

// Vertical pass.  grid: (group of 4 output pixels, output row, batch): the coefficients of a row are the same for the whole workgroup.
// Column q of y comes from column offset + q of x.  FUSED: y float32 [B, 3, out_h, out_w] = lut[resampled byte], mirrored where flip[b];
// otherwise y dense uint8 [B, out_h, out_w, 3], columns < count.
template <bool FUSED>
__global__ __launch_bounds__(64) void image_resample_v_kernel(RsArgs a) {
    const int g = blockIdx.x * 64 + threadIdx.x, yy = blockIdx.y, b = blockIdx.z;
    if (g >= a.groups) return;
    int off, cols;
    other_window(a, b, a.in_w, a.out_w, off, cols);
    const int j0 = g * 4, n = min(4, cols - j0);
    if (n <= 0) return;
    const size_t tab = (size_t)b * a.table_stride * a.out_h + yy;
    const int y0 = min(max(a.bounds[tab * 2], 0), a.in_h);
    const int cnt = max(min(min(a.bounds[tab * 2 + 1], a.kmax), a.in_h - y0), 0);
    const int* cf = a.coeff + tab * a.kmax;
    const bool fl = FUSED && a.flip[b] != 0, full = n == 4;
    const uint8_t* src = a.x + (long long)b * a.sample_stride + (long long)y0 * a.row_stride + 3LL * (off + (fl ? cols - j0 - n : j0));
    int acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = HALF;
    for (int k = 0; k < cnt; ++k) {
        u32 r[3];
        if (full) load_bytes<3>(src + (long long)k * a.row_stride, r);
        else      load_tail<3>(src + (long long)k * a.row_stride, n, fl, r);
        const int c = cf[k];
#pragma unroll
        for (int e = 0; e < 12; ++e) acc[e] += (int)byte_of<3>(r, e) * c;
    }
    if (FUSED) {
        const bool rev = fl && full;
        const size_t plane = (size_t)a.out_h * a.out_w;
        float* dst = a.yf + (size_t)b * 3 * plane + (size_t)yy * a.out_w + j0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float u[4], v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) u[q] = a.lut[to_byte(acc[3 * q + c])];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = rev ? u[3 - q] : u[q];
            float* d = dst + c * plane;
            if (full && a.vst) gc::stream_store4(d, v[0], v[1], v[2], v[3]);
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < n) d[q] = v[q];
            }
        }
    } else {
        u32 o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e >> 2] |= to_byte(acc[e]) << ((e & 3) * 8);
        store_u8_group(a.yu + (((size_t)b * a.out_h + yy) * a.out_w + j0) * 3, o, n, a.vst != 0);
    }
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// Everything the two resample entries check before a launch; the tables are checked through their HOST copies.
int check_resample(const char* what, const void* x, int64_t row_stride, int64_t sample_stride, int in_h, int in_w, const void* y, int batch,
                   int out_h, int out_w, int axis, const void* coeff, const void* bounds, const int32_t* bounds_host, int kmax, int table_stride,
                   const void* other, const int32_t* other_host, bool fused) {
    if (!x || !y || !coeff || !bounds || !bounds_host) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if ((other != nullptr) != (other_host != nullptr)) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer (other and other_host go together)", what);
    if (batch <= 0 || batch > 65535 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || (axis != 0 && axis != 1) || (axis == 1 && out_h > 65535))
        return gc::fail(GC_ERR_BAD_ARG, "%s: batch %d, %d x %d -> %d x %d, axis %d", what, batch, in_h, in_w, out_h, out_w, axis);
    if (kmax < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: kmax %d < 1", what, kmax);
    if (table_stride != 0 && table_stride != 1) return gc::fail(GC_ERR_BAD_ARG, "%s: table_stride %d (0: shared tables, 1: one per sample)", what, table_stride);
    if (row_stride < 3LL * in_w || sample_stride < 0) return gc::fail(GC_ERR_BAD_ARG, "%s: row stride %lld < %d bytes or negative sample stride", what, (long long)row_stride, 3 * in_w);
    const int tables = table_stride ? batch : 1, out = axis == 0 ? out_w : out_h, extent = axis == 0 ? in_w : in_h;
    for (int s = 0; s < tables; ++s)
        for (int o = 0; o < out; ++o) {
            const int first = bounds_host[((size_t)s * out + o) * 2], count = bounds_host[((size_t)s * out + o) * 2 + 1];
            if (first < 0 || count < 1 || count > kmax || first > extent - count)
                return gc::fail(GC_ERR_BAD_ARG, "%s: bounds[%d][%d] = (%d, %d) reads outside [0, %d) or holds more than kmax = %d taps", what, s, o, first, count, extent, kmax);
        }
    if (other_host) {
        const int o_in = axis == 0 ? in_h : in_w, o_out = axis == 0 ? out_h : out_w;
        for (int s = 0; s < tables; ++s) {
            const int first = other_host[s * 2], count = other_host[s * 2 + 1];
            if (first < 0 || count < 1 || count > o_out || first > o_in - count || (fused && count != o_out))
                return gc::fail(GC_ERR_BAD_ARG, "%s: other[%d] = (%d, %d) outside [0, %d), or not the %d of the output", what, s, first, count, o_in, o_out);
        }
    } else if ((axis == 0 ? in_h : in_w) < (axis == 0 ? out_h : out_w))
        return gc::fail(GC_ERR_BAD_ARG, "%s: the input has fewer %s than the output", what, axis == 0 ? "rows" : "columns");
    return GC_OK;
}

}  // namespace

extern "C" int gc_image_u8_to_f32(const uint8_t* x, int64_t row_stride, int64_t sample_stride, const float* lut, const int32_t* flip, float* y,
                                  int batch, int h, int w, gc_stream_t stream) {
    if (!x || !lut || !flip || !y) return gc::fail(GC_ERR_BAD_ARG, "gc_image_u8_to_f32: null pointer");
    if (batch <= 0 || batch > 65535 || h <= 0 || w <= 0) return gc::fail(GC_ERR_BAD_ARG, "gc_image_u8_to_f32: batch %d, %d x %d", batch, h, w);
    if (row_stride < 3LL * w || sample_stride < 0)
        return gc::fail(GC_ERR_BAD_ARG, "gc_image_u8_to_f32: row stride %lld < %d bytes or negative sample stride", (long long)row_stride, 3 * w);
    CvtArgs a{x, row_stride, sample_stride, lut, flip, y, h, w, 0, aligned_to(y, 16) && w % 4 == 0};
    hipStream_t s = (hipStream_t)stream;
    a.groups = (w + 3) / 4;
    const dim3 grid((unsigned)(((long long)h * a.groups + 255) / 256), batch);
    hipLaunchKernelGGL(image_u8_to_f32_kernel, grid, dim3(256), 0, s, a);
    return gc::check_launch("gc_image_u8_to_f32");
}

extern "C" int gc_image_resample_u8(const uint8_t* x, int64_t row_stride, int64_t sample_stride, int in_h, int in_w, uint8_t* y, int batch,
                                    int out_h, int out_w, int axis, const int32_t* coeff, const int32_t* bounds, const int32_t* bounds_host,
                                    int kmax, int table_stride, const int32_t* other, const int32_t* other_host, gc_stream_t stream) {
    int rc = check_resample("gc_image_resample_u8", x, row_stride, sample_stride, in_h, in_w, y, batch, out_h, out_w, axis, coeff, bounds, bounds_host,
                            kmax, table_stride, other, other_host, false);
    if (rc) return rc;
    RsArgs a{x, row_stride, sample_stride, in_h, in_w, coeff, bounds, kmax, table_stride, other, nullptr, nullptr, nullptr, y,
             out_h, out_w, (out_w + 3) / 4, aligned_to(y, 4) && out_w % 4 == 0};
    hipStream_t s = (hipStream_t)stream;
    if (axis == 0)
        hipLaunchKernelGGL(image_resample_h_kernel, dim3((unsigned)(((long long)out_h * a.groups + 255) / 256), batch), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(image_resample_v_kernel<false>, dim3((a.groups + 63) / 64, out_h, batch), dim3(64), 0, s, a);
    return gc::check_launch("gc_image_resample_u8");
}

extern "C" int gc_image_resample_v_u8_to_f32(const uint8_t* x, int64_t row_stride, int64_t sample_stride, int in_h, int in_w, const float* lut,
                                             const int32_t* flip, float* y, int batch, int out_h, int out_w, const int32_t* coeff,
                                             const int32_t* bounds, const int32_t* bounds_host, int kmax, int table_stride, const int32_t* other,
                                             const int32_t* other_host, gc_stream_t stream) {
    if (!lut || !flip) return gc::fail(GC_ERR_BAD_ARG, "gc_image_resample_v_u8_to_f32: null pointer");
    int rc = check_resample("gc_image_resample_v_u8_to_f32", x, row_stride, sample_stride, in_h, in_w, y, batch, out_h, out_w, 1, coeff, bounds,
                            bounds_host, kmax, table_stride, other, other_host, true);
    if (rc) return rc;
    RsArgs a{x, row_stride, sample_stride, in_h, in_w, coeff, bounds, kmax, table_stride, other, lut, flip, y, nullptr,
             out_h, out_w, (out_w + 3) / 4, aligned_to(y, 16) && out_w % 4 == 0};
    hipLaunchKernelGGL(image_resample_v_kernel<true>, dim3((a.groups + 63) / 64, out_h, batch), dim3(64), 0, (hipStream_t)stream, a);
    return gc::check_launch("gc_image_resample_v_u8_to_f32");
}
