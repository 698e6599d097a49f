// The image output path: float32 planar [B, 3, h, w] in [-1, 1] -> ONE uint8 interleaved image grid [grid_h, grid_w, 3], the mirror image of
// image_input.hip.  It replaces the host chain of the reference's evaluation/generation.py:14-22 / :87-94 --
// t.mul(0.5).add(0.5).clamp(min=0., max=1.).cpu(), torchvision.utils.make_grid, transforms.ToPILImage (mul(255).byte()) -- with one launch
// that reads every float once (12 B per pixel) and writes every byte of the grid once (3 B per pixel), padding bands and empty tiles included.
//   image_f32_to_u8_grid_kernel     byte = trunc(clamp(x * 0.5f + 0.5f, 0, 1) * 255.0f), every operation rounded to float32 on its own
// Ownership is by OUTPUT bytes: a lane owns three ALIGNED dwords (12 bytes) of one grid row, wherever the row starts (the grid may be a view at
// any byte offset, and tile k starts at byte 3 * (padding + col * (w + padding)) of its row, which takes every residue mod 4).  12 bytes
// starting at row byte s touch the pixels s / 3 .. (s + 11) / 3: four, or five when s is no multiple of 3.  Where all of them lie in one tile
// (all but two lanes per tile row) the lane loads 4 consecutive floats of each plane in one 16-byte access (4-byte aligned: gfx9 takes
// those) plus the fifth as a scalar, so a wave's loads of a plane cover one contiguous 1 KiB run and its stores one contiguous 768 B run.
// The 12 - 15 bytes are assembled in registers and shifted into place with a funnel shift.  Lanes that straddle a tile edge, a padding
// band or an end of the row take the same route with per-pixel scalar loads; only a lane whose dwords reach outside the row (its first or
// its last) stores single bytes.  Nothing outside the row's 3 * grid_w bytes is stored, nothing outside the batch * 3 * h * w floats loaded.
#include <algorithm>

#include "common.h"

namespace {

typedef uint32_t u32;
typedef u32 u32x2u_t __attribute__((ext_vector_type(2), aligned(4)));

struct GridArgs {
    const float* x; long long row_stride, plane_stride, sample_stride;          // elements
    uint8_t* y; long long y_stride;                                             // bytes
    int batch, h, w, grid_h, grid_w, xmaps, padding;
    u32 pad;                                                                    // the padding byte
};

// The reference's five float32 operations, none contracted into another; NaN -> 0 (fmaxf returns the other operand), +-inf follow the clamp.
__device__ __forceinline__ u32 quantize(float x) {
#pragma clang fp contract(off)
    float v = x * 0.5f;
    v = v + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    v = v * 255.0f;
    return (u32)(int)v;
}

// grid: (group of 12 aligned output bytes, grid row [strided by gridDim.y])
__global__ __launch_bounds__(256) void image_f32_to_u8_grid_kernel(GridArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int row_bytes = 3 * a.grid_w, cell_h = a.h + a.padding, cell_w = a.w + a.padding;
    for (int gy = blockIdx.y; gy < a.grid_h; gy += gridDim.y) {
        uint8_t* row = a.y + (long long)gy * a.y_stride;
        const int r = (int)(reinterpret_cast<uintptr_t>(row) & 3);
        const int s = 12 * t - r;                        // the row byte of this lane's first byte; >= -3
        if (s >= row_bytes) continue;
        const bool full = s >= 0 && s + 12 <= row_bytes;
        const int p0 = (s + 3) / 3 - 1, m = s - 3 * p0;  // the first pixel touched (-1: only its bytes before the row) and the lane's offset in it
        const int np = m ? 5 : 4;
        // the tile row of this grid row
        const int gyp = gy - a.padding;
        const int ty = gyp >= 0 ? gyp / cell_h : 0, iy = gyp - ty * cell_h;
        const bool row_in_tile = gyp >= 0 && iy < a.h;
        u32 q[5][3];
        bool fast = false;
        if (full && row_in_tile && p0 >= a.padding) {
            const int px0 = p0 - a.padding, tx = px0 / cell_w, ix0 = px0 - tx * cell_w, k = ty * a.xmaps + tx;
            if (ix0 + np <= a.w && k < a.batch) {
                fast = true;
                const float* src = a.x + k * a.sample_stride + iy * a.row_stride + ix0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const gc::f32x4u_t v = gc::stream_load4u(src + c * a.plane_stride);
                    q[0][c] = quantize(v.x); q[1][c] = quantize(v.y); q[2][c] = quantize(v.z); q[3][c] = quantize(v.w);
                    q[4][c] = m ? quantize(src[c * a.plane_stride + 4]) : 0u;
                }
            }
        }
        if (!fast) {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int p = p0 + i;
                q[i][0] = q[i][1] = q[i][2] = a.pad;
                if (i >= np || p < 0 || p >= a.grid_w) continue;          // no byte of the row: never stored
                const int px = p - a.padding;
                if (!row_in_tile || px < 0) continue;
                const int tx = px / cell_w, ix = px - tx * cell_w, k = ty * a.xmaps + tx;
                if (ix >= a.w || k >= a.batch) continue;                  // a padding column, or an empty tile of a ragged last row
                const float* src = a.x + k * a.sample_stride + iy * a.row_stride + ix;
#pragma unroll
                for (int c = 0; c < 3; ++c) q[i][c] = quantize(src[c * a.plane_stride]);
            }
        }
        // byte 3 * i + c of the 15 is pixel i, channel c; the lane's 12 start at byte m
        u32 wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 15; ++e) wd[e >> 2] |= q[e / 3][e % 3] << ((e & 3) * 8);
        u32 o[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) o[d] = __funnelshift_r(wd[d], wd[d + 1], m * 8);
        uint8_t* dst = row + s;                          // 4-byte aligned
        if (full) {
            *reinterpret_cast<u32x2u_t*>(dst) = u32x2u_t{o[0], o[1]};
            reinterpret_cast<u32*>(dst)[2] = o[2];
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j)
                if (s + j >= 0 && s + j < row_bytes) dst[j] = (uint8_t)((o[j >> 2] >> ((j & 3) * 8)) & 255u);
        }
    }
}

}  // namespace

extern "C" int gc_image_f32_to_u8_grid(const float* x, int64_t row_stride, int64_t plane_stride, int64_t sample_stride, uint8_t* y,
                                       int64_t y_row_stride, int batch, int h, int w, int nrow, int padding, int pad_value, int grid_h,
                                       int grid_w, gc_stream_t stream) {
    const char* what = "gc_image_f32_to_u8_grid";
    if (!x || !y) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (batch <= 0 || h <= 0 || w <= 0 || nrow <= 0 || padding < 0 || pad_value < 0 || pad_value > 255)
        return gc::fail(GC_ERR_BAD_ARG, "%s: batch %d, %d x %d, nrow %d, padding %d, pad_value %d", what, batch, h, w, nrow, padding, pad_value);
    const long long xmaps = std::min(nrow, batch), ymaps = (batch + xmaps - 1) / xmaps;
    const long long want_h = ymaps * ((long long)h + padding) + padding, want_w = xmaps * ((long long)w + padding) + padding;
    if (want_h > (1 << 30) || want_w > (1 << 29)) return gc::fail(GC_ERR_BAD_ARG, "%s: a %lld x %lld grid is too large", what, want_h, want_w);
    if (grid_h != want_h || grid_w != want_w)
        return gc::fail(GC_ERR_BAD_ARG, "%s: grid_h x grid_w = %d x %d, but %d tiles of %d x %d with nrow %d and padding %d make %lld x %lld", what,
                        grid_h, grid_w, batch, h, w, nrow, padding, want_h, want_w);
    const long long plane_span = (long long)(h - 1) * row_stride + w;
    if (row_stride < w || plane_stride < plane_span || sample_stride < 2 * plane_stride + plane_span)
        return gc::fail(GC_ERR_BAD_ARG, "%s: short stride: row %lld (< %d), plane %lld or sample %lld elements are less than dense", what,
                        (long long)row_stride, w, (long long)plane_stride, (long long)sample_stride);
    if (y_row_stride < 3LL * grid_w) return gc::fail(GC_ERR_BAD_ARG, "%s: short stride: output row stride %lld < %d bytes", what, (long long)y_row_stride, 3 * grid_w);
    GridArgs a{x, row_stride, plane_stride, sample_stride, y, y_row_stride, batch, h, w, grid_h, grid_w, (int)xmaps, padding, (u32)pad_value};
    const int groups = (3 * grid_w + 3 + 11) / 12;        // a row that starts 3 bytes past a dword boundary
    const dim3 grid((groups + 255) / 256, std::min(grid_h, 65535));
    hipLaunchKernelGGL(image_f32_to_u8_grid_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    return gc::check_launch(what);
}
