// All-pairs distances between two sets of feature rows, with the masked column minima of the separability evaluation in the same call.
// See gc_pairwise_f32 in include/gancontrol_hip.h.
//
// D[i, j] = sum_k |S[i, k] - Q[j, k]| / K (ABS) or sum_k (S[i, k] - Q[j, k])^2 (SQ): a GEMM-shaped loop nest whose inner operation is not a
// product, so neither MFMA nor a BLAS takes it.  It is a register-tiled VALU kernel:
//   - a workgroup of 256 threads owns a T x T tile of D, T = 64 R; thread (ty, tx) = (tid / 16, tid % 16) keeps R x R blocks of 4 x 4
//     accumulators: rows h * 64 + 4 ty + a, columns g * 64 + 4 tx + b.  R = 2 (a 128 x 128 tile, 64 accumulators: 16 bytes of operand per
//     32 pair-elements, half the L2 / HBM traffic per pair-element of R = 1) where both extents exceed one small tile and the shape has the
//     work to fill the chip with big tiles; R = 1 otherwise (plan_of);
//   - both operands are staged through LDS in chunks of KC = 32 columns, TRANSPOSED: image[kk][row], rows of T + 4 floats.  A thread reads
//     its operands of one kk as 16-byte words at 4 ty (the 16 lanes that share ty read the same word: a broadcast) and at 4 tx (16 lanes, 16
//     consecutive words = the 64 banks once): every lane group of ds_read_b128 (MI355X_MICROARCH, LDS) is conflict-free.  The staging
//     stores are 4-byte and 4-way conflicted (LD = 4 mod 32); they are 1 / 32 of the LDS cycles of the chunk's reads;
//   - the next chunk's global loads are issued before the current chunk is computed (registers) and stored after it;
//   - rows are read with 16-byte loads when both bases are 16-byte aligned and both strides and K are multiples of 4, else with 4-byte
//     loads; columns past K and rows past the extent are ZERO in both images (|0 - 0| = 0) and never addressed.
// m = n = 1000 is 64 .. 256 tiles on 256 CUs, so long rows are split along K over gridDim.z: split s writes its partial tile to the
// caller's workspace [splits, m, n] and pairwise_finish_kernel adds the partials of an element in ascending s, divides (ABS), stores D and
// takes min / first argmin over the rows whose pid differs from the column's.  No workgroup waits for another one: no atomics, no flags,
// no grid barrier; every sum in an order fixed by (m, n, K): the same inputs give the same bits.  At most two launches per call.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "pairwise_tile.h"          // fetch / stage: the transposed LDS staging, shared with manifold.hip

namespace {

using gc_tile::KC;
using gc_tile::NT;
using gc_tile::fetch;
using gc_tile::stage;
constexpr int MIN_SPLIT_CHUNKS = 8;    // a K split is at least 8 chunks (256 columns) long
constexpr int TARGET_GROUPS = 1024;    // workgroups wanted per launch (4 per CU)
constexpr int BIG_TILE_GROUPS = 256;   // R = 2 only where 128 x 128 tiles x possible splits reach one workgroup per CU
constexpr int FC = 16, FR = 64;        // finish kernel: columns per workgroup x row groups

struct Plan {
    int r;                   // 1: 64 x 64 tiles, 2: 128 x 128
    int tiles_m, tiles_n;
    int chunks, per, splits;          // K chunks in all, per split, and the number of splits
};

// a function of (m, n, k) alone: gc_pairwise_workspace and gc_pairwise_f32 agree whatever the pointers are
Plan plan_of(int m, int n, int k) {
    Plan p;
    p.chunks = gc::ceil_div(k, KC);
    const int max_splits = std::max(1, p.chunks / MIN_SPLIT_CHUNKS);
    const int64_t big = (int64_t)gc::ceil_div(m, 128) * gc::ceil_div(n, 128);
    p.r = (m > 64 && n > 64 && big * max_splits >= BIG_TILE_GROUPS) ? 2 : 1;
    const int t = 64 * p.r;
    p.tiles_m = gc::ceil_div(m, t);
    p.tiles_n = gc::ceil_div(n, t);
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n;
    const int want = (int)std::max<int64_t>(1, gc::ceil_div64(TARGET_GROUPS, tiles));
    p.splits = std::min(want, max_splits);
    p.per = gc::ceil_div(p.chunks, p.splits);
    p.splits = gc::ceil_div(p.chunks, p.per);
    return p;
}

// grid: (column tile, row tile, K split).  out: D (one split; div = K for ABS) or the workspace (split_stride = m * n; div = 1).
template <int R, int MODE, bool VEC>
__global__ __launch_bounds__(NT) void pairwise_tile_kernel(const float* __restrict__ s, long long s_stride, const float* __restrict__ q,
                                                           long long q_stride, int m, int n, int k, int per, int chunks, float* __restrict__ out,
                                                           long long split_stride, float div) {
    constexpr int T = 64 * R, LD = T + 4, M = 4 * R;
    __shared__ __attribute__((aligned(16))) float a_img[KC * LD];
    __shared__ __attribute__((aligned(16))) float b_img[KC * LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.y * T, col0 = blockIdx.x * T;
    const int c_begin = blockIdx.z * per, c_end = min(c_begin + per, chunks);
    float acc[M][M];
#pragma unroll
    for (int x = 0; x < M; ++x)
#pragma unroll
        for (int y = 0; y < M; ++y) acc[x][y] = 0.f;
    float4 ra[2 * R], rb[2 * R];
    fetch<R, VEC>(ra, s, s_stride, m, row0, k, c_begin * KC, tid);
    fetch<R, VEC>(rb, q, q_stride, n, col0, k, c_begin * KC, tid);
    for (int c = c_begin; c < c_end; ++c) {
        __syncthreads();          // the previous chunk has been read by every wave
        stage<R>(ra, a_img, tid);
        stage<R>(rb, b_img, tid);
        __syncthreads();
        if (c + 1 < c_end) {
            fetch<R, VEC>(ra, s, s_stride, m, row0, k, (c + 1) * KC, tid);
            fetch<R, VEC>(rb, q, q_stride, n, col0, k, (c + 1) * KC, tid);
        }
#pragma unroll 4
        for (int kk = 0; kk < KC; ++kk) {
            float a[M], b[M];
#pragma unroll
            for (int h = 0; h < R; ++h) {
                const float4 va = *reinterpret_cast<const float4*>(a_img + kk * LD + h * 64 + ty * 4);
                const float4 vb = *reinterpret_cast<const float4*>(b_img + kk * LD + h * 64 + tx * 4);
                a[4 * h] = va.x; a[4 * h + 1] = va.y; a[4 * h + 2] = va.z; a[4 * h + 3] = va.w;
                b[4 * h] = vb.x; b[4 * h + 1] = vb.y; b[4 * h + 2] = vb.z; b[4 * h + 3] = vb.w;
            }
#pragma unroll
            for (int x = 0; x < M; ++x)
#pragma unroll
                for (int y = 0; y < M; ++y) {
                    const float d = a[x] - b[y];
                    acc[x][y] = MODE == GC_PAIRWISE_ABS ? acc[x][y] + fabsf(d) : fmaf(d, d, acc[x][y]);
                }
        }
    }
    float* dst = out + (long long)blockIdx.z * split_stride;
#pragma unroll
    for (int x = 0; x < M; ++x) {
        const int i = row0 + (x >> 2) * 64 + ty * 4 + (x & 3);
        if (i >= m) continue;
#pragma unroll
        for (int y = 0; y < M; ++y) {
            const int j = col0 + (y >> 2) * 64 + tx * 4 + (y & 3);
            if (j < n) dst[(long long)i * n + j] = acc[x][y] / div;
        }
    }
}

// grid: ceil(n / FC) workgroups of FC columns x FR row groups.  splits > 1: D[i, j] = (ws[0, i, j] + ws[1, i, j] + ...) / div; splits == 1:
// D is read.  With pids: best / best_idx of the column over the rows with another pid; the (value, row) pairs of the row groups meet in a
// tree whose order is by value, then by row: the lowest row that attains the minimum, whatever the grouping.
__global__ __launch_bounds__(FC * FR) void pairwise_finish_kernel(const float* __restrict__ ws, int splits, float* __restrict__ d, int m, int n,
                                                                  float div, const int32_t* __restrict__ s_pid, const int32_t* __restrict__ q_pid,
                                                                  float* __restrict__ best, int32_t* __restrict__ best_idx) {
    __shared__ float sv[FR][FC];
    __shared__ int si[FR][FC];
    const int tx = threadIdx.x % FC, g = threadIdx.x / FC;
    const int j = blockIdx.x * FC + tx;
    const long long plane = (long long)m * n;
    float bv = __builtin_inff();
    int bi = 0x7fffffff;
    if (j < n) {
        const int qp = q_pid ? q_pid[j] : 0;
        for (int i = g; i < m; i += FR) {
            const long long at = (long long)i * n + j;
            float v;
            if (splits > 1) {
                v = ws[at];
                for (int sp = 1; sp < splits; ++sp) v += ws[sp * plane + at];
                v /= div;
                d[at] = v;
            } else {
                v = d[at];
            }
            if (s_pid && s_pid[i] != qp && v < bv) { bv = v; bi = i; }          // rows ascend: the first of equal values stays
        }
    }
    if (!s_pid) return;
    sv[g][tx] = bv;
    si[g][tx] = bi;
    __syncthreads();
    for (int off = FR / 2; off > 0; off >>= 1) {
        if (g < off) {
            const float ov = sv[g + off][tx];
            const int oi = si[g + off][tx];
            if (ov < sv[g][tx] || (ov == sv[g][tx] && oi < si[g][tx])) { sv[g][tx] = ov; si[g][tx] = oi; }
        }
        __syncthreads();
    }
    if (g == 0 && j < n) {
        best[j] = sv[0][tx];
        best_idx[j] = si[0][tx] == 0x7fffffff ? -1 : si[0][tx];
    }
}

template <int R, int MODE>
void launch_tiles(bool vec, dim3 grid, hipStream_t stream, const float* s, long long s_stride, const float* q, long long q_stride, int m, int n, int k,
                  const Plan& p, float* out, long long split_stride, float div) {
    if (vec)
        hipLaunchKernelGGL((pairwise_tile_kernel<R, MODE, true>), grid, dim3(NT), 0, stream, s, s_stride, q, q_stride, m, n, k, p.per, p.chunks, out,
                           split_stride, div);
    else
        hipLaunchKernelGGL((pairwise_tile_kernel<R, MODE, false>), grid, dim3(NT), 0, stream, s, s_stride, q, q_stride, m, n, k, p.per, p.chunks, out,
                           split_stride, div);
}

}  // namespace

extern "C" size_t gc_pairwise_workspace(int m, int n, int k) {
    if (m < 1 || n < 1 || k < 1) return 0;
    const Plan p = plan_of(m, n, k);
    return p.splits > 1 ? (size_t)p.splits * (size_t)m * (size_t)n * sizeof(float) : 0;
}

extern "C" int gc_pairwise_f32(const float* s, int64_t s_stride, const float* q, int64_t q_stride, int m, int n, int k, int mode, float* d,
                               const int32_t* s_pid, const int32_t* q_pid, float* best, int32_t* best_idx, void* workspace,
                               size_t workspace_bytes, gc_stream_t stream) {
    const char* what = "gc_pairwise_f32";
    if (!s || !q || !d) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (m < 1 || n < 1 || k < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: extents m %d, n %d, k %d: at least 1 each", what, m, n, k);
    if (s_stride < k || q_stride < k)
        return gc::fail(GC_ERR_BAD_ARG, "%s: row strides %lld / %lld are shorter than the rows (%d)", what, (long long)s_stride, (long long)q_stride, k);
    if (mode != GC_PAIRWISE_ABS && mode != GC_PAIRWISE_SQ) return gc::fail(GC_ERR_BAD_ARG, "%s: unknown mode %d", what, mode);
    if ((s_pid == nullptr) != (q_pid == nullptr)) return gc::fail(GC_ERR_BAD_ARG, "%s: signature and query pids go together", what);
    if (s_pid && (!best || !best_idx)) return gc::fail(GC_ERR_BAD_ARG, "%s: pids without best / best_idx (null pointer)", what);
    const Plan p = plan_of(m, n, k);
    if (p.tiles_m > 65535) return gc::fail(GC_ERR_UNSUPPORTED, "%s: m %d: at most %d rows are built", what, m, 65535 * 64);
    const size_t need = gc_pairwise_workspace(m, n, k);
    if (need && (!workspace || workspace_bytes < need))
        return gc::fail(GC_ERR_WORKSPACE, "%s: workspace too small: %zu bytes given, %zu needed", what, workspace ? workspace_bytes : (size_t)0, need);
    const bool vec = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(q)) & 15) == 0 && s_stride % 4 == 0 && q_stride % 4 == 0 && k % 4 == 0;
    const bool split = p.splits > 1;
    float* out = split ? static_cast<float*>(workspace) : d;
    const long long split_stride = split ? (long long)m * n : 0;
    const float kdiv = mode == GC_PAIRWISE_ABS ? (float)k : 1.f;
    const float div = split ? 1.f : kdiv;
    const dim3 grid(p.tiles_n, p.tiles_m, p.splits);
    hipStream_t st = (hipStream_t)stream;
    if (p.r == 2) {
        if (mode == GC_PAIRWISE_ABS) launch_tiles<2, GC_PAIRWISE_ABS>(vec, grid, st, s, s_stride, q, q_stride, m, n, k, p, out, split_stride, div);
        else                         launch_tiles<2, GC_PAIRWISE_SQ>(vec, grid, st, s, s_stride, q, q_stride, m, n, k, p, out, split_stride, div);
    } else {
        if (mode == GC_PAIRWISE_ABS) launch_tiles<1, GC_PAIRWISE_ABS>(vec, grid, st, s, s_stride, q, q_stride, m, n, k, p, out, split_stride, div);
        else                         launch_tiles<1, GC_PAIRWISE_SQ>(vec, grid, st, s, s_stride, q, q_stride, m, n, k, p, out, split_stride, div);
    }
    if (int rc = gc::check_launch(what)) return rc;
    if (split || s_pid) {
        hipLaunchKernelGGL(pairwise_finish_kernel, dim3(gc::ceil_div(n, FC)), dim3(FC * FR), 0, st, static_cast<const float*>(workspace), p.splits, d, m, n,
                           kdiv, s_pid, q_pid, best, best_idx);
        if (int rc = gc::check_launch(what)) return rc;
    }
    return GC_OK;
}
