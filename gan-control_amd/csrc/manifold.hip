// The distance passes of the sample-quality metrics (fid_utils/precision_recall.py, fid_utils/kid.py): k-nearest-neighbour radii, manifold
// membership and the polynomial-kernel sums of KID.  See gc_knn_radius_f32, gc_manifold_hits_f32 and gc_poly_mmd_f32 in
// include/gancontrol_hip.h.
//
// All three are the loop nest of pairwise.hip -- a 256-thread workgroup owns a T x T tile (T = 64 R), thread (ty, tx) keeps R x R blocks of
// 4 x 4 accumulators, both operands go through the transposed LDS images of pairwise_tile.h in chunks of 32 columns with the next chunk's
// loads in flight -- with an epilogue that consumes the tile instead of storing it.  No m x n value ever reaches memory:
//   - a workgroup walks a STRIP of tiles and keeps what the epilogue reduces to (a row's kth + 1 smallest values; hit flags; float64 sums);
//     the number of strips per side is at most STRIPS whatever the extents, so the partial results are O((m + n) * STRIPS);
//   - a finish launch merges the strips' partial results in ascending strip order.
// Rows are never split along K (a tile's sum runs over the chunks in ascending order), no workgroup waits for another one (no atomics, no
// flags, no grid barrier) and every location of the workspace and of the outputs is stored by exactly one thread: the same inputs give the
// same bits.  Squared distances are sum_c (a_c - b_c)^2 with fmaf, as GC_PAIRWISE_SQ; the dot products of KID are fmaf sums and everything
// behind them is float64.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "pairwise_tile.h"

namespace {

using gc_tile::KC;
using gc_tile::NT;
using gc_tile::fetch;
using gc_tile::stage;

constexpr int STRIPS = GC_MANIFOLD_STRIPS;   // strips of tiles per side, at most
constexpr int BIG_TILE_GROUPS = 256;   // R = 2 only where 128 x 128 tiles reach one workgroup per CU
constexpr int KMAX = GC_KNN_MAX_KTH + 1;     // values kept per row, at most
constexpr int MAX_TILES = 65535;       // tiles per side (65535 * 64 rows with R = 1)

struct Side {
    int tiles, per, strips;          // tiles on this side, tiles per strip, strips
};

Side side_of(int rows, int t) {
    Side s;
    s.tiles = gc::ceil_div(rows, t);
    s.per = gc::ceil_div(s.tiles, STRIPS);
    s.strips = gc::ceil_div(s.tiles, s.per);
    return s;
}

// a function of the extents alone: the workspace queries and the launchers agree whatever the pointers are
int tile_r(int m, int n, int64_t batches) {
    const int64_t big = (int64_t)gc::ceil_div(m, 128) * gc::ceil_div(n, 128) * batches;
    return (m > 64 && n > 64 && big >= BIG_TILE_GROUPS) ? 2 : 1;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// acc[x][y] over the whole K of one tile: rows row0 + .. of a (through a_idx when GATHER), columns col0 + .. of b.
// DOT: sum a b, else sum (a - b)^2.  smem: 2 * KC * (T + 4) floats.  Ends behind a barrier-free compute phase: the caller synchronises
// before it touches smem again.
template <int R, bool DOT, bool VEC, bool GATHER>
__device__ __forceinline__ void tile_sums(float (&acc)[4 * R][4 * R], float* smem, const float* __restrict__ a, long long a_stride, int a_rows,
                                          int row0, const int32_t* __restrict__ a_idx, const float* __restrict__ b, long long b_stride, int b_rows,
                                          int col0, const int32_t* __restrict__ b_idx, int k, int tid) {
    constexpr int T = 64 * R, LD = T + 4, M = 4 * R;
    float* a_img = smem;
    float* b_img = smem + KC * LD;
    const int tx = tid & 15, ty = tid >> 4;
    const int chunks = (k + KC - 1) / KC;
#pragma unroll
    for (int x = 0; x < M; ++x)
#pragma unroll
        for (int y = 0; y < M; ++y) acc[x][y] = 0.f;
    float4 ra[2 * R], rb[2 * R];
    fetch<R, VEC, GATHER>(ra, a, a_stride, a_rows, row0, k, 0, tid, a_idx);
    fetch<R, VEC, GATHER>(rb, b, b_stride, b_rows, col0, k, 0, tid, b_idx);
    for (int c = 0; c < chunks; ++c) {
        __syncthreads();          // the previous chunk (or the previous tile's epilogue) is done with the images
        stage<R>(ra, a_img, tid);
        stage<R>(rb, b_img, tid);
        __syncthreads();
        if (c + 1 < chunks) {
            fetch<R, VEC, GATHER>(ra, a, a_stride, a_rows, row0, k, (c + 1) * KC, tid, a_idx);
            fetch<R, VEC, GATHER>(rb, b, b_stride, b_rows, col0, k, (c + 1) * KC, tid, b_idx);
        }
#pragma unroll 4
        for (int kk = 0; kk < KC; ++kk) {
            float av[M], bv[M];
#pragma unroll
            for (int h = 0; h < R; ++h) {
                const float4 va = *reinterpret_cast<const float4*>(a_img + kk * LD + h * 64 + ty * 4);
                const float4 vb = *reinterpret_cast<const float4*>(b_img + kk * LD + h * 64 + tx * 4);
                av[4 * h] = va.x; av[4 * h + 1] = va.y; av[4 * h + 2] = va.z; av[4 * h + 3] = va.w;
                bv[4 * h] = vb.x; bv[4 * h + 1] = vb.y; bv[4 * h + 2] = vb.z; bv[4 * h + 3] = vb.w;
            }
#pragma unroll
            for (int x = 0; x < M; ++x)
#pragma unroll
                for (int y = 0; y < M; ++y) {
                    if (DOT) {
                        acc[x][y] = fmaf(av[x], bv[y], acc[x][y]);
                    } else {
                        const float d = av[x] - bv[y];
                        acc[x][y] = fmaf(d, d, acc[x][y]);
                    }
                }
        }
    }
}

// The KMAX smallest values seen so far, ascending, in registers (every index is a compile-time constant).  The list as a set of values
// does not depend on the order of the insertions; a value equal to the largest kept one changes nothing.
struct Smallest {
    float v[KMAX];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int p = 0; p < KMAX; ++p) v[p] = __builtin_inff();
    }
    __device__ __forceinline__ void insert(float x) {
        if (!(x < v[KMAX - 1])) return;
        v[KMAX - 1] = x;
#pragma unroll
        for (int p = KMAX - 1; p > 0; --p) {
            const float lo = fminf(v[p - 1], v[p]), hi = fmaxf(v[p - 1], v[p]);
            v[p - 1] = lo; v[p] = hi;
        }
    }
    __device__ __forceinline__ float at(int q) const {
        float r = v[0];
#pragma unroll
        for (int p = 1; p < KMAX; ++p) r = q == p ? v[p] : r;
        return r;
    }
};

// ---- gc_knn_radius_f32 ------------------------------------------------------------------------------------------------------------
// grid: (column strip, row tile).  ws [strips, n, kk]: the kk = kth + 1 smallest values of row i over the strip's columns, ascending
// (+inf where the strip has fewer columns).  After a tile's sums its 64-row halves go through LDS (the staging images' bytes), one row per
// thread of the half: thread t < T owns row t of the tile and its list for the whole walk.
// Only one wave scans a half (T reads of a conflict-free row each) while the other three wait at the barrier, R times per tile.  Behind
// rows of 2048 that is under 1 % of a tile's time; at small F it dominates the kernel.  Splitting a row's columns over the four waves
// with a merge of the quarter lists after the walk was built and measured: no faster at F = 2048 from N = 10 000 on, and 14 % slower at
// N = 1000, where a workgroup has one tile and the merge costs what the scan saved (profiles/quality_metrics.md).
template <int R, bool VEC>
__global__ __launch_bounds__(NT) void knn_tile_kernel(const float* __restrict__ a, long long a_stride, int n, int k, int kk, int per, int tiles,
                                                      float* __restrict__ ws) {
    constexpr int T = 64 * R, LD = T + 4, M = 4 * R, DL = T + 1;
    static_assert(64 * DL <= 2 * KC * LD, "a 64-row half of the tile fits the staging images");
    __shared__ __attribute__((aligned(16))) float smem[2 * KC * LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.y * T;
    const int j_begin = blockIdx.x * per, j_end = min(j_begin + per, tiles);
    Smallest best;
    best.clear();
    float acc[M][M];
    for (int jt = j_begin; jt < j_end; ++jt) {
        const int col0 = jt * T;
        tile_sums<R, false, VEC, false>(acc, smem, a, a_stride, n, row0, nullptr, a, a_stride, n, col0, nullptr, k, tid);
        const int cols = min(T, n - col0);
#pragma unroll
        for (int h = 0; h < R; ++h) {
            __syncthreads();          // the images (or the previous half) have been read
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < M; ++y) smem[(ty * 4 + x) * DL + (y >> 2) * 64 + tx * 4 + (y & 3)] = acc[4 * h + x][y];
            __syncthreads();
            if (tid >= 64 * h && tid < 64 * h + 64) {
                const float* row = smem + (tid - 64 * h) * DL;
                for (int c = 0; c < cols; ++c) best.insert(row[c]);
            }
        }
    }
    const int i = row0 + tid;
    if (tid < T && i < n) {
        float* dst = ws + ((long long)blockIdx.x * n + i) * kk;
#pragma unroll
        for (int p = 0; p < KMAX; ++p)
            if (p < kk) dst[p] = best.v[p];
    }
}

// one thread per row: the strips' lists in ascending strip order
__global__ __launch_bounds__(NT) void knn_finish_kernel(const float* __restrict__ ws, int strips, int n, int kk, float* __restrict__ radius2) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    Smallest best;
    best.clear();
    for (int s = 0; s < strips; ++s) {
        const float* src = ws + ((long long)s * n + i) * kk;
        for (int p = 0; p < kk; ++p) best.insert(src[p]);
    }
    radius2[i] = best.at(kk - 1);
}

// ---- gc_manifold_hits_f32 ---------------------------------------------------------------------------------------------------------
// grid: (column strip sx, row strip sy); rows are ref, columns are probe.  ws_col [row strips, n] bytes: column j has a hit among the rows of
// strip sy; ws_row [column strips, m] bytes: row i has a hit among the columns of strip sx.  Per tile the hits meet in two LDS flag arrays
// (plain stores of 1); thread t < T then owns row t / column t of the tile: it clears the flags, reads them behind the barrier, and is the
// only thread that ever stores ws_row[sx, row] (once, after the walk over the columns) and ws_col[sy, column] (the flag at the strip's first
// row tile, a 1 over it where a later row tile hits).
template <int R, bool VEC>
__global__ __launch_bounds__(NT) void hits_tile_kernel(const float* __restrict__ ref, long long ref_stride, const float* __restrict__ ref_r2, int m,
                                                       const float* __restrict__ probe, long long probe_stride, const float* __restrict__ probe_r2,
                                                       int n, int k, int per_y, int per_x, uint8_t* __restrict__ ws_col,
                                                       uint8_t* __restrict__ ws_row) {
    constexpr int T = 64 * R, LD = T + 4, M = 4 * R;
    __shared__ __attribute__((aligned(16))) float smem[2 * KC * LD];
    __shared__ int rowf[T], colf[T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i_begin = blockIdx.y * per_y, i_end = min(i_begin + per_y, (m + T - 1) / T);
    const int j_begin = blockIdx.x * per_x, j_end = min(j_begin + per_x, (n + T - 1) / T);
    ws_col += (long long)blockIdx.y * n;
    if (ws_row) ws_row += (long long)blockIdx.x * m;
    float acc[M][M];
    for (int it = i_begin; it < i_end; ++it) {
        const int row0 = it * T;
        float rr[M];
#pragma unroll
        for (int x = 0; x < M; ++x) {
            const int i = row0 + (x >> 2) * 64 + ty * 4 + (x & 3);
            rr[x] = i < m ? ref_r2[i] : -1.f;
        }
        int row_hit = 0;
        for (int jt = j_begin; jt < j_end; ++jt) {
            const int col0 = jt * T;
            if (tid < T) { rowf[tid] = 0; colf[tid] = 0; }          // (the tile's first barrier orders this before the stores below)
            tile_sums<R, false, VEC, false>(acc, smem, ref, ref_stride, m, row0, nullptr, probe, probe_stride, n, col0, nullptr, k, tid);
            // rows past m and columns past n carry the radius -1 (no sum of squares is below it); their flags are never read
#pragma unroll
            for (int y = 0; y < M; ++y) {
                const int jl = (y >> 2) * 64 + tx * 4 + (y & 3), j = col0 + jl;
                const float pr = (probe_r2 && j < n) ? probe_r2[j] : -1.f;
#pragma unroll
                for (int x = 0; x < M; ++x) {
                    if (acc[x][y] <= rr[x]) colf[jl] = 1;
                    if (acc[x][y] <= pr) rowf[(x >> 2) * 64 + ty * 4 + (x & 3)] = 1;
                }
            }
            __syncthreads();
            if (tid < T) {
                row_hit |= rowf[tid];
                const int j = col0 + tid;
                if (j < n && (it == i_begin || colf[tid])) ws_col[j] = (uint8_t)(colf[tid] != 0);
            }
        }
        if (tid < T && row0 + tid < m && ws_row) ws_row[row0 + tid] = (uint8_t)(row_hit != 0);
    }
}

// one thread per output element: the strips' flags
__global__ __launch_bounds__(NT) void hits_finish_kernel(const uint8_t* __restrict__ ws_col, int strips_y, const uint8_t* __restrict__ ws_row,
                                                         int strips_x, int m, int n, uint8_t* __restrict__ probe_hit, uint8_t* __restrict__ ref_hit) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t < n) {
        int hit = 0;
        for (int s = 0; s < strips_y; ++s) hit |= ws_col[(long long)s * n + t];
        probe_hit[t] = (uint8_t)(hit != 0);
    } else if (ref_hit && t < (long long)n + m) {
        const long long i = t - n;
        int hit = 0;
        for (int s = 0; s < strips_x; ++s) hit |= ws_row[(long long)s * m + i];
        ref_hit[i] = (uint8_t)(hit != 0);
    }
}

// ---- gc_poly_mmd_f32 --------------------------------------------------------------------------------------------------------------
// grid: (column strip, row tile, 3 * subset + which); which: 0 = X x X without the diagonal, 1 = Y x Y without it, 2 = X x Y.
// ws [subsets * 3, tiles, strips] doubles: the workgroup's sum of (dot / k + 1)^3 -- per thread over its elements in tile order, then the
// 256 threads in a fixed LDS tree.  which < 2 visits only the tiles on and above the diagonal.
template <int R, bool VEC>
__global__ __launch_bounds__(NT) void mmd_tile_kernel(const float* __restrict__ x, long long x_stride, const float* __restrict__ y, long long y_stride,
                                                      int k, const int32_t* __restrict__ idx_x, const int32_t* __restrict__ idx_y, int m, int per,
                                                      int tiles, double* __restrict__ ws) {
    constexpr int T = 64 * R, LD = T + 4, M = 4 * R;
    __shared__ __attribute__((aligned(16))) float smem[2 * KC * LD];
    __shared__ double red[NT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int which = blockIdx.z % 3, s = blockIdx.z / 3;
    const float* a = which == 1 ? y : x;
    const long long a_stride = which == 1 ? y_stride : x_stride;
    const int32_t* a_idx = (which == 1 ? idx_y : idx_x) + (long long)s * m;
    const float* b = which == 0 ? x : y;
    const long long b_stride = which == 0 ? x_stride : y_stride;
    const int32_t* b_idx = (which == 0 ? idx_x : idx_y) + (long long)s * m;
    const int row0 = blockIdx.y * T;
    const int j_begin = blockIdx.x * per, j_end = min(j_begin + per, tiles);
    const double kd = (double)k;
    double sum = 0.0;
    float acc[M][M];
    for (int jt = j_begin; jt < j_end; ++jt) {
        // X x X and Y x Y are symmetric (the same products in the same order on both sides of the diagonal): a tile below the diagonal is
        // the doubled weight of its mirror image (exact: a power of two)
        if (which != 2 && jt < (int)blockIdx.y) continue;
        const double weight = (which != 2 && jt > (int)blockIdx.y) ? 2.0 : 1.0;
        const int col0 = jt * T;
        tile_sums<R, true, VEC, true>(acc, smem, a, a_stride, m, row0, a_idx, b, b_stride, m, col0, b_idx, k, tid);
        double part = 0.0;
#pragma unroll
        for (int xx = 0; xx < M; ++xx) {
            const int i = row0 + (xx >> 2) * 64 + ty * 4 + (xx & 3);
#pragma unroll
            for (int yy = 0; yy < M; ++yy) {
                const int j = col0 + (yy >> 2) * 64 + tx * 4 + (yy & 3);
                if (i < m && j < m && (which == 2 || i != j)) {
                    const double t = (double)acc[xx][yy] / kd + 1.0;
                    part += t * t * t;
                }
            }
        }
        sum += weight * part;
    }
    red[tid] = sum;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) ws[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
}

// grid: subsets * 3 workgroups: the partial sums of one (subset, which) in a fixed order
__global__ __launch_bounds__(NT) void mmd_finish_kernel(const double* __restrict__ ws, int parts, double* __restrict__ sums) {
    __shared__ double red[NT];
    const double* src = ws + (long long)blockIdx.x * parts;
    double sum = 0.0;
    for (int p = threadIdx.x; p < parts; p += NT) sum += src[p];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}

int short_workspace(const char* what, const void* workspace, size_t given, size_t need) {
    if (need && (!workspace || given < need))
        return gc::fail(GC_ERR_WORKSPACE, "%s: workspace too small: %zu bytes given, %zu needed", what, workspace ? given : (size_t)0, need);
    return GC_OK;
}

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

extern "C" size_t gc_knn_radius_workspace(int n, int k, int kth) {
    if (n < 1 || k < 1 || kth < 1 || kth >= KMAX) return 0;
    const Side s = side_of(n, 64 * tile_r(n, n, 1));
    return (size_t)s.strips * (size_t)n * (size_t)(kth + 1) * sizeof(float);
}

extern "C" int gc_knn_radius_f32(const float* a, int64_t a_stride, int n, int k, int kth, float* radius2, void* workspace, size_t workspace_bytes,
                                 gc_stream_t stream) {
    const char* what = "gc_knn_radius_f32";
    if (!a || !radius2) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (n < 1 || k < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: extents n %d, k %d: at least 1 each", what, n, k);
    if (kth < 1 || kth >= KMAX) return gc::fail(GC_ERR_BAD_ARG, "%s: kth %d is outside 1 .. %d", what, kth, KMAX - 1);
    if (n < kth + 1) return gc::fail(GC_ERR_BAD_ARG, "%s: %d rows have no neighbour number %d (n >= kth + 1)", what, n, kth);
    if (a_stride < k) return gc::fail(GC_ERR_BAD_ARG, "%s: row stride %lld is shorter than the rows (%d)", what, (long long)a_stride, k);
    const int r = tile_r(n, n, 1);
    const Side s = side_of(n, 64 * r);
    if (s.tiles > MAX_TILES) return gc::fail(GC_ERR_UNSUPPORTED, "%s: n %d: at most %d rows are built", what, n, MAX_TILES * 64);
    if (int rc = short_workspace(what, workspace, workspace_bytes, gc_knn_radius_workspace(n, k, kth))) return rc;
    const bool vec = aligned16(a) && a_stride % 4 == 0 && k % 4 == 0;
    float* ws = static_cast<float*>(workspace);
    const dim3 grid(s.strips, s.tiles);
    hipStream_t st = (hipStream_t)stream;
    if (r == 2) {
        if (vec) hipLaunchKernelGGL((knn_tile_kernel<2, true>), grid, dim3(NT), 0, st, a, a_stride, n, k, kth + 1, s.per, s.tiles, ws);
        else     hipLaunchKernelGGL((knn_tile_kernel<2, false>), grid, dim3(NT), 0, st, a, a_stride, n, k, kth + 1, s.per, s.tiles, ws);
    } else {
        if (vec) hipLaunchKernelGGL((knn_tile_kernel<1, true>), grid, dim3(NT), 0, st, a, a_stride, n, k, kth + 1, s.per, s.tiles, ws);
        else     hipLaunchKernelGGL((knn_tile_kernel<1, false>), grid, dim3(NT), 0, st, a, a_stride, n, k, kth + 1, s.per, s.tiles, ws);
    }
    if (int rc = gc::check_launch(what)) return rc;
    hipLaunchKernelGGL(knn_finish_kernel, dim3(gc::ceil_div(n, NT)), dim3(NT), 0, st, ws, s.strips, n, kth + 1, radius2);
    return gc::check_launch(what);
}

extern "C" size_t gc_manifold_hits_workspace(int m, int n, int k) {
    if (m < 1 || n < 1 || k < 1) return 0;
    const int t = 64 * tile_r(m, n, 1);
    return round16((size_t)side_of(m, t).strips * (size_t)n) + (size_t)side_of(n, t).strips * (size_t)m;
}

extern "C" int gc_manifold_hits_f32(const float* ref, int64_t ref_stride, const float* ref_radius2, int m, const float* probe, int64_t probe_stride,
                                    const float* probe_radius2, int n, int k, uint8_t* probe_hit, uint8_t* ref_hit, void* workspace,
                                    size_t workspace_bytes, gc_stream_t stream) {
    const char* what = "gc_manifold_hits_f32";
    if (!ref || !ref_radius2 || !probe || !probe_hit) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (m < 1 || n < 1 || k < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: extents m %d, n %d, k %d: at least 1 each", what, m, n, k);
    if (ref_stride < k || probe_stride < k)
        return gc::fail(GC_ERR_BAD_ARG, "%s: row strides %lld / %lld are shorter than the rows (%d)", what, (long long)ref_stride, (long long)probe_stride, k);
    if ((probe_radius2 == nullptr) != (ref_hit == nullptr)) return gc::fail(GC_ERR_BAD_ARG, "%s: probe_radius2 and ref_hit go together", what);
    const int r = tile_r(m, n, 1);
    const Side sy = side_of(m, 64 * r), sx = side_of(n, 64 * r);
    if (sy.tiles > MAX_TILES || sx.tiles > MAX_TILES)
        return gc::fail(GC_ERR_UNSUPPORTED, "%s: m %d, n %d: at most %d rows a side are built", what, m, n, MAX_TILES * 64);
    if (int rc = short_workspace(what, workspace, workspace_bytes, gc_manifold_hits_workspace(m, n, k))) return rc;
    const bool vec = aligned16(ref) && aligned16(probe) && ref_stride % 4 == 0 && probe_stride % 4 == 0 && k % 4 == 0;
    uint8_t* ws_col = static_cast<uint8_t*>(workspace);
    uint8_t* ws_row = ref_hit ? ws_col + round16((size_t)sy.strips * (size_t)n) : nullptr;
    const dim3 grid(sx.strips, sy.strips);
    hipStream_t st = (hipStream_t)stream;
#define GC_HITS_LAUNCH(RR, VV)                                                                                                                   \
    hipLaunchKernelGGL((hits_tile_kernel<RR, VV>), grid, dim3(NT), 0, st, ref, ref_stride, ref_radius2, m, probe, probe_stride, probe_radius2, n, k, \
                       sy.per, sx.per, ws_col, ws_row)
    if (r == 2) {
        if (vec) GC_HITS_LAUNCH(2, true); else GC_HITS_LAUNCH(2, false);
    } else {
        if (vec) GC_HITS_LAUNCH(1, true); else GC_HITS_LAUNCH(1, false);
    }
#undef GC_HITS_LAUNCH
    if (int rc = gc::check_launch(what)) return rc;
    const int64_t outs = (int64_t)n + (ref_hit ? m : 0);
    hipLaunchKernelGGL(hits_finish_kernel, dim3((unsigned)gc::ceil_div64(outs, NT)), dim3(NT), 0, st, ws_col, sy.strips, ws_row, sx.strips, m, n, probe_hit,
                       ref_hit);
    return gc::check_launch(what);
}

extern "C" size_t gc_poly_mmd_workspace(int subsets, int m, int k) {
    if (subsets < 1 || m < 1 || k < 1) return 0;
    const Side s = side_of(m, 64 * tile_r(m, m, 3 * (int64_t)subsets));
    return (size_t)subsets * 3 * (size_t)s.tiles * (size_t)s.strips * sizeof(double);
}

extern "C" int gc_poly_mmd_f32(const float* x, int64_t x_stride, int nx, const float* y, int64_t y_stride, int ny, int k, const int32_t* idx_x,
                               const int32_t* idx_y, int subsets, int m, double* sums, void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    const char* what = "gc_poly_mmd_f32";
    if (!x || !y || !idx_x || !idx_y || !sums) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (nx < 1 || ny < 1 || k < 1 || subsets < 1 || m < 1)
        return gc::fail(GC_ERR_BAD_ARG, "%s: extents nx %d, ny %d, k %d, subsets %d, m %d: at least 1 each", what, nx, ny, k, subsets, m);
    if (x_stride < k || y_stride < k)
        return gc::fail(GC_ERR_BAD_ARG, "%s: row strides %lld / %lld are shorter than the rows (%d)", what, (long long)x_stride, (long long)y_stride, k);
    if (subsets > MAX_TILES / 3) return gc::fail(GC_ERR_UNSUPPORTED, "%s: subsets %d: at most %d are built", what, subsets, MAX_TILES / 3);
    const int r = tile_r(m, m, 3 * (int64_t)subsets);
    const Side s = side_of(m, 64 * r);
    if (s.tiles > MAX_TILES) return gc::fail(GC_ERR_UNSUPPORTED, "%s: m %d: at most %d rows are built", what, m, MAX_TILES * 64);
    if (int rc = short_workspace(what, workspace, workspace_bytes, gc_poly_mmd_workspace(subsets, m, k))) return rc;
    const bool vec = aligned16(x) && aligned16(y) && x_stride % 4 == 0 && y_stride % 4 == 0 && k % 4 == 0;
    double* ws = static_cast<double*>(workspace);
    const dim3 grid(s.strips, s.tiles, 3 * subsets);
    hipStream_t st = (hipStream_t)stream;
    if (r == 2) {
        if (vec) hipLaunchKernelGGL((mmd_tile_kernel<2, true>), grid, dim3(NT), 0, st, x, x_stride, y, y_stride, k, idx_x, idx_y, m, s.per, s.tiles, ws);
        else     hipLaunchKernelGGL((mmd_tile_kernel<2, false>), grid, dim3(NT), 0, st, x, x_stride, y, y_stride, k, idx_x, idx_y, m, s.per, s.tiles, ws);
    } else {
        if (vec) hipLaunchKernelGGL((mmd_tile_kernel<1, true>), grid, dim3(NT), 0, st, x, x_stride, y, y_stride, k, idx_x, idx_y, m, s.per, s.tiles, ws);
        else     hipLaunchKernelGGL((mmd_tile_kernel<1, false>), grid, dim3(NT), 0, st, x, x_stride, y, y_stride, k, idx_x, idx_y, m, s.per, s.tiles, ws);
    }
    if (int rc = gc::check_launch(what)) return rc;
    hipLaunchKernelGGL(mmd_finish_kernel, dim3(3 * subsets), dim3(NT), 0, st, ws, s.tiles * s.strips, sums);
    return gc::check_launch(what);
}
