// The same / not-same hinge loss of one feature level of the attribute stage (LossModelClass.calc_mini_batch_loss), forward and backward.
// See gc_pair_hinge_fwd_f32 / gc_pair_hinge_bwd_f32 in include/gancontrol_hip.h.
//
// n <= 64 rows of K values, read in place: row i of the pair order is row rows.at[i] of the caller's buffer (the host index travels BY VALUE in
// the kernel arguments: no device index, no gather, no cat).  Forward:
//   - n K <= ONE_LAUNCH_VALUES (every last-layer shape of the shipped configs): ONE launch of one workgroup.  The rows go to LDS (row pitch
//     K | 1: lanes that hold different pairs hit different banks), a pair (i > j) is summed by a group of G adjacent lanes (lane g takes the
//     columns g, g + G, ... in ascending order, then an xor butterfly inside the group: an order fixed by (n, K)), the raw sums meet in LDS
//     and hinge_finish turns them into D, the coefficient matrix C = dloss / dD and the loss;
//   - longer rows (an intermediate level, K up to 200 704): the 64 x 64 tile of pairwise.hip with ONE operand image (both sides are the same
//     rows), split along K over the grid; split s writes its partial lower triangle to the workspace [splits, n, n] and a second launch of
//     one workgroup adds the partials of a pair (G lanes a pair, ascending s, the same butterfly) and runs hinge_finish.
// Backward, one launch: a thread owns a column k, the workgroup stages its 128 columns of the n rows and the symmetric, pre-scaled
// coefficients coef[i][j] = g C[max, min] v_i v_j m in LDS (g is read from the device: no host sync), and walks the rows of the WHOLE
// mini-batch: an indexed row with a non-zero coefficient gets sum_j coef[i][j] phi(F_i,k - F_j,k), every other row a zero.
// No atomics, no flags, no workgroup waits for another; every sum in an order fixed by (n, K): the same inputs give the same bits.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "pairwise_tile.h"          // fetch / stage: the transposed LDS staging of the tile kernels

namespace {

using gc_tile::KC;
using gc_tile::NT;
using gc_tile::fetch;
using gc_tile::stage;

constexpr int MAX_ROWS = GC_PAIR_HINGE_MAX_ROWS;
constexpr int MAX_BATCH_ROWS = GC_PAIR_HINGE_MAX_BATCH_ROWS;
constexpr int ONE_LAUNCH_VALUES = GC_PAIR_HINGE_ONE_LAUNCH_VALUES;
constexpr int MIN_SPLIT_CHUNKS = 8;    // a K split is at least 8 chunks (256 columns) long
constexpr int MAX_SPLITS = 512;        // two workgroups per CU: each one's chunk loop is a chain of HBM latencies
constexpr int FIN_NT = 1024;           // threads of the finish workgroup
constexpr int BWD_NT = 128;            // columns per backward workgroup

struct Rows { int32_t at[MAX_ROWS]; };          // pair order -> row of the caller's buffer (zeros past n)

struct Hinge {
    int n, k, mode;
    float scale;
    int s_begin, s_end;          // the 'same' set: pairs (j + 1, j), j even, s_begin <= j < s_end; every other pair below the diagonal is 'rest'
    float lower, upper, weight;
    float count_same, count_rest;
};

struct Plan {
    bool one_launch;
    int chunks, per, splits;
};

// a function of (n, k) alone
Plan plan_of(int n, int k) {
    Plan p;
    p.one_launch = (int64_t)n * k <= ONE_LAUNCH_VALUES;
    p.chunks = gc::ceil_div(k, KC);
    p.splits = std::min(MAX_SPLITS, std::max(1, p.chunks / MIN_SPLIT_CHUNKS));
    p.per = gc::ceil_div(p.chunks, p.splits);
    p.splits = gc::ceil_div(p.chunks, p.per);
    return p;
}

// lanes per pair: the largest power of two (at most one wavefront) that still gives every pair of one sweep its own group
int group_of(int pairs, int threads) {
    int g = 1;
    while (g < 64 && (int64_t)pairs * (2 * g) <= threads) g *= 2;
    return g;
}

__device__ __forceinline__ void pair_of(int p, int& i, int& j) {          // p = i (i - 1) / 2 + j, i > j
    i = 1;
    while (i * (i + 1) / 2 <= p) ++i;
    j = p - i * (i - 1) / 2;
}

__device__ __forceinline__ float group_butterfly(float s, int group) {
    for (int off = 1; off < group; off <<= 1) s += __shfl_xor(s, off);          // both partners add the same two values: one result
    return s;
}

// dm: the raw sums of the pairs below the diagonal (LDS, [n, n]); vv: 1 / 0 per pair-order row (LDS).  Writes D, C (zeros on and above the
// diagonal) and the loss.  Thread t takes the elements t, t + NTH, ... in ascending order; the two hinge sums meet in a tree over LDS.
template <int NTH>
__device__ void hinge_finish(const float* dm, const float* vv, float* red, const Hinge h, float* __restrict__ d_out, float* __restrict__ c_out,
                             float* __restrict__ loss) {
    const int tid = threadIdx.x, n = h.n;
    const float w_same = h.weight / h.count_same, w_rest = -h.weight / h.count_rest;
    float sum_same = 0.f, sum_rest = 0.f;
    for (int p = tid; p < n * n; p += NTH) {
        const int i = p / n, j = p - i * n;
        float d = 0.f, c = 0.f;
        if (i > j) {
            d = dm[p];
            if (h.mode == GC_PAIR_HINGE_ABS) d = d / (float)h.k * (vv[i] * vv[j]);
            else if (h.mode == GC_PAIR_HINGE_MSQ) d = d / (float)h.k * h.scale;
            const bool same = i == j + 1 && (j & 1) == 0 && j >= h.s_begin && j < h.s_end;
            const float t = same ? d - h.lower : h.upper - d;
            if (t >= 0.f) {          // torch.clamp(min=0) passes the gradient at 0 too
                if (same) { sum_same += t; c = w_same; }
                else      { sum_rest += t; c = w_rest; }
            }
        }
        d_out[p] = d;
        c_out[p] = c;
    }
    red[tid] = sum_same;
    red[NTH + tid] = sum_rest;
    __syncthreads();
    for (int off = NTH / 2; off > 0; off >>= 1) {
        if (tid < off) {
            red[tid] += red[tid + off];
            red[NTH + tid] += red[NTH + tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) *loss = h.weight * (red[0] / h.count_same + red[NTH] / h.count_rest);
}

__device__ __forceinline__ void stage_valid(float* vv, const float* __restrict__ valid, const Rows& rows, int n) {
    const int tid = threadIdx.x;
    if (tid < n) vv[tid] = (valid == nullptr || valid[rows.at[tid]] != 0.f) ? 1.f : 0.f;
}

__global__ __launch_bounds__(NT) void pair_hinge_small_kernel(const float* __restrict__ f, long long stride, const Rows rows,
                                                              const float* __restrict__ valid, const Hinge h, int group, float* __restrict__ d_out,
                                                              float* __restrict__ c_out, float* __restrict__ loss) {
    __shared__ float img[ONE_LAUNCH_VALUES + MAX_ROWS];          // n (K | 1) <= n K + n
    __shared__ float dm[MAX_ROWS * MAX_ROWS];
    __shared__ float red[2 * NT];
    __shared__ float vv[MAX_ROWS];
    const int tid = threadIdx.x, n = h.n, k = h.k, pitch = k | 1;
    for (int i = 0; i < n; ++i) {
        const float* src = f + (long long)rows.at[i] * stride;
        for (int c = tid; c < k; c += NT) img[i * pitch + c] = src[c];
    }
    stage_valid(vv, valid, rows, n);
    __syncthreads();
    const int pairs = n * (n - 1) / 2, g = tid & (group - 1);
    for (int p = tid / group; p < pairs; p += NT / group) {
        int i, j;
        pair_of(p, i, j);
        const float* a = img + i * pitch;
        const float* b = img + j * pitch;
        float s = 0.f;
        if (h.mode == GC_PAIR_HINGE_ABS) {
            for (int c = g; c < k; c += group) s += fabsf(a[c] - b[c]);
        } else {
            for (int c = g; c < k; c += group) {
                const float d = a[c] - b[c];
                s = fmaf(d, d, s);
            }
        }
        s = group_butterfly(s, group);
        if (g == 0) dm[i * n + j] = s;
    }
    __syncthreads();
    hinge_finish<NT>(dm, vv, red, h, d_out, c_out, loss);
}

// grid: K splits.  The micro-tile of pairwise.hip on one operand image; only the blocks on or below the diagonal and inside the n rows run.
template <bool SQ, bool VEC>
__global__ __launch_bounds__(NT) void pair_hinge_tile_kernel(const float* __restrict__ f, long long stride, const Rows rows, int n, int k, int per,
                                                             int chunks, float* __restrict__ ws) {
    constexpr int LD = 64 + 4;
    __shared__ __attribute__((aligned(16))) float img[KC * LD];
    __shared__ int32_t gidx[MAX_ROWS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < MAX_ROWS) gidx[tid] = rows.at[tid];
    __syncthreads();
    const int c_begin = blockIdx.x * per, c_end = min(c_begin + per, chunks);
    const bool mine = ty >= tx && ty * 4 < n;
    float acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = 0.f;
    float4 ra[2];
    fetch<1, VEC, true>(ra, f, stride, n, 0, k, c_begin * KC, tid, gidx);
    for (int c = c_begin; c < c_end; ++c) {
        __syncthreads();          // the previous chunk has been read by every wave
        stage<1>(ra, img, tid);
        __syncthreads();
        if (c + 1 < c_end) fetch<1, VEC, true>(ra, f, stride, n, 0, k, (c + 1) * KC, tid, gidx);
        if (!mine) continue;
#pragma unroll 4
        for (int kk = 0; kk < KC; ++kk) {
            const float4 va = *reinterpret_cast<const float4*>(img + kk * LD + ty * 4);
            const float4 vb = *reinterpret_cast<const float4*>(img + kk * LD + tx * 4);
            const float a[4] = {va.x, va.y, va.z, va.w}, b[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const float d = a[x] - b[y];
                    acc[x][y] = SQ ? fmaf(d, d, acc[x][y]) : acc[x][y] + fabsf(d);
                }
        }
    }
    if (!mine) return;
    float* dst = ws + (long long)blockIdx.x * n * n;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int i = ty * 4 + x;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int j = tx * 4 + y;
            if (i < n && j < i) dst[i * n + j] = acc[x][y];
        }
    }
}

__global__ __launch_bounds__(FIN_NT) void pair_hinge_finish_kernel(const float* __restrict__ ws, int splits, const Rows rows,
                                                                   const float* __restrict__ valid, const Hinge h, int group, float* __restrict__ d_out,
                                                                   float* __restrict__ c_out, float* __restrict__ loss) {
    __shared__ float dm[MAX_ROWS * MAX_ROWS];
    __shared__ float red[2 * FIN_NT];
    __shared__ float vv[MAX_ROWS];
    const int tid = threadIdx.x, n = h.n;
    stage_valid(vv, valid, rows, n);
    const int pairs = n * (n - 1) / 2, g = tid & (group - 1);
    const long long plane = (long long)n * n;
    for (int p = tid / group; p < pairs; p += FIN_NT / group) {
        int i, j;
        pair_of(p, i, j);
        float s = 0.f;
        for (int sp = g; sp < splits; sp += group) s += ws[sp * plane + i * n + j];
        s = group_butterfly(s, group);
        if (g == 0) dm[i * n + j] = s;
    }
    __syncthreads();
    hinge_finish<FIN_NT>(dm, vv, red, h, d_out, c_out, loss);
}

// grid: ceil(K / BWD_NT).  mul: 1 / K (ABS), 2 (SQ), 2 scale / K (MSQ).
template <bool ABS>
__global__ __launch_bounds__(BWD_NT) void pair_hinge_bwd_kernel(const float* __restrict__ f, long long stride, int n_rows, const Rows rows,
                                                                const float* __restrict__ valid, int n, int k, float mul, const float* __restrict__ c_in,
                                                                const float* __restrict__ g_in, float* __restrict__ df) {
    __shared__ float ft[MAX_ROWS * BWD_NT];
    __shared__ float coef[MAX_ROWS * MAX_ROWS];
    __shared__ float vv[MAX_ROWS];
    __shared__ int active[MAX_ROWS];
    __shared__ int inv[MAX_BATCH_ROWS];
    const int tid = threadIdx.x, col = blockIdx.x * BWD_NT + tid;
    for (int r = tid; r < n_rows; r += BWD_NT) inv[r] = -1;
    stage_valid(vv, valid, rows, n);
    __syncthreads();
    if (tid < n) inv[rows.at[tid]] = tid;
    const float gm = g_in[0] * mul;
    for (int p = tid; p < n * n; p += BWD_NT) {
        const int i = p / n, j = p - i * n;
        coef[p] = i == j ? 0.f : c_in[max(i, j) * n + min(i, j)] * gm * (vv[i] * vv[j]);
    }
    if (col < k)
        for (int i = 0; i < n; ++i) ft[i * BWD_NT + tid] = f[(long long)rows.at[i] * stride + col];
    __syncthreads();
    if (tid < n) {
        int any = 0;
        for (int j = 0; j < n; ++j) any |= coef[tid * n + j] != 0.f;
        active[tid] = any;
    }
    __syncthreads();
    if (col >= k) return;
    for (int r = 0; r < n_rows; ++r) {
        const int i = inv[r];
        float acc = 0.f;
        if (i >= 0 && active[i]) {
            const float fi = ft[i * BWD_NT + tid];
            for (int j = 0; j < n; ++j) {
                const float c = coef[i * n + j];          // the same word for every lane: a broadcast, and a uniform branch
                if (c == 0.f) continue;
                const float d = fi - ft[j * BWD_NT + tid];
                acc = ABS ? acc + (d > 0.f ? c : (d < 0.f ? -c : 0.f)) : fmaf(c, d, acc);
            }
        }
        df[(long long)r * k + col] = acc;
    }
}

// the checks both entries share; fills rows (identity without an index)
int check_rows(const char* what, const float* f, int64_t stride, int n_rows, const int32_t* row_index, int n, int k, int mode, Rows& rows) {
    if (!f) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (k < 1 || n < 2 || n_rows < n) return gc::fail(GC_ERR_BAD_ARG, "%s: extents n %d, n_rows %d, k %d: k at least 1, n at least 2, n_rows at least n", what, n, n_rows, k);
    if (n > MAX_ROWS) return gc::fail(GC_ERR_UNSUPPORTED, "%s: n %d: at most %d rows are built", what, n, MAX_ROWS);
    if (n_rows > MAX_BATCH_ROWS) return gc::fail(GC_ERR_UNSUPPORTED, "%s: n_rows %d: at most %d rows are built", what, n_rows, MAX_BATCH_ROWS);
    if (stride < k) return gc::fail(GC_ERR_BAD_ARG, "%s: row stride %lld is shorter than the rows (%d)", what, (long long)stride, k);
    if (mode != GC_PAIR_HINGE_ABS && mode != GC_PAIR_HINGE_SQ && mode != GC_PAIR_HINGE_MSQ) return gc::fail(GC_ERR_BAD_ARG, "%s: unknown mode %d", what, mode);
    if (!row_index && n_rows != n) return gc::fail(GC_ERR_BAD_ARG, "%s: n_rows %d != n %d without a row index", what, n_rows, n);
    bool seen[MAX_BATCH_ROWS] = {};
    for (int i = 0; i < MAX_ROWS; ++i) rows.at[i] = 0;
    for (int i = 0; i < n; ++i) {
        const int r = row_index ? row_index[i] : i;
        if (r < 0 || r >= n_rows || seen[r]) return gc::fail(GC_ERR_BAD_ARG, "%s: row_index[%d] = %d: distinct rows in [0, %d) expected", what, i, r, n_rows);
        seen[r] = true;
        rows.at[i] = r;
    }
    return GC_OK;
}

}  // namespace

extern "C" size_t gc_pair_hinge_workspace(int n, int k) {
    if (n < 2 || n > MAX_ROWS || k < 1) return 0;
    const Plan p = plan_of(n, k);
    return p.one_launch ? 0 : (size_t)p.splits * (size_t)n * (size_t)n * sizeof(float);
}

extern "C" int gc_pair_hinge_fwd_f32(const float* f, int64_t stride, int n_rows, const int32_t* row_index, const float* row_valid, int n_same,
                                     int n_not_same, int k, int mode, float scale, int focus, float lower, float upper, float weight, float* loss,
                                     float* d, float* c, void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    const char* what = "gc_pair_hinge_fwd_f32";
    if (!loss || !d || !c) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (n_same < 0 || n_not_same < 0) return gc::fail(GC_ERR_BAD_ARG, "%s: n_same %d, n_not_same %d: negative", what, n_same, n_not_same);
    const int64_t n64 = (int64_t)n_same + n_not_same;
    const int n = n64 > MAX_ROWS ? MAX_ROWS + 1 : (int)n64;
    Rows rows;
    if (int rc = check_rows(what, f, stride, n_rows, row_index, n, k, mode, rows)) return rc;
    if (focus != GC_PAIR_HINGE_FOCUS_SAME && focus != GC_PAIR_HINGE_FOCUS_NOT_SAME) return gc::fail(GC_ERR_BAD_ARG, "%s: unknown focus %d", what, focus);
    if (mode != GC_PAIR_HINGE_ABS) row_valid = nullptr;          // the flags belong to the ABS form alone
    Hinge h;
    h.n = n; h.k = k; h.mode = mode; h.scale = scale;
    h.lower = lower; h.upper = upper; h.weight = weight;
    const int half_same = 2 * (n_same / 2), half_not = 2 * (n_not_same / 2);
    h.s_begin = focus == GC_PAIR_HINGE_FOCUS_SAME ? 0 : half_same;
    h.s_end = focus == GC_PAIR_HINGE_FOCUS_SAME ? half_same : half_same + half_not;
    const int pairs = n * (n - 1) / 2, count_same = (h.s_end - h.s_begin) / 2;
    if (count_same < 1 || pairs - count_same < 1)
        return gc::fail(GC_ERR_BAD_ARG, "%s: empty pair set (%d same pairs, %d others): the mean of an empty set is not built", what, count_same, pairs - count_same);
    h.count_same = (float)count_same;
    h.count_rest = (float)(pairs - count_same);
    const Plan p = plan_of(n, k);
    const size_t need = gc_pair_hinge_workspace(n, k);
    if (need && (!workspace || workspace_bytes < need))
        return gc::fail(GC_ERR_WORKSPACE, "%s: workspace too small: %zu bytes given, %zu needed", what, workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    if (p.one_launch) {
        hipLaunchKernelGGL(pair_hinge_small_kernel, dim3(1), dim3(NT), 0, st, f, (long long)stride, rows, row_valid, h, group_of(pairs, NT), d, c, loss);
        return gc::check_launch(what);
    }
    float* ws = static_cast<float*>(workspace);
    const bool vec = (reinterpret_cast<uintptr_t>(f) & 15) == 0 && stride % 4 == 0 && k % 4 == 0;
    const bool sq = mode != GC_PAIR_HINGE_ABS;
    const dim3 grid(p.splits);
    if (sq && vec)       hipLaunchKernelGGL((pair_hinge_tile_kernel<true, true>), grid, dim3(NT), 0, st, f, (long long)stride, rows, n, k, p.per, p.chunks, ws);
    else if (sq)         hipLaunchKernelGGL((pair_hinge_tile_kernel<true, false>), grid, dim3(NT), 0, st, f, (long long)stride, rows, n, k, p.per, p.chunks, ws);
    else if (vec)        hipLaunchKernelGGL((pair_hinge_tile_kernel<false, true>), grid, dim3(NT), 0, st, f, (long long)stride, rows, n, k, p.per, p.chunks, ws);
    else                 hipLaunchKernelGGL((pair_hinge_tile_kernel<false, false>), grid, dim3(NT), 0, st, f, (long long)stride, rows, n, k, p.per, p.chunks, ws);
    if (int rc = gc::check_launch(what)) return rc;
    hipLaunchKernelGGL(pair_hinge_finish_kernel, dim3(1), dim3(FIN_NT), 0, st, ws, p.splits, rows, row_valid, h, group_of(pairs, FIN_NT), d, c, loss);
    return gc::check_launch(what);
}

extern "C" int gc_pair_hinge_bwd_f32(const float* f, int64_t stride, int n_rows, const int32_t* row_index, const float* row_valid, int n, int k, int mode,
                                     float scale, const float* c, const float* g, float* df, gc_stream_t stream) {
    const char* what = "gc_pair_hinge_bwd_f32";
    if (!c || !g || !df) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    Rows rows;
    if (int rc = check_rows(what, f, stride, n_rows, row_index, n, k, mode, rows)) return rc;
    if (mode != GC_PAIR_HINGE_ABS) row_valid = nullptr;
    const float mul = mode == GC_PAIR_HINGE_ABS ? 1.f / (float)k : (mode == GC_PAIR_HINGE_SQ ? 2.f : 2.f * scale / (float)k);
    const dim3 grid(gc::ceil_div(k, BWD_NT));
    hipStream_t st = (hipStream_t)stream;
    if (mode == GC_PAIR_HINGE_ABS)
        hipLaunchKernelGGL((pair_hinge_bwd_kernel<true>), grid, dim3(BWD_NT), 0, st, f, (long long)stride, n_rows, rows, row_valid, n, k, mul, c, g, df);
    else
        hipLaunchKernelGGL((pair_hinge_bwd_kernel<false>), grid, dim3(BWD_NT), 0, st, f, (long long)stride, n_rows, rows, row_valid, n, k, mul, c, g, df);
    return gc::check_launch(what);
}
