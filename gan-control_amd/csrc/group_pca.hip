// Per-group latent PCA: the moments of every attribute group's slice of w, and the projection of latents onto the retained subspaces.
// See gc_group_moments_f32 / gc_group_project_f32 in include/gancontrol_hip.h.
//
// Moments.  Group g owns columns [lo_g, lo_g + D_g) of w [n, stride].  Its covariance is cut into 64 x 64 tiles; only tiles on or above the
// diagonal exist, and all groups' tiles form ONE flat list (Groups::tile0).  The rows are cut into splits of GC_GROUP_ROW_SPLIT rows, or of
// more rows (whole chunks) where that would make more than GC_GROUP_MAX_SPLITS splits: the workspace holds at most that many partial sets.
// moments_tile_kernel: grid (tile, split), 256 threads; thread (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 entries (ty + 16 u, tx + 16 v)
// of its tile in float64 registers.  Chunks of KC rows are staged through LDS as float64 images A[kk][64] (the tile's row columns) and
// B[kk][64] (its column columns); a thread reads A[kk][ty + 16 u] (two addresses per 32-lane half: a broadcast) and B[kk][tx + 16 v] (16
// consecutive doubles: the 32 banks once), every read a conflict-free ds_read_b64.  The product of two widened floats is exact, so the only
// rounding is in the sums.  Wave 0 of a diagonal tile also sums its 64 columns (S1).  Rows past n and columns past D_g are zero in the images
// and never addressed.  Loads: 16-byte words where the group's first column, the base and the stride allow (lo % 4 == 0, base 16-byte aligned,
// stride % 4 == 0) and the word ends inside the group; 4-byte loads otherwise.  Both stage the same doubles.
// Partial sums (S1 per column, S2 per upper-tile entry) go to the workspace, one slice per split; moments_finish_kernel (one workgroup per
// (group, row i)) adds them in ascending split order, forms (S2 - S1_a S1_c / n) / (n - 1) with (a, c) = (min, max)(i, j) -- the same
// operands in the same order for cov[i, j] and cov[j, i] -- and writes the means.  No atomics, no flags: the same inputs give the same bits.
//
// Projection.  project_kernel: grid (row, group), 256 threads.  d = x_g - m_g staged in LDS; c = P_g d, one wave per component (lanes over
// the columns in ascending steps of 64, then a fixed butterfly); x_g = m_g + P_g^T c, one thread per column over the components in
// ascending order.  A workgroup reads its slice completely before it writes it, and groups do not overlap: in place is safe.
#include <cstdint>

#include "common.h"

namespace {

constexpr int T = 64;                       // tile edge
constexpr int NT = 256;                     // threads per workgroup
constexpr int KC = 16;                      // rows per LDS chunk
constexpr int SPLIT = GC_GROUP_ROW_SPLIT;   // rows per split, while that makes at most GC_GROUP_MAX_SPLITS splits
static_assert(SPLIT % KC == 0, "a split is whole chunks");
static_assert(KC * T == 4 * NT, "one 4-float word per thread and operand per chunk");

struct Groups {
    int count;
    int vec;                     // bit g: group g takes 16-byte loads
    int split_rows;              // rows per split (split_of)
    int lo[GC_GROUP_MAX];
    int width[GC_GROUP_MAX];
    int tile0[GC_GROUP_MAX + 1]; // first flat tile of group g; tile0[count] = all tiles
    int row0[GC_GROUP_MAX + 1];  // first packed mean element of group g; row0[count] = sum of widths
    long long cov0[GC_GROUP_MAX + 1];  // first packed covariance element of group g
};

int tiles_of(int width) {
    const int t = gc::ceil_div(width, T);
    return t * (t + 1) / 2;
}

// One 4-float word of a T-column operand chunk: rows row0 .. row0 + KC - 1, columns col0 .. col0 + T - 1 of the group (cols valid ones).
__device__ __forceinline__ float4 fetch(const float* __restrict__ base, long long stride, int n, int row0, int col0, int cols, bool vec, int tid) {
    const int row = row0 + (tid >> 4), c = (tid & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n && c < cols) {
        const float* p = base + (long long)row * stride + col0 + c;
        if (vec && c + 4 <= cols) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            v.x = p[0];
            if (c + 1 < cols) v.y = p[1];
            if (c + 2 < cols) v.z = p[2];
            if (c + 3 < cols) v.w = p[3];
        }
    }
    return v;
}

__device__ __forceinline__ void stage(const float4& v, double* image, int tid) {
    double* dst = image + (tid >> 4) * T + (tid & 15) * 4;
    dst[0] = (double)v.x; dst[1] = (double)v.y; dst[2] = (double)v.z; dst[3] = (double)v.w;
}

// grid: (flat upper tile, split).  ws: per split, [row0[count] S1 values | cov0[count] S2 values].
__global__ __launch_bounds__(NT) void moments_tile_kernel(const float* __restrict__ w, long long stride, int n, Groups gr, double* __restrict__ ws) {
    __shared__ double a_img[KC * T];
    __shared__ double b_img[KC * T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int flat = blockIdx.x, split = blockIdx.y;
    int g = 0;
    while (g + 1 < gr.count && flat >= gr.tile0[g + 1]) ++g;
    const int width = gr.width[g], nt = (width + T - 1) / T;
    int t = flat - gr.tile0[g], ti = 0;
    while (t >= nt - ti) { t -= nt - ti; ++ti; }
    const int tj = ti + t;
    const int i0 = ti * T, j0 = tj * T;
    const int ci = min(T, width - i0), cj = min(T, width - j0);
    const bool diag = ti == tj, vec = (gr.vec >> g) & 1;
    const float* base = w + gr.lo[g];
    const int r_begin = split * gr.split_rows, r_end = min(r_begin + gr.split_rows, n);
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    double s1 = 0.0;
    float4 ra = fetch(base, stride, r_end, r_begin, i0, ci, vec, tid);
    float4 rb = diag ? ra : fetch(base, stride, r_end, r_begin, j0, cj, vec, tid);
    for (int r = r_begin; r < r_end; r += KC) {
        __syncthreads();          // every wave has read the previous chunk
        stage(ra, a_img, tid);
        stage(rb, b_img, tid);
        __syncthreads();
        if (r + KC < r_end) {
            ra = fetch(base, stride, r_end, r + KC, i0, ci, vec, tid);
            rb = diag ? ra : fetch(base, stride, r_end, r + KC, j0, cj, vec, tid);
        }
        if (diag && tid < T) {          // wave 0: the column sums, rows in ascending order
#pragma unroll 4
            for (int kk = 0; kk < KC; ++kk) s1 += a_img[kk * T + tid];
        }
#pragma unroll 4
        for (int kk = 0; kk < KC; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = a_img[kk * T + ty + 16 * u];
                b[u] = b_img[kk * T + tx + 16 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
        }
    }
    const long long per = (long long)gr.row0[gr.count] + gr.cov0[gr.count];
    double* slice = ws + (long long)split * per;
    if (diag && tid < ci) slice[gr.row0[g] + i0 + tid] = s1;
    double* s2 = slice + gr.row0[gr.count] + gr.cov0[g];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = ty + 16 * u;
        if (i >= ci) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = tx + 16 * v;
            if (j < cj) s2[(long long)(i0 + i) * width + j0 + j] = acc[u][v];
        }
    }
}

// grid: row0[count] workgroups, one per (group, row i).
__global__ __launch_bounds__(NT) void moments_finish_kernel(const double* __restrict__ ws, int splits, int n, Groups gr, double* __restrict__ mean,
                                                            double* __restrict__ cov) {
    __shared__ double s1[GC_GROUP_MAX_WIDTH];
    const int tid = threadIdx.x, b = blockIdx.x;
    int g = 0;
    while (g + 1 < gr.count && b >= gr.row0[g + 1]) ++g;
    const int width = gr.width[g], i = b - gr.row0[g];
    const long long per = (long long)gr.row0[gr.count] + gr.cov0[gr.count];
    const double dn = (double)n, dn1 = (double)(n - 1);
    for (int j = tid; j < width; j += NT) {
        const double* p = ws + gr.row0[g] + j;
        double s = p[0];
        for (int sp = 1; sp < splits; ++sp) s += p[sp * per];
        s1[j] = s;
        if (i == 0) mean[gr.row0[g] + j] = s / dn;
    }
    __syncthreads();
    const double* s2 = ws + gr.row0[gr.count] + gr.cov0[g];
    double* out = cov + gr.cov0[g] + (long long)i * width;
    for (int j = tid; j < width; j += NT) {
        const int a = min(i, j), c = max(i, j);
        const double* p = s2 + (long long)a * width + c;
        double s = p[0];
        for (int sp = 1; sp < splits; ++sp) s += p[sp * per];
        out[j] = (s - s1[a] * s1[c] / dn) / dn1;
    }
}

struct Proj {
    int count;
    int lo[GC_GROUP_MAX];
    int width[GC_GROUP_MAX];
    int rank[GC_GROUP_MAX];
    const float* p[GC_GROUP_MAX];
};

// grid: (row, group)
__global__ __launch_bounds__(NT) void project_kernel(float* __restrict__ x, long long stride, const float* __restrict__ mean, Proj pr) {
    __shared__ float d[GC_GROUP_MAX_WIDTH];
    __shared__ float c[GC_GROUP_MAX_WIDTH];
    const int tid = threadIdx.x, g = blockIdx.y;
    const int width = pr.width[g], rank = pr.rank[g];
    float* xr = x + (long long)blockIdx.x * stride + pr.lo[g];
    const float* m = mean + pr.lo[g];
    const float* __restrict__ p = pr.p[g];
    for (int j = tid; j < width; j += NT) d[j] = xr[j] - m[j];
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = wave; k < rank; k += NT / 64) {
        const float* row = p + (long long)k * width;
        float s = 0.f;
        for (int j = lane; j < width; j += 64) s = fmaf(row[j], d[j], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);          // a + b == b + a: every lane holds the same bits
        if (lane == 0) c[k] = s;
    }
    __syncthreads();
    for (int j = tid; j < width; j += NT) {
        float y = 0.f;
        for (int k = 0; k < rank; ++k) y = fmaf(p[(long long)k * width + j], c[k], y);
        xr[j] = m[j] + y;
    }
}

// Validates a group table; fills widths.  0 or an error code (the message is set).
int check_groups(const int32_t* lo, const int32_t* hi, int groups, int64_t stride, int* width, const char* what) {
    if (!lo || !hi) return gc::fail(GC_ERR_BAD_ARG, "%s: null group table", what);
    if (groups < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: %d groups: at least 1", what, groups);
    if (groups > GC_GROUP_MAX) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d groups: at most %d are built", what, groups, GC_GROUP_MAX);
    for (int g = 0; g < groups; ++g) {
        if (lo[g] < 0 || hi[g] <= lo[g] || hi[g] > stride)
            return gc::fail(GC_ERR_BAD_ARG, "%s: group %d [%d, %d) is empty or outside rows of stride %lld", what, g, lo[g], hi[g], (long long)stride);
        width[g] = hi[g] - lo[g];
        if (width[g] > GC_GROUP_MAX_WIDTH)
            return gc::fail(GC_ERR_UNSUPPORTED, "%s: group %d is %d wide: at most %d columns are built", what, g, width[g], GC_GROUP_MAX_WIDTH);
    }
    return GC_OK;
}

bool moments_table(int n, const int32_t* lo, const int32_t* hi, int groups, int64_t stride, Groups& gr, int& splits) {
    int width[GC_GROUP_MAX];
    if (n < 2 || n > GC_GROUP_MAX_ROWS || check_groups(lo, hi, groups, stride, width, "gc_group_moments") != GC_OK) return false;
    gr.count = groups;
    gr.vec = 0;
    gr.tile0[0] = gr.row0[0] = 0;
    gr.cov0[0] = 0;
    for (int g = 0; g < groups; ++g) {
        gr.lo[g] = lo[g];
        gr.width[g] = width[g];
        gr.tile0[g + 1] = gr.tile0[g] + tiles_of(width[g]);
        gr.row0[g + 1] = gr.row0[g] + width[g];
        gr.cov0[g + 1] = gr.cov0[g] + (long long)width[g] * width[g];
    }
    // SPLIT rows per split up to GC_GROUP_MAX_SPLITS splits; beyond, longer splits (whole chunks) keep the workspace at most
    // GC_GROUP_MAX_SPLITS partial sets whatever n is
    gr.split_rows = SPLIT;
    if (gc::ceil_div(n, SPLIT) > GC_GROUP_MAX_SPLITS) gr.split_rows = gc::ceil_div(gc::ceil_div(n, GC_GROUP_MAX_SPLITS), KC) * KC;
    splits = gc::ceil_div(n, gr.split_rows);
    return true;
}

}  // namespace

extern "C" size_t gc_group_moments_workspace(int n, const int32_t* lo, const int32_t* hi, int groups) {
    Groups gr;
    int splits;
    if (!moments_table(n, lo, hi, groups, INT64_MAX, gr, splits)) return 0;
    return (size_t)splits * (size_t)(gr.row0[groups] + gr.cov0[groups]) * sizeof(double);
}

extern "C" int gc_group_moments_f32(const float* w, int64_t stride, int n, const int32_t* lo, const int32_t* hi, int groups, double* mean,
                                    double* cov, void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    const char* what = "gc_group_moments_f32";
    if (!w || !mean || !cov) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (n < 2) return gc::fail(GC_ERR_BAD_ARG, "%s: %d rows: at least 2", what, n);
    int width[GC_GROUP_MAX];
    if (int rc = check_groups(lo, hi, groups, stride, width, what)) return rc;
    if (n > GC_GROUP_MAX_ROWS) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d rows: at most %d are built", what, n, GC_GROUP_MAX_ROWS);
    if (stride > (INT64_MAX - stride) / n) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d rows of stride %lld overflow the index", what, n, (long long)stride);
    Groups gr;
    int splits;
    moments_table(n, lo, hi, groups, stride, gr, splits);
    const size_t need = gc_group_moments_workspace(n, lo, hi, groups);
    if (!workspace || workspace_bytes < need)
        return gc::fail(GC_ERR_WORKSPACE, "%s: workspace too small: %zu bytes given, %zu needed", what, workspace ? workspace_bytes : (size_t)0, need);
    const bool aligned = (reinterpret_cast<uintptr_t>(w) & 15) == 0 && stride % 4 == 0;
    for (int g = 0; g < groups; ++g)
        if (aligned && lo[g] % 4 == 0) gr.vec |= 1 << g;
    hipStream_t st = (hipStream_t)stream;
    double* ws = static_cast<double*>(workspace);
    hipLaunchKernelGGL(moments_tile_kernel, dim3(gr.tile0[groups], splits), dim3(NT), 0, st, w, (long long)stride, n, gr, ws);
    if (int rc = gc::check_launch(what)) return rc;
    hipLaunchKernelGGL(moments_finish_kernel, dim3(gr.row0[groups]), dim3(NT), 0, st, static_cast<const double*>(ws), splits, n, gr, mean, cov);
    return gc::check_launch(what);
}

extern "C" int gc_group_project_f32(float* x, int64_t stride, int rows, const float* mean, const float* const* components, const int32_t* ranks,
                                    const int32_t* lo, const int32_t* hi, int groups, gc_stream_t stream) {
    const char* what = "gc_group_project_f32";
    if (!x || !mean || !components || !ranks) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (rows < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: %d rows: at least 1", what, rows);
    int width[GC_GROUP_MAX];
    if (int rc = check_groups(lo, hi, groups, stride, width, what)) return rc;
    Proj pr;
    pr.count = groups;
    for (int g = 0; g < groups; ++g) {
        if (!components[g]) return gc::fail(GC_ERR_BAD_ARG, "%s: group %d: null component matrix", what, g);
        if (ranks[g] < 1 || ranks[g] > width[g]) return gc::fail(GC_ERR_BAD_ARG, "%s: group %d: %d components of a %d-wide group", what, g, ranks[g], width[g]);
        for (int h = 0; h < g; ++h)
            if (lo[g] < hi[h] && lo[h] < hi[g]) return gc::fail(GC_ERR_BAD_ARG, "%s: groups %d and %d overlap", what, h, g);
        pr.lo[g] = lo[g];
        pr.width[g] = width[g];
        pr.rank[g] = ranks[g];
        pr.p[g] = components[g];
    }
    if (stride > (INT64_MAX - stride) / rows) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d rows of stride %lld overflow the index", what, rows, (long long)stride);
    hipLaunchKernelGGL(project_kernel, dim3(rows, groups), dim3(NT), 0, (hipStream_t)stream, x, (long long)stride, mean, pr);
    return gc::check_launch(what);
}
