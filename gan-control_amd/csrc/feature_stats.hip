// Streaming feature statistics: raw float64 moments of float32 feature rows, accumulated call by call, and their mean / covariance.
// See gc_feature_moments_accumulate_f32 / _finish_f64 / _merge_f64 in include/gancontrol_stats.h (the error bound is derived there).
//
// Accumulate.  s2 [F, F] is cut into T x T tiles (T = 64); only tiles on or above the diagonal exist, as one flat list, and ONE workgroup
// (256 threads, 4 waves) owns one tile: it walks all n rows of x and then does the read-modify-write of its own tile, so there are no
// atomics, no flags and no workspace, and the same calls give the same bits.  Rows are staged KC = 32 at a time through LDS as FLOAT
// images A[kk][T] (the tile's row columns) and B[kk][T] (its column columns); the next chunk is already on its way into registers while
// the current one is consumed: 32 MFMAs per wave, which take longer than the loads take to return (profiles/feature_stats.md).
// Wave (wi, wj) owns the 32 x 32 quarter (32 wi, 32 wj) of the tile as 2 x 2 blocks of v_mfma_f64_16x16x4_f64: per K = 4 step
// lane l reads A[4 ks + (l >> 4)][.. + (l & 15)] and B likewise -- the f64 operand map (one value per lane, i / j on l & 15, k on l >> 4); with
// row-major x the 16 i of one k are 16 adjacent floats, so no transpose is needed -- widens them to double and issues the four MFMAs.  A
// product of two widened floats is exact in float64.  The image rows are T + 16 floats apart: the four rows of one read then fall on
// banks 0-15, 16-31, 0-15, 16-31, two lanes per bank, which is what a 64-lane 4-byte read costs at best.  The C/D map of the f64 MFMA is
// col = l & 15, row = (l >> 4) + 4 reg (NOT the f32 one).  Threads 0 .. 63 of a diagonal tile also sum its columns (s1), rows ascending.
// Rows past n - 1 and columns past F - 1 are zeros in the images and never addressed (fetch clamps every address into the n rows of F
// elements).  Loads: 16-byte words where base, stride and F allow (base 16-byte aligned, stride % 4 == 0, F % 4 == 0; tile columns start at
// multiples of 64); 4-byte loads otherwise.  Both stage the same floats.
//
// Finish: one workgroup per upper tile (ti, tj).  It reads the tile of s2 row by row, forms c = (s2[i][j] - s1[i] s1[j] / n) / (n - 1) once per
// element, writes it to cov[i][j] and keeps it in LDS; the mirror tile cov[j][i] is then written row by row from the LDS image, so both
// triangles hold the SAME value and every global access runs along a row.  In a diagonal tile only the elements j >= i are computed (what
// lies below the diagonal of s2 is undefined) and the mirror pass fills the rest.  Merge: one workgroup per row, the elements j >= i.
#include <cstdint>

#include "common.h"
#include "gancontrol_stats.h"

namespace {

constexpr int T = GC_STATS_TILE;            // tile edge
constexpr int NT = 256;                     // threads per workgroup
constexpr int KC = 32;                      // rows per LDS chunk
constexpr int LDW = T + 16;                 // floats between image rows (bank spread, above)
constexpr int WORDS = KC * T / (4 * NT);    // 4-float words per thread and operand per chunk: word h is row 16 h + tid / 16 of the chunk
static_assert(T == 64 && KC * T == 4 * NT * WORDS && KC % 4 == 0, "whole words per thread; 2 x 2 waves of 32 x 32; whole K steps");
static_assert((LDW * 4) % 16 == 0, "16-byte LDS stores");

typedef double f64x4_t __attribute__((ext_vector_type(4)));

// One 4-float word of a T-column operand chunk: rows row0 .. row0 + KC - 1 of x, columns col0 .. col0 + T - 1 (cols valid ones).  Branch-free,
// in two halves: fetch issues every load, from an address clamped into the rows and columns that exist; keep turns what lies outside into
// zeros by selects, and is applied only when the word is staged, one chunk later.  (With branches around the loads, or with the selects next
// to them, the compiler waits for each prefetch at once and nothing overlaps the MFMAs.)  VEC: the base is 16-byte aligned, stride % 4 == 0
// and F % 4 == 0, so a word is whole inside the row's F elements or whole outside (cols % 4 == 0).
template <bool VEC>
__device__ __forceinline__ float4 fetch(const float* __restrict__ x, long long stride, int n, long long row0, int col0, int cols, int tid) {
    const long long row = row0 + (tid >> 4);          // (the caller adds 16 h to row0)
    const int c = (tid & 15) * 4;
    const float* p = x + (row < n ? row : (long long)n - 1) * stride + col0;
    if (VEC) return *reinterpret_cast<const float4*>(p + (c < cols ? c : 0));
    const int last = cols - 1;
    return make_float4(p[min(c, last)], p[min(c + 1, last)], p[min(c + 2, last)], p[min(c + 3, last)]);
}

__device__ __forceinline__ float4 keep(float4 v, int n, long long row0, int cols, int tid) {
    const bool in_row = row0 + (tid >> 4) < n;
    const int c = (tid & 15) * 4;
    v.x = in_row && c < cols ? v.x : 0.f;
    v.y = in_row && c + 1 < cols ? v.y : 0.f;
    v.z = in_row && c + 2 < cols ? v.z : 0.f;
    v.w = in_row && c + 3 < cols ? v.w : 0.f;
    return v;
}

__device__ __forceinline__ void stage(const float4& v, float* image, int h, int tid) {
    *reinterpret_cast<float4*>(image + (16 * h + (tid >> 4)) * LDW + (tid & 15) * 4) = v;
}

// grid: the flat upper tiles of s2.
template <bool VEC>
__global__ __launch_bounds__(NT) void accumulate_kernel(const float* __restrict__ x, long long stride, int n, int f, double* __restrict__ s1,
                                                        double* __restrict__ s2) {
    __shared__ __attribute__((aligned(16))) float a_img[KC * LDW];
    __shared__ __attribute__((aligned(16))) float b_img[KC * LDW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int nt = (f + T - 1) / T;
    int t = blockIdx.x, ti = 0;
    while (t >= nt - ti) { t -= nt - ti; ++ti; }
    const int tj = ti + t;
    const int i0 = ti * T, j0 = tj * T;
    const int ci = min(T, f - i0), cj = min(T, f - j0);
    const bool diag = ti == tj;
    f64x4_t acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    double c1 = 0.0;
    const int kr = lane >> 4, col = lane & 15;
    float4 ra[WORDS], rb[WORDS];
#pragma unroll
    for (int h = 0; h < WORDS; ++h) {
        ra[h] = fetch<VEC>(x, stride, n, 16 * h, i0, ci, tid);
        rb[h] = fetch<VEC>(x, stride, n, 16 * h, j0, cj, tid);
    }
    for (long long r = 0; r < n; r += KC) {
        __syncthreads();          // every wave has read the previous chunk
#pragma unroll
        for (int h = 0; h < WORDS; ++h) {
            stage(keep(ra[h], n, r + 16 * h, ci, tid), a_img, h, tid);
            stage(keep(rb[h], n, r + 16 * h, cj, tid), b_img, h, tid);
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < WORDS; ++h) {          // (past the last chunk: clamped loads of row n - 1, never staged)
            ra[h] = fetch<VEC>(x, stride, n, r + KC + 16 * h, i0, ci, tid);
            rb[h] = fetch<VEC>(x, stride, n, r + KC + 16 * h, j0, cj, tid);
        }
        const int rows = (int)min((long long)KC, n - r);          // the rows of this chunk that exist: whole K steps beyond them are skipped
        if (diag && tid < T) {          // the column sums, rows in ascending order
            for (int kk = 0; kk < rows; ++kk) c1 += (double)a_img[kk * LDW + tid];
        }
#pragma unroll
        for (int ks = 0; ks < KC / 4; ++ks) {
            if (ks * 4 >= rows) break;
            const float* pa = a_img + (ks * 4 + kr) * LDW + 32 * wi + col;
            const float* pb = b_img + (ks * 4 + kr) * LDW + 32 * wj + col;
            const double a0 = (double)pa[0], a1 = (double)pa[16];
            const double b0 = (double)pb[0], b1 = (double)pb[16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    if (diag && tid < ci) s1[i0 + tid] += c1;
    // the read-modify-write of the tile; the f64 C/D map: register reg of block (u, v) is row 32 wi + 16 u + (l >> 4) + 4 reg, column 32 wj + 16 v + (l & 15)
    double* out = s2 + (long long)(i0 + 32 * wi + kr) * f + j0 + 32 * wj + col;
    if (ci == T && cj == T) {          // a whole tile: every load is issued before the first add
        double old[2][2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) old[u][v][reg] = out[(long long)(16 * u + 4 * reg) * f + 16 * v];
        asm volatile("" ::: "memory");          // (keeps the compiler from sinking each load to its add: sixteen round trips one after another)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) out[(long long)(16 * u + 4 * reg) * f + 16 * v] = old[u][v][reg] + acc[u][v][reg];
        return;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (32 * wj + 16 * v + col >= cj) continue;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (32 * wi + 16 * u + kr + 4 * reg < ci) out[(long long)(16 * u + 4 * reg) * f + 16 * v] += acc[u][v][reg];
        }
}

// grid: the flat upper tiles, as accumulate_kernel.
__global__ __launch_bounds__(NT) void finish_kernel(const double* __restrict__ s1, const double* __restrict__ s2, double dn, int f, double* __restrict__ mean,
                                                    double* __restrict__ cov) {
    __shared__ double img[T][T + 1];
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int nt = (f + T - 1) / T;
    int t = blockIdx.x, ti = 0;
    while (t >= nt - ti) { t -= nt - ti; ++ti; }
    const int tj = ti + t;
    const int i0 = ti * T, j0 = tj * T;
    const int ci = min(T, f - i0), cj = min(T, f - j0);
    const bool diag = ti == tj;
    const double dn1 = dn - 1.0;
    const double sj = tx < cj ? s1[j0 + tx] : 0.0;
    if (diag && ty == 0 && tx < ci) mean[i0 + tx] = s1[i0 + tx] / dn;
    for (int i = ty; i < ci; i += NT / T) {
        if (tx < cj && (!diag || tx >= i)) {
            const double c = (s2[(long long)(i0 + i) * f + j0 + tx] - s1[i0 + i] * sj / dn) / dn1;
            cov[(long long)(i0 + i) * f + j0 + tx] = c;
            img[i][tx] = c;
        }
    }
    __syncthreads();
    for (int j = ty; j < cj; j += NT / T)          // row j0 + j of the mirror tile: columns i0 .. i0 + ci - 1
        if (tx < ci && (!diag || tx < j)) cov[(long long)(j0 + j) * f + i0 + tx] = img[tx][j];
}

// grid: F workgroups, one per row i.
__global__ __launch_bounds__(NT) void merge_kernel(double* __restrict__ s1a, double* __restrict__ s2a, const double* __restrict__ s1b,
                                                   const double* __restrict__ s2b, int f) {
    const int i = blockIdx.x;
    for (int j = i + threadIdx.x; j < f; j += NT) s2a[(long long)i * f + j] += s2b[(long long)i * f + j];
    if (i == 0)
        for (int j = threadIdx.x; j < f; j += NT) s1a[j] += s1b[j];
}

int check_features(int f, const char* what) {
    if (f < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: %d features: at least 1", what, f);
    if (f > GC_STATS_MAX_FEATURES) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d features: at most %d are built", what, f, GC_STATS_MAX_FEATURES);
    return GC_OK;
}

// every grid here is one-dimensional: the upper tiles (at most 2080) or the F rows (at most 4096), far inside the 2^31 - 1 blocks of grid.x
constexpr int MAX_TILES = (GC_STATS_MAX_FEATURES / T) * (GC_STATS_MAX_FEATURES / T + 1) / 2;
static_assert(GC_STATS_MAX_FEATURES % T == 0 && MAX_TILES <= 65535 && GC_STATS_MAX_FEATURES <= 65535, "grids stay inside every hardware limit");

}  // namespace

extern "C" int gc_feature_moments_accumulate_f32(const float* x, int64_t stride, int n, int features, double* s1, double* s2, gc_stream_t stream) {
    const char* what = "gc_feature_moments_accumulate_f32";
    if (!x || !s1 || !s2) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (n < 1) return gc::fail(GC_ERR_BAD_ARG, "%s: %d rows: at least 1", what, n);
    if (int rc = check_features(features, what)) return rc;
    if (stride < features) return gc::fail(GC_ERR_BAD_ARG, "%s: rows of %d features %lld elements apart", what, features, (long long)stride);
    if (stride > (INT64_MAX - stride) / n) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d rows of stride %lld overflow the index", what, n, (long long)stride);
    const int nt = gc::ceil_div(features, T), tiles = nt * (nt + 1) / 2;
    if (tiles > MAX_TILES) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d tiles: at most %d fit the grid", what, tiles, MAX_TILES);
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && stride % 4 == 0 && features % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(accumulate_kernel<true>, dim3(tiles), dim3(NT), 0, (hipStream_t)stream, x, (long long)stride, n, features, s1, s2);
    else
        hipLaunchKernelGGL(accumulate_kernel<false>, dim3(tiles), dim3(NT), 0, (hipStream_t)stream, x, (long long)stride, n, features, s1, s2);
    return gc::check_launch(what);
}

extern "C" int gc_feature_moments_finish_f64(const double* s1, const double* s2, int64_t n, int features, double* mean, double* cov, gc_stream_t stream) {
    const char* what = "gc_feature_moments_finish_f64";
    if (!s1 || !s2 || !mean || !cov) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (n < 2) return gc::fail(GC_ERR_BAD_ARG, "%s: %lld rows: at least 2", what, (long long)n);
    if (int rc = check_features(features, what)) return rc;
    const int nt = gc::ceil_div(features, T);
    hipLaunchKernelGGL(finish_kernel, dim3(nt * (nt + 1) / 2), dim3(NT), 0, (hipStream_t)stream, s1, s2, (double)n, features, mean, cov);
    return gc::check_launch(what);
}

extern "C" int gc_feature_moments_merge_f64(double* s1a, double* s2a, const double* s1b, const double* s2b, int features, gc_stream_t stream) {
    const char* what = "gc_feature_moments_merge_f64";
    if (!s1a || !s2a || !s1b || !s2b) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (int rc = check_features(features, what)) return rc;
    hipLaunchKernelGGL(merge_kernel, dim3(features), dim3(NT), 0, (hipStream_t)stream, s1a, s2a, s1b, s2b, features);
    return gc::check_launch(what);
}
