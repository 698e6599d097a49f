// The noise regulariser and the noise normaliser of image projection (reference: projection/projection.py:126-154) over a whole LIST of noise
// maps [B, 1, S, S] in a number of launches that depends neither on the length of the list nor on the depth of the pyramids:
//   forward   pyramid_kernel     every map's 2x2-mean pyramid, tile-locally through LDS (a 128 x 128 tile of the finest level reaches one pixel:
//                                1024^2 reaches its last, 8 x 8, level exactly) -> workspace
//             products_kernel    per (map, level, chunk of 4096 elements): sum n * roll(n, 1, x) and sum n * roll(n, 1, y) -> partial sums
//             finish_kernel      the partials of every (map, level) added in a fixed order (float64), means, loss = sum of squared means and
//                                the coefficients 2 * mean / N the gradient needs
//   backward  reg_bwd_kernel     a pure gather: d loss / d n0[b, y, x] = sum_l 0.25^l * (cx_l * (n_l[Y, X - 1] + n_l[Y, X + 1]) + cy_l * (n_l[Y - 1, X]
//                                + n_l[Y + 1, X])) at the pixel's ancestors (Y, X) = (y >> l, x >> l), indices wrapped, read from the stored pyramid
//   normalise norm_stats_kernel  per chunk of 4096 elements: its mean, then the squared deviations from THAT mean (the values stay in registers)
//             norm_merge_kernel  per map: mean = sum n_c mean_c / N and M2 = sum M2_c + sum n_c (mean_c - mean)^2 in float64 (the many-way form
//                                of Chan's merge: nothing is ever squared before its mean is taken off), std = sqrt(M2 / (N - 1))
//             norm_apply_kernel  n = (n - mean) / std in place
// Every reduction is store-and-sum in an order fixed by the shapes: no float atomics, the same bits every time.  The maps' pointers and
// extents travel BY VALUE in the kernel arguments (at most 32 maps: the 1024^2 generator has 17), so there is no device table to upload or cache.
#include <algorithm>

#include "common.h"

namespace {

constexpr int MAX_MAPS = 32, CHUNK = 4096, TILE = 128, MAX_SIZE = 1024;

struct Table {
    float* map[MAX_MAPS];
    long long pyr[MAX_MAPS];          // floats from the workspace's first to level 1 of the map's pyramid (levels 1 .. L - 1 back to back)
    int size[MAX_MAPS], batch[MAX_MAPS];
    int pair0[MAX_MAPS];              // index of (map, level 0) among all (map, level) pairs
    int part0[MAX_MAPS];              // index of the first partial sum of (map, level 0)
    int blk0[MAX_MAPS + 1];           // first workgroup of the map in the launch at hand (pyramid / backward)
    int n;
};

struct Pointers { float* p[MAX_MAPS]; };

struct NormTable {
    float* map[MAX_MAPS];
    long long count[MAX_MAPS];
    int part0[MAX_MAPS];
    int n;
};

// the reference's loop: terms at the current size, stop if size <= 8, otherwise halve
__host__ __device__ inline int levels_of(int s) { int l = 1; while (s > 8) { s >>= 1; ++l; } return l; }
__host__ __device__ inline int rows_per_chunk(int s) { return CHUNK / s > 0 ? CHUNK / s : 1; }
__host__ __device__ inline int chunks_of(int b, int s) { const int rpc = rows_per_chunk(s); return (b * s + rpc - 1) / rpc; }

struct Plan { long long coef, parts, pyramid, total; int pairs, nparts; };          // offsets in floats from the workspace's first

// workspace: | coef[2 * pairs] | parts[2 * nparts] | the pyramids |
inline int make_plan(const int32_t* sizes, const int32_t* batches, int n, Table* t, Plan* p, const char* what) {
    if (!sizes || !batches) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (n <= 0) return gc::fail(GC_ERR_BAD_ARG, "%s: empty list", what);
    if (n > MAX_MAPS) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d maps, at most %d", what, n, MAX_MAPS);
    int pairs = 0, nparts = 0;
    long long pyr = 0;
    for (int m = 0; m < n; ++m) {
        const int s = sizes[m], b = batches[m];
        if (s < 4 || (s & (s - 1)) || b <= 0) return gc::fail(GC_ERR_BAD_ARG, "%s: map %d is [%d, 1, %d, %d]: the size must be a power of two >= 4", what, m, b, s, s);
        if (s > MAX_SIZE) return gc::fail(GC_ERR_UNSUPPORTED, "%s: map %d is [%d, 1, %d, %d]: sizes above %d are not built", what, m, b, s, s, MAX_SIZE);
        if ((long long)b * s * s > INT32_MAX) return gc::fail(GC_ERR_UNSUPPORTED, "%s: map %d has more than 2^31 elements", what, m);
        t->size[m] = s; t->batch[m] = b; t->pair0[m] = pairs; t->part0[m] = nparts; t->pyr[m] = pyr;
        const int levels = levels_of(s);
        for (int l = 0; l < levels; ++l) {
            nparts += chunks_of(b, s >> l);
            if (l) pyr += (long long)b * (s >> l) * (s >> l);
        }
        pairs += levels;
    }
    t->n = n;
    p->pairs = pairs; p->nparts = nparts;
    p->coef = 0; p->parts = 2LL * pairs; p->pyramid = p->parts + 2LL * nparts; p->total = p->pyramid + pyr;
    for (int m = 0; m < n; ++m) t->pyr[m] += p->pyramid;
    return GC_OK;
}

__device__ __forceinline__ int map_of_block(const Table& t, int blk) {
    int m = 0;
    while (m + 1 < t.n && blk >= t.blk0[m + 1]) ++m;
    return m;
}

__device__ __forceinline__ int map_of_pair(const Table& t, int pair) {
    int m = 0;
    while (m + 1 < t.n && pair >= t.pair0[m + 1]) ++m;
    return m;
}

// level l of map m: the map itself, or its place in the workspace
__device__ __forceinline__ const float* level_ptr(const Table& t, const float* ws, int m, int l) {
    if (l == 0) return t.map[m];
    long long off = t.pyr[m];
    for (int k = 1; k < l; ++k) off += (long long)t.batch[m] * (t.size[m] >> k) * (t.size[m] >> k);
    return ws + off;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the sum over the 256 lanes of the workgroup, in every lane
__device__ __forceinline__ float block_sum_all(float v, float* lds) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                       // lds may still be read from the previous call
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// One workgroup per (map, sample, TILE x TILE tile of the finest level); maps of one level (size <= 8) have no workgroup.
__global__ __launch_bounds__(256) void pyramid_kernel(Table t, float* __restrict__ ws) {
    __shared__ float lds0[(TILE / 2) * (TILE / 2)], lds1[(TILE / 4) * (TILE / 4)];
    const int m = map_of_block(t, blockIdx.x);
    const int S = t.size[m], B = t.batch[m], L = levels_of(S);
    const int T = S < TILE ? S : TILE, tpr = S / T;
    int local = blockIdx.x - t.blk0[m];
    const int tx = local % tpr; local /= tpr;
    const int ty = local % tpr, b = local / tpr;
    const float* src = t.map[m] + (size_t)b * S * S + (size_t)(ty * T) * S + tx * T;
    int e = T >> 1, Sl = S >> 1;
    long long level = t.pyr[m];
    float* dst = ws + level + (size_t)b * Sl * Sl + (size_t)(ty * e) * Sl + tx * e;
    for (int i = threadIdx.x; i < e * e; i += 256) {
        const int oy = i / e, ox = i - oy * e;
        const gc::f32x2u_t a = *reinterpret_cast<const gc::f32x2u_t*>(src + (size_t)(2 * oy) * S + 2 * ox);
        const gc::f32x2u_t c = *reinterpret_cast<const gc::f32x2u_t*>(src + (size_t)(2 * oy + 1) * S + 2 * ox);
        const float v = ((a.x + a.y) + (c.x + c.y)) * 0.25f;
        lds0[i] = v;
        dst[(size_t)oy * Sl + ox] = v;
    }
    __syncthreads();
    float *cur = lds0, *nxt = lds1;
    for (int l = 2; l < L; ++l) {
        const int pe = e;
        level += (long long)B * Sl * Sl;
        e >>= 1; Sl >>= 1;
        dst = ws + level + (size_t)b * Sl * Sl + (size_t)(ty * e) * Sl + tx * e;
        for (int i = threadIdx.x; i < e * e; i += 256) {
            const int oy = i / e, ox = i - oy * e;
            const float* r0 = cur + (2 * oy) * pe + 2 * ox;
            const float v = ((r0[0] + r0[1]) + (r0[pe] + r0[pe + 1])) * 0.25f;
            nxt[i] = v;
            dst[(size_t)oy * Sl + ox] = v;
        }
        __syncthreads();
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
}

// grid: (chunk, (map, level) pair); the chunks a pair does not have return at once
__global__ __launch_bounds__(256) void products_kernel(Table t, float* __restrict__ ws, long long parts_off) {
    __shared__ float lds[4];
    const int pair = blockIdx.y, m = map_of_pair(t, pair), l = pair - t.pair0[m];
    const int S = t.size[m] >> l, B = t.batch[m];
    const int chunks = chunks_of(B, S), j = blockIdx.x;
    if (j >= chunks) return;
    const float* src = level_ptr(t, ws, m, l);
    const int rpc = rows_per_chunk(S), r0 = j * rpc, r1 = min(B * S, r0 + rpc);
    const int count = (r1 - r0) * S, mask = S - 1;
    float sx = 0.f, sy = 0.f;
    for (int i = threadIdx.x; i < count; i += 256) {
        const int r = r0 + i / S, x = i & mask, y = r & mask;
        const float* row = src + (size_t)r * S;
        const float v = row[x];
        sx = fmaf(v, row[(x - 1) & mask], sx);
        sy = fmaf(v, src[(size_t)(y ? r - 1 : r + S - 1) * S + x], sy);
    }
    int part = t.part0[m] + j;
    for (int k = 0; k < l; ++k) part += chunks_of(B, t.size[m] >> k);
    const float tx = block_sum_all(sx, lds), ty = block_sum_all(sy, lds);
    if (threadIdx.x == 0) {
        ws[parts_off + 2LL * part] = tx;
        ws[parts_off + 2LL * part + 1] = ty;
    }
}

// one workgroup of 16 waves, a wave per (map, level) pair at a time
__global__ __launch_bounds__(1024) void finish_kernel(Table t, float* __restrict__ ws, long long coef_off, long long parts_off, int pairs,
                                                      float* __restrict__ loss) {
    __shared__ double term[MAX_MAPS * 8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int pair = wave; pair < pairs; pair += 16) {
        const int m = map_of_pair(t, pair), l = pair - t.pair0[m];
        const int S = t.size[m] >> l, B = t.batch[m], chunks = chunks_of(B, S);
        int part = t.part0[m];
        for (int k = 0; k < l; ++k) part += chunks_of(B, t.size[m] >> k);
        double ax = 0.0, ay = 0.0;
        for (int j = lane; j < chunks; j += 64) {
            ax += (double)ws[parts_off + 2LL * (part + j)];
            ay += (double)ws[parts_off + 2LL * (part + j) + 1];
        }
        ax = wave_sum(ax); ay = wave_sum(ay);
        if (lane == 0) {
            const double count = (double)B * S * S, mx = ax / count, my = ay / count;
            ws[coef_off + 2LL * pair] = (float)(2.0 * mx / count);
            ws[coef_off + 2LL * pair + 1] = (float)(2.0 * my / count);
            term[pair] = mx * mx + my * my;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int pair = 0; pair < pairs; ++pair) acc += term[pair];
        loss[0] = (float)acc;
    }
}

// a lane per pixel of the finest level
__global__ __launch_bounds__(256) void reg_bwd_kernel(Table t, Pointers grads, const float* __restrict__ ws, long long coef_off,
                                                      const float* __restrict__ gout) {
    const int m = map_of_block(t, blockIdx.x);
    const int S = t.size[m], B = t.batch[m], L = levels_of(S);
    const long long i = (long long)(blockIdx.x - t.blk0[m]) * 256 + threadIdx.x;
    if (i >= (long long)B * S * S) return;
    const int x = (int)(i & (S - 1)), y = (int)((i / S) & (S - 1)), b = (int)(i / ((long long)S * S));
    const float* coef = ws + coef_off + 2LL * t.pair0[m];
    float acc = 0.f, weight = 1.f;
    long long level = t.pyr[m];
    for (int l = 0; l < L; ++l) {
        const int s = S >> l, mask = s - 1, X = x >> l, Y = y >> l;
        const float* base = (l == 0 ? t.map[m] : ws + level) + (size_t)b * s * s;
        const float* row = base + (size_t)Y * s;
        const float hx = row[(X - 1) & mask] + row[(X + 1) & mask];
        const float hy = base[(size_t)((Y - 1) & mask) * s + X] + base[(size_t)((Y + 1) & mask) * s + X];
        acc = fmaf(weight, fmaf(coef[2 * l], hx, coef[2 * l + 1] * hy), acc);
        weight *= 0.25f;
        if (l) level += (long long)B * s * s;
    }
    grads.p[m][i] = gout[0] * acc;
}

// grid: (chunk, map)
__global__ __launch_bounds__(256) void norm_stats_kernel(NormTable t, float* __restrict__ parts) {
    __shared__ float lds[4];
    const int m = blockIdx.y;
    const long long count = t.count[m], lo = (long long)blockIdx.x * CHUNK;
    if (lo >= count) return;
    const long long hi = min(count, lo + CHUNK);
    const float* src = t.map[m];
    float v[CHUNK / 256];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long i = lo + k * 256 + threadIdx.x;
        v[k] = i < hi ? src[i] : 0.f;
        sum += v[k];
    }
    const float here = (float)(hi - lo), mean = block_sum_all(sum, lds) / here;
    float m2 = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long long i = lo + k * 256 + threadIdx.x;
        const float d = v[k] - mean;
        if (i < hi) m2 = fmaf(d, d, m2);
    }
    m2 = block_sum_all(m2, lds);
    if (threadIdx.x == 0) {
        float* out = parts + 3LL * (t.part0[m] + blockIdx.x);
        out[0] = mean; out[1] = m2; out[2] = here;
    }
}

// one workgroup of 16 waves, a wave per map at a time; stats[2 m] = mean, stats[2 m + 1] = unbiased standard deviation
__global__ __launch_bounds__(1024) void norm_merge_kernel(NormTable t, const float* __restrict__ parts, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int m = wave; m < t.n; m += 16) {
        const long long count = t.count[m];
        const int chunks = (int)((count + CHUNK - 1) / CHUNK);
        const float* p = parts + 3LL * t.part0[m];
        double acc = 0.0;
        for (int j = lane; j < chunks; j += 64) acc += (double)p[3 * j + 2] * (double)p[3 * j];
        acc = wave_sum(acc);
        const double mean = __shfl(acc, 0, 64) / (double)count;
        double m2 = 0.0;
        for (int j = lane; j < chunks; j += 64) {
            const double d = (double)p[3 * j] - mean;
            m2 += (double)p[3 * j + 1] + (double)p[3 * j + 2] * d * d;
        }
        m2 = wave_sum(m2);
        if (lane == 0) {
            stats[2 * m] = (float)mean;
            stats[2 * m + 1] = (float)sqrt(m2 / (double)(count - 1));
        }
    }
}

// grid: (chunk, map)
__global__ __launch_bounds__(256) void norm_apply_kernel(NormTable t, const float* __restrict__ stats) {
    const int m = blockIdx.y;
    const long long count = t.count[m], lo = (long long)blockIdx.x * CHUNK;
    if (lo >= count) return;
    const long long hi = min(count, lo + CHUNK);
    const float mean = stats[2 * m], sd = stats[2 * m + 1];
    float* p = t.map[m];
    for (long long i = lo + threadIdx.x; i < hi; i += 256) p[i] = (p[i] - mean) / sd;
}

struct NormPlan { long long stats, total; int nparts, max_chunks; };          // workspace: | parts[3 * nparts] | stats[2 * n] |

inline int make_norm_plan(const int64_t* counts, int n, NormTable* t, NormPlan* p, const char* what) {
    if (!counts) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    if (n <= 0) return gc::fail(GC_ERR_BAD_ARG, "%s: empty list", what);
    if (n > MAX_MAPS) return gc::fail(GC_ERR_UNSUPPORTED, "%s: %d maps, at most %d", what, n, MAX_MAPS);
    int nparts = 0, most = 0;
    for (int m = 0; m < n; ++m) {
        if (counts[m] < 2) return gc::fail(GC_ERR_BAD_ARG, "%s: map %d has %lld elements: a standard deviation needs two", what, m, (long long)counts[m]);
        if (counts[m] > INT32_MAX) return gc::fail(GC_ERR_UNSUPPORTED, "%s: map %d has more than 2^31 elements", what, m);
        const int chunks = (int)((counts[m] + CHUNK - 1) / CHUNK);
        t->count[m] = counts[m]; t->part0[m] = nparts;
        nparts += chunks;
        most = std::max(most, chunks);
    }
    t->n = n;
    p->nparts = nparts; p->max_chunks = most; p->stats = 3LL * nparts; p->total = p->stats + 2LL * n;
    return GC_OK;
}

}  // namespace

extern "C" size_t gc_noise_reg_workspace(const int32_t* sizes, const int32_t* batches, int n) {
    Table t; Plan p;
    if (make_plan(sizes, batches, n, &t, &p, "gc_noise_reg_workspace")) return 0;
    return (size_t)p.total * sizeof(float);
}

extern "C" int gc_noise_reg_fwd_f32(const float* const* maps, const int32_t* sizes, const int32_t* batches, int n, float* loss,
                                    void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    const char* what = "gc_noise_reg_fwd_f32";
    Table t; Plan p;
    if (!maps || !loss) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    int rc = make_plan(sizes, batches, n, &t, &p, what);
    if (rc) return rc;
    for (int m = 0; m < n; ++m) {
        if (!maps[m]) return gc::fail(GC_ERR_BAD_ARG, "%s: map %d is a null pointer", what, m);
        t.map[m] = const_cast<float*>(maps[m]);
    }
    if (!workspace || workspace_bytes < (size_t)p.total * sizeof(float))
        return gc::fail(GC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, (size_t)p.total * sizeof(float));
    hipStream_t s = (hipStream_t)stream;
    float* ws = static_cast<float*>(workspace);
    int blocks = 0, most = 0;
    for (int m = 0; m < n; ++m) {
        t.blk0[m] = blocks;
        const int tiles = t.size[m] / std::min(t.size[m], TILE);
        if (levels_of(t.size[m]) > 1) blocks += t.batch[m] * tiles * tiles;
        most = std::max(most, chunks_of(t.batch[m], t.size[m]));          // level 0 has the most chunks
    }
    t.blk0[n] = blocks;
    if (blocks > 0) {
        hipLaunchKernelGGL(pyramid_kernel, dim3(blocks), dim3(256), 0, s, t, ws);
        if ((rc = gc::check_launch("gc_noise_reg_fwd_f32(pyramid)"))) return rc;
    }
    hipLaunchKernelGGL(products_kernel, dim3(most, p.pairs), dim3(256), 0, s, t, ws, p.parts);
    if ((rc = gc::check_launch("gc_noise_reg_fwd_f32(products)"))) return rc;
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1024), 0, s, t, ws, p.coef, p.parts, p.pairs, loss);
    return gc::check_launch("gc_noise_reg_fwd_f32(finish)");
}

extern "C" int gc_noise_reg_bwd_f32(const float* const* maps, const int32_t* sizes, const int32_t* batches, int n, const float* gout,
                                    float* const* grads, const void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    const char* what = "gc_noise_reg_bwd_f32";
    Table t; Plan p; Pointers g;
    if (!maps || !grads || !gout) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    int rc = make_plan(sizes, batches, n, &t, &p, what);
    if (rc) return rc;
    for (int m = 0; m < n; ++m) {
        if (!maps[m] || !grads[m]) return gc::fail(GC_ERR_BAD_ARG, "%s: map or gradient %d is a null pointer", what, m);
        t.map[m] = const_cast<float*>(maps[m]);
        g.p[m] = grads[m];
    }
    if (!workspace || workspace_bytes < (size_t)p.total * sizeof(float))
        return gc::fail(GC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, (size_t)p.total * sizeof(float));
    long long blocks = 0;
    for (int m = 0; m < n; ++m) {
        t.blk0[m] = (int)blocks;
        blocks += ((long long)t.batch[m] * t.size[m] * t.size[m] + 255) / 256;
        if (blocks > INT32_MAX) return gc::fail(GC_ERR_UNSUPPORTED, "%s: more than 2^31 blocks", what);
    }
    t.blk0[n] = (int)blocks;
    hipLaunchKernelGGL(reg_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t, g, static_cast<const float*>(workspace), p.coef, gout);
    return gc::check_launch(what);
}

extern "C" size_t gc_noise_normalize_workspace(const int64_t* counts, int n) {
    NormTable t; NormPlan p;
    if (make_norm_plan(counts, n, &t, &p, "gc_noise_normalize_workspace")) return 0;
    return (size_t)p.total * sizeof(float);
}

extern "C" int gc_noise_normalize_f32(float* const* maps, const int64_t* counts, int n, void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    const char* what = "gc_noise_normalize_f32";
    NormTable t; NormPlan p;
    if (!maps) return gc::fail(GC_ERR_BAD_ARG, "%s: null pointer", what);
    int rc = make_norm_plan(counts, n, &t, &p, what);
    if (rc) return rc;
    for (int m = 0; m < n; ++m) {
        if (!maps[m]) return gc::fail(GC_ERR_BAD_ARG, "%s: map %d is a null pointer", what, m);
        t.map[m] = maps[m];
    }
    if (!workspace || workspace_bytes < (size_t)p.total * sizeof(float))
        return gc::fail(GC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, (size_t)p.total * sizeof(float));
    hipStream_t s = (hipStream_t)stream;
    float* parts = static_cast<float*>(workspace);
    float* stats = parts + p.stats;
    hipLaunchKernelGGL(norm_stats_kernel, dim3(p.max_chunks, n), dim3(256), 0, s, t, parts);
    if ((rc = gc::check_launch("gc_noise_normalize_f32(stats)"))) return rc;
    hipLaunchKernelGGL(norm_merge_kernel, dim3(1), dim3(1024), 0, s, t, static_cast<const float*>(parts), stats);
    if ((rc = gc::check_launch("gc_noise_normalize_f32(merge)"))) return rc;
    hipLaunchKernelGGL(norm_apply_kernel, dim3(p.max_chunks, n), dim3(256), 0, s, t, static_cast<const float*>(stats));
    return gc::check_launch("gc_noise_normalize_f32(apply)");
}
