// Weight gradient in split-bf16:  dW[tap][k][n] = sum_px X[k][px + tap] * dY[n][px]   (down = 1)
// The MFMA reduction index is the PIXEL, so a lane's fragment is 8 consecutive pixels of one channel.  Both
// tiles sit in LDS pixel-contiguous as 16-byte units of 8 pixels (hi and lo parts).  A horizontal tap shift of
// tx pixels is a funnel shift over two neighbouring units (4 v_perm for tx = 1, register moves for tx = 2) --
// every ds_read_b128 stays 16-byte aligned.  Each wave owns a 32k x 32n block for all taps (144 accumulators).
// (the arithmetic and the staging helpers: conv_bf16x3.hip, conv_bf16x3_shared.h)
#include "conv_common.h"
#include "conv_bf16x3_shared.h"

namespace {

using namespace gcconv;

#if defined(GC_ABL) && GC_ABL == 3      // dev ablation: no global loads in the weight-gradient staging
#define WG_LOAD(r, off, imm) make_uint4((off), (off) + 1u, (off) + 2u, (off) + 3u)
#else
#define WG_LOAD(r, off, imm) buf_load_u128(r, off, imm)
#endif
// (plain loads: the halo rows of a tile and the neighbouring pixel splits re-read the lines a non-temporal hint evicts -- DESIGN.md, "Tried and rejected")
// XCD-aware block order for the weight-gradient grids (k blocks x n blocks x pixel splits).  Workgroups go to the eight XCDs round-robin
// in linear block order, so the 8 x 8 (k, n) blocks of ONE pixel split -- which all stream the same X and dY tiles -- land on eight
// different L2s and every tile crosses the fabric eight times.  Re-deal the linear ids so that each XCD gets a contiguous range of
// (x fastest, then y, then z): the blocks that share operands then share one L2.
struct WgBlock { int x, y, z; };
template <bool XCD>
__device__ __forceinline__ WgBlock wg_block() {
  if (XCD) {
    const unsigned gx = gridDim.x, gy = gridDim.y, total = gx * gy * gridDim.z;
    unsigned l = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    if (total % 8 == 0) l = (l % 8) * (total / 8) + l / 8;
    return {(int)(l % gx), (int)((l / gx) % gy), (int)(l / (gx * gy))};
  }
    return {(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
}

struct WgArgs {
    const float* x; const float* dy; const float* si; const float* so; float* ws;
    int B, K, N, in_h, in_w, out_h, out_w, pad_y, pad_x;
    int tiles_x, tiles_y, tiles_per_split;
    int x_pitch;          // floats between the rows of x (wgrad_bf16x3_s2_kernel; in_w when dense)
    int spb;              // > 0: per-sample mode -- split z works on sample z / spb only (its tiles spb apart), so ws[z] is a partial sum of ONE sample
};

__device__ __forceinline__ uint4 shift_px(const uint4 a, const uint4 b, int tx) {
    if (tx == 0) return a;
    if (tx == 2) return make_uint4(a.y, a.z, a.w, b.x);
    return make_uint4(__builtin_amdgcn_alignbit(a.y, a.x, 16), __builtin_amdgcn_alignbit(a.z, a.y, 16),
                      __builtin_amdgcn_alignbit(a.w, a.z, 16), __builtin_amdgcn_alignbit(b.x, a.w, 16));
}

template <bool SCALED = true>
__device__ __forceinline__ void split8(const float (&v)[8], float scale, uint4* h, uint4* l) {
#if defined(GC_ABL) && GC_ABL == 2      // dev ablation: staging without the conversions
    *h = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    *l = make_uint4(__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7]));
    return;
#endif
    unsigned hh[4], ll[4];
#pragma unroll
    for (int q = 0; q < 8; q += 2) {       // pairs: see cvt_pk_bf16 (the same bits as the element-by-element `(__bf16)f` form)
        const float f0 = SCALED ? v[q] * scale : v[q], f1 = SCALED ? v[q + 1] * scale : v[q + 1];
        const unsigned pk = cvt_pk_bf16(f0, f1);
        const float t0 = __uint_as_float(pk << 16), t1 = __uint_as_float(pk & 0xffff0000u);
        float d0, d1;
        asm("v_sub_f32 %0, %1, %2" : "=v"(d0) : "v"(f0), "v"(t0));      // plain, not packed: v_pk_add_f32 stalls the matrix pipe (profiles/pmc_r01.md); +3..4 % at >= 64 channels
        asm("v_sub_f32 %0, %1, %2" : "=v"(d1) : "v"(f1), "v"(t1));
        hh[q / 2] = pk;
        ll[q / 2] = cvt_pk_bf16(d0, d1);
    }
    *h = make_uint4(hh[0], hh[1], hh[2], hh[3]);
    *l = make_uint4(ll[0], ll[1], ll[2], ll[3]);
}

template <int WK, int WN, int WP, int TR, int KS>
struct WgCfg {
    static constexpr int KT = WK * 32, NTL = WN * 32;
    static constexpr int PH = TR + KS - 1;
    static constexpr int XU = KS == 3 ? 5 : 4, YU = 4;            // 8-pixel units per patch row / dY row
    static constexpr int CSX = (PH * XU) | 1, CSY = (TR * YU) | 1;   // odd unit strides between channels: conflict-free b128 reads
    static constexpr int NXU = KT * PH * XU, NYU = NTL * TR * YU;
    static constexpr int NPX = (NXU + 255) / 256, NPY = (NYU + 255) / 256;
    static constexpr int RED_UNITS = (WP - 1) * WK * WN * 16 * 64 / 4;      // cross-wave reduction scratch (floats / 4)
    static constexpr int SMEM_UNITS = cmax(2 * (KT * CSX + NTL * CSY), RED_UNITS);
    static constexpr int NT = KS * KS;
};

template <int WK, int WN, int WP, int TR, int KS>
__global__ __launch_bounds__(256, 2) void wgrad_bf16x3_kernel(WgArgs p) {
    using C = WgCfg<WK, WN, WP, TR, KS>;
    static_assert(WK * WN * WP == 4, "4 waves per workgroup");
    static_assert((2 * TR) % WP == 0, "pixel steps split evenly over the pixel waves");
    constexpr int KT = C::KT, NTL = C::NTL, PH = C::PH, XU = C::XU, YU = C::YU, NT = C::NT;
    __shared__ uint4 smem[C::SMEM_UNITS];
    uint4* xh = smem;
    uint4* xl = xh + KT * C::CSX;
    uint4* yh = xl + KT * C::CSX;
    uint4* yl = yh + NTL * C::CSY;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wp = wave % WP, wn = (wave / WP) % WN, wk = wave / (WP * WN);
    const WgBlock blk = wg_block<false>();      // hardware order: the XCD-aware order measured no gain at stride 1 (same-box A/B within +-3 %)
    const int k0 = blk.x * KT, n0 = blk.y * NTL, split = blk.z;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int tiles_per_sample = p.tiles_x * p.tiles_y;
    const int total_tiles = tiles_per_sample * p.B;
    // Tiles run ACROSS the rows and the tiles of one split are gridDim.z apart, so the resident workgroups read a band
    // of neighbouring rows (contiguous in DRAM, halo rows shared through L2) instead of one 32-column strip each, all over the batch.
    const int sb = p.spb ? split / p.spb : 0;        // per-sample mode (gc_conv2d_wgrad_samples_*): the splits of one sample walk that sample's tiles only
    const int tstep = p.spb ? p.spb : (int)gridDim.z;
    const int t_begin = p.spb ? sb * tiles_per_sample + (split - sb * p.spb) : split;
    const int t_end = p.spb ? (sb + 1) * tiles_per_sample : total_tiles;
    const int xchan = p.in_h * p.in_w, ychan = p.out_h * p.out_w;

    // Staging is kept LEAN: with two workgroups per CU the vector ALUs (index arithmetic, masks, conversions), not the
    // matrix pipes, bound this kernel.  Everything that depends only on the lane is computed once -- the byte offset of each
    // staged unit inside a sample and a packed descriptor (LDS unit offset, patch row, unit column, channel) -- so a tile costs
    // ~6 vector instructions per unit to address and ~40 to convert.  The per-sample scales sit in an LDS table (refilled
    // when a split crosses into the next sample).
    __shared__ float s_scale[KT + NTL];
    int b_tab = -1;
    float4 xreg[C::NPX][2], yreg[C::NPY][2];
    unsigned xdesc[C::NPX], ydesc[C::NPY];       // LDS unit offset | unit column << 16 | patch row << 20 | channel << 24 | idle lane << 31
    constexpr unsigned OUTSIDE = 0x80000000u;    // beyond every buffer
#pragma unroll
    for (int j = 0; j < C::NPX; ++j) {
        const int u = tid + 256 * j;
        const int xu = u % XU, row = u / XU;
        const int r = row % PH, kk = min(row / PH, KT - 1);
        const bool live = u < C::NXU && k0 + kk < p.K;
        xdesc[j] = (unsigned)(kk * C::CSX + r * XU + xu) | (unsigned)xu << 16 | (unsigned)r << 20 | (unsigned)kk << 24 | (live ? 0u : OUTSIDE);
    }
#pragma unroll
    for (int j = 0; j < C::NPY; ++j) {
        const int u = tid + 256 * j;
        const int yu = u % YU, row = u / YU;
        const int r = row % TR, nn = min(row / TR, NTL - 1);
        const bool live = u < C::NYU && n0 + nn < p.N;
        ydesc[j] = (unsigned)(nn * C::CSY + r * YU + yu) | (unsigned)yu << 16 | (unsigned)r << 20 | (unsigned)nn << 24 | (live ? 0u : OUTSIDE);
    }
    const unsigned xbytes = (unsigned)p.K * xchan * 4u, ybytes = (unsigned)p.N * ychan * 4u;
    auto prefetch = [&](int tile) {
        const int b = tile / tiles_per_sample;
        const int rem = tile - b * tiles_per_sample;
        const int oy0 = (rem / p.tiles_x) * TR, ox0 = (rem % p.tiles_x) * 32;      // see the tile loop
#if defined(GC_ABL) && (GC_ABL == 4 || GC_ABL == 5)      // dev ablation (wrong results): the patch rows start on the tile's own 128-byte line instead of one pixel left of it
        const int iy0 = oy0 - p.pad_y, ix0 = ox0;
#else
        const int iy0 = oy0 - p.pad_y, ix0 = ox0 - p.pad_x;
#endif
        const int xoff = (k0 * xchan + iy0 * p.in_w + ix0) * 4, yoff = (n0 * ychan + oy0 * p.out_w + ox0) * 4;
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x + (size_t)b * p.K * xchan, xbytes);
        const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.dy + (size_t)b * p.N * ychan, ybytes);
#pragma unroll
        for (int j = 0; j < C::NPX; ++j) {
            // rows start at odd offsets (pad - 1, 1025-wide planes): the 16-byte loads are only 4-byte aligned, which
            // buffer_load_dwordx4 accepts; each dword is range-checked separately.  The very first unit of a sample
            // (channel 0, row 0, left halo) would start at a NEGATIVE offset, which the range check rejects as a whole:
            // it is loaded from offset 0 and patched after the commit (fix_first_unit).
            const unsigned d = (unsigned)opaque((int)xdesc[j]);       // opaque: nothing derived from the descriptor may be hoisted out of the tile loop (registers)
            const int r = (int)((d >> 20) & 15u);
            const int lin = (int)((d >> 24) & 63u) * (xchan * 4) + r * (p.in_w * 4) + (int)((d >> 16) & 15u) * 32 + xoff;
#if defined(GC_ABL) && GC_ABL == 5      // ... and the fifth (halo) unit of every row is not fetched: exactly one 128-byte line per row
            const unsigned off = ((int)d >= 0 && (unsigned)(iy0 + r) < (unsigned)p.in_h && ((d >> 16) & 15u) < 4u) ? (unsigned)max(lin, 0) : OUTSIDE;
#else
            const unsigned off = ((int)d >= 0 && (unsigned)(iy0 + r) < (unsigned)p.in_h) ? (unsigned)max(lin, 0) : OUTSIDE;
#endif
            xreg[j][0] = __builtin_bit_cast(float4, WG_LOAD(rx, off, 0));
            xreg[j][1] = __builtin_bit_cast(float4, WG_LOAD(rx, off, 16));
        }
#pragma unroll
        for (int j = 0; j < C::NPY; ++j) {
            const unsigned d = (unsigned)opaque((int)ydesc[j]);
            const int r = (int)((d >> 20) & 15u);
            const int lin = (int)((d >> 24) & 63u) * (ychan * 4) + r * (p.out_w * 4) + (int)((d >> 16) & 15u) * 32 + yoff;
            const unsigned off = ((int)d >= 0 && oy0 + r < p.out_h) ? (unsigned)lin : OUTSIDE;
            yreg[j][0] = __builtin_bit_cast(float4, WG_LOAD(ry, off, 0));
            yreg[j][1] = __builtin_bit_cast(float4, WG_LOAD(ry, off, 16));
        }
    };
    // `edge_t`: the column masks exist only in the variant that border tiles take.  (Round 5: written as a per-lane `if (unit straddles a border)`
    // the compiler predicated the masks for EVERY lane and tile -- two compares, a scalar and, a select per value: 448 of the 1 021 vector
    // instructions of the conversion phase; the tile-uniform switch in commit() makes it a scalar branch that 30 of 32 tile columns skip.)
    auto unit8 = [&](auto scaled_t, auto edge_t, const float4 (&r)[2], int col0, int width, float scale, uint4* h, uint4* l) {
        float v[8] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w};
        if (decltype(edge_t)::value) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (col0 + q >= 0 && col0 + q < width) ? v[q] : 0.f;
        }
        split8<decltype(scaled_t)::value>(v, scale, h, l);
    };
    auto commit = [&](int tile) {
        const int b = tile / tiles_per_sample;
        const int rem = tile - b * tiles_per_sample;
        const int oy0 = (rem / p.tiles_x) * TR, ox0 = (rem % p.tiles_x) * 32;
        const bool scaled = p.si != nullptr || p.so != nullptr;
        if (scaled && b != b_tab) {          // uniform: every lane of the workgroup sees the same tile
            __syncthreads();
            if (tid < KT) s_scale[tid] = p.si ? p.si[(size_t)b * p.K + min(k0 + tid, p.K - 1)] : 1.f;
            else if (tid < KT + NTL) s_scale[tid] = p.so ? p.so[(size_t)b * p.N + min(n0 + tid - KT, p.N - 1)] : 1.f;
            __syncthreads();
            b_tab = b;
        }
        wait_staged_loads();
        auto items = [&](auto scaled_t, auto edge_t) {          // without modulation (every layer of D) the multiply by one is not issued: it is packed fp32, which stalls the matrix pipe
            constexpr bool SC = decltype(scaled_t)::value;
#pragma unroll
            for (int j = 0; j < C::NPX; ++j) {
                const unsigned d = (unsigned)opaque((int)xdesc[j]);       // opaque: nothing derived from the descriptor may be hoisted out of the tile loop (registers)
                const float sc = SC ? s_scale[(d >> 24) & 63u] : 1.f;
                uint4 h, l;
                unit8(scaled_t, edge_t, xreg[j], ox0 - p.pad_x + 8 * (int)((d >> 16) & 15u), p.in_w, sc, &h, &l);      // rows / channels outside the image were loaded as zeros
                if (256 * (j + 1) <= C::NXU || tid + 256 * j < C::NXU) { xh[d & 0xffffu] = h; GC_LO(xl[d & 0xffffu] = l;) }
            }
#pragma unroll
            for (int j = 0; j < C::NPY; ++j) {
                const unsigned d = (unsigned)opaque((int)ydesc[j]);
                const float sc = SC ? s_scale[KT + ((d >> 24) & 63u)] : 1.f;
                uint4 h, l;
                unit8(scaled_t, edge_t, yreg[j], ox0 + 8 * (int)((d >> 16) & 15u), p.out_w, sc, &h, &l);
                if (256 * (j + 1) <= C::NYU || tid + 256 * j < C::NYU) { yh[d & 0xffffu] = h; GC_LO(yl[d & 0xffffu] = l;) }
            }
        };
        // tile-uniform: does any staged unit of this tile reach over the left / right image border?
        const bool edge = ox0 - p.pad_x < 0 || ox0 - p.pad_x + 8 * XU > p.in_w || ox0 + 8 * YU > p.out_w;
        if (scaled) { if (edge) items(std::true_type{}, std::true_type{}); else items(std::true_type{}, std::false_type{}); }
        else        { if (edge) items(std::false_type{}, std::true_type{}); else items(std::false_type{}, std::false_type{}); }
        // the one unit per sample that was fetched from offset 0 instead of -pad (see prefetch): channel 0, image row 0, left halo
        if (k0 == 0 && ox0 == 0 && p.pad_x > 0 && oy0 < PH && oy0 - p.pad_y <= 0) {          // uniform and rare
            __syncthreads();
            if (tid == 0) {
                const int r = p.pad_y - oy0;                 // patch row that holds image row 0
                const float* row0 = p.x + (size_t)b * p.K * xchan;
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { const int c = q - p.pad_x; v[q] = (c >= 0 && c < p.in_w) ? row0[c] : 0.f; }
                uint4 h, l;
                split8(v, scaled ? s_scale[0] : 1.f, &h, &l);
                xh[r * XU] = h; GC_LO(xl[r * XU] = l;)
            }
        }
    };

    if (t_begin < t_end) {
        prefetch(t_begin);
        commit(t_begin);
        __syncthreads();
        const int xa = (wk * 32 + l31) * C::CSX + hi, yb_ = (wn * 32 + l31) * C::CSY + hi;
        for (int tile = t_begin; tile < t_end; tile += tstep) {
            wait_staged_loads();    // no-op in hardware (commit retired them); clears the compiler's pending-load model at the loop header
            const bool more = tile + tstep < t_end;
            prefetch(more ? tile + tstep : tile);       // unconditional: a conditional prefetch merges through register copies, which wait for the loads
            __builtin_amdgcn_s_setprio(GC_MFMA_PRIO);
#pragma unroll 1
            for (int step = 0; step < 2 * TR / WP; ++step) {
                {
                    const int sidx = step * WP + wp;            // this wave's pixel step: row r, half-row st
                    const int r = sidx >> 1, st = sidx & 1;
                    const uint4 ubh = yh[yb_ + r * YU + 2 * st], ubl = yl[yb_ + r * YU + 2 * st];
                    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&ubh), bl = *reinterpret_cast<const bf16x8*>(&ubl);
#pragma unroll
                    for (int ty = 0; ty < KS; ++ty) {
                        const int o = xa + (r + ty) * XU + 2 * st;
                        const uint4 a0h = xh[o], a0l = xl[o];
                        uint4 a1h = a0h, a1l = a0l;
                        if (KS == 3) { a1h = xh[o + 1]; a1l = xl[o + 1]; }
#pragma unroll
                        for (int tx = 0; tx < KS; ++tx) {
                            const uint4 uh = shift_px(a0h, a1h, tx), ul = shift_px(a0l, a1l, tx);
                            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&uh), al = *reinterpret_cast<const bf16x8*>(&ul);
                            f32x16 c = acc[ty * KS + tx];
                            GC_MFMA3(c, ah, al, bh, bl);
                            acc[ty * KS + tx] = c;
                        }
                        if (KS == 3) __builtin_amdgcn_sched_barrier(0x100);
                    }
                }
            }
            __builtin_amdgcn_s_setprio(0);
            __syncthreads();
            if (!more) break;       // leave here: no path may reach the loop header with staged loads in flight
            {
                commit(tile + tstep);
                __syncthreads();
            }
        }
    }

    if (WP > 1) {
        // the WP pixel-waves of a (wk, wn) group hold partial sums of the same (k, n) block: add them through LDS
        float* red = reinterpret_cast<float*>(smem) + (wk * WN + wn) * (WP - 1) * 16 * 64;
        for (int t = 0; t < NT; ++t) {
            __syncthreads();
            if (wp > 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) red[((wp - 1) * 16 + r) * 64 + lane] = acc[t][r];
            }
            __syncthreads();
            if (wp == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[t][r];
                    for (int o = 0; o < WP - 1; ++o) v += red[(o * 16 + r) * 64 + lane];
                    acc[t][r] = v;
                }
            }
        }
        if (wp != 0) return;
    }

    float* out = p.ws + (size_t)split * NT * p.K * p.N;
    const int n = n0 + wn * 32 + l31;
    if (n < p.N) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0 + wk * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (k < p.K) out[((size_t)t * p.K + k) * p.N + n] = acc[t][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Wave-specialised weight gradient (round 5; 3 x 3, stride 1, K and N multiples of 64): the role split and the two-deep staging of the
// stride-1 forward kernel applied to dW.  wgrad_bf16x3_kernel alternates stage -> barrier -> multiply -> barrier with one LDS stage; two
// co-resident workgroups overlap by luck (1.45 x of one).  Here ONE workgroup of 16 waves owns a CU:
//  * 12 MULTIPLYING waves = 3 tap rows x (2 x 2) blocks of 32 k x 32 n: wave (ty, wk, wn) holds the three accumulators of taps (ty, 0..2)
//    -- 48 registers instead of 144 -- and issues nothing but LDS fragment reads, the funnel shifts of the tap columns and MFMAs;
//  * 4 STAGING waves load, split and write what the NEXT item needs while the loads of the item after next are in flight.
// The pixel space is walked in STRIPS: a strip is 32 columns x RB consecutive output rows of one sample, an ITEM is one output row of a strip.
// Item r needs X rows r - 1, r, r + 1 (tap row ty reads row r - 1 + ty) and dY row r: the X rows live in a ring of 6 row slots, so an item
// inside a strip stages ONE new X row and one dY row (the first item of a strip: three X rows) -- every input row is converted once per strip
// instead of (TR + 2) / TR times per tile, and the staging waves are idle most of an item.  One barrier per item.
// Sums are accumulated in a fixed order (strips of a split in order, rows in order, half-rows in order): bit-identical run to run; the order
// differs from wgrad_bf16x3_kernel's, so the two agree to rounding, not bit for bit.
#ifndef GC_WG_WS
#define GC_WG_WS 1          // 1: wgrad_bf16x3_ws2_kernel takes the shapes it is built for (+5..8 % over the one-role kernel); 0: one-role kernel only (same-box A/B)
#endif
#ifndef GC_WGWS_STAGER_PRIO
#define GC_WGWS_STAGER_PRIO 3      // the staging waves bound the wave-specialised kernel (its first form, kbench, B = 4: 261-278 TF/s at priority 0, 277-298 at 3): they issue first
#endif

// ---------------------------------------------------------------------------------------------------------
// The shipped form: TWO output rows per item and the input rows staged as a stream.  (A first form with one-row items measured at parity with
// wgrad_bf16x3_kernel and was not shipped: DESIGN.md, "Tried and rejected".)  The one-row form's ablations (profiles/kernel_ab_r05_{h,j}.log) say its matrix side alone runs at ~530 TF/s and that the staging waves' path --
// load latency, conversion, LDS write -- is what an item waits for: an item was 18 MFMAs per wave, ~0.7 us, and its loads were requested two
// items = ~1.5 us ahead.  Here an item is 36 MFMAs per wave (half the barriers), the loads of an item are requested two items = ~3 us ahead, and
// every staging step is exactly five unit slots per lane:
//   * X rows 2i + 2, 2i + 3 of the strip (the two new rows of item i: 640 units = 2.5 slots), dY rows 2i, 2i + 1 (512 units = 2 slots);
//   * the idle half of the third X slot carries 128 units of the NEXT strip's first two input rows (its top halo: 640 units over the steps of
//     items 2..6), so a strip boundary costs no extra step: those two rows live in two dedicated row slots (6, 7), the other rows of all strips
//     form one running sequence through a ring of six.
// Strips are 16 rows (out_h a multiple of 16).  Same partial-sum layout and reduce pass as the other weight-gradient kernels.
struct WgWs2Cfg {
    static constexpr int XRING = 6, XR = 8, YR = 4, XU = 5, YU = 4, RB = 16;
    static constexpr int CSX = (XR * XU) | 1, CSY = (YR * YU) | 1;
    static constexpr int XUNITS = 64 * CSX, YUNITS = 64 * CSY;
    static constexpr int SMEM_UNITS = 2 * (XUNITS + YUNITS);
    static constexpr int ROW_X = 64 * XU, ROW_Y = 64 * YU;
};

__global__ __launch_bounds__(1024) void wgrad_bf16x3_ws2_kernel(WgArgs p, int bands) {
    using C = WgWs2Cfg;
    constexpr int XRING = C::XRING, YR = C::YR, XU = C::XU, YU = C::YU, CSX = C::CSX, CSY = C::CSY, RB = C::RB, IPS = RB / 2;
    __shared__ uint4 smem[C::SMEM_UNITS];
    uint4* xh = smem;
    uint4* xl = xh + C::XUNITS;
    uint4* yh = xl + C::XUNITS;
    uint4* yl = yh + C::YUNITS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 64, split = blockIdx.z;

    const int strips_per_sample = p.tiles_x * bands;
    const int sb = p.spb ? split / p.spb : 0;
    const int sstep = p.spb ? p.spb : (int)gridDim.z;
    const int s_begin = p.spb ? sb * strips_per_sample + (split - sb * p.spb) : split;
    const int s_end = p.spb ? (sb + 1) * strips_per_sample : strips_per_sample * p.B;
    const int nstrips = s_begin < s_end ? (s_end - s_begin + sstep - 1) / sstep : 0;
    const int items = nstrips * IPS;
    const int xchan = p.in_h * p.in_w, ychan = p.out_h * p.out_w;

    // row slot of input row xr (0 .. RB + 1) of the strip with ordinal `ord`: the two top rows in the dedicated slots, the rest in the running ring
    auto xslot_of = [&](int ord, int xr) { return xr < 2 ? XRING + xr : (ord * RB + xr - 2) % XRING; };

    if (wave >= 12) {
        // ---------------- staging waves ----------------
        if (GC_WGWS_STAGER_PRIO) __builtin_amdgcn_s_setprio(GC_WGWS_STAGER_PRIO);
        const int st = tid - 768;
        constexpr unsigned OUTSIDE = 0x80000000u;
        const unsigned xbytes = (unsigned)p.K * xchan * 4u, ybytes = (unsigned)p.N * ychan * 4u;
        struct Strip { int sidx, b, oy0, ox0, ord; };
        auto place = [&](Strip& c) {
            c.b = c.sidx / strips_per_sample;
            const int rem = c.sidx - c.b * strips_per_sample;
            c.oy0 = (rem / p.tiles_x) * RB;
            c.ox0 = (rem % p.tiles_x) * 32;
        };
        // One X unit of (strip c, input row xr): u in [0, 320) = (channel, unit column)
        auto x_load = [&](float4 (&v)[2], float& sc, const Strip& c, int xr, int u, bool live) {
            const int ch = min(u / XU, 63), xu = u - (u / XU) * XU;
            const int b = min(c.b, p.B - 1);
            const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x + (size_t)b * p.K * xchan, xbytes);
            const int iy = c.oy0 + xr - p.pad_y;
            // (the unit at channel 0, row 0, column -pad of a sample would start at a negative offset, which the range check rejects as a whole:
            // it is loaded from offset 0 and shifted by one pixel when it is converted)
            const int lin = ((k0 + ch) * xchan + iy * p.in_w + c.ox0 - p.pad_x) * 4 + xu * 32;
            const unsigned off = (live && (unsigned)iy < (unsigned)p.in_h && c.b < p.B) ? (unsigned)max(lin, 0) : OUTSIDE;
            v[0] = __builtin_bit_cast(float4, buf_load_u128(rx, off, 0));
            v[1] = __builtin_bit_cast(float4, buf_load_u128(rx, off, 16));
            sc = p.si ? p.si[(size_t)b * p.K + k0 + ch] : 1.f;
        };
        auto x_store = [&](auto scaled_t, auto edge_t, const float4 (&r2)[2], float sc, const Strip& c, int xr, int u, bool live) {
            const int ch = min(u / XU, 63), xu = u - (u / XU) * XU;
            float v[8] = {r2[0].x, r2[0].y, r2[0].z, r2[0].w, r2[1].x, r2[1].y, r2[1].z, r2[1].w};
            if (decltype(edge_t)::value) {
                const int col0 = c.ox0 - p.pad_x + 8 * xu;
                if (col0 < 0 && k0 + ch == 0 && c.oy0 + xr - p.pad_y == 0) {
#pragma unroll
                    for (int e = 7; e > 0; --e) v[e] = v[e - 1];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (col0 + e >= 0 && col0 + e < p.in_w) ? v[e] : 0.f;
            }
            uint4 h, l;
            split8<decltype(scaled_t)::value>(v, sc, &h, &l);
            if (live) { const int o = ch * CSX + xslot_of(c.ord, xr) * XU + xu; xh[o] = h; GC_LO(xl[o] = l;) }
        };
        auto y_load = [&](float4 (&v)[2], float& sc, const Strip& c, int r, bool live) {
            const int ych = st >> 2, yu = st & 3;
            const int b = min(c.b, p.B - 1);
            const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.dy + (size_t)b * p.N * ychan, ybytes);
            const unsigned off = (live && c.b < p.B) ? (unsigned)(((n0 + ych) * ychan + (c.oy0 + r) * p.out_w + c.ox0) * 4 + yu * 32) : OUTSIDE;
            v[0] = __builtin_bit_cast(float4, buf_load_u128(ry, off, 0));
            v[1] = __builtin_bit_cast(float4, buf_load_u128(ry, off, 16));
            sc = p.so ? p.so[(size_t)b * p.N + n0 + ych] : 1.f;
        };
        auto y_store = [&](auto scaled_t, auto edge_t, const float4 (&r2)[2], float sc, const Strip& c, int r) {
            const int ych = st >> 2, yu = st & 3;
            float v[8] = {r2[0].x, r2[0].y, r2[0].z, r2[0].w, r2[1].x, r2[1].y, r2[1].z, r2[1].w};
            if (decltype(edge_t)::value) {
                const int col0 = c.ox0 + 8 * yu;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = col0 + e < p.out_w ? v[e] : 0.f;
            }
            uint4 h, l;
            split8<decltype(scaled_t)::value>(v, sc, &h, &l);
            const int o = ych * CSY + ((c.ord * RB + r) % YR) * YU + yu;
            yh[o] = h; GC_LO(yl[o] = l;)
        };
        // A step = what item i of strip c needs that is not staged yet + (steps 2..6) a fifth of the next strip's top rows.
        // Slots: 0, 1 = X units st, st + 256 of the 640 (rows 2i + 2, 2i + 3); 2 = X unit st + 512 for st < 128, else unit (i - 2) * 128 + st - 128 of
        // the next strip's rows 0, 1; 3, 4 = dY rows 2i, 2i + 1.
        struct Step { Strip c, n; int i; bool live; };       // strip, the strip after it, item
        auto step_loads = [&](float4 (&v)[5][2], float (&sc)[5], const Step& s) {
            const int u0 = opaque(st), u1 = opaque(st) + 256, u2 = opaque(st) + 512;
            x_load(v[0], sc[0], s.c, 2 * s.i + 2, u0, s.live);                       // u0 < 320: row 2i + 2
            x_load(v[1], sc[1], s.c, 2 * s.i + 2 + (u1 >= C::ROW_X ? 1 : 0), u1 >= C::ROW_X ? u1 - C::ROW_X : u1, s.live);
            if (st < 128) {
                x_load(v[2], sc[2], s.c, 2 * s.i + 3, u2 - C::ROW_X, s.live);
            } else {
                const int hu = (s.i - 2) * 128 + st - 128;                           // unit of the next strip's top rows, [0, 640)
                x_load(v[2], sc[2], s.n, hu >= C::ROW_X ? 1 : 0, hu >= C::ROW_X ? hu - C::ROW_X : hu, s.live && s.i >= 2 && s.i <= 6);
            }
            y_load(v[3], sc[3], s.c, 2 * s.i, s.live);
            y_load(v[4], sc[4], s.c, 2 * s.i + 1, s.live);
        };
        auto step_stores = [&](const float4 (&v)[5][2], const float (&sc)[5], const Step& s) {
            if (!s.live) return;
            const bool scaled = p.si != nullptr || p.so != nullptr;
            auto is_edge = [&](const Strip& c) { return c.ox0 - p.pad_x < 0 || c.ox0 - p.pad_x + 8 * XU > p.in_w || c.ox0 + 8 * YU > p.out_w; };
            const bool edge = is_edge(s.c) || is_edge(s.n);
            auto body = [&](auto scaled_t, auto edge_t) {
                const int u0 = opaque(st), u1 = opaque(st) + 256, u2 = opaque(st) + 512;
                x_store(scaled_t, edge_t, v[0], sc[0], s.c, 2 * s.i + 2, u0, true);
                x_store(scaled_t, edge_t, v[1], sc[1], s.c, 2 * s.i + 2 + (u1 >= C::ROW_X ? 1 : 0), u1 >= C::ROW_X ? u1 - C::ROW_X : u1, true);
                if (st < 128) {
                    x_store(scaled_t, edge_t, v[2], sc[2], s.c, 2 * s.i + 3, u2 - C::ROW_X, true);
                } else {
                    const int hu = (s.i - 2) * 128 + st - 128;
                    x_store(scaled_t, edge_t, v[2], sc[2], s.n, hu >= C::ROW_X ? 1 : 0, hu >= C::ROW_X ? hu - C::ROW_X : hu, s.i >= 2 && s.i <= 6 && s.n.b < p.B);
                }
                y_store(scaled_t, edge_t, v[3], sc[3], s.c, 2 * s.i);
                y_store(scaled_t, edge_t, v[4], sc[4], s.c, 2 * s.i + 1);
            };
            if (scaled) { if (edge) body(std::true_type{}, std::true_type{}); else body(std::true_type{}, std::false_type{}); }
            else        { if (edge) body(std::false_type{}, std::true_type{}); else body(std::false_type{}, std::false_type{}); }
        };
        auto next_step = [&](Step& s, int t) {           // the step after s, which is item t overall
            if (++s.i == IPS) {
                s.i = 0;
                s.c = s.n;
                s.n.sidx += sstep; ++s.n.ord; place(s.n);
                if (s.n.sidx >= s_end) s.n.b = p.B;      // no strip after the last one: its loads read as zeros, nothing of it is stored
            }
            s.live = t < items;
        };
        Step sl;                                        // cursor of the loads
        sl.c = Strip{s_begin, 0, 0, 0, 0}; place(sl.c);
        sl.n = Strip{s_begin + sstep, 0, 0, 0, 1}; place(sl.n);
        if (sl.n.sidx >= s_end) sl.n.b = p.B;
        sl.i = 0; sl.live = items > 0;
        Step sc_ = sl;                                  // cursor of the conversions
        float4 va[5][2], vb[5][2];
        float sa[5], sb5[5];
        // prologue: the first strip's top rows (nobody staged them ahead): three slots, on the spot
        if (items > 0) {
            const bool scaled = p.si != nullptr || p.so != nullptr;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int u = opaque(st) + 256 * j;
                x_load(va[j], sa[j], sl.c, u >= C::ROW_X ? 1 : 0, u >= C::ROW_X ? u - C::ROW_X : u, u < 2 * C::ROW_X);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int u = opaque(st) + 256 * j;
                if (scaled) x_store(std::true_type{}, std::true_type{}, va[j], sa[j], sl.c, u >= C::ROW_X ? 1 : 0, u >= C::ROW_X ? u - C::ROW_X : u, u < 2 * C::ROW_X);
                else        x_store(std::false_type{}, std::true_type{}, va[j], sa[j], sl.c, u >= C::ROW_X ? 1 : 0, u >= C::ROW_X ? u - C::ROW_X : u, u < 2 * C::ROW_X);
            }
        }
        // interval t: the multiplying waves work on item t; item t + 1 is converted here (its loads were issued one interval ago), item t + 2 is fetched
        step_loads(va, sa, sl); next_step(sl, 1);
        step_loads(vb, sb5, sl); next_step(sl, 2);
        step_stores(va, sa, sc_); next_step(sc_, 1);
        __syncthreads();
        for (int t = 0; t < items; t += 2) {
            step_loads(va, sa, sl); next_step(sl, t + 3);
            step_stores(vb, sb5, sc_); next_step(sc_, t + 2);
            __syncthreads();
            if (t + 1 >= items) break;
            step_loads(vb, sb5, sl); next_step(sl, t + 4);
            step_stores(va, sa, sc_); next_step(sc_, t + 3);
            __syncthreads();
        }
        return;
    }

    // ---------------- multiplying waves ----------------
    const int ty = wave >> 2, wk = (wave >> 1) & 1, wn = wave & 1;
    f32x16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int xa = (wk * 32 + l31) * CSX + hi, yb_ = (wn * 32 + l31) * CSY + hi;
    int i = 0, ord = 0;
    __syncthreads();                 // item 0 is staged
    for (int it = 0; it < items; ++it) {
        __builtin_amdgcn_s_setprio(GC_MFMA_PRIO);
        // four quarter-steps (row, half-row): the fragments of the next one are read before the MFMAs of the current one
        uint4 fbh[2], fbl[2], a0h[2], a1h[2], a0l[2], a1l[2];
        auto read_q = [&](int q, int set) {
            const int row = q >> 1, half = q & 1;
            const int yo = yb_ + ((ord * RB + 2 * i + row) % YR) * YU + 2 * half;
            const int o = xa + xslot_of(ord, 2 * i + row + ty) * XU + 2 * half;
            fbh[set] = yh[yo]; a0h[set] = xh[o]; a1h[set] = xh[o + 1];
            GC_LO(fbl[set] = yl[yo]; a0l[set] = xl[o]; a1l[set] = xl[o + 1];)
        };
        read_q(0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q + 1 < 4) read_q(q + 1, (q + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&fbh[q & 1]);
#ifndef GC_SINGLE
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&fbl[q & 1]);
#endif
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
                const uint4 uh = shift_px(a0h[q & 1], a1h[q & 1], tx);
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&uh);
#ifndef GC_SINGLE
                const uint4 ul = shift_px(a0l[q & 1], a1l[q & 1], tx);
                const bf16x8 al = *reinterpret_cast<const bf16x8*>(&ul);
#endif
                GC_MFMA3(acc[tx], ah, al, bh, bl);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
        if (++i == IPS) { i = 0; ++ord; }
        __syncthreads();             // the rows of this item may be rewritten from the next interval on; the next item is staged
    }
    float* out = p.ws + (size_t)split * 9 * p.K * p.N;
    const int n = n0 + wn * 32 + l31;
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int k = k0 + wk * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * hi;
            out[((size_t)(ty * 3 + tx) * p.K + k) * p.N + n] = acc[tx][rr];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Stride-2 variant (down = 2, pad = 0): dW[tap][k][n] = sum_px X[k][2 px + tap] * dY[n][px] -- the weight gradient
// of D's 3x3 / 1x1 stride-2 convolutions and (operands swapped) of G's transposed convolutions.  Each input row is
// staged DE-INTERLEAVED: units of 8 even columns and units of 8 odd columns, so tap tx = 0 reads an even unit,
// tx = 1 an odd unit and tx = 2 the even units funnel-shifted by one pixel -- every ds_read_b128 stays aligned.

template <int TR, int KS, int WK, int WN = 2>
struct WgS2Cfg {
    // WK = 2: 64k x 64n, one 32 x 32 block per wave; WK = 1: 32k x 64n, two pixel-waves per block; WK = 1, WN = 4 (round 6): 32k x 128n, one block per wave --
    // the X tile (at stride 2 four times the pixels of the dY tile, and de-interleaved while staged) is then shared by four output-channel blocks instead of two:
    // 29 % fewer operand bytes and conversions per MFMA than the 64k x 64n tile
    static constexpr int KT = 32 * WK, NTL = 32 * WN;
    static constexpr int PH = (TR - 1) * 2 + KS;
    static constexpr int XE = KS == 3 ? 5 : 4, XO = KS == 3 ? 4 : 0, RU = XE + XO, YU = 4;
    static constexpr int NI = XE;                                    // 16-column staging items per row
    static constexpr int CSX = (PH * RU) | 1, CSY = (TR * YU) | 1;
    static constexpr int NXI = KT * PH * NI, NYU = NTL * TR * YU;
    static constexpr int NPX = (NXI + 255) / 256, NPY = (NYU + 255) / 256;
    static constexpr int SMEM_UNITS = 2 * (KT * CSX + NTL * CSY);
    static constexpr int NT = KS * KS;
};

// Dispatched with two workgroups per CU (64 KB of LDS each): 64k x 64n tiles of ONE output row (the second workgroup hides the
// staging phases of the first; every input row is fetched 3 instead of 2.5 times, from L2 since tiles run down a column strip),
// or 32k x 64n tiles of two rows for 32..63 input channels.  A two-row 64k x 64n tile needs 110 KB -- one workgroup per CU --
// and measured 130 against 171 TFLOP/s on 64 -> 128 channels at 513^2.
template <int TR, int KS, int WK, int WN = 2>
__global__ __launch_bounds__(256, (TR == 1 || WK == 1) ? 2 : 1) void wgrad_bf16x3_s2_kernel(WgArgs p) {
    using C = WgS2Cfg<TR, KS, WK, WN>;
    static_assert(WK * WN == 4 || WK * WN == 2, "four waves: WK x WN blocks, two pixel-waves per block when there are only two blocks");
    constexpr int WP = 4 / (WK * WN);       // waves sharing a (k, n) block: they split the half-rows and are summed at the end
    constexpr int KT = C::KT, NTL = C::NTL, PH = C::PH, XE = C::XE, RU = C::RU, YU = C::YU, NI = C::NI, NT = C::NT;
    __shared__ uint4 smem[C::SMEM_UNITS];
    uint4* xh = smem;
    uint4* xl = xh + KT * C::CSX;
    uint4* yh = xl + KT * C::CSX;
    uint4* yl = yh + NTL * C::CSY;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wn = wave % WN, wk = (wave / WN) % WK, wp = wave / (WN * WK);
    const WgBlock blk = wg_block<true>();      // stride 2: +3..10 % (same-box A/B)
    const int k0 = blk.x * KT, n0 = blk.y * NTL, split = blk.z;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int tiles_per_sample = p.tiles_x * p.tiles_y;
    const int total_tiles = tiles_per_sample * p.B;
    const int sb = p.spb ? split / p.spb : 0;
    const int tstep = p.spb ? p.spb : (int)gridDim.z;
    const int t_begin = p.spb ? sb * tiles_per_sample + (split - sb * p.spb) : split;
    const int t_end = p.spb ? (sb + 1) * tiles_per_sample : total_tiles;
    const int xchan = p.in_h * p.x_pitch, ychan = p.out_h * p.out_w;
    const unsigned xbytes = (unsigned)p.K * xchan * 4u, ybytes = (unsigned)p.N * ychan * 4u;

    // Only the loaded data lives in registers between prefetch and commit: the per-sample scales sit in an LDS table
    // (refilled when a split crosses into the next sample), and every staged item has ONE packed per-lane descriptor
    // (LDS unit offset | item column << 16 | patch row << 20 | channel << 24 | idle lane << 31), made opaque per use so that
    // nothing derived from it is hoisted into registers -- with 144 accumulators the kernel otherwise spills inside the tile loop.
    __shared__ float s_scale[KT + NTL];
    int b_tab = -1;
    float4 xreg[C::NPX][4], yreg[C::NPY][2];
    constexpr unsigned OUTSIDE = 0x80000000u;    // beyond every buffer
    auto xdesc_of = [&](int u) -> unsigned {
        const int it = u % NI, row = u / NI;
        const int r = row % PH, kk = min(row / PH, KT - 1);
        const bool live = u < C::NXI && k0 + kk < p.K;
        return (unsigned)(kk * C::CSX + r * RU + it) | (unsigned)it << 16 | (unsigned)r << 20 | (unsigned)kk << 24 | (live ? 0u : OUTSIDE);
    };
    auto ydesc_of = [&](int u) -> unsigned {
        const int yu = u % YU, row = u / YU;
        const int r = row % TR, nn = min(row / TR, NTL - 1);
        const bool live = u < C::NYU && n0 + nn < p.N;
        return (unsigned)(nn * C::CSY + r * YU + yu) | (unsigned)yu << 16 | (unsigned)r << 20 | (unsigned)nn << 24 | (live ? 0u : OUTSIDE);
    };
    // 64k x 64n: the descriptors stay in registers (6 of them); 32k x 64n has two more staged items per lane and no register to
    // spare -- it rebuilds them from the lane index per use (measured: keeping them there costs scratch reloads in front of the loads)
    constexpr bool KEEP = WK * WN == 4;
    unsigned xdesc[KEEP ? C::NPX : 1], ydesc[KEEP ? C::NPY : 1];
    if (KEEP) {
#pragma unroll
        for (int j = 0; j < C::NPX; ++j) xdesc[j] = xdesc_of(tid + 256 * j);
#pragma unroll
        for (int j = 0; j < C::NPY; ++j) ydesc[j] = ydesc_of(tid + 256 * j);
    }
    auto xd = [&](int j) -> unsigned { return KEEP ? (unsigned)opaque((int)xdesc[KEEP ? j : 0]) : xdesc_of(opaque(tid) + 256 * j); };
    auto yd = [&](int j) -> unsigned { return KEEP ? (unsigned)opaque((int)ydesc[KEEP ? j : 0]) : ydesc_of(opaque(tid) + 256 * j); };
    auto prefetch = [&](int tile) {
        const int b = tile / tiles_per_sample;
        const int rem = tile - b * tiles_per_sample;
        const int oy0 = (rem / p.tiles_x) * TR, ox0 = (rem % p.tiles_x) * 32;      // as in wgrad_bf16x3_kernel
        const int iy0 = oy0 * 2, ix0 = ox0 * 2;                      // pad = 0 (checked on the host)
        const int xoff = (k0 * xchan + iy0 * p.x_pitch + ix0) * 4, yoff = (n0 * ychan + oy0 * p.out_w + ox0) * 4;
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x + (size_t)b * p.K * xchan, xbytes);
        const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.dy + (size_t)b * p.N * ychan, ybytes);
#pragma unroll
        for (int j = 0; j < C::NPX; ++j) {
            const unsigned d = xd(j);
            const int r = (int)((d >> 20) & 15u);
            const int lin = (int)((d >> 24) & 63u) * (xchan * 4) + r * (p.x_pitch * 4) + (int)((d >> 16) & 15u) * 64 + xoff;
            const unsigned off = ((int)d >= 0 && iy0 + r < p.in_h) ? (unsigned)lin : OUTSIDE;
#pragma unroll
            for (int v = 0; v < 4; ++v) xreg[j][v] = __builtin_bit_cast(float4, WG_LOAD(rx, off, 16 * v));
        }
#pragma unroll
        for (int j = 0; j < C::NPY; ++j) {
            const unsigned d = yd(j);
            const int r = (int)((d >> 20) & 15u);
            const int lin = (int)((d >> 24) & 127u) * (ychan * 4) + r * (p.out_w * 4) + (int)((d >> 16) & 15u) * 32 + yoff;      // (dY channel: bits 24..30, up to 128 per tile)
            const unsigned off = ((int)d >= 0 && oy0 + r < p.out_h) ? (unsigned)lin : OUTSIDE;
            yreg[j][0] = __builtin_bit_cast(float4, WG_LOAD(ry, off, 0));
            yreg[j][1] = __builtin_bit_cast(float4, WG_LOAD(ry, off, 16));
        }
    };
    auto commit = [&](int tile) {
        const int b = tile / tiles_per_sample;
        const int rem = tile - b * tiles_per_sample;
        const int ox0 = (rem % p.tiles_x) * 32;
        const bool scaled = p.si != nullptr || p.so != nullptr;
        if (scaled && b != b_tab) {          // uniform: every lane of the workgroup sees the same tile
            __syncthreads();
            if (tid < KT) s_scale[tid] = p.si ? p.si[(size_t)b * p.K + min(k0 + tid, p.K - 1)] : 1.f;
            else if (tid < KT + NTL) s_scale[tid] = p.so ? p.so[(size_t)b * p.N + min(n0 + tid - KT, p.N - 1)] : 1.f;
            __syncthreads();
            b_tab = b;
        }
        wait_staged_loads();
        auto items = [&](auto scaled_t, auto edge_t) {          // edge_t: the right-border masks, compiled only into the variant the last tile column takes (see wgrad_bf16x3_kernel)
            constexpr bool SC = decltype(scaled_t)::value, EDGE = decltype(edge_t)::value;
#pragma unroll
            for (int j = 0; j < C::NPX; ++j) {
                const unsigned d = xd(j);
                const int it = (int)((d >> 16) & 15u), o = (int)(d & 0xffffu);
                const int col0 = 2 * ox0 + 16 * it;          // rows / channels outside the image were loaded as zeros already
                const float sc = SC ? s_scale[(d >> 24) & 63u] : 1.f;
                const float4* q4 = xreg[j];
                const float v[16] = {q4[0].x, q4[0].y, q4[0].z, q4[0].w, q4[1].x, q4[1].y, q4[1].z, q4[1].w,
                                     q4[2].x, q4[2].y, q4[2].z, q4[2].w, q4[3].x, q4[3].y, q4[3].z, q4[3].w};
                const int room = p.in_w - col0;             // columns of this item inside the image (pad = 0: only the right border cuts)
                float ev[8], od[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { ev[q] = (!EDGE || 2 * q < room) ? v[2 * q] : 0.f; od[q] = (!EDGE || 2 * q + 1 < room) ? v[2 * q + 1] : 0.f; }
                uint4 eh, el, oh, ol;
                split8<SC>(ev, sc, &eh, &el);
                if (256 * (j + 1) <= C::NXI || tid + 256 * j < C::NXI) {
                    xh[o] = eh; GC_LO(xl[o] = el;)
                    if (KS == 3 && it < C::XO) {
                        split8<SC>(od, sc, &oh, &ol);
                        xh[o + XE] = oh; GC_LO(xl[o + XE] = ol;)
                    }
                }
                __builtin_amdgcn_sched_barrier(0);      // one item at a time: interleaving the conversions of several items costs more registers than there are
            }
#pragma unroll
            for (int j = 0; j < C::NPY; ++j) {
                const unsigned d = yd(j);
                const int col0 = ox0 + 8 * (int)((d >> 16) & 15u);
                const float sc = SC ? s_scale[KT + ((d >> 24) & 127u)] : 1.f;
                float v[8] = {yreg[j][0].x, yreg[j][0].y, yreg[j][0].z, yreg[j][0].w, yreg[j][1].x, yreg[j][1].y, yreg[j][1].z, yreg[j][1].w};
                const int room = p.out_w - col0;
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = (!EDGE || q < room) ? v[q] : 0.f;
                uint4 h, l;
                split8<SC>(v, sc, &h, &l);
                if (256 * (j + 1) <= C::NYU || tid + 256 * j < C::NYU) { yh[d & 0xffffu] = h; GC_LO(yl[d & 0xffffu] = l;) }
            }
        };
        const bool edge = 2 * ox0 + 16 * NI > p.in_w || ox0 + 8 * YU > p.out_w;      // tile-uniform (pad = 0: only the right border cuts)
        if (scaled) { if (edge) items(std::true_type{}, std::true_type{}); else items(std::true_type{}, std::false_type{}); }
        else        { if (edge) items(std::false_type{}, std::true_type{}); else items(std::false_type{}, std::false_type{}); }
    };

    if (t_begin < t_end) {
        prefetch(t_begin);
        commit(t_begin);
        __syncthreads();
        const int xa = (wk * 32 + l31) * C::CSX + hi, yb_ = (wn * 32 + l31) * C::CSY + hi;
        for (int tile = t_begin; tile < t_end; tile += tstep) {
            wait_staged_loads();    // no-op in hardware (commit retired them); clears the compiler's pending-load model at the loop header
            const bool more = tile + tstep < t_end;
            prefetch(more ? tile + tstep : tile);       // unconditional: a conditional prefetch merges through register copies, which wait for the loads
            __builtin_amdgcn_s_setprio(GC_MFMA_PRIO);
#pragma unroll ((TR == 1 || WK == 1) ? 1 : 2)
            for (int r = 0; r < TR; ++r) {
#pragma unroll ((TR == 1 || WK == 1) ? 1 : 2)
                for (int st_ = 0; st_ < 2 / WP; ++st_) {
                    const int st = WP == 2 ? wp : st_;          // two pixel-waves: each takes one half-row
                    const uint4 ubh = yh[yb_ + r * YU + 2 * st], ubl = yl[yb_ + r * YU + 2 * st];
                    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&ubh), bl = *reinterpret_cast<const bf16x8*>(&ubl);
#pragma unroll
                    for (int ty = 0; ty < KS; ++ty) {
                        const int o = xa + (2 * r + ty) * RU + 2 * st;
                        auto tap = [&](int tx, const uint4 uh, const uint4 ul) {
                            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&uh), al = *reinterpret_cast<const bf16x8*>(&ul);
                            f32x16 c = acc[ty * KS + tx];
                            GC_MFMA3(c, ah, al, bh, bl);
                            acc[ty * KS + tx] = c;
                        };
                        // tap order 0, 2, 1: the even units (and their one-pixel shift) retire before the odd unit is live --
                        // with 144 accumulators and the staged tile in registers there is no room for all three fragments at once
                        const uint4 e0h = xh[o], e0l = xl[o];
                        if (KS == 3) {
                            const uint4 e1h = xh[o + 1], e1l = xl[o + 1];
                            const uint4 sh = shift_px(e0h, e1h, 1), sl = shift_px(e0l, e1l, 1);
                            tap(0, e0h, e0l);
                            __builtin_amdgcn_sched_barrier(0x100);
                            const uint4 o0h = xh[o + XE], o0l = xl[o + XE];
                            tap(2, sh, sl);
                            __builtin_amdgcn_sched_barrier(0x100);
                            tap(1, o0h, o0l);
                            __builtin_amdgcn_sched_barrier(0x100);
                        } else {
                            tap(0, e0h, e0l);
                        }
                    }
                }
            }
            __builtin_amdgcn_s_setprio(0);
            __syncthreads();
            if (!more) break;       // leave here: no path may reach the loop header with staged loads in flight
            {
                commit(tile + tstep);
                __syncthreads();
            }
        }
    }

    if (WP == 2) {
        // the two pixel-waves of a (k, n) block hold partial sums: add them through LDS (the staging buffers are free now)
        float* red = reinterpret_cast<float*>(smem) + wn * 16 * 64;
        for (int t = 0; t < NT; ++t) {
            __syncthreads();
            if (wp == 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) red[r * 64 + lane] = acc[t][r];
            }
            __syncthreads();
            if (wp == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] += red[r * 64 + lane];
            }
        }
        if (wp != 0) return;
    }
    float* out = p.ws + (size_t)split * NT * p.K * p.N;
    const int n = n0 + wn * 32 + l31;
    if (n < p.N) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0 + wk * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (k < p.K) out[((size_t)t * p.K + k) * p.N + n] = acc[t][r];
            }
        }
    }
}

struct WgPlan { int small, ct, kt, tr, splits, tiles_per_split, tiles_x, tiles_y, bands; };      // bands > 0: wgrad_bf16x3_ws2_kernel with that many 16-row bands
#ifndef GC_WG_S2_N128
#define GC_WG_S2_N128 1      // stride-2 weight gradients with N % 128 == 0 and K % 32 == 0 (K >= 64) on 32k x 128n tiles (wgrad_bf16x3_s2_kernel<1, KS, 1, 4>); 0: 64k x 64n
#endif
#ifndef GC_WG_SPLIT_TARGET
#define GC_WG_SPLIT_TARGET 512      // workgroups a weight-gradient launch aims for (pixel splits x channel tiles)
#endif

// the shapes of the wave-specialised kernel (wgrad_bf16x3_ws2_kernel): 3 x 3 "same" convolutions with whole 64-channel blocks on both sides, rows of >= 32
// pixels, whole 16-row strips ...
inline bool ws2_shape(const gc_conv_desc* d, bool small) {
    return GC_WG_WS && d->down == 1 && d->kh == 3 && !small && d->in_ch % 64 == 0 && d->out_ch % 64 == 0 && d->pad_x == 1 && d->pad_y == 1 &&
           d->out_w >= 32 && d->out_h == d->in_h && d->out_w == d->in_w && d->out_h % 16 == 0;
}
// ... and of those the launches that leave every split at least two strips: `per` splits share a pool of `pool` strips per row band.  The bands, else 0.
inline int ws2_bands(const gc_conv_desc* d, long long pool, int per) {
    const int bands = d->out_h / 16;
    return pool * bands >= 2LL * per ? bands : 0;
}

// 64k x 64n tiles (2 rows per pixel tile) when both channel counts reach 64, else 32k x 32n tiles with the four
// waves splitting the pixel steps of a 4-row tile
WgPlan plan_wg(const gc_conv_desc* d) {
    WgPlan pl;
    pl.small = d->down == 1 && !(d->in_ch >= 64 && d->out_ch >= 64);
    pl.ct = pl.small ? 32 : 64;
    pl.kt = (d->down == 2 && d->in_ch < 64) ? 32 : pl.ct;      // stride 2 with 32..63 input channels: 32k x 64n tiles
    // (round 3: THREE rows for the 64 x 64 tiles -- 162 MFMAs per wave between barriers, 78 KB of LDS, still two workgroups per CU -- measured
    // 15-26 % SLOWER: 64 -> 64 @512^2, B = 8: 557 -> 748 us; 512 -> 512 @64^2: 470 -> 543 us: the two extra staging register sets spill 108 bytes per lane)
    pl.tr = pl.small ? 6 : 2;          // 32 x 32 channel tiles: six rows (81 MFMAs per wave between barriers, 65 KB of LDS; four rows: 923 vs 880 us at 32 -> 32 @1024^2)
    if (d->down == 2 && pl.kt == 64) pl.tr = 1;
    // round 6: 32k x 128n tiles at stride 2 where both channel counts allow it (GC_WG_S2_N128): the X tile is shared by four output-channel blocks
    if (GC_WG_S2_N128 && d->down == 2 && d->in_ch >= 64 && d->in_ch % 32 == 0 && d->out_ch % 128 == 0) { pl.kt = 32; pl.ct = 128; pl.tr = 1; }     // stride 2, 64k x 64n: one output row per tile keeps two workgroups per CU (two-row tiles need 110 KB of LDS: 130 vs 171 TFLOP/s)     // stride 2, small planes: one output row per tile, two workgroups per CU
    pl.tiles_x = gc::ceil_div(d->out_w, 32);
    pl.tiles_y = gc::ceil_div(d->out_h, pl.tr);
    const int total = pl.tiles_x * pl.tiles_y * d->batch;
    const int ctiles = gc::ceil_div(d->in_ch, pl.kt) * gc::ceil_div(d->out_ch, pl.ct);
    // one workgroup per CU is resident (512 registers per lane): two rounds -- except on the shapes wgrad_bf16x3_ws2_kernel takes: its
    // 16-wave workgroups run longer per strip and ONE full round of 256 measured 3..12 % faster at every channel count (same box, B = 2 / 4 / 8,
    // profiles/wg_ab_r05.log: 512 ch @64^2 232 -> 220 us, 256 @128^2 222 -> 209, 128 @256^2 235 -> 221, 64 @512^2 251 -> 231 at B = 4); everything else
    // is 20..50 % slower with 256
    const bool ws2 = ws2_shape(d, pl.small);
    const long long pool = (long long)pl.tiles_x * d->batch;         // every split draws on the strips of the whole batch
    int want = gc::ceil_div(GC_WG_SPLIT_TARGET, ctiles);
    if (ws2) {
        // ... provided that kernel really takes the launch with the halved split count; 512 -> 512 @32^2 at B = 2 does not, and the one-role kernel
        // with half the splits is 9 % slower
        const int half = std::max(1, std::min(gc::ceil_div(GC_WG_SPLIT_TARGET / 2, ctiles), total));
        if (ws2_bands(d, pool, gc::ceil_div(total, gc::ceil_div(total, half)))) want = half;
    }
    if (want > total) want = total;
    if (want < 1) want = 1;
    pl.tiles_per_split = gc::ceil_div(total, want);
    pl.splits = gc::ceil_div(total, pl.tiles_per_split);
    pl.bands = ws2 ? ws2_bands(d, pool, pl.splits) : 0;
    return pl;
}
}  // namespace

namespace gcconv {
inline namespace GC_ARITH {

bool wg_eligible(const gc_conv_desc* d) {
    // Narrow planes included: a 4 .. 16-pixel row fills an eighth .. half of the 32-pixel tile (the rest is masked zeros), and the
    // split-bf16 kernels are still 2-3x the fp32 MFMA path there (512 -> 512 @16^2, B = 8: 96 vs 298 us; @4^2: 48 vs 90 us).
    if (d->up != 1 || d->out_w < 4 || pointwise_thin_wgrad(d)) return false;
    if (d->down == 1) return d->in_ch >= 32 && d->out_ch >= 32 && d->pad_x >= 0 && d->pad_x <= 1;
    return d->in_ch >= 32 && d->out_ch >= 64 && d->pad_x == 0 && d->pad_y == 0;      // stride-2 kernel: 64 (or 32) k x 64 n tiles, no padding
}

}  // namespace GC_ARITH
}  // namespace gcconv

#ifdef GC_SINGLE
// the plain-bf16 build shares the workspace layout (and its query) of the split build
#define gc_conv2d_wgrad_bf16x3_f32 gc_conv2d_wgrad_bf16_f32
#define gc_conv2d_wgrad_samples_bf16x3_f32 gc_conv2d_wgrad_samples_bf16_f32
#else
extern "C" size_t gc_conv2d_wgrad_bf16x3_workspace(const gc_conv_desc* d) {
    if (!d || d->batch <= 0 || d->in_ch <= 0 || d->out_ch <= 0 || d->out_h <= 0 || d->out_w <= 0) return 0;
    size_t need = gc_conv2d_wgrad_workspace(d);
    if (wg_eligible(d)) {
        const WgPlan pl = plan_wg(d);
        need = std::max(need, (size_t)pl.splits * d->kh * d->kw * d->in_ch * d->out_ch * sizeof(float));
    }
    return need;
}
#endif

namespace {

// per-sample mode: the pixel splits of plan_wg regrouped as B x spb, every split inside one sample
WgPlan plan_wg_samples(const gc_conv_desc* d) {
    WgPlan pl = plan_wg(d);
    const int per_sample = pl.tiles_x * pl.tiles_y;
    const int ctiles = gc::ceil_div(d->in_ch, pl.kt) * gc::ceil_div(d->out_ch, pl.ct);
    int spb = gc::ceil_div(gc::ceil_div(512, ctiles), d->batch);
    spb = std::max(1, std::min(spb, per_sample));
    pl.tiles_per_split = gc::ceil_div(per_sample, spb);
    pl.splits = spb * d->batch;
    pl.bands = ws2_shape(d, pl.small) ? ws2_bands(d, pl.tiles_x, spb) : 0;        // a sample's splits share the strips of that sample
    return pl;
}

// dw_samples == nullptr: dw = the sum over the batch (gc_conv2d_wgrad_bf16x3_f32); else also dw_samples[b] = sample b's share of it
int wgrad_launch(const gc_conv_desc* d, const float* x, const float* dy, const float* in_scale, const float* out_scale, float* dw,
                 float* dw_samples, void* workspace, size_t workspace_bytes, hipStream_t s, const char* who) {
    const WgPlan pl = dw_samples ? plan_wg_samples(d) : plan_wg(d);
    const size_t count = (size_t)d->kh * d->kw * d->in_ch * d->out_ch;
    const size_t need = (size_t)pl.splits * count * sizeof(float);
    const bool direct = pl.splits == 1 && !dw_samples;
    if (!direct && (!workspace || workspace_bytes < need)) return gc::fail(GC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    WgArgs a{x, dy, in_scale, out_scale, direct ? dw : static_cast<float*>(workspace), d->batch, d->in_ch, d->out_ch,
             d->in_h, d->in_w, d->out_h, d->out_w, d->pad_y, d->pad_x, pl.tiles_x, pl.tiles_y, pl.tiles_per_split, d->in_pitch ? d->in_pitch : d->in_w,
             dw_samples ? pl.splits / d->batch : 0};
    dim3 grid(gc::ceil_div(d->in_ch, pl.kt), gc::ceil_div(d->out_ch, pl.ct), pl.splits);
    // dispatch probe (gc_conv2d_wgrad_variant_name): "<kernel<template arguments, %d = taps>>|down,k[|samples]|plan:<split plan>"; everything in front of
    // "|plan:" names the code that runs, the plan says how the pixel tiles are dealt to the splits and whether the reduce pass is skipped
    auto probe = [&](const char* kernel_fmt, int bands) {
        char kernel[64], extra[24] = "";
        snprintf(kernel, sizeof kernel, kernel_fmt, d->kh);
        if (bands) snprintf(extra, sizeof extra, ",bands=%d", bands);
        return gc::probe_name("%s|down%d,k%d%s|plan:splits=%d,tiles_per_split=%d%s%s", kernel, d->down, d->kh, dw_samples ? "|samples" : "",
                              pl.splits, pl.tiles_per_split, extra, direct ? ",direct" : "");
    };
    if (pl.bands) {
        if (gc::probing()) return probe("wgrad_bf16x3_ws2_kernel", pl.bands);
        hipLaunchKernelGGL(wgrad_bf16x3_ws2_kernel, grid, dim3(1024), 0, s, a, pl.bands);
    } else if (d->down == 2) {
        if (pl.ct == 128) {
            if (gc::probing()) return probe("wgrad_bf16x3_s2_kernel<1,%d,1,4>", 0);
            if (d->kh == 3) hipLaunchKernelGGL((wgrad_bf16x3_s2_kernel<1, 3, 1, 4>), grid, dim3(256), 0, s, a);
            else            hipLaunchKernelGGL((wgrad_bf16x3_s2_kernel<1, 1, 1, 4>), grid, dim3(256), 0, s, a);
        } else if (pl.kt == 32) {
            if (gc::probing()) return probe("wgrad_bf16x3_s2_kernel<2,%d,1>", 0);
            if (d->kh == 3) hipLaunchKernelGGL((wgrad_bf16x3_s2_kernel<2, 3, 1>), grid, dim3(256), 0, s, a);
            else            hipLaunchKernelGGL((wgrad_bf16x3_s2_kernel<2, 1, 1>), grid, dim3(256), 0, s, a);
        } else if (pl.tr == 1) {
            if (gc::probing()) return probe("wgrad_bf16x3_s2_kernel<1,%d,2>", 0);
            if (d->kh == 3) hipLaunchKernelGGL((wgrad_bf16x3_s2_kernel<1, 3, 2>), grid, dim3(256), 0, s, a);
            else            hipLaunchKernelGGL((wgrad_bf16x3_s2_kernel<1, 1, 2>), grid, dim3(256), 0, s, a);
        } else {
            return gc::fail(GC_ERR_UNSUPPORTED, "%s: no stride-2 kernel for this tile plan", who);
        }
    } else if (pl.small) {
        if (gc::probing()) return probe("wgrad_bf16x3_kernel<1,1,4,6,%d>", 0);
        if (d->kh == 3) hipLaunchKernelGGL((wgrad_bf16x3_kernel<1, 1, 4, 6, 3>), grid, dim3(256), 0, s, a);
        else            hipLaunchKernelGGL((wgrad_bf16x3_kernel<1, 1, 4, 6, 1>), grid, dim3(256), 0, s, a);
    } else {
        if (gc::probing()) return probe("wgrad_bf16x3_kernel<2,2,1,2,%d>", 0);
#if defined(GC_ABL)      // dev ablation: GC_ABL_DYNLDS=<bytes> of dynamic LDS forces one workgroup per CU
        static const int dyn = getenv("GC_ABL_DYNLDS") ? atoi(getenv("GC_ABL_DYNLDS")) : 0;
        if (dyn > 0 && d->kh == 3) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_bf16x3_kernel<2, 2, 1, 2, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
            hipLaunchKernelGGL((wgrad_bf16x3_kernel<2, 2, 1, 2, 3>), grid, dim3(256), dyn, s, a);
        } else
#endif
        if (d->kh == 3) hipLaunchKernelGGL((wgrad_bf16x3_kernel<2, 2, 1, 2, 3>), grid, dim3(256), 0, s, a);
        else            hipLaunchKernelGGL((wgrad_bf16x3_kernel<2, 2, 1, 2, 1>), grid, dim3(256), 0, s, a);
    }
    int rc = gc::check_launch(who);
    if (rc || direct) return rc;
    if (dw_samples) return launch_wgrad_reduce_samples(static_cast<const float*>(workspace), dw, dw_samples, count, d->batch, pl.splits / d->batch, s);
    return launch_wgrad_reduce(static_cast<const float*>(workspace), dw, count, pl.splits, s);
}

}  // namespace

extern "C" int gc_conv2d_wgrad_bf16x3_f32(const gc_conv_desc* d, const float* x, const float* dy,
                                          const float* in_scale, const float* out_scale, float* dw,
                                          void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    int rc = validate(d, "gc_conv2d_wgrad_bf16x3_f32", true);
    if (rc) return rc;
    if (!x || !dy || !dw) return gc::fail(GC_ERR_BAD_ARG, "gc_conv2d_wgrad_bf16x3_f32: null pointer");
    if (d->in_pitch != 0 && d->in_pitch != d->in_w && !(wg_eligible(d) && d->down == 2))
        return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_wgrad_bf16x3_f32: in_pitch %d: only the split-bf16 stride-2 kernel reads pitched rows (gc_conv2d_in_pitch_ok)", d->in_pitch);
    if (d->batch == 0 || !wg_eligible(d) || wgrad_small_eligible(d)) return gc_conv2d_wgrad_f32(d, x, dy, in_scale, out_scale, dw, workspace, workspace_bytes, stream);
    return wgrad_launch(d, x, dy, in_scale, out_scale, dw, nullptr, workspace, workspace_bytes, (hipStream_t)stream, "gc_conv2d_wgrad_bf16x3_f32");
}

#ifndef GC_SINGLE
extern "C" size_t gc_conv2d_wgrad_samples_workspace(const gc_conv_desc* d, int mode) {
    if (!d || d->batch <= 0 || d->in_ch <= 0 || d->out_ch <= 0 || d->out_h <= 0 || d->out_w <= 0 || d->kh <= 0 || d->kw <= 0) return 0;
    if (pointwise_thin_wgrad(d)) return pointwise_wgrad_workspace(d);
    if (mode == 0 || !wg_eligible(d) || d->batch > 16384) return 0;      // the splits are a grid dimension: B x spb <= 65535 with room to spare
    return (size_t)plan_wg_samples(d).splits * d->kh * d->kw * d->in_ch * d->out_ch * sizeof(float);
}
#endif

// gc_conv2d_wgrad_samples_bf16x3_f32 / _bf16_f32: the weight gradient AND each sample's share of it (header: what the shares are for)
extern "C" int gc_conv2d_wgrad_samples_bf16x3_f32(const gc_conv_desc* d, const float* x, const float* dy, const float* in_scale, const float* out_scale,
                                                  float* dw, float* dw_samples, void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    int rc = validate(d, "gc_conv2d_wgrad_samples_bf16x3_f32", true);
    if (rc) return rc;
    if (!x || !dy || !dw || !dw_samples) return gc::fail(GC_ERR_BAD_ARG, "gc_conv2d_wgrad_samples_bf16x3_f32: null pointer");
    if (d->batch == 0) return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_wgrad_samples_bf16x3_f32: empty batch");
    if (pointwise_thin_wgrad(d)) return gc_conv2d_wgrad_samples_f32(d, x, dy, in_scale, out_scale, dw, dw_samples, workspace, workspace_bytes, stream);
    if (!wg_eligible(d) || d->batch > 16384)
        return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_wgrad_samples_bf16x3_f32: shape not taken by the split-bf16 weight-gradient kernels (gc_conv2d_wgrad_samples_workspace() == 0)");
    if (d->in_pitch != 0 && d->in_pitch != d->in_w && d->down != 2)
        return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_wgrad_samples_bf16x3_f32: in_pitch %d: only the stride-2 kernel reads pitched rows", d->in_pitch);
    return wgrad_launch(d, x, dy, in_scale, out_scale, dw, dw_samples, workspace, workspace_bytes, (hipStream_t)stream, "gc_conv2d_wgrad_samples_bf16x3_f32");
}

