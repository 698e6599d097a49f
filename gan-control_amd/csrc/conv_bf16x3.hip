// K3/K4 fast path, forward unit: the generalised convolution of include/gancontrol_hip.h on the bf16 matrix cores
// with SPLIT-bf16 ("bf16x3") arithmetic:
//
//   a = a_hi + a_lo,  a_hi = bf16(a), a_lo = bf16(a - a_hi)        (16 mantissa bits kept)
//   a * b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi                    (fp32 accumulate in the MFMA)
//
// Three v_mfma_f32_32x32x16_bf16 (32 cycles, K = 16) replace eight v_mfma_f32_32x32x2_f32
// (64 cycles, K = 2): 5.3x the fp32-MFMA rate.  Measured error vs fp64 on a 512-channel 3x3 layer:
// 5e-6 relative (fp32: 3e-7, plain bf16: 3e-3) -- two orders inside the 1e-3 parity bound.
// fp32 in HBM on both sides: the split happens while staging into LDS (activations, after the
// per-sample in_scale multiply) and in a pre-pass over the weights (pack_weights_kernel).
//
// Structure mirrors conv_mfma_kernel (conv.hip): per chunk of 16 input channels the workgroup stages
// the halo'd input patch once, channel-LAST in LDS -- one 16-byte unit = 8 consecutive channels of one
// pixel = exactly one lane's MFMA B fragment, so every tap reads it with a single conflict-free
// ds_read_b128 at a shifted unit index -- plus the [tap][2][OCT] weight units (A fragments).
// Register-prefetch pipeline over chunks, compile-time geometry, phase decomposition for up = 2.
//
// This unit: the weight pack, conv_bf16x3_kernel (every role in every wave), conv_bf16x3_ws_kernel (wave-specialised, the wide stride-1
// layers), their launchers, the plan of a forward launch (plan_conv), the forward entry points and the shape queries.  The transposed
// convolution is convt_bf16x3.hip, the weight gradient wgrad_bf16x3.hip, the wave-specialised stride-2 kernel conv_s2ws.hip.
#include "conv_common.h"
#include "conv_bf16x3_shared.h"

namespace {

using namespace gcconv;


// wp[t][kg][n] = 8 x bf16 of w[t][kg*8 + q][n], q = 0..7 (zero beyond K); hi and lo parts
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w, uint4* __restrict__ wh, uint4* __restrict__ wl,
                                                           int taps, int K, int N, int kgroups) {
    const size_t total = (size_t)taps * kgroups * N;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (size_t)gridDim.x * 256) {
        const int n = (int)(u % N);
        const size_t rest = u / N;
        const int kg = (int)(rest % kgroups), t = (int)(rest / kgroups);
        bf16x8 h, l;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = kg * 8 + q;
            const float v = k < K ? w[((size_t)t * K + k) * N + n] : 0.f;
            const __bf16 hh = (__bf16)v;
            h[q] = hh;
            l[q] = (__bf16)(v - (float)hh);
        }
        wh[u] = *reinterpret_cast<uint4*>(&h);
        wl[u] = *reinterpret_cast<uint4*>(&l);
    }
}

// The same split for MANY weight tensors in one launch (gc_conv2d_pack_weights_bf16x3_grouped): a block finds its tensor in a table.
constexpr int MAXPG = 48;
struct PackGroup { const float* w; uint4* wh; uint4* wl; int taps, K, N, kgroups, first; };
struct PackGroupArgs { PackGroup g[MAXPG]; int n_groups; };

__global__ __launch_bounds__(256) void pack_weights_grouped_kernel(PackGroupArgs a) {
    int gi = 0;
#pragma unroll 1
    for (int i = 1; i < a.n_groups; ++i) gi = ((int)blockIdx.x >= a.g[i].first) ? i : gi;
    const PackGroup& G = a.g[gi];
    const size_t total = (size_t)G.taps * G.kgroups * G.N;
    const size_t u = (size_t)(blockIdx.x - G.first) * 256 + threadIdx.x;
    if (u >= total) return;
    const int n = (int)(u % G.N);
    const size_t rest = u / G.N;
    const int kg = (int)(rest % G.kgroups), t = (int)(rest / G.kgroups);
    bf16x8 h, l;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = kg * 8 + q;
        const float v = k < G.K ? G.w[((size_t)t * G.K + k) * G.N + n] : 0.f;
        const __bf16 hh = (__bf16)v;
        h[q] = hh;
        l[q] = (__bf16)(v - (float)hh);
    }
    G.wh[u] = *reinterpret_cast<uint4*>(&h);
    G.wl[u] = *reinterpret_cast<uint4*>(&l);
}

template <int WG_OC, int WG_PX, int WOC, int WPX, int UP, int DOWN, int KS, int CB = 1>
struct BCfg {
    static constexpr int OCT = WG_OC * WOC * 32;
    static constexpr int TPH = WG_PX * WPX / CB;            // tile rows (each 32-pixel MFMA column block is one row segment); CB column blocks side by side
    static constexpr int NT1 = UP == 1 ? KS : (KS + UP - 1) / UP;
    static constexpr int PH = (TPH - 1) * DOWN + NT1, PWD = (32 * CB - 1) * DOWN + NT1;
    // Column order of a patch row in LDS.  Stride 2: de-interleaved (even columns, then odd), so that lane l's fragment
    // read of column 2 l + tap is a run of consecutive 16-byte units -- row-major order spent 41 % of the LDS cycles in
    // bank conflicts there (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE), de-interleaved 15 %, kernel -3 %.  Stride 1 stays
    // row-major: its reads are conflict-free, and none of the de-interleaved variants measured (by 2 / by 4, pitches
    // 17..20 / 9..12) moved the kernel time by more than the noise although they change the conflict count by 2.4x:
    // the LDS is not what bounds that kernel.  Column c sits at unit (c % DI) * Q + c / DI.
    static constexpr int DI = DOWN == 1 ? 1 : 2;
    static constexpr int Q = DOWN == 1 ? PWD : (PWD + 1) / 2;
    static constexpr int RP = DI * Q;                       // row pitch in units
    static constexpr int PLANE = PH * RP;                   // units per channel group
    __device__ static __forceinline__ int ucol(int c) { return (c % DI) * Q + c / DI; }
    static constexpr int WUNITS = NT1 * NT1 * KG * OCT;     // weight units per chunk (per hi / lo)
    static constexpr int PUNITS = KG * PLANE;
    static constexpr int SMEM_UNITS = 2 * (WUNITS + PUNITS);
    static constexpr int NWU = (WUNITS + 255) / 256;        // weight units prefetched per thread (x2: hi, lo)
    // Patch staging.  The texture-address unit spends ~16 cycles per wave-level load whatever its width, and at <= 64 input
    // channels that -- not HBM, not the MFMAs -- bounds the kernel (measured: 37 % of a pipeline step issuing dword loads,
    // 30 % waiting for them).  So a lane fetches FOUR consecutive pixels of a channel with one 16-byte load, eight channels
    // = eight loads, and transposes them in registers into four channel-last units: 4x fewer load instructions.
    // A patch row starts `lead` floats before a 128-byte boundary (lead = pad for 32-pixel tiles): its SEG_M aligned 32-float
    // segments are cut into 16-byte groups ("main" tasks, all four pixels used), the EDGE columns left and right of them
    // are "edge" tasks (same load, first pixel used).  Out-of-range dwords of a buffer load read as zero one by one
    // (tools/micro/buf_oob.hip), so a group may straddle the end of the tensor; pixels past the end of an image ROW are
    // masked at commit.
    static constexpr int SEG_M = PWD % 32 == 0 ? PWD / 32 : (PWD - 1) / 32;
    static constexpr int EDGE = PWD - 32 * SEG_M;
    static constexpr int MAIN_T = PH * 8 * SEG_M, EDGE_T = PH * EDGE, TASKS = MAIN_T + EDGE_T;   // per 8-channel group
    static constexpr int NT = (TASKS + 127) / 128;          // tasks per thread (128 threads per channel group)
    struct Task { int row, col, used; };                    // patch row, first patch column, pixels used (0: no task)
    __device__ static __forceinline__ Task task_of(int t, int lead) {
        Task k;
        if (t < MAIN_T) { k.row = t / (8 * SEG_M); k.col = lead + 4 * (t % (8 * SEG_M)); k.used = 4; return k; }
        const int e = t - MAIN_T, ce = e % cmax(EDGE, 1);
        k.row = e / cmax(EDGE, 1);
        k.col = ce < lead ? ce : 32 * SEG_M + ce;
        k.used = t < TASKS ? 1 : 0;
        return k;
    }
};

template <int WG_OC, int WG_PX, int WOC, int WPX, int UP, int DOWN, int KS>
__global__ __launch_bounds__(256, 2) void conv_bf16x3_kernel(Bf16Args a) {
    using C = BCfg<WG_OC, WG_PX, WOC, WPX, UP, DOWN, KS>;
    static_assert(WG_OC * WG_PX == 4, "4 waves per workgroup");
    constexpr int OCT = C::OCT, TPH = C::TPH, PWD = C::PWD, PLANE = C::PLANE;
    const ConvArgs& p = a.c;
    __shared__ uint4 smem[C::SMEM_UNITS];
    uint4* wl_h = smem;                         // [tap][kg][OCT]
    uint4* wl_l = wl_h + C::WUNITS;
    uint4* p_h = wl_l + C::WUNITS;              // [kg][PH][PWD]
    uint4* p_l = p_h + C::PUNITS;
    __shared__ __attribute__((aligned(16))) float s_si[MAX_K_BF16X3 + KCB];     // in_scale of this sample, zero-padded past K
    // out_scale and bias of this workgroup's channels.  They must NOT be fetched between the stores of the epilogue: a
    // vector load there forces s_waitcnt vmcnt(0), which also waits for every store issued before it -- one full memory
    // round trip per output row.
    __shared__ __attribute__((aligned(16))) float s_so[OCT], s_bias[OCT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wave_px = wave % WG_PX, wave_oc = wave / WG_PX;
    const int wave_oc_u = __builtin_amdgcn_readfirstlane(wave_oc);

    // A workgroup owns `tpb` consecutive pixel tiles of one (sample, phase, oc-block) and runs ONE software pipeline over all
    // their channel chunks: the first chunk of the next tile is in flight during the last MFMA phase and the stores of the
    // current tile, so neither the cold-start load latency nor the store drain is paid per tile (they dominate at K <= 64).
    int bid = blockIdx.x;
    const int grp = bid % a.groups; bid /= a.groups;
    const int phase = bid % (UP * UP);
    const int b = bid / (UP * UP);
    const int phy = phase / UP, phx = phase % UP;
    const int n0 = blockIdx.y * OCT, n0_blk = n0;
    const int qh = (p.out_h - phy + UP - 1) / UP, qw = (p.out_w - phx + UP - 1) / UP;
    // (consecutive tiles; tiles `groups` apart as in the wave-specialised kernel measured neutral here: DESIGN.md, "Tried and rejected")
    const int tstep = 1;
    const int tile_begin = grp * a.tpb;
    const int tile_end = min(p.tiles_x * p.tiles_y, tile_begin + a.tpb);
    const int kz0 = a.k_per_split ? (int)blockIdx.z * a.k_per_split : 0;
    const int kz1 = a.k_per_split ? min(p.K, kz0 + a.k_per_split) : p.K;
    if (UP > 1) {      // tpb == 1; phases other than 0 have a smaller sub-grid
        if ((tile_begin / p.tiles_x) * TPH >= qh || (tile_begin % p.tiles_x) * 32 >= qw) return;
    }

    const AxisTaps ay = axis_taps<UP, KS>(phy, p.pad_y), ax = axis_taps<UP, KS>(phx, p.pad_x);
    const int ntaps = ay.n * ax.n;
    // patch rows start at 32 * DOWN * tile_x + ax.d0: `lead` floats before an aligned 32-float segment
    const int lead = gc::pos_mod(-ax.d0, 32);      // <= C::EDGE (checked on the host)

    f32x16 acc[WOC][WPX];
#pragma unroll
    for (int i = 0; i < WOC; ++i)
#pragma unroll
        for (int j = 0; j < WPX; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    int boff[WPX];
#pragma unroll
    for (int j = 0; j < WPX; ++j) boff[j] = hi * PLANE + (wave_px * WPX + j) * DOWN * C::RP;      // row of this lane's pixels (tap row 0)

    const int aoff = hi * OCT + wave_oc * WOC * 32 + l31;

    const float* xb = p.x + (size_t)b * p.K * p.in_h * a.in_pitch;
    const float* sib = p.si ? p.si + (size_t)b * p.K : nullptr;
    const int chan = p.in_h * a.in_pitch;          // a.in_pitch floats between input rows (the pitched output of a Blur; in_w when dense)

    uint4 wreg_h[C::NWU], wreg_l[C::NWU];
    uint4 preg[C::NT][8];                       // [task][channel] = 4 consecutive pixels

    // Buffer-descriptor loads: scalar channel offset + 32-bit lane offset, hardware zero-fill outside the image, and
    // nothing touches the results until commit(), so every load stays in flight across the MFMA block.
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(xb, (unsigned)p.K * chan * 4u);
    const unsigned wbytes = (unsigned)(KS * KS) * a.kgroups * p.N * 16u;
    const __amdgpu_buffer_rsrc_t rwh = make_rsrc(a.wh, wbytes), rwl = make_rsrc(a.wl, wbytes);
    auto prefetch = [&](int tile, int k0) {
        const int t_ = tid;
        const int iy0 = (tile / p.tiles_x) * TPH * DOWN + ay.d0, ix0 = (tile % p.tiles_x) * 32 * DOWN + ax.d0;
        // weights: unit u -> (tap, kg, oc); plain 16-byte copies of the pre-split slab
#pragma unroll
        for (int j = 0; j < C::NWU; ++j) {
            const int u = t_ + 256 * j;
            const int oc = u % OCT, rest = u / OCT;
            const int kgl = rest % KG, t = rest / KG;
            const int jy = UP == 1 ? t / KS : (ax.n == 2 ? t >> 1 : t), jx = UP == 1 ? t % KS : (ax.n == 2 ? t & 1 : 0);
            const int tap = (ay.t0 + jy * UP) * KS + ax.t0 + jx * UP;
            const int kg = k0 / 8 + kgl, n = n0 + oc;
            const bool ok = u < C::WUNITS && t < ntaps && kg < a.kgroups && n < p.N;
            const unsigned gb = ok ? (unsigned)((tap * a.kgroups + kg) * p.N + n) * 16u : OOB;
            wreg_h[j] = buf_load_u128(rwh, gb, 0);
            wreg_l[j] = buf_load_u128(rwl, gb, 0);
        }
        // patch: waves 0,1 take channel group 0, waves 2,3 group 1
        const int kgl = __builtin_amdgcn_readfirstlane(t_ >> 7), tb = t_ & 127;
#pragma unroll
        for (int j = 0; j < C::NT; ++j) {
            const typename C::Task tk = C::task_of(tb + 128 * j, lead);
            const int iy = iy0 + tk.row, ix = ix0 + tk.col;
            const bool ok = tk.used > 0 && iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w;
            const unsigned boff = ok ? (unsigned)(iy * a.in_pitch + ix) * 4u : OOB;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k = min(k0 + kgl * 8 + q, p.K - 1);          // wave-uniform -> scalar offset
                if (!(DOWN == 2 && GC_S2_ABL == 2)) preg[j][q] = buf_load_u128(rx, boff, (unsigned)k * chan * 4u);
            }
        }
    };
    auto commit = [&](int tile, int k0) {
        const int t_ = tid;
#pragma unroll
        for (int j = 0; j < C::NWU; ++j) {
            const int u = t_ + 256 * j;
            if (u < C::WUNITS) { wl_h[u] = wreg_h[j]; GC_LO(wl_l[u] = wreg_l[j];) }
        }
        const int kgl = __builtin_amdgcn_readfirstlane(t_ >> 7), tb = t_ & 127;
        const int ix0 = (tile % p.tiles_x) * 32 * DOWN + ax.d0;
        // per-sample input scales of this chunk (zero beyond K: a ragged last chunk contributes nothing)
        const float4 sa = *reinterpret_cast<const float4*>(&s_si[k0 + kgl * 8]), sb = *reinterpret_cast<const float4*>(&s_si[k0 + kgl * 8 + 4]);
        const float sc[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
        // 16-byte groups start at multiples of four pixels (ix0 + lead is a multiple of 32), so in a row whose width is a multiple of
        // four a group lies entirely inside the image or entirely outside (and was then fetched as zeros): the per-pixel row-end mask --
        // 32 selects per chunk -- is only needed for the odd widths (the 1025-wide planes of the stride-2 convolutions).
        const bool ragged_rows = ((p.in_w & 3) != 0 || a.in_pitch != p.in_w) && ix0 + lead + 32 * C::SEG_M + 4 > p.in_w;      // ... and there only in the tiles that reach the row end
        auto convert = [&](auto masked, auto scaled) {
#pragma unroll
            for (int j = 0; j < C::NT; ++j) {
                const typename C::Task tk = C::task_of(tb + 128 * j, lead);
                const int inrow = p.in_w - (ix0 + tk.col);               // pixels of this group that are still inside the image row
                const int rbase = kgl * PLANE + tk.row * C::RP;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const unsigned raw = i == 0 ? preg[j][q].x : (i == 1 ? preg[j][q].y : (i == 2 ? preg[j][q].z : preg[j][q].w));
                        v[q] = (!decltype(masked)::value || i < inrow) ? __uint_as_float(raw) : 0.f;
                    }
                    uint4 h, l;
                    split8s<decltype(scaled)::value>(v, sc, &h, &l);        // plain (un-packed) multiplies and subtractions: see split8s
                    if (i < tk.used) {
                        const int u = rbase + C::ucol(tk.col + i);
                        p_h[u] = h;
                        GC_LO(p_l[u] = l;)
                    }
                }
            }
        };
        if (DOWN == 2 && GC_S2_ABL == 1) {
            // the 8 x 16 bytes of a task are 4 hi + 4 lo units' worth: stored without touching them
#pragma unroll
            for (int j = 0; j < C::NT; ++j) {
                const typename C::Task tk = C::task_of(tb + 128 * j, lead);
                const int rbase = kgl * PLANE + tk.row * C::RP;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < tk.used) { const int u = rbase + C::ucol(tk.col + i); p_h[u] = preg[j][i]; p_l[u] = preg[j][4 + i]; }
            }
        } else if (DOWN == 2 && GC_S2_ABL == 2) {
        } else if (p.si) {      // without modulation (every layer of D) the multiply by one is not issued
            if (ragged_rows) convert(std::true_type{}, std::true_type{}); else convert(std::false_type{}, std::true_type{});
        } else {
            if (ragged_rows) convert(std::true_type{}, std::false_type{}); else convert(std::false_type{}, std::false_type{});
        }
    };
    auto mfma_phase = [&]() {
        if constexpr (UP == 1) {
            // Fragment double buffer, as in the wave-specialised kernel: the LDS reads of tap t + 1 are issued BEFORE the MFMAs of tap t (the
            // scheduling barriers pin that order).  Left alone the compiler issues a tap's reads and waits for them on the spot -- the
            // disassembly of the stride-2 variant showed `ds_read x4, s_waitcnt lgkmcnt, v_mfma` with one or two MFMAs between two waits.
            bf16x8 fa[2][2 * WOC], fb[2][2 * WPX];
            auto load_tap = [&](int t, int set) {
                const int jy = t / KS, jx = t % KS;
                const int wbase = t * KG * OCT + aoff;
                const int pbase = jy * C::RP + C::ucol(l31 * DOWN + jx);
#pragma unroll
                for (int i = 0; i < WOC; ++i) {
                    const uint4 uh = wl_h[wbase + i * 32];
                    fa[set][i] = *reinterpret_cast<const bf16x8*>(&uh);
                    GC_LO(const uint4 ul = wl_l[wbase + i * 32]; fa[set][WOC + i] = *reinterpret_cast<const bf16x8*>(&ul);)
                }
#pragma unroll
                for (int j = 0; j < WPX; ++j) {
                    const uint4 uh = p_h[pbase + boff[j]];
                    fb[set][j] = *reinterpret_cast<const bf16x8*>(&uh);
                    GC_LO(const uint4 ul = p_l[pbase + boff[j]]; fb[set][WPX + j] = *reinterpret_cast<const bf16x8*>(&ul);)
                }
            };
            load_tap(0, 0);
#pragma unroll
            for (int t = 0; t < KS * KS; ++t) {
                if (t + 1 < KS * KS) load_tap(t + 1, (t + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < WOC; ++i)
#pragma unroll
                    for (int j = 0; j < WPX; ++j) { GC_MFMA3(acc[i][j], fa[t & 1][i], fa[t & 1][WOC + i], fb[t & 1][j], fb[t & 1][WPX + j]); }
                __builtin_amdgcn_sched_barrier(0);
            }
            return;
        }
        const int nty = UP == 1 ? KS : ay.n, ntx = UP == 1 ? KS : ax.n;
        for (int jy = 0; jy < nty; ++jy) {
            for (int jx = 0; jx < ntx; ++jx) {
                const int wbase = (jy * ntx + jx) * KG * OCT + aoff;
                const int pbase = jy * C::RP + C::ucol(l31 * DOWN + jx);      // LDS column of this lane's pixel under tap jx
                bf16x8 ah[WOC], al[WOC], bh[WPX], bl[WPX];
#pragma unroll
                for (int i = 0; i < WOC; ++i) {
                    const uint4 uh = wl_h[wbase + i * 32], ul = wl_l[wbase + i * 32];
                    ah[i] = *reinterpret_cast<const bf16x8*>(&uh);
                    al[i] = *reinterpret_cast<const bf16x8*>(&ul);
                }
#pragma unroll
                for (int j = 0; j < WPX; ++j) {
                    const uint4 uh = p_h[pbase + boff[j]], ul = p_l[pbase + boff[j]];
                    bh[j] = *reinterpret_cast<const bf16x8*>(&uh);
                    bl[j] = *reinterpret_cast<const bf16x8*>(&ul);
                }
#pragma unroll
                for (int i = 0; i < WOC; ++i)
#pragma unroll
                    for (int j = 0; j < WPX; ++j) { GC_MFMA3(acc[i][j], ah[i], al[i], bh[j], bl[j]); }
            }
        }
    };
    const float* sob = p.so ? p.so + (size_t)b * p.N : nullptr;
    // Output through a buffer descriptor as well: lane offset = pixel (+ the hi half's 4 channels), scalar offset = channel
    // plane; channels >= N and pixels outside the plane fall beyond num_records and are dropped by the hardware.
    const unsigned oplane = (unsigned)(p.out_h * p.out_w) * 4u;
    float* const ybase = a.k_per_split ? a.part + (size_t)blockIdx.z * a.per_slice : p.y;
    const __amdgpu_buffer_rsrc_t ry = make_rsrc(ybase + (size_t)b * p.N * p.out_h * p.out_w, (unsigned)p.N * oplane);
    // store one finished tile (demodulation + fused epilogue) and clear the accumulators for the next
    const EpilogueConsts ec = epilogue_consts(p);
    const __amdgpu_buffer_rsrc_t rres = make_rsrc(p.residual ? p.residual + (size_t)b * p.N * p.out_h * p.out_w : p.y, p.residual ? (unsigned)p.N * oplane : 0u);
    auto finish_tile = [&](int tile) {
        const int qy0 = (tile / p.tiles_x) * TPH, qx0 = (tile % p.tiles_x) * 32;
        const int n0 = opaque_s(n0_blk);          // recompute the channel offsets here rather than carry 64 of them across the loop
#pragma unroll
        for (int j = 0; j < WPX; ++j) {
            const int qy = qy0 + wave_px * WPX + j, qx = qx0 + l31;
            const int oy = qy * UP + phy, ox = qx * UP + phx;
            const bool inside = qy < qh && qx < qw;
            const unsigned voff = inside ? (unsigned)(oy * p.out_w + ox) * 4u + (unsigned)(4 * hi) * oplane : OOB;
            const float nz = (p.noise && inside) ? p.noise[((size_t)b * p.out_h + oy) * p.out_w + ox] : 0.f;
            float res[WOC][16];
            if (p.residual) {       // all residual values of this pixel row are fetched before its first store (a load between stores waits for them)
#pragma unroll
                for (int i = 0; i < WOC; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        res[i][r] = buf_load_f32(rres, voff, (unsigned)(n0 + (wave_oc_u * WOC + i) * 32 + (r & 3) + 8 * (r >> 2)) * oplane);
            }
#pragma unroll
            for (int i = 0; i < WOC; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // a register row holds channel ocs in lanes 0..31 and ocs + 4 in lanes 32..63
                    const int ocl = (wave_oc * WOC + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const int ocs = n0 + (wave_oc_u * WOC + i) * 32 + (r & 3) + 8 * (r >> 2);
                    float v = conv_epilogue(ec, acc[i][j][r], s_so[ocl], s_bias[ocl], nz);
                    if (p.residual) v += res[i][r];
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), ry, (int)voff, (int)((unsigned)ocs * oplane), GC_CONV_ST_AUX);
                    acc[i][j][r] = 0.f;
                }
            }
        }
    };

    if (ntaps == 0) {       // a phase no tap reaches: zeros (+ epilogue)
        for (int tile = tile_begin; tile < tile_end; tile += tstep) finish_tile(tile);
        return;
    }
    const int nchunks = (kz1 - kz0 + KCB - 1) / KCB;
    const int items = (tile_end - tile_begin + tstep - 1) / tstep * nchunks;
    int tile_n = tile_begin, k0_n = kz0;      // cursor of the staging side (prefetch / commit)
    int tile_c = tile_begin, k0_c = kz0;      // cursor of the compute side (MFMA / stores)
    prefetch(tile_n, k0_n);
    for (int k = tid; k < ((p.K + KCB - 1) / KCB) * KCB; k += 256) s_si[k] = k < p.K ? (sib ? sib[k] : 1.f) : 0.f;
    if (tid < OCT) {
        const int oc = min(n0 + tid, p.N - 1);
        s_so[tid] = sob ? sob[oc] : 1.f;
        s_bias[tid] = p.bias ? p.bias[oc] : 0.f;
    }
    __syncthreads();
    commit(tile_n, k0_n);
    k0_n += KCB; if (k0_n >= kz1) { k0_n = kz0; tile_n += tstep; }
    __syncthreads();
    // Steady state.  Every step is unconditional, so no control-flow path reaches the loop header with staged loads
    // in flight and the compiler plants no wait inside the next prefetch; the last item is peeled below.
    for (int it = 1; it < items; ++it) {
        prefetch(tile_n, k0_n);
        __builtin_amdgcn_s_setprio(GC_MFMA_PRIO);
        mfma_phase();
        __builtin_amdgcn_s_setprio(0);
        __syncthreads();
        commit(tile_n, k0_n);                               // retires the loads first: no store is outstanding yet
        k0_n += KCB; if (k0_n >= kz1) { k0_n = kz0; tile_n += tstep; }
        if (k0_c + KCB >= kz1) finish_tile(tile_c);         // stores drain while the next MFMA phase runs
        k0_c += KCB; if (k0_c >= kz1) { k0_c = kz0; tile_c += tstep; }
        __syncthreads();
    }
    mfma_phase();
    finish_tile(tile_c);
}

// ---------------------------------------------------------------------------------------------------------
// Wave-specialised variant of conv_bf16x3_kernel for the wide layers (up = down = 1, K a multiple of 16, N a multiple of 64):
// ONE workgroup of 12 waves per CU -- eight MULTIPLYING waves (two per SIMD; each owns 64 oc x 2 rows x 32 px of a
// 64 oc x 16 rows x 32 px tile and issues nothing but LDS fragment reads and MFMAs) and four STAGING waves (one per SIMD:
// global loads, the per-sample scale, the hi / lo split and the LDS writes of the NEXT 16-channel chunk) -- over two LDS stages
// with one barrier per chunk.  In conv_bf16x3_kernel every wave alternates between the two jobs and the matrix pipes only stay
// busy while the co-resident workgroup happens to be in the other phase (matrix pipes busy 51 %, 21 % of the wave time at the two
// barriers per chunk, profiles/pmc_r01.md); here the multiplying waves never convert and never wait for a load.
//  * The pre-split weight slab goes HBM -> LDS by LDS-DMA (global_load_lds_dwordx4: a [tap][kg] row of 64 oc units is 1 KiB,
//    contiguous on both sides = one wave-level instruction): no registers, no ds_write, no vector ALU work for 63 % of the staged bytes.
//  * A 16-row tile halves the weight staging and the halo rows (18 / 16 instead of 10 / 8) per MFMA.
//  * Ordering of the LDS-DMA data: the staging wave waits vmcnt(0) before the barrier, the multiplying waves read the stage after it;
//    a stage is rewritten one full item after its last read (the barrier in between retires the reads).
// EPK: 0 = the full fused epilogue; 1 = out_scale and / or residual only (the input-gradient launches: G's modulated layers, D's ResBlock
// convolutions); 2 = nothing to apply.  Compile-time: the epilogue runs on the MULTIPLYING waves (6 vector instructions + 2 LDS reads per output
// element in its full form, 384 per lane and tile, both waves of a SIMD at the same moment) next to only 108 MFMAs per tile at 32 input channels.
// RES: the launch adds a residual (gc_conv_epilogue.residual).  Compile-time as well: the residual form keeps 64 loads in flight next to the
// accumulators, and as a run-time branch of the SAME kernel its register pressure spilled values that live across the whole kernel (34 VGPRs,
// a -9 .. -20 % on the 64-channel layers WITHOUT a residual, same-box A/B profiles/kernel_ab_r05_b.log).
#ifndef GC_WS_TRACE
#define GC_WS_TRACE 0        // dev instrumentation (tools/ws_trace.py): workgroup 0 records s_memtime at the phase boundaries of its first items -- one multiplying and one staging wave
#endif
#if GC_WS_TRACE
__device__ unsigned long long gc_ws_trace[2][512];      // [role][event]: (tag << 56) | time
#define GC_TR(role, tag) do { if (tr_on && tr_n[role] < 512) { gc_ws_trace[role][tr_n[role]++] = ((unsigned long long)(tag) << 56) | (__builtin_amdgcn_s_memtime() & 0x00ffffffffffffffull); } } while (0)
#else
#define GC_TR(role, tag) do { } while (0)
#endif
template <int KS, int WOC, int CB, int EPK = 0, bool RES = false>
__global__ __launch_bounds__(768) void conv_bf16x3_ws_kernel(Bf16Args a) {
    using C = BCfg<1, 8, WOC, 2, 1, 1, KS, CB>;      // CB = 1: 16 rows x 32 px tiles; CB = 2: 8 rows x 64 px (longer contiguous runs per row: the HBM-bound layers)
    constexpr int OCT = 32 * WOC, TPH = C::TPH, PLANE = C::PLANE, WPX = 2, NTAP = KS * KS;
    constexpr int STAGE = C::SMEM_UNITS;                 // one stage: [weights hi | weights lo | patch hi | patch lo]
    static_assert(C::OCT == OCT && C::TPH * CB == 16, "(32 | 64) oc x 512 px tiles");
    static_assert(2 * STAGE * 16 + (MAX_K_BF16X3 + KCB + 2 * OCT) * 4 <= 160 * 1024, "two stages fit the 160 KiB of LDS");
    const ConvArgs& p = a.c;
    __shared__ uint4 smem[2 * STAGE];
    __shared__ __attribute__((aligned(16))) float s_si[MAX_K_BF16X3 + KCB];
    __shared__ __attribute__((aligned(16))) float s_so[OCT], s_bias[OCT];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;

#if GC_WS_TRACE
    const bool tr_on = blockIdx.x == GC_WS_TRACE - 1 && blockIdx.y == 0 && (threadIdx.x == 0 || threadIdx.x == 512);
    int tr_n[2] = {0, 0};
#endif
    const int bid = blockIdx.x, boc = blockIdx.y;
    const int grp = bid % a.groups;
    const int b = bid / a.groups;
    const int n0 = boc * OCT;
    // The tiles of a workgroup are `groups` apart: at any moment the 256 resident workgroups then work on ~256
    // NEIGHBOURING tiles -- a band of rows of one sample, contiguous per channel in DRAM -- instead of 256 bands spread over the batch.
    const int tiles_all = p.tiles_x * p.tiles_y;
    const int tstep = a.groups;
    const int tile_begin = grp;
    const int ntiles = (tiles_all - grp + a.groups - 1) / a.groups;
    const int nchunks = p.K / KCB;
    const int items = ntiles * nchunks;
    const int chan = p.in_h * p.in_w;

    for (int k = tid; k < p.K; k += 768) s_si[k] = p.si ? p.si[(size_t)b * p.K + k] : 1.f;
    if (tid < OCT) {
        const int oc = n0 + tid;
        s_so[tid] = p.so ? p.so[(size_t)b * p.N + oc] : 1.f;
        s_bias[tid] = p.bias ? p.bias[oc] : 0.f;
    }
    __syncthreads();

    // The weight slab of the NEXT item: rows (half, tap, kg) of 64 units, one LDS-DMA instruction each, dealt round-robin to the eight
    // multiplying waves (4 or 5 each).  The instruction is issued from an asm statement: the
    // compiler-tracked builtin makes every later LDS read of the wave (the fragment reads of THIS item) wait for the DMA first, which
    // puts its latency at the head of each MFMA phase.  Untracked, its completion is counted by hand (see the multiplying waves' loop).
    // (Who issues the slab -- all eight waves, one per SIMD, the staging waves -- and where in the item measured neutral or slower:
    //  DESIGN.md, "Tried and rejected".)
#ifdef GC_SINGLE
    constexpr int ROWS = NTAP * KG;
#else
    constexpr int ROWS = 2 * NTAP * KG;
#endif
    // one instruction moves 64 units = 64 / OCT consecutive rows (rows are adjacent in LDS; the halves hold an even number of rows)
    constexpr int RPI = 64 / OCT, INSTR = ROWS / RPI;
    static_assert(ROWS % RPI == 0 && (NTAP * KG) % RPI == 0, "row groups do not straddle the hi / lo halves");
    // (`dma_wave` and `dma_mine` say nothing new -- every multiplying wave issues its share -- but the generated code follows them: without either
    //  some instances come out with another register allocation, and this kernel's code is pinned instruction by instruction
    //  -- profiles/isa_identity_knob_retirement.md)
    const int dma_wave = wave;
    const bool dma_mine = wave < 8;          // (wave-uniform)
    auto weights = [&](int k0, int buf) {
        if (!dma_mine) return;
        uint4* const base = smem + buf * STAGE;
#pragma unroll
        for (int j = 0; j < (INSTR + 7) / 8; ++j) {
            const int q = dma_wave + 8 * j;
            if (8 * j + 7 < INSTR || q < INSTR) {
                const int r0 = q * RPI;                                   // first row of the group (wave-uniform)
                const int half = r0 / (NTAP * KG), rr0 = r0 % (NTAP * KG);
                const int rr = rr0 + lane / OCT;                          // this lane's row
                const int t = rr / KG, kg = rr % KG;
                const uint4* src = (half ? a.wl : a.wh) + ((size_t)(t * a.kgroups + k0 / 8 + kg) * p.N + n0 + lane % OCT);
                glds16(src, base + half * C::WUNITS + rr0 * OCT);
            }
        }
    };
    if (wave >= 8) {
        // ---------------- staging waves ----------------
        if (GC_WS_STAGER_PRIO) __builtin_amdgcn_s_setprio(GC_WS_STAGER_PRIO);
        const int st = tid - 512;
        const int kgl = __builtin_amdgcn_readfirstlane(st >> 7), tb = st & 127;     // waves 8, 9: channel group 0; waves 10, 11: group 1
        const float* xb = p.x + (size_t)b * p.K * chan;
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(xb, (unsigned)p.K * chan * 4u);
        const int lead = gc::pos_mod(p.pad_x, 32);           // patch rows start `lead` floats before a 128-byte boundary
        // Two register sets: the loads of item i + 2 are in flight while item i + 1 is converted and written, so the load latency
        // is never on this wave's critical path (which is then ~300 vector instructions + 16 ds_write_b128 per item).
        uint4 pa[C::NT][8], pb[C::NT][8];
        auto loads = [&](uint4 (&preg)[C::NT][8], int tile, int k0) {
            const int iy0 = (tile / p.tiles_x) * TPH - p.pad_y, ix0 = (tile % p.tiles_x) * (32 * CB) - p.pad_x;
#pragma unroll
            for (int j = 0; j < C::NT; ++j) {
                const typename C::Task tk = C::task_of(tb + 128 * j, lead);
                const int iy = iy0 + tk.row, ix = ix0 + tk.col;
                const bool ok = tk.used > 0 && iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w;      // rows past the last tile: zeros
                const unsigned boff = ok ? (unsigned)(iy * p.in_w + ix) * 4u : OOB;
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    preg[j][q] = buf_load_u128(rx, boff, (unsigned)(k0 + kgl * 8 + q) * chan * 4u);     // channels past K: beyond the descriptor, zeros
            }
        };
        auto convert = [&](uint4 (&preg)[C::NT][8], int tile, int k0, int buf) {
            uint4* const p_h = smem + buf * STAGE + 2 * C::WUNITS;
            uint4* const p_l = p_h + C::PUNITS;
            const int kk = min(k0, p.K - KCB);          // the item past the last one is converted into a stage nobody reads
            const float4 sa = *reinterpret_cast<const float4*>(&s_si[kk + kgl * 8]), sb = *reinterpret_cast<const float4*>(&s_si[kk + kgl * 8 + 4]);
            const float sc[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
            const int ix0 = (tile % p.tiles_x) * (32 * CB) - p.pad_x;
            const bool ragged_rows = (p.in_w & 3) != 0 && ix0 + lead + 32 * C::SEG_M + 4 > p.in_w;
            auto body = [&](auto masked, auto scaled) {
#pragma unroll
                for (int j = 0; j < C::NT; ++j) {
                    const typename C::Task tk = C::task_of(tb + 128 * j, lead);
                    const int inrow = p.in_w - (ix0 + tk.col);
                    const int rbase = kgl * PLANE + tk.row * C::RP;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v[8];
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const unsigned raw = i == 0 ? preg[j][q].x : (i == 1 ? preg[j][q].y : (i == 2 ? preg[j][q].z : preg[j][q].w));
                            v[q] = (!decltype(masked)::value || i < inrow) ? __uint_as_float(raw) : 0.f;
                        }
                        uint4 h, l;
                        split8s<decltype(scaled)::value>(v, sc, &h, &l);
                        if (i < tk.used) {
                            const int u = rbase + C::ucol(tk.col + i);
                            p_h[u] = h;
                            GC_LO(p_l[u] = l;)
                        }
                    }
                }
            };
            // without modulation (every layer of D) the multiply by one is not issued
            if (p.si) { if (ragged_rows) body(std::true_type{}, std::true_type{}); else body(std::false_type{}, std::true_type{}); }
            else      { if (ragged_rows) body(std::true_type{}, std::false_type{}); else body(std::false_type{}, std::false_type{}); }
        };
        auto advance = [&](int& tile, int& k0) { k0 += KCB; if (k0 >= p.K) { k0 = 0; tile += tstep; } };
        int t0 = tile_begin, k0 = 0;                    // item 0 -> set A
        loads(pa, t0, k0);
        int t1 = t0, k1 = k0; advance(t1, k1);          // item 1 -> set B
        loads(pb, t1, k1);
        convert(pa, t0, k0, 0);
        __syncthreads();
        // interval `it`: the multiplying waves work on item it; item it + 1 is converted here, item it + 2 is fetched
        for (int it = 0; it < items; it += 2) {
            int t2 = t1, k2 = k1; advance(t2, k2);
            GC_TR(1, 1);
            if (!(GC_WS_ABL & 1)) { loads(pa, t2, k2); GC_TR(1, 2); if (GC_WS_TRACE) { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(C::NT * 8) : "memory"); GC_TR(1, 3); } convert(pb, t1, k1, 1); }
            if (GC_WS_TRACE) { __builtin_amdgcn_s_waitcnt(0xC07F); GC_TR(1, 4); }
            __syncthreads();
            GC_TR(1, 5);
            if (it + 1 >= items) break;
            t1 = t2; k1 = k2; advance(t1, k1);
            GC_TR(1, 1);
            if (!(GC_WS_ABL & 1)) { loads(pb, t1, k1); GC_TR(1, 2); if (GC_WS_TRACE) { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(C::NT * 8) : "memory"); GC_TR(1, 3); } convert(pa, t2, k2, 0); }
            if (GC_WS_TRACE) { __builtin_amdgcn_s_waitcnt(0xC07F); GC_TR(1, 4); }
            __syncthreads();
            GC_TR(1, 5);
        }
#if GC_WS_TRACE
        if (tr_on) gc_ws_trace[1][511] = tr_n[1];
#endif
        return;
    }

    // ---------------- multiplying waves ----------------
    const int wave_row = (wave / CB) * 2, wave_col = (wave % CB) * 32;        // this wave: rows wave_row, wave_row + 1 of column block wave % CB
    f32x16 acc[WOC][WPX];
#pragma unroll
    for (int i = 0; i < WOC; ++i)
#pragma unroll
        for (int j = 0; j < WPX; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    int boff[WPX];
#pragma unroll
    for (int j = 0; j < WPX; ++j) boff[j] = hi * PLANE + (wave_row + j) * C::RP + wave_col;
    const int aoff = hi * OCT + l31;

    const unsigned oplane = (unsigned)(p.out_h * p.out_w) * 4u;
    const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.y + (size_t)b * p.N * p.out_h * p.out_w, (unsigned)p.N * oplane);
    const EpilogueConsts ec = epilogue_consts(p);
    const __amdgpu_buffer_rsrc_t rres = make_rsrc(p.residual ? p.residual + (size_t)b * p.N * p.out_h * p.out_w : p.y, p.residual ? (unsigned)p.N * oplane : 0u);
    auto finish_tile = [&](int tile) {
        const int qy0 = (tile / p.tiles_x) * TPH, qx0 = (tile % p.tiles_x) * (32 * CB);
        const int nb = opaque_s(n0);
        // every load of the epilogue (noise, residual) is issued before the first store: a load between two stores waits for the stores
        unsigned voff[WPX];
        float nz[WPX];
#pragma unroll
        for (int j = 0; j < WPX; ++j) {
            const int qy = qy0 + wave_row + j, qx = qx0 + wave_col + l31;
            const bool inside = qy < p.out_h && qx < p.out_w;
            voff[j] = inside ? (unsigned)(qy * p.out_w + qx) * 4u + (unsigned)(4 * hi) * oplane : OOB;
            nz[j] = (p.noise && inside) ? p.noise[((size_t)b * p.out_h + qy) * p.out_w + qx] : 0.f;
        }
        // Two phases, no control flow inside either.  (Round 5: the first version evaluated the epilogue AT each store and chose between the
        // residual / plain forms per element; the compiler turned that into one basic block per element -- two ds_read_b32 of out_scale / bias,
        // each waited for on the spot, ~12 vector instructions, the store, a branch: 128 exposed LDS round trips per lane and tile on the
        // MULTIPLYING waves, all eight of them at the same moment, next to 108 MFMAs per chunk.  tools/kernel_regs.py / the disassembly show it.)
        // Phase 1: every accumulator becomes its final value in place.  The 16 out_scale / bias values of a 32-channel block that this lane's
        // registers belong to are four runs of four consecutive channels: four 16-byte LDS reads each, issued together.
        // (with a residual its loads belong to the same block as the arithmetic: issued from a separate block after phase 1 their latency was
        // exposed once per tile -- 512 -> 512 @64^2 with scale + residual 199 -> 217 us in the first version of this change)
        auto phase1 = [&](auto with_res) {
#pragma unroll
            for (int i = 0; i < WOC; ++i) {
                float so16[16], bi16[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 s4 = *reinterpret_cast<const float4*>(&s_so[i * 32 + 8 * q + 4 * hi]);
                    so16[4 * q] = s4.x; so16[4 * q + 1] = s4.y; so16[4 * q + 2] = s4.z; so16[4 * q + 3] = s4.w;
                    if (EPK == 0) {
                        const float4 b4 = *reinterpret_cast<const float4*>(&s_bias[i * 32 + 8 * q + 4 * hi]);
                        bi16[4 * q] = b4.x; bi16[4 * q + 1] = b4.y; bi16[4 * q + 2] = b4.z; bi16[4 * q + 3] = b4.w;
                    }
                }
#pragma unroll
                for (int j = 0; j < WPX; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        // EPK 1 (out_scale and / or residual only): the product is rounded on its own, as conv_epilogue rounds it; values differ from
                        // the full epilogue's only in the sign of an exact zero (it adds +0 for the absent bias)
                        float v = EPK == 0 ? conv_epilogue(ec, acc[i][j][r], so16[r], bi16[r], nz[j]) : plain_mul(acc[i][j][r], so16[r]);
                        if (decltype(with_res)::value) v = plain_sum(v, buf_load_f32(rres, voff[j], (unsigned)(nb + i * 32 + (r & 3) + 8 * (r >> 2)) * oplane));
                        acc[i][j][r] = v;
                    }
            }
        };
        if (EPK < 2) phase1(std::integral_constant<bool, RES>{});
        // Phase 2: nothing but stores
#pragma unroll
        for (int j = 0; j < WPX; ++j)
#pragma unroll
            for (int i = 0; i < WOC; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ocs = nb + i * 32 + (r & 3) + 8 * (r >> 2);
                    const float v = acc[i][j][r];
                    if (!(GC_WS_ABL & 8) || v == 12345.678f) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), ry, (int)voff[j], (int)((unsigned)ocs * oplane), GC_CONV_ST_AUX);
                    acc[i][j][r] = 0.f;
                }
    };
    int tile_c = tile_begin, k0_c = 0;
    weights(0, 0); wait_staged_loads();
    __syncthreads();                 // stage 0 is staged
    // The weight slab of item it + 2 is requested right AFTER the barrier that ends item it -- its stage is free from
    // that moment -- and BEFORE the stores of a finished tile, instead of at the top of item it + 1 after them.  vmcnt counts loads and stores in
    // issue order, so with the request after the stores the `vmcnt(0)` in front of the next barrier also waited for the whole tile's stores to
    // reach memory -- once per tile, with only one or two items per tile at 32 / 64 input channels to hide it behind.  With the request older than
    // the stores the wait is counted: `vmcnt(S)`, S = the stores a lane issues per tile (at most 63), lets them stay in flight across the barrier.
    // The barrier is then the raw instruction (the `__syncthreads()` fence would drain the stores again).
    // The ablations without weight DMA (GC_WS_ABL & 2) or without stores (& 8: it makes the stores conditional, so no counted wait) take the plain
    // form instead: request at the top of the next item (unless & 2), vmcnt(0) and `__syncthreads()`.
    constexpr bool EARLY = !(GC_WS_ABL & (2 | 8));
    constexpr int NSTORES = WOC * WPX * 16 > 63 ? 63 : WOC * WPX * 16;
    // (the counted wait below is only right while finish_tile issues exactly WOC * WPX * 16 unconditional stores per lane AFTER the newest request,
    //  which is why the no-store ablation GC_WS_ABL & 8 is excluded from EARLY)
    bool stored = false;             // the previous item ended a tile: its stores were issued after the newest weight request
    if (EARLY) weights(KCB < p.K ? KCB : 0, 1);                       // item 1
    for (int it = 0; it < items; ++it) {
        if (!EARLY && !(GC_WS_ABL & 2)) weights(k0_c + KCB < p.K ? k0_c + KCB : 0, (it + 1) & 1);          // after the last item: a valid slab into a stage nobody reads
        const uint4* const wl_h = smem + (it & 1) * STAGE;
        const uint4* const wl_l = wl_h + C::WUNITS;
        const uint4* const p_h = wl_l + C::WUNITS;
        const uint4* const p_l = p_h + C::PUNITS;
        GC_TR(0, 1);
        __builtin_amdgcn_s_setprio(GC_MFMA_PRIO);
        // Fragment double buffer: the eight ds_read_b128 of tap t + 1 are issued BEFORE the twelve MFMAs of tap t (the scheduling
        // barriers pin that order; left alone the compiler sinks every read to 1-3 MFMAs before its use, far less than the LDS latency).
        bf16x8 fa[2][2 * WOC], fb[2][2 * WPX];          // [set][hi 0..1, lo 0..1]
        auto load_tap = [&](int t, int set) {
            const int jy = t / KS, jx = t % KS;
            const int wbase = t * KG * OCT + aoff;
            const int pbase = jy * C::RP + l31 + jx;
#pragma unroll
            for (int i = 0; i < WOC; ++i) {
                const uint4 uh = wl_h[wbase + i * 32];
                fa[set][i] = *reinterpret_cast<const bf16x8*>(&uh);
                GC_LO(const uint4 ul = wl_l[wbase + i * 32]; fa[set][WOC + i] = *reinterpret_cast<const bf16x8*>(&ul);)
            }
#pragma unroll
            for (int j = 0; j < WPX; ++j) {
                const uint4 uh = p_h[pbase + boff[j]];
                fb[set][j] = *reinterpret_cast<const bf16x8*>(&uh);
                GC_LO(const uint4 ul = p_l[pbase + boff[j]]; fb[set][WPX + j] = *reinterpret_cast<const bf16x8*>(&ul);)
            }
        };
        load_tap(0, 0);
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
            if (t + 1 < NTAP && !(GC_WS_ABL & 4)) load_tap(t + 1, (t + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < WOC; ++i)
#pragma unroll
                for (int j = 0; j < WPX; ++j) { constexpr int fs = (GC_WS_ABL & 4) ? 0 : 1; GC_MFMA3(acc[i][j], fa[t & fs][i], fa[t & fs][WOC + i], fb[t & fs][j], fb[t & fs][WPX + j]); }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
        GC_TR(0, 2);
        if (EARLY) {
            // the rows of item it + 1 were requested one item ago, before any store still in flight
            if (dma_mine) {
                if (stored) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NSTORES) : "memory");
                else        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): this wave's LDS reads have returned
            GC_TR(0, 3);
            __builtin_amdgcn_s_barrier();
            GC_TR(0, 4);
            // item it + 2 goes into the stage item it has just left: (it + 2) chunks on from the start, modulo the chunks of a tile
            const int k2 = k0_c + 2 * KCB;
            weights(k2 < p.K ? k2 : (k2 - p.K < p.K ? k2 - p.K : 0), it & 1);
            stored = false;
        } else {
            wait_staged_loads();         // the LDS-DMA rows of this wave have landed (they were issued a whole MFMA phase ago)
            __syncthreads();             // this stage may be rewritten from the next item on; the other one is staged
        }
        k0_c += KCB;
        if (k0_c >= p.K) { GC_TR(0, 5); finish_tile(tile_c); GC_TR(0, 6); k0_c = 0; tile_c += tstep; stored = true; }
    }
#if GC_WS_TRACE
    if (tr_on) gc_ws_trace[0][511] = tr_n[0];
#endif
    // the slabs requested for the two items past the last one (valid rows into stages nobody reads) must have landed before the wave ends and the
    // LDS is handed to the next workgroup: costs nothing, the wave is ending (round-5 advisor finding)
    if (EARLY) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}


// ---- the launchers: each instantiates what the plan says (tiling, grid and split are the plan's) ----

template <int WOC, int WPX, class G>
int launch(const ConvPlan& p, const Bf16Args& a, hipStream_t s) {
    using C = BCfg<1, 4, WOC, WPX, G::UP, G::DOWN, G::KS>;
    dim3 grid((unsigned)p.gx, gc::ceil_div(a.c.N, C::OCT), p.split ? p.slices : 1);
    hipLaunchKernelGGL((conv_bf16x3_kernel<1, 4, WOC, WPX, G::UP, G::DOWN, G::KS>), grid, dim3(256), 0, s, a);
    return gc::check_launch("gc_conv2d_bf16x3_f32");
}

template <class G>
int launch_one_role(const ConvPlan& p, const Bf16Args& a, hipStream_t s) {
    const int woc = p.t[2], wpx = p.t[3];
    if constexpr (G::DOWN == 2) return woc == 1 ? launch<1, 1, G>(p, a, s) : launch<2, 1, G>(p, a, s);
    else return woc == 1 ? launch<1, 2, G>(p, a, s) : (wpx == 1 ? launch<2, 1, G>(p, a, s) : launch<2, 2, G>(p, a, s));
}

// wave-specialised kernel (conv_bf16x3_ws_kernel): 64 oc x 16 rows x 32 px tiles, one 12-wave workgroup per CU
template <int KS, int WOC, int CB>
int launch_ws_inst(const ConvPlan& p, const Bf16Args& a, hipStream_t s) {
    const dim3 grid((unsigned)p.gx, a.c.N / (32 * WOC));
    with_ws_epilogue(a.c, GC_WS_BARE, [&](auto epk, auto res) {
        hipLaunchKernelGGL((conv_bf16x3_ws_kernel<KS, WOC, CB, decltype(epk)::value, decltype(res)::value>), grid, dim3(768), 0, s, a);
    });
    return gc::check_launch("gc_conv2d_bf16x3_f32(ws)");
}

template <int KS>
int launch_ws(const ConvPlan& p, const Bf16Args& a, hipStream_t s) {
    const int woc = p.t[0], cb = p.t[1];
    if (woc == 2) return cb == 2 ? launch_ws_inst<KS, 2, 2>(p, a, s) : launch_ws_inst<KS, 2, 1>(p, a, s);      // (4 x 128 px tiles of 64 channels do not fit two LDS stages)
    return cb == GC_WS_WIDE_CB32 ? launch_ws_inst<KS, 1, GC_WS_WIDE_CB32>(p, a, s) : (cb == 2 ? launch_ws_inst<KS, 1, 2>(p, a, s) : launch_ws_inst<KS, 1, 1>(p, a, s));
}

// the kernels of one geometry, in the order plan_geom considers them
template <class G>
int launch_geom(const ConvPlan& p, const Bf16Args& a, hipStream_t s) {
    if constexpr (G::UP == 1 && G::DOWN == 1) { if (p.path == ConvPath::WS) return launch_ws<G::KS>(p, a, s); }
#ifndef GC_SINGLE
    if constexpr (G::DOWN == 2 && G::KS == 3) { if (p.path == ConvPath::S2WS) return launch_s2ws(p, a, s); }
#endif
    return launch_one_role<G>(p, a, s);
}

// ---- the plan: every decision of a forward launch, taken here and nowhere else ----

template <int WOC, int WPX, class G>
void set_one_role(ConvPlan& p) {
    using C = BCfg<1, 4, WOC, WPX, G::UP, G::DOWN, G::KS>;
    p.path = ConvPath::ONE_ROLE;
    p.t[0] = 1; p.t[1] = 4; p.t[2] = WOC; p.t[3] = WPX;
    p.tile_h = C::TPH; p.tile_w = 32; p.oct = C::OCT;
}

template <int KS, int WOC, int CB>
void set_ws(ConvPlan& p) {
    using C = BCfg<1, 8, WOC, 2, 1, 1, KS, CB>;          // the configuration of conv_bf16x3_ws_kernel<KS, WOC, CB>
    p.path = ConvPath::WS;
    p.t[0] = WOC; p.t[1] = CB; p.t[2] = p.t[3] = 0;
    p.tile_h = C::TPH; p.tile_w = 32 * CB; p.oct = C::OCT;
}

// the layers the wave-specialised kernel takes (p: their unsplit one-role plan, replaced when it does): whole 16-channel chunks and 32- / 64-channel
// output blocks, enough chunks per tile to amortise its two-stage start-up, and enough tiles to give every CU a workgroup
template <int KS>
bool plan_ws(const gc_conv_desc* d, ConvPlan& p) {
#ifdef GC_NO_WS
    return false;
#endif
    const bool oc64 = d->out_ch % 64 == 0;          // 32-channel output blocks for the layers whose N is not a multiple of 64 (the 1024^2 layers: N = 32)
    if (d->in_ch % KCB != 0 || d->out_ch % 32 != 0 || d->in_ch < (oc64 ? GC_WS_MIN_K : GC_WS_MIN_K32) || d->out_w < 32 || d->out_h < 16) return false;
    ConvPlan q = p;
    if (oc64) set_ws<KS, 2, 1>(q); else set_ws<KS, 1, 1>(q);
    plan_tiles(q, d->out_h, d->out_w);
    if ((long long)q.tiles_x * q.tiles_y * d->batch * (d->out_ch / q.oct) < 192) return false;
    // wide tiles (8 rows x 64 px) where HBM, not the matrix pipe, bounds the layer: few input channels per output byte
    if (d->in_ch <= GC_WS_WIDE_MAX_K && d->out_w >= 64) {
        if (oc64) set_ws<KS, 2, 2>(q);
        else if (d->out_w >= 128) set_ws<KS, 1, GC_WS_WIDE_CB32>(q);
        else set_ws<KS, 1, 2>(q);
        plan_tiles(q, d->out_h, d->out_w);
    }
    plan_resident(q, d);
    p = q;
    return true;
}

template <class G>
void plan_geom(const gc_conv_desc* d, size_t room, ConvPlan& p) {
    constexpr int UP = G::UP, DOWN = G::DOWN, KS = G::KS;
    const int qh = gc::ceil_div(d->out_h, UP), qw = gc::ceil_div(d->out_w, UP);
    if (DOWN == 2) {
        // patch extents double: 4-row tiles only
        if (d->out_ch <= 32) set_one_role<1, 1, G>(p); else set_one_role<2, 1, G>(p);
    } else if (d->out_ch <= 32) {
        set_one_role<1, 2, G>(p);                  // 32oc x (8 rows x 32 px)
    } else {
        // 64oc x (8 rows x 32 px) unless that leaves most CUs idle (32x32 / 64x64 planes at batch 4): 4-row tiles
        set_one_role<2, 2, G>(p);
        plan_tiles(p, qh, qw);
        if ((long long)p.tiles_x * p.tiles_y * UP * UP * d->batch * gc::ceil_div(d->out_ch, p.oct) < 512) set_one_role<2, 1, G>(p);
    }
    plan_tiles(p, qh, qw);
    // small planes split over K, from the tiles of the instance chosen above (round 5: a plan of its own assumed eight rows throughout and cut the stride-1
    // layers into twice the slices they needed -- 512 -> 512 @32^2: B = 4 79 -> 71 us with two slices instead of four, B = 8 133 -> 114 us unsplit; the partial
    // sums are the cost of a slice).  A split launch stays here: the wave-specialised kernels below take unsplit launches only.
    if (UP == 1) plan_split(p, d, room);
    if (!p.split) {
        if constexpr (UP == 1 && DOWN == 1) { if (plan_ws<KS>(d, p)) return; }
#ifndef GC_SINGLE
        // round 6: the large 3x3 layers on the wave-specialised stride-2 kernel (conv_s2ws.hip: E / O half stages, 128 oc x 8 rows x 32 px tiles)
        if constexpr (DOWN == 2 && KS == 3) { if (plan_s2ws(d, p)) return; }
#endif
    }
    // tiles per workgroup: as many as keep >= 8 workgroups per CU-slot pair (2048 on 256 CUs x 2) in the launch, at most 8;
    // few channel chunks per tile is where the per-tile latencies dominate, many chunks need no help
    const int tiles = p.tiles_x * p.tiles_y;
    if (UP == 1 && !p.split) {
        const long long wgs = (long long)tiles * d->batch * gc::ceil_div(d->out_ch, p.oct);
        const int nchunks = gc::ceil_div(d->in_ch, KCB);
        int want = nchunks <= 2 ? 8 : (nchunks <= 4 ? 4 : (nchunks <= 8 ? 2 : 1));
        while (want > 1 && wgs / want < 2048) want >>= 1;
        p.tpb = want;
    }
    p.groups = gc::ceil_div(tiles, p.tpb);
    p.gx = (long long)p.groups * UP * UP * d->batch;
}

// shapes the split-bf16 kernels are built for; everything else runs on the exact fp32 kernels
bool eligible(const gc_conv_desc* d) {
    const int qw = gc::ceil_div(d->out_w, d->up);
    // 9 .. 16-pixel rows fill part of the 32-pixel tile only, yet beat the fp32 MFMA path (512 -> 512 @16^2, B = 8: 97 vs 201 us;
    // stride 2 @33^2: 128 vs 281 us); at <= 8 pixels the fp32 kernel with its split over K is faster (36 vs 92 us @8^2)
    if (d->in_ch < 16 || d->in_ch > MAX_K_BF16X3 || qw <= 8 || pointwise_thin(d)) return false;
    // the staging scheme wants the patch rows to start at most EDGE floats before a 32-float boundary (see BCfg)
    if (d->up == 1) {
        const int pwd = 31 * d->down + d->kw, edge = pwd - 32 * (pwd % 32 == 0 ? pwd / 32 : (pwd - 1) / 32);
        return d->pad_x >= 0 && d->pad_x <= edge;
    }
    return d->pad_x >= 1 && d->pad_x <= 2;      // up = 2: phase rows start 0 or 1 floats before the boundary only for these
}

// THE decision of a forward launch in split-bf16 / plain-bf16 arithmetic.  ep: the launch's epilogue (null for the queries; only the GC_CTWS
// experiments look at it); room: the bytes the caller brought for the K slices (0 for the queries and the probe: they see the unsplit decision).
ConvPlan plan_conv(const gc_conv_desc* d, const gc_conv_epilogue* ep, size_t room) {
    ConvPlan p;
    if (!eligible(d)) return p;
    if (d->kh == 3 && d->up == 2 && d->pad_y == 2 && d->pad_x == 2) plan_t(d, ep, room, p);       // the fused transposed kernel
    else with_geom(d, [&](auto g) { plan_geom<decltype(g)>(d, room, p); });
    return p;
}

// ... and what follows from it for a caller's buffers
bool reads_pitched_input(const gc_conv_desc* d, const ConvPlan& p) { return p.path != ConvPath::F32 && d->up == 1 && d->down == 2; }      // conv_bf16x3_kernel and conv_s2ws_bf16x3_kernel at stride 2
size_t packed_weight_bytes(const gc_conv_desc* d, const ConvPlan& p) { return p.path != ConvPath::F32 ? 2 * packed_units(d) * sizeof(uint4) : 0; }      // hi and lo halves

int probe_conv(const gc_conv_desc* d, const ConvPlan& p) {
    const int* t = p.t;
    switch (p.path) {
    case ConvPath::ONE_ROLE:  return gc::probe_name("conv_bf16x3_kernel<%d,%d,%d,%d>|up%d,down%d,k%d", t[0], t[1], t[2], t[3], d->up, d->down, d->kh);
    case ConvPath::WS:        return gc::probe_name("conv_bf16x3_ws_kernel<%d,%d,%d>|up1,down1,k%d", d->kh, t[0], t[1], d->kh);
    case ConvPath::S2WS:      return gc::probe_name("conv_s2ws_bf16x3_kernel<%d>|up1,down2,k3", t[0]);
    case ConvPath::CT:        return gc::probe_name("convt_fused_bf16x3_kernel<%d,%d,%d,%d>|up2,down1,k3", t[0], t[1], t[2], t[3]);
    case ConvPath::CT_EDGE:   return gc::probe_name("convt_fused_bf16x3_kernel<%d,%d,%d,%d>+edge|up2,down1,k3", t[0], t[1], t[2], t[3]);
    case ConvPath::CTWS:      return gc::probe_name("convt_bf16x3_ws_kernel<%d,%d>|up2,down1,k3", t[0], t[1]);
    case ConvPath::CTWS_EDGE: return gc::probe_name("convt_bf16x3_ws_kernel<%d,%d>+edge|up2,down1,k3", t[0], t[1]);
    case ConvPath::F32:       break;      // named by the fp32 family itself
    }
    return gc::fail(GC_ERR_BAD_ARG, "gc_conv2d_bf16x3_f32: no kernel to name");
}

}  // namespace

#ifdef GC_SINGLE
// the plain-bf16 build shares the queries, the weight pack (its lo half is simply not read) and the workspace layout of the split build
#define gc_conv2d_fused_bf16x3_packed_f32 gc_conv2d_fused_bf16_packed_f32
#else
extern "C" size_t gc_conv2d_bf16x3_workspace(const gc_conv_desc* d) {
    if (!d || d->in_ch <= 0 || d->out_ch <= 0 || d->kh <= 0 || d->kw <= 0) return 0;
    const ConvPlan p = plan_conv(d, nullptr, 0);
    if (p.path == ConvPath::F32) return conv2d_f32_workspace(d);        // runs on the fp32 kernel: split-K partial sums (small planes) or nothing
    return packed_weight_bytes(d, p) + p.slice_bytes(d);      // the split weights (gc_conv2d_fused_bf16x3_f32 packs them here), then the K slices
}

extern "C" size_t gc_conv2d_bf16x3_splitk_bytes(const gc_conv_desc* d) {
    if (!d || d->batch <= 0 || d->in_ch <= 0 || d->out_ch <= 0 || d->kh <= 0 || d->kw <= 0) return 0;
    return plan_conv(d, nullptr, 0).slice_bytes(d);
}

extern "C" int gc_conv2d_out_pitch(const gc_conv_desc* d, int mode) {
    if (!d || mode == 0 || d->in_ch <= 0 || d->out_ch <= 0 || d->out_w <= 0) return 0;          // the fp32 kernels write dense rows
    if (!plan_conv(d, nullptr, 0).fused_transposed()) return 0;
    if (d->out_w % 32 == 0 || d->out_w < 129) return 0;       // already aligned, or too small to matter
    return (d->out_w + 31) / 32 * 32;
}

extern "C" int gc_conv2d_in_pitch_ok(const gc_conv_desc* d, int mode, int wgrad) {
    if (!d || mode == 0 || d->in_ch <= 0 || d->out_ch <= 0 || d->up != 1 || d->down != 2) return 0;
    return wgrad ? (wg_eligible(d) ? 1 : 0) : (reads_pitched_input(d, plan_conv(d, nullptr, 0)) ? 1 : 0);
}

extern "C" size_t gc_conv2d_bf16x3_packed_bytes(const gc_conv_desc* d) {
    if (!d || d->in_ch <= 0 || d->out_ch <= 0 || d->kh <= 0 || d->kw <= 0) return 0;
    return packed_weight_bytes(d, plan_conv(d, nullptr, 0));
}

extern "C" int gc_conv2d_pack_weights_bf16x3(const gc_conv_desc* d, const float* w, void* packed, size_t packed_bytes, gc_stream_t stream) {
    int rc = validate(d, "gc_conv2d_pack_weights_bf16x3", false);
    if (rc) return rc;
    const size_t need = gc_conv2d_bf16x3_packed_bytes(d);
    if (need == 0) return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_pack_weights_bf16x3: this shape runs on the fp32 kernel and takes no packed weights");
    if (!w || !packed || packed_bytes < need || (reinterpret_cast<uintptr_t>(packed) & 15))
        return gc::fail(GC_ERR_WORKSPACE, "gc_conv2d_pack_weights_bf16x3: buffer %zu < %zu bytes (or null / not 16-byte aligned)", packed_bytes, need);
    const int kgroups = (d->in_ch + 7) / 8, taps = d->kh * d->kw;
    const size_t units = packed_units(d);
    uint4* wh = static_cast<uint4*>(packed);
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)std::min<size_t>((units + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                       w, wh, wh + units, taps, d->in_ch, d->out_ch, kgroups);
    return gc::check_launch("gc_conv2d_pack_weights_bf16x3");
}

extern "C" int gc_conv2d_pack_weights_bf16x3_grouped(const gc_wpack_group* groups, int n_groups, gc_stream_t stream) {
    if (n_groups < 0 || (n_groups > 0 && !groups)) return gc::fail(GC_ERR_BAD_ARG, "gc_conv2d_pack_weights_bf16x3_grouped: bad group table");
    for (int first = 0; first < n_groups; first += MAXPG) {
        PackGroupArgs a;
        a.n_groups = std::min(MAXPG, n_groups - first);
        long long blocks = 0;
        for (int i = 0; i < a.n_groups; ++i) {
            const gc_wpack_group& g = groups[first + i];
            int rc = validate(&g.desc, "gc_conv2d_pack_weights_bf16x3_grouped", false);
            if (rc) return rc;
            const size_t need = gc_conv2d_bf16x3_packed_bytes(&g.desc);
            if (need == 0) return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_pack_weights_bf16x3_grouped: group %d runs on the fp32 kernel and takes no packed weights", first + i);
            if (!g.w || !g.packed || g.packed_bytes < need || (reinterpret_cast<uintptr_t>(g.packed) & 15))
                return gc::fail(GC_ERR_WORKSPACE, "gc_conv2d_pack_weights_bf16x3_grouped: group %d: buffer %zu < %zu bytes (or null / not 16-byte aligned)", first + i, (size_t)g.packed_bytes, need);
            const int kgroups = (g.desc.in_ch + 7) / 8, taps = g.desc.kh * g.desc.kw;
            const size_t units = packed_units(&g.desc);
            uint4* wh = static_cast<uint4*>(g.packed);
            a.g[i] = PackGroup{g.w, wh, wh + units, taps, g.desc.in_ch, g.desc.out_ch, kgroups, (int)blocks};
            blocks += (long long)((units + 255) / 256);
            if (blocks > 2147483647LL) return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_pack_weights_bf16x3_grouped: too many blocks");
        }
        if (blocks) hipLaunchKernelGGL(pack_weights_grouped_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    }
    return gc::check_launch("gc_conv2d_pack_weights_bf16x3_grouped");
}
#endif

extern "C" int gc_conv2d_fused_bf16x3_packed_f32(const gc_conv_desc* d, const float* x, const float* w, const void* packed, size_t packed_bytes,
                                                 const float* in_scale, const float* out_scale, const gc_conv_epilogue* ep, float* y,
                                                 void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    int rc = validate(d, "gc_conv2d_bf16x3_f32", false);
    if (rc) return rc;
    if (!x || !w || !y) return gc::fail(GC_ERR_BAD_ARG, "gc_conv2d_bf16x3_f32: null pointer");
    if (d->batch == 0) return GC_OK;
    if ((rc = validate_epilogue(ep, "gc_conv2d_bf16x3_f32"))) return rc;
    // small planes: split over K when the caller brought room for the slices (gc_conv2d_bf16x3_splitk_bytes)
    const ConvPlan p = plan_conv(d, ep, workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 ? workspace_bytes : 0);
    if (d->in_pitch != 0 && d->in_pitch != d->in_w && !reads_pitched_input(d, p))
        return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_bf16x3_f32: in_pitch %d: only the split-bf16 stride-2 kernel reads pitched rows (gc_conv2d_in_pitch_ok)", d->in_pitch);
    if (!dense_output(d) && !p.fused_transposed())
        return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_bf16x3_f32: out_pitch %d: only the fused transposed 3x3 convolution writes pitched rows (gc_conv2d_out_pitch)", d->out_pitch);
    if (p.path == ConvPath::F32) return conv2d_f32_ws(d, x, w, in_scale, out_scale, ep, y, workspace, workspace_bytes, stream);
    const size_t need = packed_weight_bytes(d, p);
    if (!packed || packed_bytes < need || (reinterpret_cast<uintptr_t>(packed) & 15))
        return gc::fail(GC_ERR_WORKSPACE, "gc_conv2d_bf16x3_f32: packed weights %zu < %zu bytes (or null / not 16-byte aligned)", packed_bytes, need);
    // (the probe names the main region + edge forms before their grid is looked at)
    if (p.gx > 2147483647LL && !(gc::probing() && p.edge())) return gc::fail(GC_ERR_UNSUPPORTED, "gc_conv2d_bf16x3_f32: grid too large");
    if (gc::probing()) return probe_conv(d, p);
    hipStream_t s = (hipStream_t)stream;
    const uint4* wh = static_cast<const uint4*>(packed);
    Bf16Args a{{x, w, in_scale, out_scale, y, d->batch, d->in_ch, d->out_ch, d->in_h, d->in_w, d->out_h, d->out_w,
                d->pad_y, d->pad_x, 0, 0}, wh, wh + packed_units(d), (d->in_ch + 7) / 8, p.tpb, p.groups, 0, nullptr, 0, d->out_pitch ? d->out_pitch : d->out_w, d->in_pitch ? d->in_pitch : d->in_w};
    set_epilogue(a.c, ep);
    ConvArgs fin = a.c;
    a.c.tiles_x = p.tiles_x;
    a.c.tiles_y = p.tiles_y;
    if (p.split) {
        // the slices are raw partial sums; the finish pass applies out_scale and the epilogue
        a.c.so = nullptr;
        set_epilogue(a.c, nullptr);
        a.k_per_split = p.k_per_split;
        a.part = static_cast<float*>(workspace);
        a.per_slice = (long long)d->batch * d->out_ch * d->out_h * d->out_w;
    }
    rc = p.fused_transposed() ? launch_t(p, a, s) : with_geom(d, [&](auto g) { return launch_geom<decltype(g)>(p, a, s); });
    if (rc || !p.split) return rc;
    fin.part = a.part;
    return launch_splitk_finish(fin, p.slices, a.per_slice, s);
}

#ifndef GC_SINGLE
extern "C" int gc_conv2d_fused_bf16x3_f32(const gc_conv_desc* d, const float* x, const float* w,
                                          const float* in_scale, const float* out_scale, const gc_conv_epilogue* ep, float* y,
                                          void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    int rc = validate(d, "gc_conv2d_bf16x3_f32", false);
    if (rc) return rc;
    if (d->batch == 0) return GC_OK;
    const size_t need = gc_conv2d_bf16x3_packed_bytes(d);
    if (need == 0) return gc_conv2d_fused_bf16x3_packed_f32(d, x, w, nullptr, 0, in_scale, out_scale, ep, y, workspace, workspace_bytes, stream);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return gc::fail(GC_ERR_WORKSPACE, "gc_conv2d_bf16x3_f32: workspace %zu < %zu bytes (or not 16-byte aligned)", workspace_bytes, need);
    if (!w) return gc::fail(GC_ERR_BAD_ARG, "gc_conv2d_bf16x3_f32: null pointer");
    if ((rc = gc_conv2d_pack_weights_bf16x3(d, w, workspace, workspace_bytes, stream))) return rc;
    char* tail = static_cast<char*>(workspace) + need;
    return gc_conv2d_fused_bf16x3_packed_f32(d, x, w, workspace, need, in_scale, out_scale, ep, y, workspace_bytes > need ? tail : nullptr,
                                             workspace_bytes > need ? workspace_bytes - need : 0, stream);
}

extern "C" int gc_conv2d_bf16x3_f32(const gc_conv_desc* d, const float* x, const float* w,
                                    const float* in_scale, const float* out_scale, float* y,
                                    void* workspace, size_t workspace_bytes, gc_stream_t stream) {
    return gc_conv2d_fused_bf16x3_f32(d, x, w, in_scale, out_scale, nullptr, y, workspace, workspace_bytes, stream);
}
#endif

#if GC_WS_TRACE && !defined(GC_SINGLE)
// dev: copy the trace of the last conv_bf16x3_ws_kernel launches to the host (tools/ws_trace.py)
extern "C" int gc_debug_ws_trace(unsigned long long* dst) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(gc_ws_trace), sizeof(unsigned long long) * 2 * 512, 0, hipMemcpyDeviceToHost);
}
#endif
