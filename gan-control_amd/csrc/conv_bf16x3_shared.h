// Shared by the split-bf16 convolution translation units (conv_bf16x3.hip, convt_bf16x3.hip, wgrad_bf16x3.hip, conv_s2ws.hip): build knobs, the argument block, the hi / lo split of
// eight staged values, LDS-DMA helpers.  Everything sits in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "conv_common.h"

// conv_bf16x3.hip, convt_bf16x3.hip and wgrad_bf16x3.hip build a second time with -DGC_SINGLE (objects *_single.o): plain bf16 arithmetic -- ONE MFMA per product on the
// hi parts only (bf16 operands, fp32 accumulate, fp32 in HBM; ~3e-3 relative error per layer, the precision of BASELINE.json's
// config[1] "bf16").  The lo parts are then neither converted, stored to LDS nor read; entry points gc_conv2d_fused_bf16_packed_f32 /
// gc_conv2d_wgrad_bf16_f32.  It is never the default nor the parity mode.
#ifdef GC_SINGLE
#define GC_LO(...)
#define GC_MFMA3(c, ah, al, bh, bl) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0)
#else
#define GC_LO(...) __VA_ARGS__
#define GC_MFMA3(c, ah, al, bh, bl)                                        \
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);       \
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);       \
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0)
#endif

// Wave priority during the MFMA phases: the co-resident workgroup is staging (vector ALU, LDS, loads) meanwhile; letting the
// multiplying wave issue first keeps the matrix pipe fed (same-box A/B: -2 % forward, -1..3 % weight gradients).
#ifndef GC_MFMA_PRIO
#define GC_MFMA_PRIO 2
#endif
#ifndef GC_WS_MIN_K
#define GC_WS_MIN_K 64      // input channels from which the wave-specialised forward kernel takes over
#endif
#ifndef GC_WS_MIN_K32
#define GC_WS_MIN_K32 32    // ... and its 32-output-channel variant
#endif
#ifndef GC_WS_WIDE_MAX_K
#define GC_WS_WIDE_MAX_K 64   // input channels up to which the wave-specialised kernel uses 8 x 64 tiles
#endif
#ifndef GC_WS_WIDE_CB32
#define GC_WS_WIDE_CB32 4      // column blocks of the wide tiles of the 32-output-channel variant (4: 4 rows x 128 px)
#endif
#ifndef GC_CT_ABL
#define GC_CT_ABL 0           // dev ablations of convt_fused_bf16x3_kernel (wrong results): 1 no stores, 2 no MFMAs, 4 no global loads, 8 no conversion (a pre-split input)
#endif
#ifndef GC_WS_SLOTS
#define GC_WS_SLOTS 256     // workgroups the wave-specialised kernel keeps resident: one per CU
#endif
#ifndef GC_WS_STAGER_PRIO
#define GC_WS_STAGER_PRIO 0
#endif
#ifndef GC_S2_ABL
#define GC_S2_ABL 0         // dev ablations of conv_bf16x3_kernel at stride 2 (wrong results): 1 the loaded registers are written to LDS as they are -- no scale, no hi / lo
                            // split, no masks: what a PRE-SPLIT input (the producer emitting channel-last bf16 pairs, same bytes) would leave of the staging;
                            // 2 no patch loads and no patch commit at all (weights, fragment reads, MFMAs, stores only)
#endif
#ifndef GC_WS_ABL
#define GC_WS_ABL 0         // dev ablations of conv_bf16x3_ws_kernel (wrong results): 1 no patch staging, 2 no weight DMA, 4 fragments read once, 8 no stores
#endif
#include <type_traits>

// Output stores of the convolution kernels: non-temporal (aux bit 1 = the `nt` bit of gfx94x / gfx950 buffer stores) when GC_CONV_NT is set.
// Round 4, same-box A/B on the whole step (two alternations): 75.15 -> 75.44 images/s on top of the streaming kernels' own non-temporal stores
// (GC_NT_STORE, common.h: 74.17 -> 75.15).
#ifndef GC_CONV_NT
#define GC_CONV_NT 1
#endif
#define GC_CONV_ST_AUX (GC_CONV_NT ? 2 : 0)
#ifndef GC_WS_BARE
#define GC_WS_BARE 1         // reduced epilogues (EPK 1 / 2) of the wave-specialised kernel for launches without bias / noise / activation (0: always the full epilogue)
#endif
// Planes of 9 .. 32 pixels (the 16^2 / 32^2 layers, 512 channels) give the launch only B * tiles * N / 64 = 64 .. 256 workgroups, each
// walking all 32 channel chunks one after the other with nothing to hide the load latency behind (512 -> 512 @16^2, B = 4: 88 us for
// 4.8 GFLOP).  Splitting K over blockIdx.z fills the chip and shortens the dependent chain; slices of >= 4 chunks.
#ifndef GC_CT_SPLITK
#define GC_CT_SPLITK 1        // transposed 3x3 convolutions on small planes split over the input channels
#endif
#ifndef GC_SPLIT_TARGET
#define GC_SPLIT_TARGET 512   // workgroups a split launch aims for
#endif
#include <algorithm>


namespace gcconv {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int KCB = 16;   // input channels per chunk = K of one bf16 MFMA
constexpr int KG = 2;     // 8-channel groups per chunk
constexpr int MAX_K_BF16X3 = 1024;   // in_scale of one sample is kept in LDS

struct Bf16Args {
    ConvArgs c;
    const uint4* wh; const uint4* wl;   // packed weights [tap][ceil(K/8)][N] units of 8 bf16 (hi / lo parts)
    int kgroups;                        // ceil(K / 8)
    int tpb, groups;                    // conv_bf16x3_kernel: pixel tiles per workgroup, workgroups per (sample, phase)
    // grid-level split over the input channels (small planes): slice blockIdx.z covers channels [z * k_per_split, (z + 1) * k_per_split)
    // and writes RAW partial sums to part + z * per_slice; splitk_finish_kernel (conv.hip) adds the slices and applies the epilogue
    int k_per_split; float* part; long long per_slice;
    int out_pitch;                      // floats between output rows (convt_fused_bf16x3_kernel only; out_w elsewhere)
    int in_pitch;                       // floats between input rows (conv_bf16x3_kernel; in_w when dense)
};

// The decision of ONE forward launch, taken once by plan_conv (conv_bf16x3.hip) and read by everything else: the argument checks, the size and pitch
// queries, the probe name and the launchers (which only instantiate what it says).
enum class ConvPath {
    F32,            // not a shape of these kernels: the exact fp32 family (conv.hip)
    ONE_ROLE,       // conv_bf16x3_kernel<t0, t1, t2, t3, up, down, k>
    WS,             // conv_bf16x3_ws_kernel<k, t0, t1>
    S2WS,           // conv_s2ws_bf16x3_kernel<t0>
    CT, CT_EDGE,    // convt_fused_bf16x3_kernel<t0, t1, t2, t3>; _EDGE: over the H x W main region, convt_edge_bf16x3_kernel does the rest
    CTWS, CTWS_EDGE // convt_bf16x3_ws_kernel<t0, t1> (the GC_CTWS experiments)
};
struct ConvPlan {
    ConvPath path = ConvPath::F32;
    int t[4] = {0, 0, 0, 0};            // the template arguments of the instance (see ConvPath)
    int tile_h = 1, tile_w = 1, oct = 1;      // a workgroup's tile, from the instance's own config constants: rows x columns (of the phase sub-grid when up = 2) x output channels
    int slices = 1, k_per_split = 0;    // the split over the input channels as the queries size it ...
    bool split = false;                 // ... and whether THIS launch runs split: the caller brought room for the slices.  A split launch stays on the one-role kernels.
    int tiles_x = 1, tiles_y = 1, tpb = 1, groups = 1;      // pixel tiles, tiles per workgroup, workgroups per (sample, phase)
    long long gx = 0;                   // grid x
    bool fused_transposed() const { return path >= ConvPath::CT; }      // the one family that writes pitched output rows
    bool edge() const { return path == ConvPath::CT_EDGE || path == ConvPath::CTWS_EDGE; }
    size_t slice_bytes(const gc_conv_desc* d) const { return slices > 1 ? (size_t)slices * d->batch * d->out_ch * d->out_h * d->out_w * sizeof(float) : 0; }
};

// units of 8 bf16 in ONE half (hi or lo) of the packed weights: [tap][ceil(K / 8)][N]
inline size_t packed_units(const gc_conv_desc* d) { return (size_t)d->kh * d->kw * ((d->in_ch + 7) / 8) * d->out_ch; }

// tiles of the plan's tile over a qh x qw plane, and from them the split over K of a one-role instance: as many slices as bring the launch to
// GC_SPLIT_TARGET workgroups, of >= 64 channels each.  room: the bytes the caller brought for the slices.
inline void plan_tiles(ConvPlan& p, int qh, int qw) {
    p.tiles_y = gc::ceil_div(qh, p.tile_h);
    p.tiles_x = gc::ceil_div(qw, p.tile_w);
}
inline void plan_split(ConvPlan& p, const gc_conv_desc* d, size_t room) {
    if (d->in_ch < 128) return;
    const long long wgs = (long long)p.tiles_x * p.tiles_y * d->batch * gc::ceil_div(d->out_ch, p.oct);
    const int want = (int)std::min<long long>(GC_SPLIT_TARGET / std::max<long long>(wgs, 1), d->in_ch / 64);
    if (want <= 1) return;
    const int kps = gc::ceil_div(gc::ceil_div(d->in_ch, want), KCB) * KCB, slices = gc::ceil_div(d->in_ch, kps);
    if (slices <= 1) return;
    p.slices = slices;
    p.k_per_split = kps;
    p.split = room >= p.slice_bytes(d);
}
// The wave-specialised kernels keep ONE workgroup resident per CU, so nothing overlaps a workgroup's start-up (two exposed load latencies) and its
// store drain: every workgroup takes ALL the consecutive tiles its CU would get over the rounds of the launch (the staging waves then run ahead
// into the next tile while the multiplying waves store the current one).
inline void plan_resident(ConvPlan& p, const gc_conv_desc* d) {
    const int tiles = p.tiles_x * p.tiles_y;
    const long long wgs = (long long)tiles * d->batch * (d->out_ch / p.oct);
    p.tpb = (int)std::min<long long>(std::max<long long>((wgs + GC_WS_SLOTS - 1) / GC_WS_SLOTS, 1), tiles);
    p.groups = gc::ceil_div(tiles, p.tpb);
    p.gx = (long long)p.groups * d->batch;
}

// The reduced epilogues of the wave-specialised kernels -- EPK 0: the full fused epilogue, 1: out_scale and / or residual only, 2: nothing; RES: a
// residual is added -- as the template arguments of the one instance a launch needs: launch(EPK constant, RES constant).
template <class Launch>
void with_ws_epilogue(const ConvArgs& c, bool bare, Launch&& launch) {
    const bool plain = bare && !c.bias && !c.noise && !c.act, res = c.residual != nullptr;
    const int epk = !plain ? 0 : ((c.so || res) ? 1 : 2);
    using std::integral_constant;
    if (epk == 2)             launch(integral_constant<int, 2>{}, std::false_type{});
    else if (epk == 1 && res) launch(integral_constant<int, 1>{}, std::true_type{});
    else if (epk == 1)        launch(integral_constant<int, 1>{}, std::false_type{});
    else if (res)             launch(integral_constant<int, 0>{}, std::true_type{});
    else                      launch(integral_constant<int, 0>{}, std::false_type{});
}

// defined in conv_s2ws.hip (split build only): the wave-specialised stride-2 3x3 kernel; plan_s2ws turns an unsplit one-role plan into its own
// (tiling and grid included) for the shapes the kernel takes and says whether it did
bool plan_s2ws(const gc_conv_desc* d, ConvPlan& p);
int launch_s2ws(const ConvPlan& p, const Bf16Args& a, hipStream_t s);

// Host functions that cross the units built in BOTH arithmetics: an inline namespace per arithmetic keeps the split and the -DGC_SINGLE
// definitions apart at link time (callers write the plain name).
#ifdef GC_SINGLE
#define GC_ARITH single
#else
#define GC_ARITH split
#endif
inline namespace GC_ARITH {
// convt_bf16x3.hip: the transposed 3x3 stride-2 convolution (up = 2, pad' = 2) -- its whole plan (ep: the launch's epilogue, read by the GC_CTWS experiments only) and its launcher
void plan_t(const gc_conv_desc* d, const gc_conv_epilogue* ep, size_t room, ConvPlan& p);
int launch_t(const ConvPlan& p, const Bf16Args& a, hipStream_t s);
bool wg_eligible(const gc_conv_desc* d);                // wgrad_bf16x3.hip: shapes the split-bf16 weight-gradient kernels take
}

}  // namespace gcconv

namespace {

using namespace gcconv;

// Eight values with one scale EACH (a channel-last patch unit: eight channels of one pixel) -> hi / lo bf16 units.  Plain v_mul_f32 /
// v_sub_f32 by asm: left to itself the compiler pairs neighbouring channels into v_pk_mul_f32 / v_pk_add_f32, and packed fp32 does not
// run under another wave's MFMA (profiles/pmc_r01.md, co-issue table) -- in the wave-specialised kernel the staging wave shares its SIMD
// with two multiplying waves, so every packed instruction is time taken from the matrix pipe.
// Two fp32 values -> one dword of two bf16 (a in the low half), round to nearest even: ONE v_cvt_pk_bf16_f32.  Written `(__bf16)f` element by
// element the compiler spends one conversion per VALUE on the hi parts (it needs each hi back as a float for the lo part) and v_perm to pair
// them up: 5.2 vector instructions per value in the staging loops (round 5, opcode histogram of the commit phase); from the PAIR the two hi
// parts come back as floats by one shift and one mask -- 3 per value unscaled, 4 scaled, the same bits.
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <bool SCALED>
__device__ __forceinline__ void split8s(const float (&v)[8], const float (&sc)[8], uint4* h, uint4* l) {
    unsigned hh[4], ll[4];
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
        float f0 = v[q], f1 = v[q + 1];
        if (SCALED) { asm("v_mul_f32 %0, %1, %2" : "=v"(f0) : "v"(v[q]), "v"(sc[q])); asm("v_mul_f32 %0, %1, %2" : "=v"(f1) : "v"(v[q + 1]), "v"(sc[q + 1])); }
        const unsigned pk = cvt_pk_bf16(f0, f1);
        const float t0 = __uint_as_float(pk << 16), t1 = __uint_as_float(pk & 0xffff0000u);
        float d0, d1;
        // the low part of a scaled value is taken from the EXACT product (one fused multiply-subtract), so the rounding of v * sc to fp32
        // is captured as well -- what the compiler's own contraction of `v * sc - hi` does
        if (SCALED) { asm("v_fma_f32 %0, %1, %2, -%3" : "=v"(d0) : "v"(v[q]), "v"(sc[q]), "v"(t0)); asm("v_fma_f32 %0, %1, %2, -%3" : "=v"(d1) : "v"(v[q + 1]), "v"(sc[q + 1]), "v"(t1)); }
        else        { asm("v_sub_f32 %0, %1, %2" : "=v"(d0) : "v"(f0), "v"(t0)); asm("v_sub_f32 %0, %1, %2" : "=v"(d1) : "v"(f1), "v"(t1)); }
        hh[q / 2] = pk;
        ll[q / 2] = cvt_pk_bf16(d0, d1);
    }
    *h = make_uint4(hh[0], hh[1], hh[2], hh[3]);
    *l = make_uint4(ll[0], ll[1], ll[2], ll[3]);
}


// LDS-DMA of one 1 KiB row: lane l copies 16 bytes from its own global address to (wave-uniform LDS address) + 16 l.  M0 carries the LDS
// address and is compiler-reserved: saved and restored inside the statement (cdna guide, "M0 ... write it in the same statement").
__device__ __forceinline__ void glds16(const void* gsrc, const void* lds_row) {
    const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(const __attribute__((address_space(3))) void*)lds_row);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

// The same with a wave-uniform 64-bit base (SGPR pair) and a 32-bit lane byte offset: no 64-bit vector address arithmetic, one VGPR per lane.
__device__ __forceinline__ void glds16_s(const void* sbase, unsigned voff, const void* lds_row) {
    const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(const __attribute__((address_space(3))) void*)lds_row);
    const unsigned long long sb = (unsigned long long)sbase;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)sb), hi = __builtin_amdgcn_readfirstlane((unsigned)(sb >> 32));
    const unsigned long long base = ((unsigned long long)hi << 32) | lo;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
}

// a + b / a * s, never contracted with a neighbouring operation
__device__ __forceinline__ float plain_sum(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float plain_mul(float a, float s) {
#pragma clang fp contract(off)
    return a * s;
}

}  // namespace
