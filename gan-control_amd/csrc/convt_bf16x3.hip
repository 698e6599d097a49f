// Transposed 3x3 stride-2 convolution in split-bf16 (the arithmetic, the packed weights and the argument block: conv_bf16x3.hip,
// conv_bf16x3_shared.h): the fused four-phase kernel, the edge kernel of the (2H + 1) x (2W + 1) geometry and their dispatcher.
#include "conv_common.h"
#include "conv_bf16x3_shared.h"

namespace {

using namespace gcconv;

// Transposed 3x3 stride-2 convolution (up = 2, pad' = 2: ModulatedConv2d's up-sampling branch gan_model.py:295-306
// and the input gradient of every 3x3 stride-2 conv) with the four output phases FUSED in one workgroup.
// Output pixel (2q + py, 2q' + px) of phase (py, px) reads input pixels q + {-1, 0}: all phases share the same
// 2x2 input neighbourhood, so a tile of q positions is staged once and each lane keeps one accumulator per phase.
// Taps per axis: phase 0 -> (t = 0, d = -1), (t = 2, d = 0); phase 1 -> (t = 1, d = 0): 9 (phase, tap) pairs = the
// MFMA count of a plain 3x3 tile, every workgroup does the same work, and B fragments are shared across phases.
template <int WG_OC, int WG_PX, int WPX, int TPW>
struct TCfg {
    static constexpr int OCT = WG_OC * 32, RPB = 32 / TPW;
    static constexpr int TQH = WG_PX * WPX * RPB;
    static constexpr int PH = TQH + 1, PWD = TPW + 1, PLANE = PH * PWD;
    static constexpr int WUNITS = 9 * KG * OCT, PUNITS = KG * PLANE;
    static constexpr int SMEM_UNITS = 2 * (WUNITS + PUNITS);
    static constexpr int NWU = (WUNITS + 255) / 256;
};

// EPI: 0 = store the accumulators as they are (input-gradient launches), 1 = out_scale only (modulated up-sampling
// convolution), 2 = the full fused epilogue.  The epilogue is ~6 VALU instructions per output element on 256 elements per
// lane; compiled out where the launch does not need it (bare stores are 10 % faster at <= 128 input channels).
#ifndef GC_CT_OCC32
#define GC_CT_OCC32 2        // workgroups per CU the 32-output-channel instance (WG_OC = 1: the store-bound 64 -> 32 @512^2 layer) is compiled for
#endif
template <int WG_OC, int WG_PX, int WPX, int TPW, int EPI, bool WDMA = false>
__global__ __launch_bounds__(256, WG_OC == 1 ? GC_CT_OCC32 : 2) void convt_fused_bf16x3_kernel(Bf16Args a) {
    using C = TCfg<WG_OC, WG_PX, WPX, TPW>;
    static_assert(WG_OC * WG_PX == 4, "4 waves per workgroup");
    constexpr int OCT = C::OCT, RPB = C::RPB, TQH = C::TQH, PWD = C::PWD, PLANE = C::PLANE;
    const ConvArgs& p = a.c;
    __shared__ uint4 smem[C::SMEM_UNITS];
    uint4* wl_h = smem;                         // [tap][kg][OCT]
    uint4* wl_l = wl_h + C::WUNITS;
    uint4* p_h = wl_l + C::WUNITS;              // [kg][PH][PWD]
    uint4* p_l = p_h + C::PUNITS;
    __shared__ __attribute__((aligned(16))) float s_so[OCT], s_bias[OCT];    // out_scale / bias of this workgroup's channels (see conv_epilogue)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wave_px = wave % WG_PX, wave_oc = wave / WG_PX;

    int bid = blockIdx.x;
    const int tile_x = bid % p.tiles_x; bid /= p.tiles_x;
    const int tile_y = bid % p.tiles_y;
    const int b = bid / p.tiles_y;
    const int n0 = blockIdx.y * OCT;
    if (EPI > 0 && tid < OCT) {                 // read in the epilogue, many barriers later
        const int oc = min(n0 + tid, p.N - 1);
        s_so[tid] = p.so ? p.so[(size_t)b * p.N + oc] : 1.f;
        s_bias[tid] = p.bias ? p.bias[oc] : 0.f;
    }
    const int qy0 = tile_y * TQH, qx0 = tile_x * TPW;

    f32x16 acc[4][WPX];
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int j = 0; j < WPX; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ph][j][r] = 0.f;

    int boff[WPX];
#pragma unroll
    for (int j = 0; j < WPX; ++j) boff[j] = hi * PLANE + ((wave_px * WPX + j) * RPB + l31 / TPW) * PWD + l31 % TPW;
    const int aoff = hi * OCT + wave_oc * 32 + l31;

    const float* xb = p.x + (size_t)b * p.K * p.in_h * p.in_w;
    const float* sib = p.si ? p.si + (size_t)b * p.K : nullptr;
    const int chan = p.in_h * p.in_w;
    const int iy0 = qy0 - 1, ix0 = qx0 - 1;

    // WDMA (not launched: no launcher instantiates the `true` form.  It measured slower at >= 256 input channels -- DESIGN.md, "Tried and rejected" --
    // and its code stays only because taking it out changes the register allocation of the 32-output-channel instance, which a refactor
    // that pins every kernel instruction by instruction cannot do: profiles/isa_identity_knob_retirement.md): the weight slab never touches a register.  Its rows ([tap][kg] x OCT units, contiguous in HBM and in LDS) are copied by
    // LDS-DMA into the SINGLE weight stage right after the barrier that ends the MFMA phase -- every wave has read its fragments by then --
    // and land while the patch of the next chunk is converted and written; vmcnt(0) before the second barrier.  40 registers and
    // 10 ds_write_b128 per lane and chunk less than the register path.
    uint4 wreg_h[WDMA ? 1 : C::NWU], wreg_l[WDMA ? 1 : C::NWU];
#ifdef GC_SINGLE
    constexpr int DROWS = 9 * KG;
#else
    constexpr int DROWS = 2 * 9 * KG;
#endif
    constexpr int RPI = 64 / OCT, DINSTR = DROWS / RPI;
    static_assert(!WDMA || (DROWS % RPI == 0 && (9 * KG) % RPI == 0), "row groups do not straddle the hi / lo halves");
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto dma_weights = [&](int k0) {
#pragma unroll
        for (int j = 0; j < (DINSTR + 3) / 4; ++j) {
            const int q = wave_u + 4 * j;
            if (4 * j + 3 < DINSTR || q < DINSTR) {
                const int r0 = q * RPI;
                const int half = r0 / (9 * KG), rr0 = r0 % (9 * KG);
                const int rr = rr0 + lane / OCT;
                const int t = rr / KG, kg = rr % KG;
                const uint4* src = (half ? a.wl : a.wh) + ((size_t)(t * a.kgroups + k0 / 8 + kg) * p.N + n0 + lane % OCT);
                glds16(src, (half ? wl_l : wl_h) + rr0 * OCT);
            }
        }
    };
    // Patch staging as in conv_bf16x3_kernel: a lane fetches FOUR consecutive pixels of a channel with one 16-byte load (eight
    // channels = eight loads) and transposes them in registers into four channel-last units.  The texture-address unit spends
    // ~16 cycles per wave-level load whatever its width; with 24 dword loads per lane per chunk that was more than the MFMAs of a
    // chunk at <= 64 output channels.  A patch row is the halo column (one pixel, "edge" task) + TPW / 4 aligned groups.
    constexpr int GR = TPW / 4, TASKS = C::PH * (GR + 1);
    static_assert(TASKS <= 128, "one staging task per lane and channel group");
    __shared__ __attribute__((aligned(16))) float s_si[MAX_K_BF16X3 + KCB];     // in_scale of this sample, zero past K (a ragged last chunk contributes nothing)
    for (int k = tid; k < ((p.K + KCB - 1) / KCB) * KCB; k += 256) s_si[k] = k < p.K ? (sib ? sib[k] : 1.f) : 0.f;
    const int kgl_p = __builtin_amdgcn_readfirstlane(tid >> 7), tb = tid & 127;     // waves 0,1: channel group 0; waves 2,3: group 1
    const int t_row = tb / (GR + 1), t_g = tb % (GR + 1);
    const int t_col = t_g == 0 ? 0 : 4 * t_g - 3, t_used = tb < TASKS ? (t_g == 0 ? 1 : 4) : 0;
    uint4 preg[8];
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(xb, (unsigned)p.K * chan * 4u);
    const unsigned wbytes = 9u * a.kgroups * p.N * 16u;
    const __amdgpu_buffer_rsrc_t rwh = make_rsrc(a.wh, wbytes), rwl = make_rsrc(a.wl, wbytes);
    auto prefetch = [&](int k0) {
        const int t_ = tid;
        if (!WDMA) {
#pragma unroll
            for (int j = 0; j < C::NWU; ++j) {
                const int u = t_ + 256 * j;
                const int oc = u % OCT, rest = u / OCT;
                const int kgl = rest % KG, tap = rest / KG;
                const int kg = k0 / 8 + kgl, n = n0 + oc;
                const bool ok = u < C::WUNITS && kg < a.kgroups && n < p.N;
                const unsigned gb = ok ? (unsigned)((tap * a.kgroups + kg) * p.N + n) * 16u : OOB;
                wreg_h[j] = (GC_CT_ABL & 4) ? make_uint4(gb, gb, gb, gb) : buf_load_u128(rwh, gb, 0);
                wreg_l[j] = (GC_CT_ABL & 4) ? make_uint4(gb, gb, gb, gb) : buf_load_u128(rwl, gb, 0);
            }
        }
        const int iy = iy0 + t_row, ix = ix0 + t_col;
        const bool ok = t_used > 0 && iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w;
        const unsigned boff_ = ok ? (unsigned)(iy * p.in_w + ix) * 4u : OOB;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = min(k0 + kgl_p * 8 + q, p.K - 1);          // wave-uniform -> scalar offset
            preg[q] = (GC_CT_ABL & 4) ? make_uint4(boff_, k, boff_ + 1, k + 1) : buf_load_u128(rx, boff_, (unsigned)k * chan * 4u);
        }
    };
    auto commit = [&](int k0) {
        wait_staged_loads();
        const int t_ = tid;
        if (WDMA) {
            if (!(GC_CT_ABL & 4)) dma_weights(k0);          // in flight during the conversion below
        } else {
#pragma unroll
            for (int j = 0; j < C::NWU; ++j) {
                const int u = t_ + 256 * j;
                if (u < C::WUNITS) { wl_h[u] = wreg_h[j]; GC_LO(wl_l[u] = wreg_l[j];) }
            }
        }
        const float4 sa = *reinterpret_cast<const float4*>(&s_si[k0 + kgl_p * 8]), sb = *reinterpret_cast<const float4*>(&s_si[k0 + kgl_p * 8 + 4]);
        const float sc[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
        const int inrow = p.in_w - (ix0 + t_col);                    // pixels of this group that are still inside the image row
        const int ubase = kgl_p * PLANE + t_row * PWD + t_col;
        if (GC_CT_ABL & 8) {        // ablation: what a pre-split input would leave of the staging -- the loaded registers go to LDS as they are
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < t_used) { p_h[ubase + i] = preg[i]; p_l[ubase + i] = preg[4 + i]; }
        } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned raw = i == 0 ? preg[q].x : (i == 1 ? preg[q].y : (i == 2 ? preg[q].z : preg[q].w));
                v[q] = i < inrow ? __uint_as_float(raw) : 0.f;
            }
            uint4 h, l;
            if (p.si) split8s<true>(v, sc, &h, &l);        // plain (un-packed) multiplies and subtractions: see split8s
            else      split8s<false>(v, sc, &h, &l);       // D's input-gradient launches: no per-sample scale, no multiply by one
            if (i < t_used) {
                p_h[ubase + i] = h;
                GC_LO(p_l[ubase + i] = l;)
            }
        }
        }
        if (WDMA) wait_staged_loads();           // the LDS-DMA rows of this wave have landed (untracked by the compiler: counted by hand)
    };

    // split over the input channels (small planes, see plan_splitk_bf16): slice blockIdx.z covers [kz0, kz1) and stores raw partial sums
    const int kz0 = a.k_per_split ? (int)blockIdx.z * a.k_per_split : 0;
    const int kz1 = a.k_per_split ? min(p.K, kz0 + a.k_per_split) : p.K;
    prefetch(kz0);
    __syncthreads();        // s_si
    commit(kz0);
    __syncthreads();
    for (int k0 = kz0; k0 < kz1; k0 += KCB) {
        wait_staged_loads();    // no-op in hardware (commit retired them); clears the compiler's pending-load model at the loop header
        const bool more = k0 + KCB < kz1;
        prefetch(more ? k0 + KCB : k0);       // unconditional: a conditional prefetch merges through register copies, which wait for the loads
        __builtin_amdgcn_s_setprio(GC_MFMA_PRIO);
        if (!(GC_CT_ABL & 2)) {
            // The nine (phase, tap) steps of a chunk as one software pipeline: the weight fragment of step s + 1 -- and the patch fragments of the
            // next neighbour group when the group changes -- are read BEFORE the MFMAs of step s (scheduling barriers pin the order); the compiler's
            // own order waited `lgkmcnt(0)` a dozen times per chunk with one to five MFMAs in between.
            // step s -> neighbour group g = (dyi, dxi): s = 0: (0,0); 1, 2: (0,1); 3, 4: (1,0); 5..8: (1,1)
            bf16x8 fbh[WDMA ? 2 : 1][WPX], fbl[WDMA ? 2 : 1][WPX], fah[2], fal[2];
            auto grp = [](int s_) { return s_ == 0 ? 0 : (s_ < 3 ? 1 : (s_ < 5 ? 2 : 3)); };
            auto load_b = [&](int g, int set) {
                const int dyi = g >> 1, dxi = g & 1;
#pragma unroll
                for (int j = 0; j < WPX; ++j) {
                    const uint4 uh = p_h[boff[j] + dyi * PWD + dxi];
                    fbh[set][j] = *reinterpret_cast<const bf16x8*>(&uh);
                    GC_LO(const uint4 ul = p_l[boff[j] + dyi * PWD + dxi]; fbl[set][j] = *reinterpret_cast<const bf16x8*>(&ul);)
                }
            };
            auto step_of = [&](int s_, int& py, int& px, int& ty, int& tx) {
                const int g = grp(s_), dyi = g >> 1, dxi = g & 1;
                const int iy = g == 2 ? s_ - 3 : (g == 3 ? (s_ - 5) >> 1 : 0), ix = g == 1 ? s_ - 1 : (g == 3 ? (s_ - 5) & 1 : 0);
                py = (dyi == 1 && iy == 1) ? 1 : 0; ty = dyi == 0 ? 0 : (iy == 0 ? 2 : 1);
                px = (dxi == 1 && ix == 1) ? 1 : 0; tx = dxi == 0 ? 0 : (ix == 0 ? 2 : 1);
            };
            auto load_a = [&](int s_, int set) {
                int py, px, ty, tx;
                step_of(s_, py, px, ty, tx);
                const int wbase = (ty * 3 + tx) * KG * OCT + aoff;
                const uint4 uh = wl_h[wbase];
                fah[set] = *reinterpret_cast<const bf16x8*>(&uh);
                GC_LO(const uint4 ul = wl_l[wbase]; fal[set] = *reinterpret_cast<const bf16x8*>(&ul);)
            };
            // (two sets of patch fragments only where the registers allow it: with the weight slab staged through registers -- WDMA = false,
            // 40 more live registers -- the second set spilled INSIDE the chunk loop, a scratch reload in front of every prefetch pair)
            constexpr int BSETS = WDMA ? 2 : 1;
            load_b(0, 0);
            load_a(0, 0);
#pragma unroll
            for (int s_ = 0; s_ < 9; ++s_) {
                if (BSETS == 1 && s_ > 0 && grp(s_) != grp(s_ - 1)) load_b(grp(s_), 0);
                if (s_ + 1 < 9) {
                    load_a(s_ + 1, (s_ + 1) & 1);
                    if (BSETS == 2 && grp(s_ + 1) != grp(s_)) load_b(grp(s_ + 1), grp(s_ + 1) & 1);
                }
                __builtin_amdgcn_sched_barrier(0);
                int py, px, ty, tx;
                step_of(s_, py, px, ty, tx);
                const int bs = BSETS == 2 ? grp(s_) & 1 : 0;
#pragma unroll
                for (int j = 0; j < WPX; ++j) { GC_MFMA3(acc[py * 2 + px][j], fah[s_ & 1], fal[s_ & 1], fbh[bs][j], fbl[bs][j]); }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else
#pragma unroll
        for (int dyi = 0; dyi < 2; ++dyi) {
#pragma unroll
            for (int dxi = 0; dxi < 2; ++dxi) {
                bf16x8 bh[WPX], bl[WPX];
#pragma unroll
                for (int j = 0; j < WPX; ++j) {
                    const uint4 uh = p_h[boff[j] + dyi * PWD + dxi], ul = p_l[boff[j] + dyi * PWD + dxi];
                    bh[j] = *reinterpret_cast<const bf16x8*>(&uh);
                    bl[j] = *reinterpret_cast<const bf16x8*>(&ul);
                }
                // (phase, tap) pairs reading the neighbour at offset d = dyi - 1: d = -1 -> (0, t=0); d = 0 -> (0, t=2), (1, t=1)
#pragma unroll
                for (int iy = 0; iy < 1 + dyi; ++iy) {
                    const int py = (dyi == 1 && iy == 1) ? 1 : 0, ty = dyi == 0 ? 0 : (iy == 0 ? 2 : 1);
#pragma unroll
                    for (int ix = 0; ix < 1 + dxi; ++ix) {
                        const int px = (dxi == 1 && ix == 1) ? 1 : 0, tx = dxi == 0 ? 0 : (ix == 0 ? 2 : 1);
                        const int wbase = (ty * 3 + tx) * KG * OCT + aoff;
                        const uint4 uh = wl_h[wbase], ul = wl_l[wbase];
                        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&uh), al = *reinterpret_cast<const bf16x8*>(&ul);
#pragma unroll
                        for (int j = 0; j < WPX; ++j) {
                            f32x16 c = acc[py * 2 + px][j];
                            if (GC_CT_ABL & 2) { c[0] += __builtin_bit_cast(float, ((const uint4&)ah).x ^ ((const uint4&)bh[j]).x ^ ((const uint4&)al).x ^ ((const uint4&)bl[j]).x); }
                            else { GC_MFMA3(c, ah, al, bh[j], bl[j]); }
                            acc[py * 2 + px][j] = c;
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        __syncthreads();
        if (!more) break;       // leave here: no path may reach the loop header with staged loads in flight
        {
            commit(k0 + KCB);
            __syncthreads();
        }
    }

    // The phases px = 0 / 1 of one input column are NEIGHBOURS in the output row: they leave as one 8-byte store (4-byte aligned:
    // rows of a 1025-wide plane start anywhere), half the store instructions and whole 128-byte segments per 16 lanes.
    typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
    const int opitch = a.out_pitch;          // rows of a (2H + 1)-wide output are never 16-byte aligned: a pitch that is a multiple of 32 floats gives every 128-byte store run whole cache lines
    float* yb = (a.k_per_split ? a.part + (size_t)blockIdx.z * a.per_slice : p.y) + (size_t)b * p.N * p.out_h * opitch;
    const EpilogueConsts ec = epilogue_consts(p);
    float nz[WPX][2][2];         // fetched before the first store: a load between stores waits for every store before it
#pragma unroll
    for (int j = 0; j < WPX; ++j) {
        const int qy = qy0 + (wave_px * WPX + j) * RPB + l31 / TPW, qx = qx0 + l31 % TPW;
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            const int oy = min(2 * qy + (ph >> 1), p.out_h - 1), ox = min(2 * qx + (ph & 1), p.out_w - 1);
            nz[j][ph >> 1][ph & 1] = (EPI == 2 && p.noise) ? p.noise[((size_t)b * p.out_h + oy) * p.out_w + ox] : 0.f;
        }
    }
    // out_scale / bias of this lane's 16 channels (four runs of four consecutive ones), fetched ONCE before the store loops: read at each
    // store they cost one exposed LDS round trip per output pair (round 5, found in the disassembly: 124 of 128 stores behind an lgkmcnt wait)
    float so16[16], bi16[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 s4 = EPI > 0 ? *reinterpret_cast<const float4*>(&s_so[wave_oc * 32 + 8 * q + 4 * hi]) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 b4 = EPI == 2 ? *reinterpret_cast<const float4*>(&s_bias[wave_oc * 32 + 8 * q + 4 * hi]) : make_float4(0.f, 0.f, 0.f, 0.f);
        so16[4 * q] = s4.x; so16[4 * q + 1] = s4.y; so16[4 * q + 2] = s4.z; so16[4 * q + 3] = s4.w;
        bi16[4 * q] = b4.x; bi16[4 * q + 1] = b4.y; bi16[4 * q + 2] = b4.z; bi16[4 * q + 3] = b4.w;
    }
#pragma unroll
    for (int j = 0; j < WPX; ++j) {
        const int qy = qy0 + (wave_px * WPX + j) * RPB + l31 / TPW, qx = qx0 + l31 % TPW;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            const int oy = 2 * qy + py, ox = 2 * qx;
            if (oy >= p.out_h || ox >= p.out_w) continue;
            const bool pair = ox + 1 < p.out_w;
            float res[2][16];
            if (EPI == 2 && p.residual) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int oc = min(n0 + wave_oc * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi, p.N - 1);
                    const float* rp = p.residual + (((size_t)b * p.N + oc) * p.out_h + oy) * p.out_w + ox;
                    res[0][r] = rp[0];
                    res[1][r] = pair ? rp[1] : 0.f;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ocl = wave_oc * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (n0 + ocl < p.N) {
                    float v0 = acc[py * 2][j][r], v1 = acc[py * 2 + 1][j][r];
                    if (EPI == 1) { v0 *= so16[r]; v1 *= so16[r]; }
                    if (EPI == 2) { v0 = conv_epilogue(ec, v0, so16[r], bi16[r], nz[j][py][0]); v1 = conv_epilogue(ec, v1, so16[r], bi16[r], nz[j][py][1]); }
                    if (EPI == 2 && p.residual) { v0 += res[0][r]; v1 += res[1][r]; }
                    float* yp = yb + ((size_t)(n0 + ocl) * p.out_h + oy) * opitch + ox;
                    if ((GC_CT_ABL & 1) && v0 != 12345.678f) continue;
#if GC_CONV_NT
                    if (pair) { f2u v = {v0, v1}; __builtin_nontemporal_store(v, reinterpret_cast<f2u*>(yp)); }
                    else __builtin_nontemporal_store(v0, yp);
#else
                    if (pair) { f2u v = {v0, v1}; *reinterpret_cast<f2u*>(yp) = v; }
                    else yp[0] = v0;
#endif
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// The last output row and column of a (2H + 1) x (2W + 1) transposed convolution (round 5).  q-space is (H + 1) x (W + 1): the kernel above
// tiles it in 4 x 32 or 8 x 16 blocks, and at H = W = 32 / 64 / 128 the one extra q-row and q-column cost 47 / 29 / 16 % more tiles than the
// H x W region, which tiles exactly.  With GC_CT_EDGE the fused kernel is launched over the H x W region only (output rows 0 .. 2H - 1, columns
// 0 .. 2W - 1) and this kernel computes the rest: output row 2H (2W + 1 values, from input row H - 1 under the taps ty = 0) and output column 2W
// (2H values, from input column W - 1 under the taps tx = 0) -- 1-D problems, (H + W + 1) q-positions of three taps each instead of H + W + 1
// positions padded to whole 2-D tiles.  One workgroup = 32 q-positions x 64 output channels; its four waves take a quarter of the input
// channels each, straight from global memory into registers (no LDS staging: 16 scalar loads of x and 12 16-byte loads of the packed weights
// per lane and chunk, two chunks in flight), and wave 0 adds the quarters in a fixed order and applies the epilogue.
// Same arithmetic as the fused kernel (split operands, three MFMAs per product); the sums run over the quarters one after the other instead
// of chunk by chunk, so the edge values differ from the one-kernel form in the last bits.
#ifndef GC_CT_EDGE
#define GC_CT_EDGE 1
#endif
#ifndef GC_CT_EDGE_MIN_WGS
#define GC_CT_EDGE_MIN_WGS 512      // workgroups of the main region from which the two-launch form is used (see ct_edge_eligible)
#endif
__global__ __launch_bounds__(256) void convt_edge_bf16x3_kernel(Bf16Args a) {
    const ConvArgs& p = a.c;
    __shared__ float red[3][64][64];                       // [wave - 1][accumulator register][lane]
    const int H = p.in_h, W = p.in_w, chan = H * W;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rblocks = (W + 1 + 31) / 32;                 // blocks of the bottom row first, then those of the right column
    const bool col = (int)blockIdx.x >= rblocks;
    const int e = ((int)blockIdx.x - (col ? rblocks : 0)) * 32 + l31;         // q-position along the edge
    const int n0 = blockIdx.y * 64, b = blockIdx.z;
    // the two input pixels of this position: `cur` (offset d = 0) and `prev` (d = -1) along the edge
    const bool okc = col ? e < H : e < W, okp = col ? (e >= 1 && e < H) : (e >= 1 && e <= W);
    const int cur = okc ? (col ? e * W + W - 1 : (H - 1) * W + e) : 0;
    const int prev = okp ? (col ? (e - 1) * W + W - 1 : (H - 1) * W + e - 1) : 0;
    // taps: prev -> phase 0 under (0, 0); cur -> phase 0 under (0, 2) | (2, 0) and -> phase 1 under (0, 1) | (1, 0)
    const int tB = col ? 6 : 2, tC = col ? 3 : 1;
    const float* xb = p.x + (size_t)b * p.K * chan;
    const float* sib = p.si ? p.si + (size_t)b * p.K : nullptr;
    const int chunks = p.K / KCB, c0 = wave * chunks / 4, c1 = (wave + 1) * chunks / 4;
    f32x16 acc[2][2];
#pragma unroll
    for (int ph = 0; ph < 2; ++ph)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ph][i][r] = 0.f;
#pragma unroll 2
    for (int c = c0; c < c1; ++c) {
        const int kb = c * KCB + hi * 8;
        float vp[8], vc[8], sc[8];
        // `prev` of a lane is `cur` of the lane before it: only the first lane of each 32-lane half loads it (a column block's loads touch one
        // cache line per lane -- 64 line requests per instruction -- so loading both pixels everywhere doubled what the texture unit had to do)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            vc[q] = xb[(size_t)(kb + q) * chan + cur];
            vp[q] = l31 == 0 ? xb[(size_t)(kb + q) * chan + prev] : 0.f;
            sc[q] = sib ? sib[kb + q] : 1.f;
        }
        uint4 wa_h[2], wa_l[2], wb_h[2], wb_l[2], wc_h[2], wc_l[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const size_t col_ = (size_t)n0 + i * 32 + l31, kg = c * KG + hi;
            wa_h[i] = a.wh[(0 * (size_t)a.kgroups + kg) * p.N + col_];  GC_LO(wa_l[i] = a.wl[(0 * (size_t)a.kgroups + kg) * p.N + col_];)
            wb_h[i] = a.wh[(tB * (size_t)a.kgroups + kg) * p.N + col_]; GC_LO(wb_l[i] = a.wl[(tB * (size_t)a.kgroups + kg) * p.N + col_];)
            wc_h[i] = a.wh[(tC * (size_t)a.kgroups + kg) * p.N + col_]; GC_LO(wc_l[i] = a.wl[(tC * (size_t)a.kgroups + kg) * p.N + col_];)
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            vc[q] = okc ? vc[q] : 0.f;
            const float up = __shfl_up(vc[q], 1, 32);             // (zero where the lane before is past the plane, like its own `cur`)
            vp[q] = okp ? (l31 == 0 ? vp[q] : up) : 0.f;
        }
        uint4 ph_, pl_, ch_, cl_;
        if (sib) { split8s<true>(vp, sc, &ph_, &pl_); split8s<true>(vc, sc, &ch_, &cl_); }
        else     { split8s<false>(vp, sc, &ph_, &pl_); split8s<false>(vc, sc, &ch_, &cl_); }
        const bf16x8 bph = *reinterpret_cast<const bf16x8*>(&ph_), bch = *reinterpret_cast<const bf16x8*>(&ch_);
        GC_LO(const bf16x8 bpl = *reinterpret_cast<const bf16x8*>(&pl_); const bf16x8 bcl = *reinterpret_cast<const bf16x8*>(&cl_);)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&wa_h[i]), bh = *reinterpret_cast<const bf16x8*>(&wb_h[i]), chh = *reinterpret_cast<const bf16x8*>(&wc_h[i]);
            GC_LO(const bf16x8 al = *reinterpret_cast<const bf16x8*>(&wa_l[i]); const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&wb_l[i]); const bf16x8 cll = *reinterpret_cast<const bf16x8*>(&wc_l[i]);)
            GC_MFMA3(acc[0][i], ah, al, bph, bpl);
            GC_MFMA3(acc[0][i], bh, bl, bch, bcl);
            GC_MFMA3(acc[1][i], chh, cll, bch, bcl);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[wave - 1][(ph * 2 + i) * 16 + r][lane] = acc[ph][i][r];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ph][i][r] += red[w][(ph * 2 + i) * 16 + r][lane];
    // Epilogue in two phases like the other kernels: every value this lane needs (out_scale / bias of its 32 channels, noise, residual) is loaded BEFORE
    // the first store -- a load between two stores waits for every store issued so far, and as first written (loads inside the store loop) this
    // kernel took 45 us, most of it in 64 such round trips.
    const EpilogueConsts ec = epilogue_consts(p);
    const int opitch = a.out_pitch;
    float so_[2][16], bi_[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            so_[i][r] = p.so ? p.so[(size_t)b * p.N + n] : 1.f;
            bi_[i][r] = p.bias ? p.bias[n] : 0.f;
        }
    int oy_[2], ox_[2];
    bool ok_[2];
    float nz_[2];
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
        oy_[ph] = col ? 2 * e + ph : 2 * H;
        ox_[ph] = col ? 2 * W : 2 * e + ph;
        ok_[ph] = oy_[ph] < p.out_h && ox_[ph] < p.out_w && !(col && e >= H);
        nz_[ph] = (p.noise && ok_[ph]) ? p.noise[((size_t)b * p.out_h + oy_[ph]) * p.out_w + ox_[ph]] : 0.f;
    }
    if (p.residual) {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = n0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const float rv = ok_[ph] ? p.residual[(((size_t)b * p.N + n) * p.out_h + oy_[ph]) * p.out_w + ox_[ph]] : 0.f;
                    acc[ph][i][r] = conv_epilogue(ec, acc[ph][i][r], so_[i][r], bi_[i][r], nz_[ph]) + rv;
                }
    } else {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ph][i][r] = conv_epilogue(ec, acc[ph][i][r], so_[i][r], bi_[i][r], nz_[ph]);      // absent parts are exact no-ops (conv_common.h)
    }
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
        if (!ok_[ph]) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                p.y[(((size_t)b * p.N + n) * p.out_h + oy_[ph]) * opitch + ox_[ph]] = acc[ph][i][r];
            }
    }
}

// the launches that take the H x W main region + edge form: the (2H + 1) x (2W + 1) geometry, whole chunks and 64-channel output blocks, >= 256 input
// channels (below that the layer is bound by its stores, not by its tiles), an H x W region that the 4 x 32 tile covers exactly, and >= 10 % fewer tiles
// than the whole q-space has in the tiling `p` gave it
inline bool ct_edge_eligible(const gc_conv_desc* d, const ConvPlan& p) {
    if (!GC_CT_EDGE || d->out_h != 2 * d->in_h + 1 || d->out_w != 2 * d->in_w + 1) return false;
    if (d->in_ch % KCB != 0 || d->in_ch < 256 || d->in_ch / KCB < 4 || d->out_ch % 64 != 0 || d->in_w % 32 != 0 || d->in_h % 4 != 0) return false;
    const long long full = (long long)p.tiles_x * p.tiles_y, main_ = (long long)(d->in_w / 32) * (d->in_h / 4);
    // ... and enough workgroups for two per CU: with one per CU nothing overlaps its staging (512 -> 512 @32^2, B = 4: 256 workgroups, 127 -> 137 us;
    // 512 -> 256 @64^2, B = 2: 99 -> 133 us -- against B = 8 / B = 4 of the same layers: 226 -> 175, 197 -> 162 us; profiles/convt_ab_r05.log)
    return 10 * main_ <= 9 * full && main_ * d->batch * (d->out_ch / 64) >= GC_CT_EDGE_MIN_WGS;
}

// ---------------------------------------------------------------------------------------------------------
// Wave-specialised form of the transposed 3x3 convolution above (round 4): same geometry, same packed weights, same pitched output and
// the same order of accumulation per output element (bit-identical results), on the structure of conv_bf16x3_ws_kernel -- ONE workgroup
// of 12 waves per CU, eight MULTIPLYING waves that issue nothing but LDS fragment reads and MFMAs, four STAGING waves (loads of the item
// after next in flight while the next item is converted), one barrier per item.  convt_fused_bf16x3_kernel spends 22-31 % of its time
// waiting for the patch of the next chunk (GC_CT_ABL = 4) because four accumulator sets (128 registers) leave room for ONE chunk of
// prefetch at two workgroups per CU.  Here the four output phases are produced in TWO PASSES over the input channels:
//   pass 0: output rows 2 qy     = phases (0,0), (0,1): taps ty in {0, 2} -> 6 taps, patch rows qy - 1 and qy
//   pass 1: output rows 2 qy + 1 = phases (1,0), (1,1): tap  ty = 1       -> 3 taps, patch row qy
// so a multiplying wave carries 2 phases x 2 pixel blocks x 32 oc = 64 accumulator registers, as in the stride-1 kernel.  The patch of a
// chunk is staged once per pass (twice per chunk: 1.9 x the conversions per MFMA of the stride-1 kernel, well inside what four staging
// waves do), the weight slab of a (pass, chunk) item is its 6 or 3 tap rows.  An item is short (36 / 18 MFMAs per wave), shorter than an
// LDS-DMA round trip: the weight slabs therefore live in a THREE-slot ring filled TWO items ahead (the DMA of item i + 2 is issued at the
// start of item i), and completion is counted by hand -- at the end of item i a wave waits `vmcnt(n)` with n = the DMA instructions it has
// just issued for item i + 2; loads complete in order, so everything older (the rows of item i + 1, and any store of a finished tile) is
// done, whatever the stores' own completion order.
// MEASURED AND NOT ENABLED (round 4, tools/kbench.py, B = 4, same box; profiles/convt_ws_r04.md): correct on every test shape and bit-identical
// run to run, but no faster than the one-role kernel -- 512 -> 256 @64^2 199 vs 213 us, 256 -> 128 @128^2 190 vs 180, 128 -> 64 @256^2 205 vs 191,
// 64 -> 32 @512^2 302 vs 243.  Ablation builds (GC_CTWS_ABL) say why: with neither patch staging nor weight DMA the multiplying side alone
// runs 159 / 131 / 125 / 173 us -- (i) the (H + 1)^2 q-space of a (2H + 1)-wide output tiles badly (65 = 4 x 16 + 1: 66 % of the MFMA work of a
// 512 -> 256 @64^2 launch is useful) and one long-lived workgroup per CU quantises what is left (208 of 256 CUs busy); (ii) at <= 128 input
// channels the second pass re-reads the patch the layer is HBM-bound on (64 -> 32: 170 us without patch staging).  An edge-row / edge-column
// path that would make the main region H x H (perfect tiling: ~115 us projected for 512 -> 256) is the open continuation.
#ifndef GC_CTWS
#define GC_CTWS 0             // 1: transposed 3x3 convolutions with K % 16 == 0, N % 32 == 0 on convt_bf16x3_ws_kernel
#endif
#ifndef GC_CTWS_ABL
#define GC_CTWS_ABL 0         // dev ablations (wrong results): 1 no patch staging, 2 no weight DMA, 8 no stores
#endif
#if GC_CTWS
#include "experiments/convt_ws.inc.h"
#endif      // GC_CTWS

template <int WG_OC, int WG_PX, int WPX, int TPW>
int launch_t_inst(const ConvPlan& p, const Bf16Args& a, hipStream_t s) {
    using C = TCfg<WG_OC, WG_PX, WPX, TPW>;
    dim3 grid((unsigned)p.gx, gc::ceil_div(a.c.N, C::OCT), p.split ? p.slices : 1);
    const int epi = (a.c.bias || a.c.noise || a.c.act || a.c.residual) ? 2 : (a.c.so ? 1 : 0);
    if (epi == 2)      hipLaunchKernelGGL((convt_fused_bf16x3_kernel<WG_OC, WG_PX, WPX, TPW, 2>), grid, dim3(256), 0, s, a);
    else if (epi == 1) hipLaunchKernelGGL((convt_fused_bf16x3_kernel<WG_OC, WG_PX, WPX, TPW, 1>), grid, dim3(256), 0, s, a);
    else               hipLaunchKernelGGL((convt_fused_bf16x3_kernel<WG_OC, WG_PX, WPX, TPW, 0>), grid, dim3(256), 0, s, a);
    return gc::check_launch("gc_conv2d_bf16x3_f32(fused transposed)");
}

template <int WG_OC, int WG_PX, int WPX, int TPW>
void set_t(ConvPlan& p, ConvPath path) {
    using C = TCfg<WG_OC, WG_PX, WPX, TPW>;
    p.path = path;
    p.t[0] = WG_OC; p.t[1] = WG_PX; p.t[2] = WPX; p.t[3] = TPW;
    p.tile_h = C::TQH; p.tile_w = TPW; p.oct = C::OCT;
}

}  // namespace

namespace gcconv {
inline namespace GC_ARITH {

void plan_t(const gc_conv_desc* d, const gc_conv_epilogue* ep, size_t room, ConvPlan& p) {
    const int qh = gc::ceil_div(d->out_h, 2), qw = gc::ceil_div(d->out_w, 2);
    // <= 32 output channels: the layer is bound by its stores, and 32-column q-tiles write 256-byte runs per row instead of 128-byte
    // ones (64 -> 32 @512^2: 254 -> 232 us) -- worth more than the 16 columns of lanes a 513-wide q-row wastes.
    // Otherwise: q-space is (H + 1) wide for a (2H + 1)-wide output, take the tile width that wastes fewer lanes
    if (d->out_ch <= 32) set_t<1, 4, 2, 32>(p, ConvPath::CT);
    else if (gc::ceil_div(qw, 16) * 16 < gc::ceil_div(qw, 32) * 32) set_t<2, 2, 2, 16>(p, ConvPath::CT);
    else set_t<2, 2, 2, 32>(p, ConvPath::CT);
    plan_tiles(p, qh, qw);
    // split over K (round 5: 512 -> 512 @8^2 / @16^2 were 64 / 160 workgroups walking all 32 chunks: 90 us each whatever the plane): dense rows only
    // (the finish pass writes dense rows), the 64-channel tiles only
    if (GC_CT_SPLITK && d->out_ch > 32 && dense_output(d)) plan_split(p, d, room);
    p.gx = (long long)p.tiles_x * p.tiles_y * d->batch;
    if (p.split) return;
#if GC_CTWS == 1
    if (plan_tws(d, ep, p)) return;
#endif
    if (ct_edge_eligible(d, p)) {
        // the fused kernel over the H x W main region, which its 4 x 32 q-tiles cover exactly
        set_t<2, 2, 2, 32>(p, ConvPath::CT_EDGE);
        plan_tiles(p, d->in_h, d->in_w);
        p.gx = (long long)p.tiles_x * p.tiles_y * d->batch;
#if GC_CTWS == 2
        // round 6 experiment: the main region on the wave-specialised kernel (its 8 x 32 q-tiles then cover the region exactly)
        if (d->in_h % 8 == 0 && !(ep && (ep->bias || ep->noise || ep->activate || ep->residual))) {
            set_tws<2, 32>(p, ConvPath::CTWS_EDGE);
            plan_tiles(p, d->in_h, d->in_w);
            plan_resident(p, d);
        }
#endif
    }
}

int launch_t(const ConvPlan& p, const Bf16Args& a, hipStream_t s) {
    int rc;
#if GC_CTWS
    if (p.path == ConvPath::CTWS || p.path == ConvPath::CTWS_EDGE) rc = launch_tws(p, a, s);
    else
#endif
    if (p.t[0] == 1) rc = launch_t_inst<1, 4, 2, 32>(p, a, s);
    else rc = p.t[3] == 32 ? launch_t_inst<2, 2, 2, 32>(p, a, s) : launch_t_inst<2, 2, 2, 16>(p, a, s);
    if (rc || !p.edge()) return rc;
    const dim3 grid((unsigned)(gc::ceil_div(a.c.in_w + 1, 32) + gc::ceil_div(a.c.in_h, 32)), (unsigned)(a.c.N / 64), (unsigned)a.c.B);
    hipLaunchKernelGGL(convt_edge_bf16x3_kernel, grid, dim3(256), 0, s, a);
    return gc::check_launch("gc_conv2d_bf16x3_f32(transposed, edge)");
}

}  // namespace GC_ARITH
}  // namespace gcconv
