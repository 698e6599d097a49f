/*
 * gancontrol_hip.h -- C ABI of the MI355X (gfx950) StyleGAN2 hot-path kernels for gan-control.
 *
 * This is the drop-in boundary.  Every entry point takes raw device pointers, explicit
 * extents and a HIP stream (as void*); the library never allocates or frees memory the
 * caller can see, keeps no mutable global state, launches asynchronously on the stream it is
 * given and never synchronises.  All tensors are contiguous NCHW float32 unless stated.
 *
 * Return value: 0 on success, negative on failure (GC_ERR_*).  gc_last_error() returns a
 * thread-local, human-readable description of the last failure on the calling thread.
 *
 * The reference (amazon-science/gan-control) ships no native code: its operator socket is the
 * module-level "if FUSED:" block of src/gan_control/models/gan_model.py:19-50, which binds the
 * names FusedLeakyReLU / fused_leaky_relu / upfirdn2d, and falls back to ATen calls
 * (F.conv2d, F.conv_transpose2d, F.pad, F.leaky_relu).  Each function below cites the reference
 * lines whose arithmetic it replaces.  INTEGRATION.md shows the binding a maintainer adds.
 */
#ifndef GANCONTROL_HIP_H
#define GANCONTROL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct below changes layout or an entry point changes its signature (2: gc_conv_desc.in_pitch / out_pitch and
 * gc_conv_epilogue.residual, added during ABI 1 without a bump, + gc_struct_sizes).  A binding must check BOTH gc_abi_version() and
 * gc_struct_sizes() against its own mirrors before the first call: a stale library otherwise mis-reads every descriptor. */
#define GC_ABI_VERSION 2

#define GC_OK 0
#define GC_ERR_BAD_ARG (-1)      /* null pointer, non-positive extent, inconsistent geometry */
#define GC_ERR_UNSUPPORTED (-2)  /* legal request outside what the kernels implement */
#define GC_ERR_HIP (-3)          /* the HIP runtime reported a launch error */
#define GC_ERR_WORKSPACE (-4)    /* workspace too small */

typedef void* gc_stream_t; /* hipStream_t */

int gc_abi_version(void);
const char* gc_last_error(void);
/* sizeof() of the library's own view of every struct of this header, in declaration order: gc_conv_desc, gc_conv_epilogue, gc_wlayout_group,
 * gc_wpack_group, gc_glin_group, gc_wsq_group.  Writes min(n, count) entries and returns count. */
#define GC_STRUCT_COUNT 6
int gc_struct_sizes(size_t* sizes, int n);
/* sha256 (first 16 hex digits) over the kernel sources and build flags this library was compiled from, stamped at build time (csrc/Makefile,
 * tools/build_alt.sh): measurements are tagged with it so that counters collected on one build are never quoted for another. */
const char* gc_source_hash(void);

/* ------------------------------------------------------------------------------------------
 * K1  upfirdn2d: zero-stuff by (up) -> pad / crop -> 2-D FIR -> decimate by (down).
 *
 * Replaces upfirdn2d() gan_model.py:45-50 -> upfirdn2d_native() pytorch_upfirdn2d.py:9-51
 * (callers: Blur gan_model.py:126-129, Upsample :86-89, Downsample :107-110,
 * non_leaking.py:338,359).
 *
 *   y[p,oy,ox] = sum_{a<kh, b<kw} T[a][b] * U[oy*down_y + a - pad_y0][ox*down_x + b - pad_x0]
 *   U[v][u]    = x[p][v/up_y][u/up_x] if up_y | v, up_x | u and the source is inside, else 0
 *   T[a][b]    = taps[kh-1-a][kw-1-b] if flip_taps (the forward op: a true convolution)
 *              = taps[a][b]           otherwise   (the adjoint uses the un-flipped kernel)
 *
 * planes = N*C.  taps is a DEVICE pointer to kh*kw floats (the module's `kernel` buffer).
 * out_h/out_w are the caller's: (in*up + pad0 + pad1 - k)/down + 1; negative pads crop.
 * The gradient w.r.t. x is the same call with up<->down, flip_taps toggled and
 * pad0' = k - 1 - pad0; the double-backward is the forward call again.
 */
int gc_upfirdn2d_f32(const float* x, const float* taps, float* y,
                     int planes, int in_h, int in_w, int out_h, int out_w,
                     int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                     int pad_x0, int pad_y0, int flip_taps, gc_stream_t stream);

/* The kernel gc_upfirdn2d_f32 runs for this shape (up_x = up_y = up, down_x = down_y = down), from the launcher's own plan; no launch, no
 * GPU needed.  name (>= 128 bytes) receives one of fir44_tile_kernel, fir44_small_kernel, fir44_down2_kernel, fir44_up2_kernel,
 * firK_tile_kernel<12>, upfirdn2d_generic_kernel.  The fused and pitched entries below take exactly the shapes named fir44_tile_kernel.
 * GC_ERR_UNSUPPORTED for a shape no kernel takes (more than 1024 taps), GC_ERR_BAD_ARG for a non-positive extent or factor. */
int gc_upfirdn2d_variant_name(int planes, int out_h, int out_w, int kh, int kw, int up, int down, char* name, int name_bytes);

/* K1 with the NoiseInjection + FusedLeakyReLU that follow the Blur of an up-sampling StyledConv
 * (gan_model.py:295-307 then :402-408) applied before the result is stored:
 *
 *   y[b,c,o] = gain * lrelu( FIR(x)[b,c,o] + noise_w[0] * noise[b,o] + bias[c], slope )
 *
 * in the arithmetic order of gc_bias_act_f32 (bit-identical to the two-pass result, one write + one read of the tensor
 * saved).  4x4 taps, up = down = 1, planes at least 64 x 16: GC_ERR_UNSUPPORTED otherwise (callers then run K1 + K2).
 * bias ([channels]) may be NULL; noise ([batch, out_h*out_w]) and noise_w go together. */
/* gc_upfirdn2d_f32 / gc_upfirdn2d_act_f32 over an input whose rows are in_pitch >= in_w floats apart (planes in_h * in_pitch apart): the
 * pitched output of a transposed convolution (gc_conv_desc.out_pitch) read by the Blur that follows it (gan_model.py:304-307) -- and / or
 * writing rows out_pitch >= out_w floats apart (0 = dense): the (H + 1)-wide output of the Blur in front of a stride-2 convolution
 * (ConvLayer gan_model.py:866-872), whose 16-byte stores otherwise straddle cache lines (4.4 vs 5.6 TB/s).
 * up = down = 1 with 4 x 4 taps on planes the tile kernel takes (out_w >= 64, out_h >= 16); bias / noise / noise_w NULL and
 * slope = gain = 1, activate = 0 give the plain FIR. */
int gc_upfirdn2d_pitched_f32(const float* x, const float* taps, float* y, int batch, int channels, int in_h, int in_w, int in_pitch,
                             int out_h, int out_w, int out_pitch, int kh, int kw, int pad_x0, int pad_y0, int flip_taps, int activate,
                             const float* bias, const float* noise, const float* noise_w, float slope, float gain, gc_stream_t stream);

int gc_upfirdn2d_act_f32(const float* x, const float* taps, float* y,
                         int batch, int channels, int in_h, int in_w, int out_h, int out_w,
                         int kh, int kw, int pad_x0, int pad_y0, int flip_taps,
                         const float* bias, const float* noise, const float* noise_w, float slope, float gain,
                         gc_stream_t stream);

/* y = FIR(x) * (mask_ref > 0 ? gain : gain * slope): the Blur ADJOINT followed by the backward of the bias + leaky-ReLU whose output the
 * Blur read (ResBlock: conv1 -> FusedLeakyReLU -> Blur -> stride-2 conv2, gan_model.py:893-922, 844-890) in one pass -- the product is
 * applied to the fp32 FIR result, so the values equal gc_upfirdn2d_f32 followed by gc_bias_act_bwd_f32 bit for bit, while the
 * gradient makes one round trip to HBM less.  mask_ref: [batch, channels, out_h, out_w] dense (the activation output); x rows in_pitch
 * floats apart (0 = dense); 4 x 4 taps, up = down = 1, planes the tile kernel takes (out_w >= 64, out_h >= 16). */
int gc_upfirdn2d_mask_f32(const float* x, const float* taps, float* y, int batch, int channels, int in_h, int in_w, int in_pitch,
                          int out_h, int out_w, int kh, int kw, int pad_x0, int pad_y0, int flip_taps,
                          const float* mask_ref, float slope, float gain, gc_stream_t stream);

/* The backward of StyledConv's up-sampling tail (Blur -> NoiseInjection -> FusedLeakyReLU, gan_model.py:402-408 after :304-307) in one pass
 * over the gradient:  g_pre = gy * (y_ref > 0 ? gain : gain * slope) is formed while gy is staged, gx = FIR(g_pre) (the Blur adjoint) is
 * stored, and per (plane, tile)  psum = sum g_pre,  pdot = sum g_pre * noise[b]  over the input elements the tile owns (every element once):
 * the bias gradient is the sum of psum over batch and tiles, the noise-strength gradient the sum of all pdot.  g_pre never travels to HBM
 * (gc_bias_act_bwd_reduce_f32 + gc_upfirdn2d_f32 write and re-read it).  gy, y_ref: [batch, channels, in_h, in_w] dense; noise
 * [batch, in_h * in_w] with pdot, or both NULL; gx rows out_pitch floats apart (0 = dense); psum / pdot: [batch * channels,
 * gc_upfirdn2d_actbwd_tiles(out_h, out_w)].  4 x 4 taps on planes the tile kernel takes. */
int gc_upfirdn2d_actbwd_tiles(int out_h, int out_w);
int gc_upfirdn2d_actbwd_f32(const float* gy, const float* y_ref, const float* noise, const float* taps, float* gx, float* psum, float* pdot,
                            int batch, int channels, int in_h, int in_w, int out_h, int out_w, int out_pitch, int kh, int kw,
                            int pad_x0, int pad_y0, int flip_taps, float slope, float gain, gc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K2  fused (noise +) bias + leaky-ReLU * gain.
 *
 * Replaces FusedLeakyReLU.forward gan_model.py:32-35, fused_leaky_relu gan_model.py:39-41 and,
 * when `noise` is given, the NoiseInjection add that always precedes it
 * (gan_model.py:340-345, 402-408).
 *
 *   y[b,c,i] = gain * lrelu(x[b,c,i] + bias[c] + noise_w[0] * noise[b,i], slope)
 *
 * inner = product of the dims after the channel dim (1 for [B,F] inputs).  bias may be null;
 * noise ([batch, inner]) and noise_w (DEVICE scalar) are both null or both set.
 */
int gc_bias_act_f32(const float* x, const float* bias, const float* noise, const float* noise_w,
                    float* y, int batch, int channels, int64_t inner,
                    float slope, float gain, gc_stream_t stream);

/* Gradient (and, being linear in dy, also the double-backward) of K2 through the activation,
 * masked by the sign of the forward OUTPUT:
 *   dx[i] = dy[i] * (y_ref[i] > 0 ? gain : gain * slope)
 */
int gc_bias_act_bwd_f32(const float* dy, const float* y_ref, float* dx, int64_t count,
                        float slope, float gain, gc_stream_t stream);

/* The same gradient with the NOISE-MAP gradient taken in the same pass: what image projection needs, where the per-layer noise maps are
 * optimised (reference: projection/projection.py; the injection itself is NoiseInjection, gan_model.py:334-345):
 *   g_pre[b,c,i] = dy[b,c,i] * (y_ref[b,c,i] > 0 ? gain : gain * slope);   dx = g_pre  (the bits of gc_bias_act_bwd_f32)
 *   dnoise[b,i]  = noise_w[0] * sum_c g_pre[b,c,i]
 * dy and y_ref are read once.  With y_ref == NULL, dy is taken as an already computed g_pre: nothing is stored to dx (it may be NULL) and only
 * the pixel sums are made -- for callers whose reduce pass (gc_bias_act_bwd_reduce_self_f32) has produced g_pre already.  The channels are
 * added in an order fixed by the shape (ascending; where a plane has few pixels, four interleaved channel slices added as (s0 + s1) +
 * (s2 + s3)): no atomics, the same bits for the same inputs.  noise_w is a DEVICE scalar.  16-byte accesses wherever four pixels of a plane
 * remain, the ragged tail per element; every base need only be 4-byte aligned.  Null dy / noise_w / dnoise, y_ref without dx and
 * non-positive extents return GC_ERR_BAD_ARG, batch > 65535 GC_ERR_UNSUPPORTED; neither launches anything. */
int gc_bias_act_bwd_noise_f32(const float* dy, const float* y_ref, const float* noise_w, float* dx, float* dnoise,
                              int batch, int channels, int64_t inner, float slope, float gain, gc_stream_t stream);

/* The same gradient fused with the reductions its caller needs (one pass instead of three):
 *   dx = dy * mask(y_ref);   psum[(b*C + c)*chunks + j] = sum over chunk j of dx[b,c,:]
 *   pdot[(b*C + c)*chunks + j] = sum over chunk j of dx[b,c,:] * noise[b,:]      (only when noise != null)
 * with chunks = gc_bias_act_bwd_chunks(inner).  Bias gradient = psum summed over b and j; noise-strength
 * gradient = pdot summed over everything.  Deterministic (fixed-order block reductions, no atomics). */
int gc_bias_act_bwd_chunks(int64_t inner);
int gc_bias_act_bwd_reduce_f32(const float* dy, const float* y_ref, const float* noise, float* dx,
                               float* psum, float* pdot, int batch, int channels, int64_t inner,
                               float slope, float gain, gc_stream_t stream);

/* The same pass with one more reduction, for a convolution whose activation ran in its epilogue (gc_conv_epilogue) so
 * that the pre-activation tensor was never written:
 *   pself[(b*C + c)*chunks + j] = sum over chunk j of dx[b,c,:] * x_pre[b,c,:],
 *   x_pre = lrelu^-1(y_ref / gain) - bias[c] - noise_w[0] * noise[b,:]      (the activation's input, rebuilt from its output)
 * Summed over the chunks and divided by out_scale[b,c] this is the out_scale (demodulation) gradient of K3, which would
 * otherwise need gc_plane_dot_f32 over (dx, pre-activation).  bias / noise / noise_w / pdot / pself may be NULL
 * (noise_w is required with noise when pself is requested); slope and gain must be non-zero for pself. */
int gc_bias_act_bwd_reduce_self_f32(const float* dy, const float* y_ref, const float* noise, const float* bias, const float* noise_w,
                                    float* dx, float* psum, float* pdot, float* pself, int batch, int channels, int64_t inner,
                                    float slope, float gain, gc_stream_t stream);

/* ADJOINT of gc_bias_act_bwd_reduce_self_f32 with respect to dy (and to y_ref through pself): the second-order pass of the R1 and
 * path-length regularisers (d_r1_loss / g_path_regularize, generator_trainer.py / gan_model.py) through an activation backward.
 * Cotangents: ggx [B,C,inner] of dx (may be NULL), cs / cd / cw [B,C,chunks] of psum / pdot / pself (each may be NULL).  With
 *   total = ggx + cs + cd * noise + cw * x_pre      (x_pre as above)
 *   g_dy   = total * (y_ref > 0 ? gain : gain * slope)
 *   g_yref = cw * dx * (y_ref > 0 ? 1 / gain : 1 / (gain * slope))            (only with cw; dx = the first pass's output)
 *   pgb[(b*C + c)*chunks + j] = sum over chunk j of cw * dx          (bias gradient   = -sum over b, j)
 *   pgn[(b*C + c)*chunks + j] = sum over chunk j of cw * dx * noise  (noise_w gradient = -sum over everything)
 * one read of each input and one write of each output instead of ~14 elementwise passes.  g_yref / pgb / pgn may be NULL;
 * dx is required when cw is given. */
int gc_bias_act_bwd_reduce_adjoint_f32(const float* ggx, const float* cs, const float* cd, const float* cw, const float* y_ref, const float* dx,
                                       const float* noise, const float* bias, const float* noise_w, float* g_dy, float* g_yref, float* pgb, float* pgn,
                                       int batch, int channels, int64_t inner, float slope, float gain, gc_stream_t stream);

/* partial[p*chunks + j] = sum over chunk j of a[p,:] * b[p,:], chunks = gc_bias_act_bwd_chunks(inner); planes = B*C.
 * Gradients of the per-sample modulation / demodulation factors of K3 (sum_hw x * dx and sum_hw dy * y). */
int gc_plane_dot_f32(const float* a, const float* b, float* partial, int planes, int64_t inner, gc_stream_t stream);

/* The same reduction over planes of `rows` x `width` elements whose rows are a_pitch / b_pitch floats apart (planes rows * pitch apart):
 * partial[p * chunks + j] with chunks = gc_plane_dot_pitched_chunks(rows). */
int gc_plane_dot_pitched_chunks(int rows);
int gc_plane_dot_pitched_f32(const float* a, const float* b, float* partial, int planes, int rows, int width, int a_pitch, int b_pitch, gc_stream_t stream);

/* out[r] = (sum_j partial[r*chunks + j]) / den[r]; den may be NULL (plain sum), a zero denominator counts as one.
 * The second stage of gc_plane_dot_f32 / the pself sums of gc_bias_act_bwd_reduce_self_f32 fused with the division by the modulation
 * (in_scale) / demodulation (out_scale) factor: `sum_hw x * dx / s` of ModulatedConv2d's weight algebra (gan_model.py:284-293) in one
 * launch.  chunks = 1 is an element-wise safe division of two [rows] vectors. */
int gc_rows_sum_div_f32(const float* partial, const float* den, float* out, int rows, int chunks, gc_stream_t stream);

/* Per-channel sum over batch and inner dims: out[c] = sum_{b,i} x[b,c,i]  (bias gradient).
 * Deterministic two-stage reduction; workspace must hold gc_channel_sum_workspace() bytes. */
size_t gc_channel_sum_workspace(int batch, int channels, int64_t inner);
int gc_channel_sum_f32(const float* x, float* out, int batch, int channels, int64_t inner,
                       void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K3/K4  generalised 2-D convolution on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32).
 *
 * One contraction covers F.conv2d (EqualConv2d.forward gan_model.py:154-160 and the plain
 * ModulatedConv2d branch gan_model.py:325-329: up = 1, down = stride), F.conv_transpose2d
 * (ModulatedConv2d up-sampling branch gan_model.py:295-306 and every input-gradient:
 * up = stride, down = 1) and, through in_scale / out_scale, StyleGAN2 weight (de)modulation
 * WITHOUT materialising per-sample weights (gan_model.py:284-293):
 *
 *   y[b,n,oy,ox] = out_scale[b,n] * sum_{ty,tx,k} w[ty,tx,k,n] * in_scale[b,k]
 *                                   * U(x)[b,k, oy*down + ty - pad_y, ox*down + tx - pad_x]
 *
 * U zero-stuffs x by `up` as in K1.  w is [kh, kw, in_ch, out_ch] (out_ch contiguous) in
 * CORRELATION order; in_scale [batch, in_ch] and out_scale [batch, out_ch] may be null (= 1).
 * Supported: kh = kw in {1, 3}; (up, down) in {(1,1), (1,2), (2,1)}.
 */
typedef struct gc_conv_desc {
    int32_t batch;
    int32_t in_ch, out_ch;
    int32_t in_h, in_w;
    int32_t out_h, out_w;
    int32_t kh, kw;
    int32_t up, down;
    int32_t pad_y, pad_x;
    int32_t in_pitch;    /* floats between the starts of two INPUT rows (planes in_h * in_pitch apart); 0 (or in_w) = dense.  Honoured by the
                          * stride-2 launches gc_conv2d_in_pitch_ok() names (forward and weight gradient), whose input is the (H + 1)-wide
                          * output of a Blur written with aligned rows (gc_upfirdn2d_pitched_f32, out_pitch). */
    int32_t out_pitch;   /* floats between the starts of two output rows; 0 (or out_w) = dense.  Only the launches gc_conv2d_out_pitch()
                          * names honour another value (a plane is then out_h * out_pitch floats): rows of a (2H + 1)-wide transposed-
                          * convolution output are never 16-byte aligned, and their partial-line stores bound that kernel. */
} gc_conv_desc;

/* Products with a tiny INNER extent (the weight gradients of the style path: EqualLinear gan_model.py:171-202 on [B, 512] latents, the
 * modulation / demodulation algebra of ModulatedConv2d gan_model.py:284-293 -- g[B, C]^T @ x[B, 512], a rank-B update):
 *
 *   out[M, N] (dense, row-major) = alpha * (a[M, K] @ b[K, N]) + beta * bias[N]        K <= 8
 *
 * a and b are addressed through element strides (transposed views need no copy); bias may be NULL.
 * torch.addmm(bias, a, b, beta=beta, alpha=alpha) for the shape where a library GEMM is all latency.
 * gc_small_gemm_ok() says whether a shape is taken (1: K <= 8 and M * N <= 2^19) or should go to a GEMM library (0). */
int gc_small_gemm_ok(int M, int K, int N, int64_t sb0, int64_t sb1);
int gc_small_gemm_f32(const float* a, int64_t sa0, int64_t sa1, const float* b, int64_t sb0, int64_t sb1,
                      const float* bias, float beta, float alpha, float* out, int M, int K, int N, gc_stream_t stream);

/* The row pitch (floats, a multiple of 32) the convolution of `d` in arithmetic `mode` (0 f32, 1 bf16x3, 2 bf16) can write its output with
 * when that pays -- the fused transposed 3x3 convolution with an odd output width -- or 0: write dense rows. */
int gc_conv2d_out_pitch(const gc_conv_desc* d, int mode);

/* 1 when the forward convolution (wgrad = 0) / weight gradient (wgrad = 1) of `d` in arithmetic `mode` reads a row-pitched input
 * (gc_conv_desc.in_pitch) in place: the split-bf16 stride-2 kernels. */
int gc_conv2d_in_pitch_ok(const gc_conv_desc* d, int mode, int wgrad);

int gc_conv2d_f32(const gc_conv_desc* d, const float* x, const float* w,
                  const float* in_scale, const float* out_scale, float* y, gc_stream_t stream);

/* Fused epilogue: the (noise +) bias + leaky-ReLU pass K2 that follows every convolution of the path (EqualConv2d ->
 * FusedLeakyReLU in ConvLayer gan_model.py:844-890; ModulatedConv2d -> NoiseInjection -> FusedLeakyReLU in StyledConv
 * gan_model.py:402-408; `+ self.bias` in ToRGB gan_model.py:430) applied to the accumulators before they are stored:
 *
 *   y[b,n,o] = A( out_scale[b,n] * sum(...) + noise_w[0] * noise[b,o] + bias[n] ) + residual[b,n,o],
 *   A(v) = activate ? gain * lrelu(v, slope) : v
 *
 * `residual` (same shape as y, may be NULL) is the second operand of an add that follows the convolution: the
 * `out + skip` of ResBlock.forward (gan_model.py:919-921) and -- on the backward side -- the gradient arriving from the
 * other consumer of a tensor that feeds two layers (what autograd would sum with a separate elementwise pass).
 *
 * with the arithmetic of gc_bias_act_f32 in the same order, so conv + epilogue equals gc_conv2d_f32 followed by
 * gc_bias_act_f32 bit for bit while saving one write and one read of the activation tensor.  ep == NULL: plain convolution.
 */
typedef struct gc_conv_epilogue {
    const float* bias;     /* [out_ch] or NULL */
    const float* noise;    /* [batch, out_h * out_w] or NULL */
    const float* noise_w;  /* DEVICE scalar; set exactly when noise is */
    float slope, gain;     /* used when activate != 0 */
    int32_t activate;
    const float* residual; /* [batch, out_ch, out_h, out_w] or NULL; must not alias y */
} gc_conv_epilogue;

int gc_conv2d_fused_f32(const gc_conv_desc* d, const float* x, const float* w,
                        const float* in_scale, const float* out_scale, const gc_conv_epilogue* ep,
                        float* y, gc_stream_t stream);

/* gc_conv2d_fused_f32 with scratch memory: with gc_conv2d_f32_workspace(d) bytes (0 for most shapes) the layers whose output planes are
 * <= 16 pixels wide are split over the input channels -- one 16 / 32-channel weight slab per workgroup over every sample (in groups of
 * samples when their planes exceed the LDS) for planes <= 8 x 8 and for transposed 3x3 onto planes <= 10 x 10 (conv_f32_small_kernel),
 * K slices of conv_mfma_kernel otherwise -- and a fixed-order pass adds the slices and applies
 * out_scale and the epilogue: same arithmetic (exact fp32), 256 workgroups instead of 8..64.  Without workspace (or with too little) it
 * is gc_conv2d_fused_f32. */
size_t gc_conv2d_f32_workspace(const gc_conv_desc* d);
int gc_conv2d_fused_f32_ws(const gc_conv_desc* d, const float* x, const float* w,
                           const float* in_scale, const float* out_scale, const gc_conv_epilogue* ep,
                           float* y, void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* The same contraction on the bf16 matrix cores with split-bf16 ("bf16x3") arithmetic: every fp32
 * operand is split into bf16 hi + lo parts and a*b is formed as hi*hi + hi*lo + lo*hi with fp32
 * accumulation (~5e-6 relative error per layer, 5.3x the fp32 MFMA rate).  Inputs and outputs stay
 * fp32; `workspace` (gc_conv2d_bf16x3_workspace() bytes, 16-byte aligned) receives the split weights.
 * Shapes the fast kernel does not cover (in_ch < 16, planes <= 8 px wide) run on gc_conv2d_f32.  Transposed 3x3 launches of the
 * (2H + 1) x (2W + 1) geometry with >= 256 input channels run as an H x W main region plus an edge launch (last row and column).
 */
size_t gc_conv2d_bf16x3_workspace(const gc_conv_desc* d);
int gc_conv2d_bf16x3_f32(const gc_conv_desc* d, const float* x, const float* w,
                         const float* in_scale, const float* out_scale, float* y,
                         void* workspace, size_t workspace_bytes, gc_stream_t stream);

int gc_conv2d_fused_bf16x3_f32(const gc_conv_desc* d, const float* x, const float* w,
                               const float* in_scale, const float* out_scale, const gc_conv_epilogue* ep, float* y,
                               void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* The split weights as a separate, reusable object.  A parameter changes once per optimiser step but is used by several
 * launches in between (forward and input gradient of D over the fake and real batches, R1, the generator passes of the D and G
 * steps), so the caller may split a weight tensor ONCE -- gc_conv2d_pack_weights_bf16x3 into a buffer of
 * gc_conv2d_bf16x3_packed_bytes(d) bytes, 16-byte aligned; the buffer depends on (kh, kw, in_ch, out_ch) and w only -- and hand
 * it to every launch that uses the same w (the reference recomputes `weight * scale` per call, gan_model.py:154, 284).
 * gc_conv2d_bf16x3_packed_bytes returns 0 for shapes that run on the fp32 kernel: pass packed = NULL and a workspace of
 * gc_conv2d_bf16x3_workspace(d) bytes then.  Same results as gc_conv2d_fused_bf16x3_f32, bit for bit.
 */
size_t gc_conv2d_bf16x3_packed_bytes(const gc_conv_desc* d);
/* Small planes (9 .. 32 pixels wide, >= 128 input channels) are split over the input channels to fill the chip; the slices are summed in
 * a fixed order by a finish pass that applies out_scale and the epilogue.  gc_conv2d_bf16x3_splitk_bytes(d) is the workspace that takes
 * (0 when the shape is not split); without it the launch runs unsplit -- same result up to fp32 summation order. */
size_t gc_conv2d_bf16x3_splitk_bytes(const gc_conv_desc* d);
int gc_conv2d_pack_weights_bf16x3(const gc_conv_desc* d, const float* w, void* packed, size_t packed_bytes, gc_stream_t stream);
int gc_conv2d_fused_bf16x3_packed_f32(const gc_conv_desc* d, const float* x, const float* w, const void* packed, size_t packed_bytes,
                                      const float* in_scale, const float* out_scale, const gc_conv_epilogue* ep, float* y,
                                      void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* Plain bf16 arithmetic: the kernels of the split-bf16 path with ONE MFMA per product on the bf16-rounded operands (fp32 accumulate,
 * fp32 in HBM on both sides; ~3e-3 relative error per layer) -- the precision BASELINE.json's config[1] names.  Same arguments,
 * packed weights (gc_conv2d_pack_weights_bf16x3; the lo half is not read) and workspaces as the split-bf16 entry points. */
int gc_conv2d_fused_bf16_packed_f32(const gc_conv_desc* d, const float* x, const float* w, const void* packed, size_t packed_bytes,
                                    const float* in_scale, const float* out_scale, const gc_conv_epilogue* ep, float* y,
                                    void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* Name of the kernel variant the dispatcher picks for a shape ("conv_bf16x3_kernel<1,4,2,2>|up1,down1,k3", ...), written by the
 * dispatch code itself (the launchers run in a no-launch probe mode): what a host-side profiler keys its per-kernel statistics on.
 * mode: 0 = exact fp32, 1 = split-bf16, 2 = plain bf16.  name must hold >= 128 bytes. */
int gc_conv2d_variant_name(const gc_conv_desc* d, int mode, char* name, int name_bytes);

/* Weight gradient of the same contraction (up must be 1):
 *
 *   dw[ty,tx,k,n] = sum_{b,oy,ox} in_scale[b,k] * x[b,k, oy*down + ty - pad_y, ox*down + tx - pad_x]
 *                                 * out_scale[b,n] * dy[b,n,oy,ox]
 *
 * Replaces the weight half of aten::convolution_backward reached from gan_model.py:154,304,327.
 * Deterministic: partial sums go to `workspace` (gc_conv2d_wgrad_workspace() bytes) and are
 * reduced in a fixed order.
 */
size_t gc_conv2d_wgrad_workspace(const gc_conv_desc* d);
int gc_conv2d_wgrad_f32(const gc_conv_desc* d, const float* x, const float* dy,
                        const float* in_scale, const float* out_scale, float* dw,
                        void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* Split-bf16 variant of the weight gradient (same contract; shapes it does not cover -- fewer than 32 channels, planes < 4 px
 * wide, and 3x3 gradients onto planes <= 8 x 8, which one exact-fp32 launch computes without a workspace -- run on
 * gc_conv2d_wgrad_f32, so size the workspace with this function). */
size_t gc_conv2d_wgrad_bf16x3_workspace(const gc_conv_desc* d);
int gc_conv2d_wgrad_bf16x3_f32(const gc_conv_desc* d, const float* x, const float* dy,
                               const float* in_scale, const float* out_scale, float* dw,
                               void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* Plain-bf16 variant (see gc_conv2d_fused_bf16_packed_f32); workspace as for the split-bf16 weight gradient. */
int gc_conv2d_wgrad_bf16_f32(const gc_conv_desc* d, const float* x, const float* dy,
                             const float* in_scale, const float* out_scale, float* dw,
                             void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* Name of the kernel variant the WEIGHT-GRADIENT dispatchers pick for a shape, written by the dispatch code itself as
 * gc_conv2d_variant_name does for the forward direction (no launch, no GPU needed):
 *
 *   "<kernel<template arguments>>|down<d>,k<taps>[|samples]|plan:<how the pixels are split>"
 *
 * e.g. "wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|plan:splits=64,tiles_per_split=33".  The part in front of "|plan:" names the code
 * that runs; the plan holds the split count, the tiles (wgrad_bf16x3_ws2_kernel: 16-row strips) per split, that kernel's row bands
 * ("bands=") and ",direct" when the kernel writes dw itself instead of partial sums for a reduce pass.
 * mode: 0 = exact fp32, 1 = split-bf16, 2 = plain bf16.  samples != 0: the gc_conv2d_wgrad_samples_* entry point of that mode
 * (GC_ERR_UNSUPPORTED where the shape has no per-sample form).  name must hold >= 128 bytes. */
int gc_conv2d_wgrad_variant_name(const gc_conv_desc* d, int mode, int samples, char* name, int name_bytes);

/* Weight gradient together with each sample's share of it:
 *
 *   dw_samples[b,ty,tx,k,n] = in_scale[b,k] * out_scale[b,n] * sum_{oy,ox} x[b,k, oy*down + ty - pad_y, ...] * dy[b,n,oy,ox]
 *   dw = sum_b dw_samples[b]                                       (both reduced in a fixed order)
 *
 * What the shares are for: ModulatedConv2d (gan_model.py:281-331) multiplies its weight by the per-sample style,
 * `weight = self.scale * self.weight * style` (and by the demodulation factor), so the gradients of those factors are contractions of
 * the SAME per-sample products with the weight (gc_wgrad_samples_contract_f32 below) -- autograd's route through
 * aten::convolution_backward of the grouped convolution materialises them per sample as well.  Taking them from here replaces two
 * full-plane products per layer, sum_p x * dx and sum_p dy * y (gc_plane_dot_f32), by reads of [B, taps, K, N].
 * The pixel splits of the plain weight gradient are regrouped so that every split stays inside one sample; same kernels, same
 * arithmetic.  gc_conv2d_wgrad_samples_workspace(): bytes of scratch for `mode` (0 = fp32, 1 = split-bf16, 2 = plain bf16), 0 when
 * the shape has no per-sample form: fp32 has one for the thin 1x1 shapes only (<= 4 channels on one side: ToRGB), the bf16 modes
 * additionally for everything their own weight-gradient kernels take (>= 32 channels on both sides, planes >= 4 px wide). */
size_t gc_conv2d_wgrad_samples_workspace(const gc_conv_desc* d, int mode);
int gc_conv2d_wgrad_samples_f32(const gc_conv_desc* d, const float* x, const float* dy, const float* in_scale, const float* out_scale,
                                float* dw, float* dw_samples, void* workspace, size_t workspace_bytes, gc_stream_t stream);
int gc_conv2d_wgrad_samples_bf16x3_f32(const gc_conv_desc* d, const float* x, const float* dy, const float* in_scale, const float* out_scale,
                                       float* dw, float* dw_samples, void* workspace, size_t workspace_bytes, gc_stream_t stream);
int gc_conv2d_wgrad_samples_bf16_f32(const gc_conv_desc* d, const float* x, const float* dy, const float* in_scale, const float* out_scale,
                                     float* dw, float* dw_samples, void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* The scale gradients from the per-sample shares (w and dw_samples[b] are [taps, a, c], the kernel layout [kh*kw, K, N]):
 *
 *   g_a[b,a] = sum_{t,c} w[t,a,c] * dw_samples[b,t,a,c] / scale_a[b,a]          (d loss / d in_scale:  the modulation, gan_model.py:283-284)
 *   g_c[b,c] = sum_{t,a} w[t,a,c] * dw_samples[b,t,a,c] / scale_c[b,c]          (d loss / d out_scale: the demodulation, gan_model.py:286-288)
 *
 * (dw_samples carries both scales as factors; dividing one out leaves the derivative with respect to it.  A scale of exactly 0 divides
 * by 1, as gc_rows_sum_div_f32 does.)  g_a or g_c may be null, a null scale divides by 1.  Fixed summation order.
 * workspace: gc_wgrad_samples_contract_workspace(batch, a, c) bytes, needed for g_c only. */
size_t gc_wgrad_samples_contract_workspace(int batch, int a, int c);
int gc_wgrad_samples_contract_f32(const float* dw_samples, const float* w, const float* scale_a, const float* scale_c, float* g_a, float* g_c,
                                  int batch, int taps, int a, int c, void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Weight re-layout: scale + permute + optional tap mirror in one pass.
 *
 *   dst[t' * dst_stride[0] + k * dst_stride[1] + n * dst_stride[2]]
 *       = scale * src[t * src_stride[0] + k * src_stride[1] + n * src_stride[2]],   t' = flip_taps ? taps - 1 - t : t
 *
 * for t < taps (= kh*kw), k < in_ch, n < out_ch; strides in ELEMENTS, non-negative.  Replaces the ATen passes the
 * reference spends per call on `self.weight * self.scale` (gan_model.py:154, 284), the transpose / view of the
 * up-sampling branch (gan_model.py:295-303) and the permutes inside aten::convolution_backward:
 *   parameter [N,K,taps] -> kernel layout [taps,K,N]      src_stride = {1, taps, K*taps}, dst_stride = {K*N, N, 1}
 *   kernel layout -> input-gradient weights [taps',N,K]   src_stride = {K*N, N, 1},       dst_stride = {N*K, 1, K}, flip
 *   weight gradient [taps,K,N] -> parameter layout        src_stride = {K*N, N, 1},       dst_stride = {1, taps, K*taps}
 * src and dst must not overlap.
 */
int gc_weight_layout_f32(const float* src, float* dst, int taps, int k, int n,
                         const int64_t src_stride[3], const int64_t dst_stride[3],
                         int flip_taps, float scale, gc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Image-space pieces of the ADA augmentation (random_apply_affine, non_leaking.py:316-371) besides its two FIR passes.
 *
 * gc_affine_warp_bilinear_f32: bilinear resampling of x [batch, channels, in_h, in_w] into y [batch, channels, out_h, out_w]
 * under a per-sample affine map mat [batch, 6]: output pixel (ox, oy) reads the input at
 *     sx = m0*ox + m1*oy + m2,  sy = m3*ox + m4*oy + m5        (input PIXEL coordinates, pixel centres at integers)
 * with zeros outside -- what F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False) computes for the grid the
 * reference builds with make_grid / affine_grid (non_leaking.py:244-263, 338-357: an affine function of the output pixel index,
 * which the host folds into mat).  adjoint != 0: the transposed map -- x is then the gradient of the OUTPUT
 * [batch, channels, out_h, out_w] and y receives the gradient of the input [batch, channels, in_h, in_w] (scatter-add).
 *
 * gc_reflect_pad_f32: y = F.pad(x, (left, right, top, bottom), mode='reflect') on `planes` planes of in_h x in_w
 * (non_leaking.py:288-313); adjoint != 0: x is the gradient of the padded tensor, y receives the folded-back gradient.
 */
int gc_affine_warp_bilinear_f32(const float* x, const float* mat, float* y, int batch, int channels,
                                int in_h, int in_w, int out_h, int out_w, int adjoint, gc_stream_t stream);
int gc_reflect_pad_f32(const float* x, float* y, int planes, int in_h, int in_w, int left, int right, int top, int bottom,
                       int adjoint, gc_stream_t stream);

/* The derived weight forms of a whole network in a few launches.  After an optimiser step every convolution weight of a network is needed
 * again as kernel layout, as input-gradient layout and (split-bf16 mode) as hi / lo packs of both: ~4 launches of 4 - 6 us per layer and
 * weight version when done one tensor at a time (gc_weight_layout_f32, gc_conv2d_pack_weights_bf16x3).  The grouped entry points take a
 * table of the same arguments and produce bit-identical results (the per-element arithmetic is shared). */
typedef struct gc_wlayout_group {
    const float* src;
    float* dst;
    int32_t taps, k, n, flip_taps;
    int64_t src_stride[3], dst_stride[3];
    float scale;
} gc_wlayout_group;
int gc_weight_layout_grouped_f32(const gc_wlayout_group* groups, int n_groups, gc_stream_t stream);

typedef struct gc_wpack_group {
    gc_conv_desc desc;        /* as for gc_conv2d_pack_weights_bf16x3 */
    const float* w;           /* [kh, kw, in_ch, out_ch] */
    void* packed;             /* gc_conv2d_bf16x3_packed_bytes(&desc) bytes, 16-byte aligned */
    size_t packed_bytes;
} gc_wpack_group;
int gc_conv2d_pack_weights_bf16x3_grouped(const gc_wpack_group* groups, int n_groups, gc_stream_t stream);

/* One pass per parameter for everything between an optimiser step and the next forward pass: the EMA copy and every derived form of a
 * convolution weight, each parameter read once.  Two kinds of item share the table:
 *   weight item (taps = 1 or 9)   src: the parameter [n, k, taps], taps fastest.  Every output is optional (NULL = not wanted):
 *     ema       [n, k, taps]   ema = decay * ema + alpha * src in place: the bits of torch._foreach_mul_(ema, decay) followed by
 *                              torch._foreach_add_(ema, src, alpha=alpha), both scalars rounded to float once
 *     w_t       [taps, k, n]   scale * src, taps mirrored if flip_taps                        (gc_weight_layout_f32, parameter -> kernel layout)
 *     adj       [taps, n, k]   adj[taps - 1 - t][n][k] = w_t[t][k][n]                         (gc_weight_layout_f32, the adjoint layout)
 *     adj2      [taps, k, n]   adj(adj): the values of w_t in a tensor of its own (the weights of a double-backward convolution)
 *     pack_w    hi / lo packs of w_t, the format and size of gc_conv2d_pack_weights_bf16x3 for in_ch = k, out_ch = n: 2 * taps *
 *               ceil(k / 8) * n units of 16 bytes, 16-byte aligned
 *     pack_adj  the same of adj (in_ch = n, out_ch = k)
 *     wsq       [n, k]         sum over the taps of src^2                                     (gc_weight_sq_grouped_f32)
 *   flat item (taps = 0)          src, ema: count floats; the EMA only.  n, k and the form pointers are unused (NULL).
 * Every value is bit-identical to the entry named next to it.  src is only read.  Outputs must not overlap src or each other.
 * Any other tap count returns GC_ERR_UNSUPPORTED, null or non-positive operands GC_ERR_BAD_ARG; everything is checked before the first
 * launch.  The table is cut into as many launches as its items need (16 weight items and 76 flat items each).
 * gc_weight_refresh_launches: kernel launches the entry has issued in this process so far (tests count the launches of a refresh with it).
 * gc_weight_refresh_item_bytes: sizeof(gc_wrefresh_item) of the built library (the binding compares it with its mirror). */
typedef struct gc_wrefresh_item {
    const float* src;
    float* ema;
    float* w_t;
    float* adj;
    float* adj2;
    void* pack_w;
    void* pack_adj;
    float* wsq;
    int64_t count;
    int32_t n, k, taps, flip_taps;
    float scale, decay, alpha;
} gc_wrefresh_item;
int gc_weight_refresh_grouped_f32(const gc_wrefresh_item* items, int n_items, gc_stream_t stream);
int64_t gc_weight_refresh_launches(void);
size_t gc_weight_refresh_item_bytes(void);

/* The backward of a fused (k <= 3 -> n) 1x1 convolution + bias + leaky-ReLU -- the discriminator's FromRGB ConvLayer (gan_model.py:955,
 * 844-890), whose output [B, 32, 1024, 1024] is the largest activation of D -- without a separate activation-backward pass: the gradient dy
 * that arrives at the activation output is multiplied by the mask (y_ref > 0 ? gain : gain * slope) while it is loaded.
 *   gc_pw_act_wgrad_f32  dw_db[j, :] = sum_{b,p} x[b, j, p] * dy_masked[b, :, p]  for j < k, and dw_db[k, :] = sum_{b,p} dy_masked[b, :, p]
 *                        (the weight gradient in [k, n] order followed by the bias gradient; fixed summation order)
 *   gc_pw_act_dgrad_f32  gx[b, j, p] = sum_i w[i, j] * dy_masked[b, i, p]          w: [n, k] (the input-gradient weights), k <= 4
 * x: [batch, k, plane], dy / y_ref: [batch, n, plane], gx: [batch, k, plane]; planes dense. */
size_t gc_pw_act_wgrad_workspace(int batch, int k, int n, int64_t plane);
int gc_pw_act_wgrad_f32(const float* x, const float* dy, const float* y_ref, float* dw_db, int batch, int k, int n, int64_t plane,
                        float slope, float gain, void* workspace, size_t workspace_bytes, gc_stream_t stream);
int gc_pw_act_dgrad_f32(const float* dy, const float* y_ref, const float* w, float* gx, int batch, int n, int k, int64_t plane,
                        float slope, float gain, gc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Grouped dense layers of the style path: every EqualLinear of one kind in ONE launch.
 *
 * Replaces, per generator pass, the 26 `self.modulation(style)` calls of ModulatedConv2d.forward (gan_model.py:281-283; EqualLinear
 * :171-202: F.linear(input, weight * scale, bias * lr_mul)) and the 18 demodulation sums `rsqrt((weight ** 2).sum([2, 3, 4]) + 1e-8)`
 * (:284-293; here `scale^2 * (s^2) @ (sum_taps W^2)^T + eps`), and their ATen backward / double-backward GEMMs.
 *
 * Group g:   y_g[b, j] = alpha_g * sum_k x_g[b, k] * w_g[j, k] + beta_g * bias_g[j]        b < batch, j < n_g, k < k_g
 *   x_g: rows x_stride floats apart (>= k), w_g: [n, k] row-major (the EqualLinear parameter layout), bias_g: [n] or NULL, y_g: [batch, n]
 *   contiguous.  k and x_stride multiples of 4, x / w 16-byte aligned.  Any number of groups (the table is cut into launches of 32).
 * The three entry points are each other's derivatives and share the table type; the comments give the role of each pointer:
 *   gc_grouped_linear_f32        reads x, w, bias          writes y
 *   gc_grouped_linear_bwd_x_f32  reads y (= dL/dy), w      writes x (= dL/dx = alpha * gy @ w)
 *   gc_grouped_linear_bwd_w_f32  reads y (= dL/dy), x      writes w (= dL/dw = alpha * gy^T @ x) and, when non-NULL, bias (= beta * sum_b gy)
 * Fixed summation order: bit-identical from run to run. */
typedef struct gc_glin_group {
    float* x;
    float* w;
    float* bias;
    float* y;
    int32_t n, k;
    int64_t x_stride;
    float alpha, beta;
} gc_glin_group;
int gc_grouped_linear_f32(const gc_glin_group* groups, int n_groups, int batch, gc_stream_t stream);
int gc_grouped_linear_bwd_x_f32(const gc_glin_group* groups, int n_groups, int batch, gc_stream_t stream);
int gc_grouped_linear_bwd_w_f32(const gc_glin_group* groups, int n_groups, int batch, gc_stream_t stream);

/* sum over the taps of W^2 -- the weight half of ModulatedConv2d's demodulation `rsqrt(weight.pow(2).sum([2, 3, 4]) + 1e-8)`
 * (gan_model.py:289-290), which only changes with the weight -- for many weight tensors in one launch, and its gradient:
 *   gc_weight_sq_grouped_f32      out[r] = sum_t w[r, t]^2                 r < rows (= out_ch * in_ch), t < taps;   g unused
 *   gc_weight_sq_bwd_grouped_f32  out[r, t] = 2 * w[r, t] * g[r] */
typedef struct gc_wsq_group {
    const float* w;
    const float* g;
    float* out;
    int32_t rows, taps;
} gc_wsq_group;
int gc_weight_sq_grouped_f32(const gc_wsq_group* groups, int n_groups, gc_stream_t stream);
int gc_weight_sq_bwd_grouped_f32(const gc_wsq_group* groups, int n_groups, gc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * f-2  Forward pass of the FID feature network (inference, fp32): src/gan_control/fid_utils/inception.py:17-165 over
 * overwrite_inception.py.  Replaces BasicConv2d.forward (conv -> BatchNorm(eval) -> ReLU, overwrite_inception.py:424-434), the
 * F.avg_pool2d / F.max_pool2d calls of the Inception blocks (inception.py:204-305, overwrite_inception.py:252-341), the
 * nn.MaxPool2d / nn.AdaptiveAvgPool2d of the wrapper (inception.py:92-125) and its F.interpolate + `2 * x - 1` (inception.py:147-154).
 * ------------------------------------------------------------------------------------------ */

/* y[b, chan_off + n, :, :] = relu?(scale[n] * conv(x, w)[b, n] + shift[n]);  w is [out_ch, in_ch, kh, kw] (the reference layout),
 * taps up to 7 x 7 (also 1 x 7, 7 x 1, 1 x 3, 3 x 1, 5 x 5), stride 1 or 2, zero padding; scale / shift (the folded BatchNorm) may be
 * NULL (1 / 0).  The output tensor has out_channels planes per sample: a block's branches write their slices of the concatenation. */
int gc_conv2d_bn_relu_f32(const float* x, const float* w, const float* scale, const float* shift, float* y,
                          int batch, int in_ch, int out_ch, int in_h, int in_w, int kh, int kw, int stride, int pad_y, int pad_x,
                          int relu, int out_channels, int chan_off, gc_stream_t stream);

/* k x k pooling with stride / zero padding; mode 0 = max, 1 = average over the taps inside the image (count_include_pad = False,
 * the FID patch of inception.py:204-207).  Output at a channel offset as above. */
int gc_pool2d_f32(const float* x, float* y, int batch, int channels, int in_h, int in_w, int k, int stride, int pad, int mode,
                  int out_channels, int chan_off, gc_stream_t stream);

/* y[p] = mean(x[p, :]): nn.AdaptiveAvgPool2d((1, 1)) over planes = B * C. */
int gc_global_avgpool_f32(const float* x, float* y, int planes, int inner, gc_stream_t stream);

/* y = mul * bilinear(x) + add, F.interpolate(mode='bilinear', align_corners=False) semantics. */
int gc_resize_bilinear_f32(const float* x, float* y, int planes, int in_h, int in_w, int out_h, int out_w, float mul, float add, gc_stream_t stream);

/* ---- the identity predictor of the embedding loss (losses/arc_face.py, csrc/arcface.hip): forward and input gradient ---------------- */

/* adjoint = 0: y [planes, out_h, out_w] = F.interpolate(crop, (out_h, out_w), mode='bilinear', align_corners=True) of the crop
 *   x[p, top:top + crop_h, left:left + crop_w] of x [planes, in_h, in_w] (read in place: an offset and the row pitch in_w).
 * adjoint = 1: x is the gradient [planes, out_h, out_w] and y the full-size input gradient [planes, in_h, in_w], zero outside the crop;
 *   one deterministic gather pass (no atomics).  The crop must lie inside the image. */
int gc_crop_resize_ac_f32(const float* x, float* y, int planes, int in_h, int in_w, int top, int left, int crop_h, int crop_w,
                          int out_h, int out_w, int adjoint, gc_stream_t stream);

/* y[b,c,:] = prelu(x[b,c,:] * scale[c] + shift[c], alpha[c]); scale / shift / alpha may each be NULL (1, 0, no PReLU). */
int gc_affine_prelu_f32(const float* x, const float* scale, const float* shift, const float* alpha, float* y, int batch, int channels,
                        int hw, gc_stream_t stream);

/* Input gradient of gc_affine_prelu_f32: gx = g * scale[c] * (pre > 0 ? 1 : alpha[c]), pre = x * scale[c] + shift[c] (x is read only with
 * alpha), plus a second incoming gradient g2: g2_mode 0 none, 1 dense [B,C,h,w], 2 [B,C,ceil(h/2),ceil(w/2)] added at the even pixels
 * (the adjoint of the MaxPool2d(1, 2) subsample). */
int gc_affine_prelu_bwd_f32(const float* g, const float* x, const float* scale, const float* shift, const float* alpha, const float* g2,
                            int g2_mode, float* gx, int batch, int channels, int h, int w, gc_stream_t stream);

/* out[p] = mul * sum_i a[p,i] * b[p,i] over planes of `inner` elements (b may be NULL: plain sum); one workgroup per plane, fixed order. */
int gc_plane_reduce_f32(const float* a, const float* b, float* out, int planes, int inner, float mul, gc_stream_t stream);

/* Squeeze-excitation MLP per sample: z[b,:] = relu(fc1 @ m[b,:]), s[b,:] = sigmoid(fc2 @ z[b,:]); fc1 [red, channels], fc2 [channels, red]
 * (channels <= 2048, red <= 256). */
int gc_se_mlp_f32(const float* m, const float* fc1, const float* fc2, float* z, float* s, int batch, int channels, int red, gc_stream_t stream);

/* Its backward from t = dL/ds: gm[b,:] = mul * fc1^T (relu'(z) * (fc2^T (t * s * (1 - s)))). */
int gc_se_mlp_bwd_f32(const float* t, const float* s, const float* z, const float* fc1, const float* fc2, float* gm, int batch, int channels,
                      int red, float mul, gc_stream_t stream);

/* out[p, y, x] = r[p, y, x] * s[p] + sc[p, y * sc_stride, x * sc_stride] over planes of h x w; sc [planes, sc_h, sc_w] may be NULL. */
int gc_se_apply_f32(const float* r, const float* s, const float* sc, float* out, int planes, int h, int w, int sc_h, int sc_w, int sc_stride,
                    gc_stream_t stream);

/* ---- the real-image input path after the decode (datasets/image_ops.py, csrc/image_input.hip) ----------------------------------------
 * The reference builds a training batch on the host, in DataLoader workers: PIL decode, transforms.Resize (FFHQ, MetFaces:
 * ffhq_dataset.py:56-64) or RandomResizedCrop + Resize (AFHQ: afhq_dataset.py:50-59), RandomHorizontalFlip, ToTensor, Normalize(0.5, 0.5),
 * and moves float32 to the device.  Here the workers hand over the decoded uint8 [B, H, W, 3] and these three entries do the rest, with the
 * same bits: the resize is PIL's 8-bit bilinear resample (two separable passes with 22-bit fixed-point coefficients and a uint8
 * intermediate), the normalisation a 256-entry table the host fills with the reference's own float32 operation sequence.
 *
 * Common to all three: x is interleaved uint8, pixel (b, i, j) at x + b * sample_stride + i * row_stride + 3 * j (strides in BYTES, any
 * alignment: a view of a larger buffer); lut 256 floats and flip `batch` int32, both on the device; outputs are dense.  No byte of x
 * outside the pixels named below influences the result.  Bad arguments (null pointers, kmax < 1, tables that reach outside the input)
 * return GC_ERR_BAD_ARG and launch nothing.
 *
 * gc_image_u8_to_f32: y [batch, 3, h, w], y[b, c, i, j] = lut[x[b, i, jj, c]], jj = w - 1 - j where flip[b] != 0, else j.  One launch.
 *
 * gc_image_resample_u8: one resample pass along one axis, uint8 -> uint8: y [batch, out_h, out_w, 3].
 *   axis 0 (horizontal): y[b, r, o, c] = P(x[b, off_b + r, first + k, c]) for r < count_b;   axis 1 (vertical): y[b, o, q, c] =
 *   P(x[b, first + k, off_b + q, c]) for q < count_b, where for output index o (first, taps) = bounds[s, o, :] and
 *   P = clamp((2^21 + sum_{k < taps} pixel_k * coeff[s, o, k]) >> 22, 0, 255) in int32.  coeff int32 [S, out, kmax], bounds int32
 *   [S, out, 2] on the device; s = b * table_stride with table_stride 0 (S = 1: every sample shares the tables) or 1 (S = batch: per-sample
 *   crops).  `first` already includes the crop offset; coefficient slots at or past `taps` are never read.  other int32 [S, 2] on the device
 *   = (off, count) along the axis that is NOT resampled (the crop there; rows / columns of y at or past count are not produced), or NULL
 *   for (0, the output extent).  bounds_host / other_host are HOST copies of the two tables: they are what the entry validates before the
 *   launch (first >= 0, 1 <= taps <= kmax, first + taps <= the input extent; off + count inside the input, count <= the output extent);
 *   the kernels clamp what they read from the device copies to the same limits, so a device table that differs cannot read outside x.
 *
 * gc_image_resample_v_u8_to_f32: the vertical pass fused with the table lookup, the flip and the planar store:
 *   y [batch, 3, out_h, out_w], y[b, c, o, j] = lut[P(x[b, first + k, off_b + jj, c])], jj mirrored within the out_w columns where flip[b].
 *   Arguments as above (axis 1); other's count must be out_w.
 * A resize is gc_image_resample_u8(axis 0) into a uint8 intermediate followed by this entry: two launches, no float intermediate. */
int gc_image_u8_to_f32(const uint8_t* x, int64_t row_stride, int64_t sample_stride, const float* lut, const int32_t* flip, float* y,
                       int batch, int h, int w, gc_stream_t stream);
int gc_image_resample_u8(const uint8_t* x, int64_t row_stride, int64_t sample_stride, int in_h, int in_w, uint8_t* y, int batch,
                         int out_h, int out_w, int axis, const int32_t* coeff, const int32_t* bounds, const int32_t* bounds_host,
                         int kmax, int table_stride, const int32_t* other, const int32_t* other_host, gc_stream_t stream);
int gc_image_resample_v_u8_to_f32(const uint8_t* x, int64_t row_stride, int64_t sample_stride, int in_h, int in_w, const float* lut,
                                  const int32_t* flip, float* y, int batch, int out_h, int out_w, const int32_t* coeff,
                                  const int32_t* bounds, const int32_t* bounds_host, int kmax, int table_stride, const int32_t* other,
                                  const int32_t* other_host, gc_stream_t stream);

/* ---- the image output path (evaluation/image_grid.py, csrc/image_output.hip) ------------------------------------------------------------
 * The mirror image of the entries above: float32 planar images in [-1, 1] -> ONE uint8 interleaved image grid, in one launch.  It stands for
 * the reference's host chain t.mul(0.5).add(0.5).clamp(min=0., max=1.) -> torchvision.utils.make_grid -> ToPILImage (mul(255).byte())
 * (evaluation/generation.py:14-22, :87-94), with the same bytes.
 *
 * x: float32 [batch, 3, h, w] on the device, element (b, c, i, j) at x + b * sample_stride + c * plane_stride + i * row_stride + j (strides in
 * ELEMENTS, at least dense: row_stride >= w, plane_stride >= (h - 1) * row_stride + w, sample_stride >= 2 * plane_stride + (h - 1) * row_stride
 * + w; a slice of a larger batch or rows with a pitch are fine).  y: uint8 [grid_h, grid_w, 3] on the device, byte (r, q, c) at
 * y + r * y_row_stride + 3 * q + c (y_row_stride in BYTES, >= 3 * grid_w; y may start at any byte).
 *
 * Geometry (make_grid's): xmaps = min(nrow, batch), ymaps = ceil(batch / xmaps), grid_h = ymaps * (h + padding) + padding, grid_w = xmaps *
 * (w + padding) + padding; tile k occupies rows (k / xmaps) * (h + padding) + padding + [0, h) and columns (k % xmaps) * (w + padding) +
 * padding + [0, w).  The caller passes grid_h and grid_w; they are recomputed here and a mismatch is refused.  nrow 1 with padding 0 gives
 * [batch * h, w, 3]: a dense uint8 [batch, h, w, 3].
 *
 * A tile byte is trunc(v4), v1 = x * 0.5f, v2 = v1 + 0.5f, v3 = min(max(v2, 0), 1), v4 = v3 * 255.0f, every step rounded to float32 on its own
 * (x * 127.5f + 127.5f is another function: it differs on 223 of the 510 floats next to a byte boundary).  +-inf follow the clamp (255 / 0);
 * NaN gives byte 0.  Every other byte of the grid -- the padding bands and the empty tiles of a ragged last row -- is pad_value (0 .. 255).
 * Every byte of y[0:grid_h, 0:3 * grid_w] is stored exactly once (y may be uninitialised), nothing else is stored, and nothing outside the
 * batch * 3 * h * w floats named above is loaded.  Null pointers, non-positive extents, padding < 0, a pad_value outside a byte, grid_h /
 * grid_w that differ from the geometry and short strides return GC_ERR_BAD_ARG and launch nothing. */
int gc_image_f32_to_u8_grid(const float* x, int64_t row_stride, int64_t plane_stride, int64_t sample_stride, uint8_t* y, int64_t y_row_stride,
                            int batch, int h, int w, int nrow, int padding, int pad_value, int grid_h, int grid_w, gc_stream_t stream);

/* ---- image projection: the noise regulariser and the noise normaliser (projection/, csrc/noise_reg.hip) ------------------------------------
 * The reference's noise_regularize and noise_normalize_ (projection/projection.py:126-154) over a whole LIST of noise maps in a number of
 * launches that depends neither on the length of the list nor on the depth of the pyramids (forward 3, backward 1, normalise 3).
 *
 * maps / grads: HOST arrays of n DEVICE pointers, map m a dense float32 [batches[m], 1, sizes[m], sizes[m]] (4-byte alignment is enough);
 * sizes / batches / counts: HOST arrays.  sizes[m] is a power of two in [4, 1024]; n <= 32.  Pointers and extents travel by value in the
 * kernel arguments: nothing is uploaded.
 *
 * gc_noise_reg_fwd_f32:  loss[0] (DEVICE) = sum over maps and pyramid levels of mean(n_l * roll(n_l, 1, x))^2 + mean(n_l * roll(n_l, 1, y))^2,
 * the means over the whole tensor, batch included; n_0 = the map, n_(l+1) = the 2 x 2 means of n_l; the level loop is the reference's: the
 * terms, stop if size <= 8, otherwise halve (a 4 x 4 and an 8 x 8 map contribute one level).  The workspace (gc_noise_reg_workspace bytes)
 * receives the pyramids and the coefficients 2 * mean / N and must reach gc_noise_reg_bwd_f32 unchanged, together with unchanged maps.
 * gc_noise_reg_bwd_f32:  grads[m][b,0,y,x] = gout[0] * d loss / d maps[m][b,0,y,x], gout a DEVICE scalar (no host synchronisation): a gather of
 * sum_l 0.25^l * (cx_l * (n_l[Y, X-1] + n_l[Y, X+1]) + cy_l * (n_l[Y-1, X] + n_l[Y+1, X])) at (Y, X) = (y >> l, x >> l), indices wrapped.
 * gc_noise_normalize_f32:  every map becomes (n - mean) / std IN PLACE, mean and the unbiased standard deviation over all counts[m] >= 2
 * elements; the variance is centred per chunk of 4096 elements and the chunks merged in float64 (nothing is squared before its mean is taken
 * off).  Workspace: gc_noise_normalize_workspace bytes.
 * Every sum is store-and-add in an order fixed by the shapes (no float atomics): the same inputs give the same bits.  Null pointers, an empty
 * list, a size that is no power of two >= 4 or a count below 2 return GC_ERR_BAD_ARG, more than 32 maps, a size above 1024 or more than 2^31
 * elements GC_ERR_UNSUPPORTED, a short workspace GC_ERR_WORKSPACE; the workspace queries return 0 for such a list.  Nothing is launched then. */
size_t gc_noise_reg_workspace(const int32_t* sizes, const int32_t* batches, int n);
int gc_noise_reg_fwd_f32(const float* const* maps, const int32_t* sizes, const int32_t* batches, int n, float* loss,
                         void* workspace, size_t workspace_bytes, gc_stream_t stream);
int gc_noise_reg_bwd_f32(const float* const* maps, const int32_t* sizes, const int32_t* batches, int n, const float* gout,
                         float* const* grads, const void* workspace, size_t workspace_bytes, gc_stream_t stream);
size_t gc_noise_normalize_workspace(const int64_t* counts, int n);
int gc_noise_normalize_f32(float* const* maps, const int64_t* counts, int n, void* workspace, size_t workspace_bytes, gc_stream_t stream);

/* ---- whole EqualLinear stacks: the mapping networks and the controllers of the inference API (models/op/fc_stack.py, csrc/fc_stack.hip) -----
 * n_stacks independent stacks of EqualLinear(activation='fused_lrelu') layers (gan_model.py:171-202, :25-41) on `batch` rows each, in one
 * launch per 8 stacks: what Generator.style (MultiFcStack, gan_model.py:489-502: PixelNorm on the group's slice, gan_model.py:58-63) and the
 * controllers' FcStack (controller_model.py:13-53) compute layer by layer.  Stack s:
 *   h_0     = pixel_norm[s] ? x_s * rsqrt(mean_k(x_s^2) + 1e-8) : x_s                       (the mean over the stack's own in_dim[s] columns)
 *   h_(l+1) = leaky_relu(alpha_l * h_l @ W_l^T + beta_l * bias_l, 0.2) * sqrt(2)            (alpha = lr_mul / sqrt(in), beta = lr_mul)
 *   y_s[b, :] = h_(n_layers[s])[b, :]
 * Per stack (HOST arrays of n_stacks entries): x[s] / y[s] DEVICE pointers, row b at x[s] + b * x_stride[s] and y[s] + b * y_stride[s]
 * (strides in ELEMENTS, at least the row's width; any 4-byte alignment: a column slice of a wider [batch, 512] tensor is fine, which is
 * how one call reads the groups of z, writes the groups of w without a cat, and splices a controller's output into w), in_dim[s],
 * n_layers[s], pixel_norm[s].  Per layer (HOST arrays of sum_s n_layers[s] entries, stack after stack): w DEVICE [out_dim, in] dense, the
 * parameter layout (in = the previous layer's out_dim, or in_dim[s]); bias DEVICE [out_dim] or NULL; out_dim; alpha; beta.  A layer whose
 * `in` is a multiple of 4 and whose w is 16-byte aligned streams its rows with 16-byte loads, any other one with 4-byte loads.
 * No y row may overlap an x row or a y row of another stack of the same call.  Only the out_dim columns of the `batch` rows of y are
 * stored; no byte outside the in_dim columns of the `batch` rows of x, the weights and the biases is loaded.  fp32 FMA, every sum in an
 * order fixed by the shapes: the same inputs give the same bits.  The tables travel by value in the kernel arguments: nothing is uploaded.
 * Built: 1 .. 8 layers per stack, widths 1 .. 512, batch >= 1, any number of stacks; anything else returns GC_ERR_UNSUPPORTED (batch < 1
 * included); null pointers, n_stacks < 0 and short strides GC_ERR_BAD_ARG.  Nothing is launched then.  n_stacks == 0 is a no-op. */
int gc_fc_stacks_fwd_f32(const float* const* x, const int64_t* x_stride, float* const* y, const int64_t* y_stride,
                         const int32_t* in_dim, const int32_t* n_layers, const int32_t* pixel_norm,
                         const float* const* w, const float* const* bias, const int32_t* out_dim, const float* alpha, const float* beta,
                         int n_stacks, int batch, gc_stream_t stream);

/* ---- one optimisation step of one FC stack: controller training (models/op/fc_train.py, csrc/fc_train.hip) ------------------------------
 * What ControllerTrainer.controller_update computes for the `latent_rec` objective (controller_trainer.py:202-229) -- forward, L1 / MSE
 * against a column slice of the w latents, backward, torch.optim.Adam -- in n_layers + 2 launches.  The stack is ONE stack of
 * gc_fc_stacks_fwd_f32 without PixelNorm, described by the same per-layer HOST arrays (w DEVICE [out_dim, in] dense, bias DEVICE [out_dim]
 * and required here, out_dim, alpha, beta) and the same input description (x, x_stride in ELEMENTS, in_dim; any 4-byte alignment).
 * Workspaces: `acts` and `grads` are DEVICE float arrays of batch * sum_l out_dim[l] elements; layer l's part is the dense
 * [batch, out_dim[l]] block at element offset batch * sum_(i<l) out_dim[i] of either.
 * Built: 1 .. 8 layers, every width 1 .. 512 (any alignment of the first weight), batch 1 .. 64; anything else returns GC_ERR_UNSUPPORTED;
 * a null table, pointer or workspace and a row stride shorter than the row GC_ERR_BAD_ARG.  Everything is checked before the first launch.
 * fp32 FMA only, every sum in an order fixed by the shapes, no atomics, no flags, no grid barrier: the same inputs give the same bits.
 *
 * gc_fc_stack_fwd_save_f32: the forward of gc_fc_stacks_fwd_f32 (the same layer code: the same bits), which also stores every layer's
 * output into its block of acts; the last block is the prediction.  Only acts is stored.
 *
 * gc_rec_loss_grad_f32: pred DEVICE dense [batch, n]; target row b at target + b * target_stride (ELEMENTS, at least n: a column slice of
 * the w latent rows is read in place).  With d = pred - target and N = batch * n:
 *   GC_REC_LOSS_L1:  *loss = sum |d| / N,   dy = sign(d) / N   (sign(0) = 0)
 *   GC_REC_LOSS_MSE: *loss = sum d^2 / N,   dy = 2 d / N
 * dy DEVICE dense [batch, n] (the last block of grads), loss one DEVICE float.  One workgroup.  Only dy and *loss are stored.
 *
 * gc_fc_stack_bwd_adam_f32: one launch per layer, last to first.  On entry the last block of grads holds d(loss) / d(prediction) and acts
 * what gc_fc_stack_fwd_save_f32 stored for the same x and parameters.  Layer l, with dY its block of grads, A_l its block of acts,
 * A_(l-1) the block before it (x for l = 0) and W [n, k]:
 *   g = dY * (A_l > 0 ? 1 : 0.2) * sqrt(2)      (the sign of an output is the sign of its pre-activation; an output of 0 takes the 0.2 slope)
 *   db = beta sum_b g,   dW = alpha g^T A_(l-1),   dX = alpha g W -> the block of grads before it (not computed for l = 0)
 * and, in the same launch, torch.optim.Adam's update (weight_decay 0, no amsgrad, no maximize) of W, bias and their moments in place:
 *   m = beta1 m + (1 - beta1) grad,   v = beta2 v + (1 - beta2) grad^2,
 *   p -= (lr / bias_correction1) * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with bias_correction1 = 1 - beta1^t and bias_correction2_sqrt = sqrt(1 - beta2^t) computed by the caller (both > 0, else
 * GC_ERR_BAD_ARG).  The six scalars arrive in float64; beta, 1 - beta, lr / bias_correction1, bias_correction2_sqrt and eps are each rounded
 * to float32 once, as torch.optim.Adam hands them to its kernels (1 - beta2 formed from a float32 beta2 is off by up to 4e-6 of its value).
 * w_m / w_v / b_m / b_v: HOST arrays of n_layers DEVICE pointers to the moments, shaped like w / bias.  A workgroup owns 8 columns of W and
 * produces dX and dW for them completely, so the gradients of the parameters never reach memory.  Stored: w, bias, the moments and all
 * blocks of grads but the last.
 *
 * gc_fc_train_launches: the number of kernel launches the three entries have issued in this process so far (one each for the forward and the
 * loss, n_layers for the backward); a refused call adds nothing. */
#define GC_REC_LOSS_L1 0
#define GC_REC_LOSS_MSE 1
int gc_fc_stack_fwd_save_f32(const float* x, int64_t x_stride, int in_dim, int n_layers, const float* const* w, const float* const* bias,
                             const int32_t* out_dim, const float* alpha, const float* beta, float* acts, int batch, gc_stream_t stream);
int gc_rec_loss_grad_f32(const float* pred, const float* target, int64_t target_stride, int batch, int n, int kind, float* dy, float* loss,
                         gc_stream_t stream);
int gc_fc_stack_bwd_adam_f32(const float* x, int64_t x_stride, int in_dim, int n_layers, float* const* w, float* const* bias,
                             const int32_t* out_dim, const float* alpha, const float* beta, float* const* w_m, float* const* w_v,
                             float* const* b_m, float* const* b_v, const float* acts, float* grads, int batch, double lr, double beta1,
                             double beta2, double eps, double bias_correction1, double bias_correction2_sqrt, gc_stream_t stream);
int64_t gc_fc_train_launches(void);

/* ---- all-pairs feature distances of the separability evaluation (models/op/pairwise.py, csrc/pairwise.hip) -----------------------------
 * What LossModelClass.calc_distances computes chunk pair by chunk pair (loss_model.py:252-285) and the per-query minimum of
 * calc_same_not_same_list (loss_model.py:214-229), in one call.  s [m, k] (signatures) and q [n, k] (queries): row i at s + i * s_stride,
 * row j at q + j * q_stride (strides in ELEMENTS, at least k; elements of a row adjacent; any 4-byte alignment: features[::2] is read in
 * place with stride 2 k).  d [m, n] dense:
 *   GC_PAIRWISE_ABS: d[i, j] = (sum_c |s[i, c] - q[j, c]|) / k        (L1Expend, loss_model.py:308-321; the mean-absolute criteria)
 *   GC_PAIRWISE_SQ:  d[i, j] = sum_c (s[i, c] - q[j, c])^2            (arc_face_criterion.py:15-21; the difference itself, no expansion)
 * With s_pid [m] and q_pid [n] (DEVICE int32, both or neither) also, for every column j over the rows i with s_pid[i] != q_pid[j]:
 * best[j] = min d[i, j] and best_idx[j] = the lowest such i that attains it -- taken over the float32 values stored in d, so min / argmin
 * of the returned matrix reproduce them exactly (a column without such a row: +inf and -1).  Inputs are assumed finite.
 * A tile kernel (operands staged through LDS, a register micro-tile per thread; 16-byte loads when both bases are 16-byte aligned and both
 * strides and k are multiples of 4, else 4-byte loads) and, where long rows are split along k over workgroups or pids are given, a second
 * launch that adds the partial sums of the workspace in ascending order, divides, stores d and takes the minima: at most two launches, no
 * atomics, every sum in an order fixed by (m, n, k) -- the same inputs give the same bits.  Only d, best, best_idx and the workspace are
 * stored; no byte outside the k columns of the m / n rows and the pids is loaded.  Workspace: gc_pairwise_workspace(m, n, k) bytes (0
 * where nothing is split, and for extents below 1).  Null s / q / d, extents below 1, a stride below k, an unknown mode, one pid array
 * without the other and pids without best / best_idx return GC_ERR_BAD_ARG, a short workspace GC_ERR_WORKSPACE, more than 65535 * 64 rows
 * GC_ERR_UNSUPPORTED.  Nothing is launched then. */
#define GC_PAIRWISE_ABS 0
#define GC_PAIRWISE_SQ 1
size_t gc_pairwise_workspace(int m, int n, int k);
int gc_pairwise_f32(const float* s, int64_t s_stride, const float* q, int64_t q_stride, int m, int n, int k, int mode, float* d,
                    const int32_t* s_pid, const int32_t* q_pid, float* best, int32_t* best_idx, void* workspace, size_t workspace_bytes,
                    gc_stream_t stream);

/* ---- the same / not-same hinge loss of one feature level of the attribute stage (models/op/pair_hinge.py, csrc/pair_hinge.hip) ------------
 * What LossModelClass.calc_mini_batch_loss computes per level (loss_model.py:121-181) and its gradient, without the cat / mask gathers.
 * f: n_rows rows of k values, row r at f + r * stride (stride in ELEMENTS, at least k; elements of a row adjacent; any 4-byte alignment: a
 * column slice vec[:, 227:254] is read in place).  row_index: HOST int32 [n] or null -- the rows of f in pair order ("same block, then the
 * rest"), distinct and inside [0, n_rows); it is checked and copied into the kernel arguments by the call (null: n_rows == n, in order).
 * row_valid: DEVICE float [n_rows] or null -- v_r = 1 where the entry is non-zero, else 0 (null: all 1); GC_PAIR_HINGE_ABS only reads it.
 * With n = n_same + n_not_same, for the pairs i > j of the pair order:
 *   GC_PAIR_HINGE_ABS: D[i, j] = v_i v_j (sum_c |F_i,c - F_j,c|) / k      (the mean-absolute criteria, L1Expend, the hair criterion)
 *   GC_PAIR_HINGE_SQ:  D[i, j] = sum_c (F_i,c - F_j,c)^2                    (squared L2)
 *   GC_PAIR_HINGE_MSQ: D[i, j] = (sum_c (F_i,c - F_j,c)^2) / k * scale      (the style criterion, scale = 1e5)
 * The pair sets are those of LossModelClass.pair_masks + _level_loss: 'same' = the pairs (j + 1, j), j even, with j < 2 (n_same / 2)
 * (GC_PAIR_HINGE_FOCUS_SAME) or 2 (n_same / 2) <= j < 2 (n_same / 2) + 2 (n_not_same / 2) (GC_PAIR_HINGE_FOCUS_NOT_SAME); 'rest' = every
 * other pair below the diagonal.  Forward writes loss[0] = weight * (mean over same of max(D - lower, 0) + mean over rest of max(upper - D, 0)),
 * d [n, n] = D and c [n, n] = dloss / dD (weight / count where the hinge is active -- at zero too, as torch.clamp -- else 0); both are zero
 * on and above the diagonal.  n k <= GC_PAIR_HINGE_ONE_LAUNCH_VALUES: one launch of one workgroup; longer rows: a tile launch split along k
 * that writes partial sums to the workspace and a one-workgroup launch that adds them in a fixed order and finishes.
 * Backward, one launch: df [n_rows, k] DENSE, df[row_index[i], c] = g[0] * sum_{j != i} C[max(i, j), min(i, j)] v_i v_j phi'(F_i,c - F_j,c) with
 * phi'(x) = sign(x) / k (ABS; sign(0) = 0), 2 x (SQ), 2 scale x / k (MSQ); rows of f outside row_index get zeros.  g: DEVICE float [1].
 * No atomics; every sum in an order fixed by (n, k): the same inputs give the same bits.  Workspace: gc_pair_hinge_workspace(n, k) bytes (0
 * for one-launch shapes and for refused extents).  Null pointers, k < 1, n < 2, n_rows < n (or != n without an index), a stride below k, an
 * unknown mode or focus, a bad or repeated row_index entry and an empty pair set return GC_ERR_BAD_ARG, n > GC_PAIR_HINGE_MAX_ROWS or
 * n_rows > GC_PAIR_HINGE_MAX_BATCH_ROWS GC_ERR_UNSUPPORTED, a short workspace GC_ERR_WORKSPACE.  Nothing is launched then. */
#define GC_PAIR_HINGE_ABS 0
#define GC_PAIR_HINGE_SQ 1
#define GC_PAIR_HINGE_MSQ 2
#define GC_PAIR_HINGE_FOCUS_SAME 0
#define GC_PAIR_HINGE_FOCUS_NOT_SAME 1
#define GC_PAIR_HINGE_MAX_ROWS 64
#define GC_PAIR_HINGE_MAX_BATCH_ROWS 1024
#define GC_PAIR_HINGE_ONE_LAUNCH_VALUES 8192
size_t gc_pair_hinge_workspace(int n, int k);
int gc_pair_hinge_fwd_f32(const float* f, int64_t stride, int n_rows, const int32_t* row_index, const float* row_valid, int n_same, int n_not_same,
                          int k, int mode, float scale, int focus, float lower, float upper, float weight, float* loss, float* d, float* c,
                          void* workspace, size_t workspace_bytes, gc_stream_t stream);
int gc_pair_hinge_bwd_f32(const float* f, int64_t stride, int n_rows, const int32_t* row_index, const float* row_valid, int n, int k, int mode,
                          float scale, const float* c, const float* g, float* df, gc_stream_t stream);

/* ---- group interpolation of the inference API (models/op/interp.py, csrc/interp.hip) --------------------------------------------------------
 * The blends of Inference.interpolate_by_group (reference: evaluation/inference_class.py:125-185), each in one launch.
 *
 * gc_latent_interp_f32: every frame of one interpolation segment, both films.  fixed, from, to: DEVICE [batch, latent] float32, elements of
 * a row adjacent, row b at p + b * stride (strides in ELEMENTS: at least latent, or 0 -- the inputs are only read and the reference's latent_1
 * is one expanded row; any 4-byte alignment).  0 <= lo < hi <= latent names the group G = [lo, hi); S = [0, lo), E = [hi, latent).  wa, wb: HOST
 * arrays of `frames` floats (1 .. 64), carried in the kernel arguments.  out: DEVICE dense [2, frames, batch, latent]:
 *   out[0, f, b] = [ blend_f(from, to) on S | fixed on G | blend_f(from, to) on E ]          (the group is frozen)
 *   out[1, f, b] = [ fixed on S | blend_f(from, to) on G | fixed on E ]                      (only the group moves)
 *   GC_INTERP_LINEAR, GC_INTERP_SQRT: blend_f(x, y) = fl(fl(wa[f] * x) + fl(wb[f] * y)) -- two rounded products and a rounded sum, never an
 *     FMA: bit for bit what ATen computes for a * x + b * y with float32 scalars (the two modes differ in the weights the caller passes);
 *   GC_INTERP_SLERP: per row and per slice (S, G and E each on its own), omega = acos(x.y / (|x| |y|)), ca = sin(wa[f] omega) / sin(omega),
 *     cb = sin(wb[f] omega) / sin(omega), blend_f(x, y) = fl(fl(ca * x) + fl(cb * y)).  The row sums are taken once per row in float64 in an
 *     order fixed by the extents (no atomics: the same inputs give the same bits), the coefficients computed in float64 and rounded once.
 *     Nothing is clamped: parallel slices are as undefined as in the reference.
 * An empty S (lo == 0) or E (hi == latent) is neither read nor written and forms no coefficient.  Only out is stored; no byte outside the
 * `latent` columns of the rows is loaded.  Null pointers, extents below 1, a group outside the row, frames < 1, an unknown mode and a stride
 * that is negative or in (0, latent) return GC_ERR_BAD_ARG, more than 64 frames or 2^31 output elements GC_ERR_UNSUPPORTED; nothing is
 * launched then.
 *
 * gc_noise_blend_f32: out[m][i] = fl(fl(wa * a[m][i]) + fl(wb * b[m][i])) for i < counts[m], over a whole list of maps in ONE launch.
 * a, b, out: HOST arrays of n (1 .. 32) DEVICE pointers to dense float32; counts: HOST array, counts[m] >= 1.  A map whose three pointers
 * are 16-byte aligned moves in 16-byte words with a 4-byte tail of counts[m] % 4 elements, any other one in 4-byte words.  a[m] and b[m] may
 * be the same memory; no output may overlap an input or another output.  Null pointers, n < 1, a count below 1 and an overlap return
 * GC_ERR_BAD_ARG, more than 32 maps GC_ERR_UNSUPPORTED; nothing is launched then. */
#define GC_INTERP_LINEAR 0
#define GC_INTERP_SLERP 1
#define GC_INTERP_SQRT 2
int gc_latent_interp_f32(const float* fixed, int64_t fixed_stride, const float* from, int64_t from_stride, const float* to, int64_t to_stride,
                         int batch, int latent, int lo, int hi, const float* wa, const float* wb, int frames, int mode, float* out,
                         gc_stream_t stream);
int gc_noise_blend_f32(const float* const* a, const float* const* b, float* const* out, const int64_t* counts, int n, float wa, float wb,
                       gc_stream_t stream);

/* ---- per-group latent PCA (projection/pca.py through models/op/group_pca.py, csrc/group_pca.hip) ------------------------------------------
 * A group table is two HOST arrays lo, hi of `groups` int32: group g is the columns [lo[g], hi[g]) of a row, width D_g = hi[g] - lo[g].
 * Limits: 1 <= groups <= GC_GROUP_MAX, 1 <= D_g <= GC_GROUP_MAX_WIDTH, hi[g] <= stride; n * stride must fit an int64.
 *
 * gc_group_moments_f32: w: DEVICE float32 [n, stride] (row r at w + r * stride, stride in ELEMENTS, any 4-byte alignment), 2 <= n <=
 * GC_GROUP_MAX_ROWS.  mean: DEVICE float64 [sum D_g] and cov: DEVICE float64 [sum D_g^2], both packed group after group in table order; cov
 * of a group is a full row-major symmetric D_g x D_g matrix with divisor n - 1 (scikit-learn's explained_variance_ convention):
 *   mean[g][i] = S1_i / n,   cov[g][i, j] = (S2_ij - S1_a S1_c / n) / (n - 1),   (a, c) = (min(i, j), max(i, j)),
 * S1 = sum_r x_r and S2 = sum_r x_r x_r^T over the group's columns, values widened to float64 on load, products exact, sums in float64 over
 * splits of R = GC_GROUP_ROW_SPLIT rows in ascending row order -- R = 16 * ceil(ceil(n / GC_GROUP_MAX_SPLITS) / 16) where n / GC_GROUP_ROW_SPLIT
 * would make more than GC_GROUP_MAX_SPLITS splits --, the splits' partial sums added in ascending order by a second launch of the same call.  cov[g][i, j] and cov[g][j, i] are the same bits; no atomics: the same inputs give the same bits on every run.  Only tiles on or above
 * the diagonal are computed.  No byte outside the D_g columns of the n rows of each group is loaded (columns of no group are never read);
 * 16-byte loads where w is 16-byte aligned, stride % 4 == 0 and lo[g] % 4 == 0, 4-byte loads otherwise: both stage the same values.  Only
 * mean, cov and the workspace are stored.  Workspace: gc_group_moments_workspace(n, lo, hi, groups) bytes = ceil(n / R) * (sum D_g +
 * sum D_g^2) * 8, at most GC_GROUP_MAX_SPLITS partial sets (0 for arguments outside the limits).  Null pointers, n < 2, an empty group or one outside the stride return
 * GC_ERR_BAD_ARG, more than GC_GROUP_MAX groups, a group wider than GC_GROUP_MAX_WIDTH or more than GC_GROUP_MAX_ROWS rows
 * GC_ERR_UNSUPPORTED, a short workspace GC_ERR_WORKSPACE; nothing is launched then.
 *
 * gc_group_project_f32: in place, for every row r < rows of x (DEVICE float32, row r at x + r * stride) and every group:
 *   x_g <- m_g + P_g^T (P_g (x_g - m_g))
 * with m_g = mean[lo[g] .. hi[g]) (DEVICE float32, indexed by column) and P_g = components[g] (a HOST array of DEVICE pointers to dense
 * float32 [ranks[g], D_g] matrices, 1 <= ranks[g] <= D_g).  float32 arithmetic in a fixed order: d = fl(x - m); c_k = sum over columns in
 * ascending steps of 64 (fused multiply-adds) and a fixed butterfly over the 64 partial sums; y_j = fused multiply-adds over k ascending,
 * then fl(m_j + y_j).  Columns outside every group keep their bits; one launch.  Null pointers, rows < 1, ranks outside [1, D_g], groups
 * that overlap and the group-table errors above return GC_ERR_BAD_ARG / GC_ERR_UNSUPPORTED; nothing is launched then. */
#define GC_GROUP_MAX 16
#define GC_GROUP_MAX_WIDTH 512
#define GC_GROUP_ROW_SPLIT 256
#define GC_GROUP_MAX_SPLITS 64
#define GC_GROUP_MAX_ROWS (65535 * GC_GROUP_ROW_SPLIT)
size_t gc_group_moments_workspace(int n, const int32_t* lo, const int32_t* hi, int groups);
int gc_group_moments_f32(const float* w, int64_t stride, int n, const int32_t* lo, const int32_t* hi, int groups, double* mean, double* cov,
                         void* workspace, size_t workspace_bytes, gc_stream_t stream);
int gc_group_project_f32(float* x, int64_t stride, int rows, const float* mean, const float* const* components, const int32_t* ranks,
                         const int32_t* lo, const int32_t* hi, int groups, gc_stream_t stream);

/* ---- distance passes of the sample-quality metrics (models/op/manifold.py, csrc/manifold.hip) ---------------------------------------------
 * Improved precision / recall (Kynkaanniemi et al. 2019) and KID (Binkowski et al. 2018) on DEVICE float32 feature rows: row i of a set at
 * p + i * stride (strides in ELEMENTS, at least k; elements of a row adjacent; any 4-byte alignment: features[::2] is read in place).
 * Squared distances are D[i, j] = sum_c (a[i, c] - b[j, c])^2 in float32 fused multiply-adds over c ascending: the difference itself, as
 * GC_PAIRWISE_SQ, never |a|^2 + |b|^2 - 2 a.b.  The loop nest and the LDS staging are those of gc_pairwise_f32 (16-byte loads when every
 * base is 16-byte aligned and every stride and k are multiples of 4, else 4-byte loads; no byte past a row's k-th element is loaded), but no
 * m x n value is stored: a workgroup walks a strip of tiles and keeps what the tile epilogue reduces to, and a second launch merges the
 * strips' partial results from the workspace in ascending strip order.  At most GC_MANIFOLD_STRIPS strips a side whatever the extents, so
 * every workspace is O((m + n) * GC_MANIFOLD_STRIPS); the queries are functions of the extents alone (0 for extents outside the limits).
 * At most two launches per call, no atomics, no workgroup waits for another, every sum and merge in an order fixed by the extents: the same
 * inputs give the same bits.  Every element of the outputs is stored by the call; the caller zeroes nothing.  Inputs are assumed finite.
 * Each entry refuses null pointers, extents below 1 and strides below k with GC_ERR_BAD_ARG, a short workspace with GC_ERR_WORKSPACE and more
 * than 65535 * 64 rows a side with GC_ERR_UNSUPPORTED; nothing is launched and no output is touched then.
 *
 * gc_knn_radius_f32: radius2[i] (float[n]) = the (kth + 1)-th smallest value of row i of D(a, a), the row's own 0 included: the squared
 * distance to the kth nearest OTHER row (torch's kthvalue(kth + 1)).  1 <= kth <= GC_KNN_MAX_KTH and n >= kth + 1, else GC_ERR_BAD_ARG.
 * The tile epilogue keeps each row's kth + 1 smallest values of the columns of its strip, ascending; the finish pass merges the lists.
 *
 * gc_manifold_hits_f32: one pass over D(ref [m, k], probe [n, k]):
 *   probe_hit[j] (uint8[n]) = any_i D[i, j] <= ref_radius2[i]            (probe j lies in the ref manifold)
 *   ref_hit[i]   (uint8[m]) = any_j D[i, j] <= probe_radius2[j]          (with probe_radius2 and ref_hit: both given or both null)
 * The comparison is <=: a tie is a hit.  With ref = real and probe = fake features, mean(probe_hit) is precision and mean(ref_hit) recall.
 * One of the pair without the other returns GC_ERR_BAD_ARG.
 *
 * gc_poly_mmd_f32: for each subset s < subsets, with X_i = x[idx_x[s, i]] and Y_i = y[idx_y[s, i]], i < m (idx_*: DEVICE int32 [subsets, m];
 * the rows are gathered inside the kernel; values outside [0, nx) / [0, ny) are the caller's error) and kappa(u, v) = (u.v / k + 1)^3:
 *   sums[s, 0] = sum_{i != j} kappa(X_i, X_j)      sums[s, 1] = sum_{i != j} kappa(Y_i, Y_j)      sums[s, 2] = sum_{i, j} kappa(X_i, Y_j)
 * (DEVICE double [subsets, 3]).  u.v in float32 fused multiply-adds over c ascending; the division, the cube and every partial and final
 * sum in float64.  subsets <= 21845, else GC_ERR_UNSUPPORTED. */
#define GC_MANIFOLD_STRIPS 32
#define GC_KNN_MAX_KTH 7
size_t gc_knn_radius_workspace(int n, int k, int kth);
int gc_knn_radius_f32(const float* a, int64_t a_stride, int n, int k, int kth, float* radius2, void* workspace, size_t workspace_bytes,
                      gc_stream_t stream);
size_t gc_manifold_hits_workspace(int m, int n, int k);
int gc_manifold_hits_f32(const float* ref, int64_t ref_stride, const float* ref_radius2, int m, const float* probe, int64_t probe_stride,
                         const float* probe_radius2, int n, int k, uint8_t* probe_hit, uint8_t* ref_hit, void* workspace,
                         size_t workspace_bytes, gc_stream_t stream);
size_t gc_poly_mmd_workspace(int subsets, int m, int k);
int gc_poly_mmd_f32(const float* x, int64_t x_stride, int nx, const float* y, int64_t y_stride, int ny, int k, const int32_t* idx_x,
                    const int32_t* idx_y, int subsets, int m, double* sums, void* workspace, size_t workspace_bytes, gc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GANCONTROL_HIP_H */
