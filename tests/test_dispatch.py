"""Which kernel takes which layer of the FFHQ-1024 step (no GPU needed: gc_conv2d_variant_name runs the dispatch code in a no-launch probe mode).

The launchers decide by shape -- tile counts, LDS fit, workgroups per CU -- and several of those rules were MEASURED (DESIGN.md section 8, items 6 and 7:
a transposed layer on the H x W + edge form below 512 main-region workgroups is slower, more K slices than ~512 workgroups need are slower, ...).  These
tests pin the decisions for the shapes the training step launches, so that a change of one eligibility rule shows up here and not only as a slower bench line.
"""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'gan-control_amd'))

from gan_control_amd import _lib                                        # noqa: E402
from gan_control_amd.models.op._backend import ConvGeom                 # noqa: E402
from gan_control_amd.utils.profiling import conv_variant, wgrad_variant   # noqa: E402


def _out(n, k, up, down, pad):
    return (n - 1) * up + k - 2 * (k - 1 - pad) if up > 1 else (n + 2 * pad - k) // down + 1


def _probe(b, K, N, h, k, up, down, pad, mode='bf16x3'):
    o = _out(h, k, up, down, pad)
    geom = ConvGeom(k, k, up, down, pad, pad, o, o)
    desc = _lib.ConvDesc(b, K, N, h, h, o, o, k, k, up, down, pad, pad)
    return conv_variant(geom, N, b, K, mode, (h, h)), int(_lib.load().gc_conv2d_bf16x3_splitk_bytes(desc))


# (batch, K, N, plane, taps, up, down, pad) -> (kernel name prefix, split over K?)
STEP_SHAPES = [
    # stride 1: wave-specialised from 64^2 up, one-role kernel with K slices below, the exact-fp32 small-plane kernel at <= 8 x 8
    ((4, 512, 512, 64, 3, 1, 1, 1), 'conv_bf16x3_ws_kernel<3,2,1>', False),
    ((4, 32, 32, 1024, 3, 1, 1, 1), 'conv_bf16x3_ws_kernel<3,1,', False),
    ((4, 512, 512, 32, 3, 1, 1, 1), 'conv_bf16x3_kernel<1,4,2,1>|up1,down1', True),
    ((8, 512, 512, 32, 3, 1, 1, 1), 'conv_bf16x3_kernel<1,4,2,1>|up1,down1', False),      # 512 workgroups of 4-row tiles already: unsplit (round 5)
    ((4, 512, 512, 16, 3, 1, 1, 1), 'conv_bf16x3_kernel<1,4,2,1>|up1,down1', True),
    ((4, 512, 512, 8, 3, 1, 1, 1), 'conv_f32_small_kernel<3,1,2,1>|up1,down1', False),
    ((4, 513, 512, 4, 3, 1, 1, 1), 'conv_f32_small_kernel<3,2,1,1>|up1,down1', False),
    # stride 2 (after the Blur: 2H + 1 -> H); 17 -> 8 at B = 8 in two sample groups of the small-plane kernel (round 5: was conv_mfma_kernel)
    # (round 6: the layers with >= 192 eight-row tiles x samples x oc blocks on the wave-specialised E / O kernel; 128- or 64-channel output blocks)
    ((4, 128, 256, 257, 3, 1, 2, 0), 'conv_s2ws_bf16x3_kernel<2>|up1,down2', False),
    ((8, 32, 64, 1025, 3, 1, 2, 0), 'conv_s2ws_bf16x3_kernel<1>|up1,down2', False),
    ((4, 256, 512, 129, 3, 1, 2, 0), 'conv_s2ws_bf16x3_kernel<2>|up1,down2', False),
    ((8, 512, 512, 65, 3, 1, 2, 0), 'conv_bf16x3_kernel<1,4,2,1>|up1,down2', False),      # 128 workgroups of that form: one-role kernel
    ((4, 512, 512, 65, 3, 1, 2, 0), 'conv_bf16x3_kernel<1,4,2,1>|up1,down2', True),
    ((8, 512, 512, 17, 3, 1, 2, 0), 'conv_f32_small_kernel<3,2,1,2>|up1,down2', False),
    ((4, 512, 512, 9, 3, 1, 2, 0), 'conv_f32_small_kernel<3,2,1,2>|up1,down2', False),
    # transposed: small planes on the zero-stuffed small-plane kernel / split over K; H x W main region + edge kernel only with >= 512 main-region workgroups
    ((4, 512, 512, 4, 3, 2, 1, 2), 'conv_f32_small_kernel<3,1,2,1>|up2,down1', False),
    ((8, 512, 512, 4, 3, 2, 1, 2), 'conv_f32_small_kernel<3,1,2,1>|up2,down1', False),
    ((4, 512, 512, 8, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<2,2,2,16>|up2', True),
    ((4, 512, 512, 16, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<2,2,2,32>|up2', True),
    ((4, 512, 512, 32, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<2,2,2,16>|up2', False),
    ((8, 512, 512, 32, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<2,2,2,32>+edge|up2', False),
    ((2, 512, 256, 64, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<2,2,2,16>|up2', False),
    ((4, 512, 256, 64, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<2,2,2,32>+edge|up2', False),
    ((4, 256, 128, 128, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<2,2,2,32>+edge|up2', False),
    ((4, 128, 64, 256, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<2,2,2,16>|up2', False),      # < 256 input channels: bound by its stores, one-kernel form
    ((4, 64, 32, 512, 3, 2, 1, 2), 'convt_fused_bf16x3_kernel<1,4,2,32>|up2', False),
]


@pytest.mark.parametrize('shape,prefix,split', STEP_SHAPES)
def test_step_shapes_reach_their_kernels(shape, prefix, split):
    name, slice_bytes = _probe(*shape)
    assert name.startswith(prefix), (shape, name)
    assert (slice_bytes > 0) == split, (shape, name, slice_bytes)


def test_exact_fp32_mode_takes_the_same_small_plane_kernels():
    for shape in [(4, 512, 512, 8, 3, 1, 1, 1), (4, 512, 512, 4, 3, 2, 1, 2), (8, 512, 512, 17, 3, 1, 2, 0)]:
        assert _probe(*shape, mode='f32')[0] == _probe(*shape)[0], shape
    assert _probe(4, 512, 512, 64, 3, 1, 1, 1, mode='f32')[0].startswith('conv_mfma_kernel')


def test_split_workspace_covers_the_slices():
    """gc_conv2d_bf16x3_workspace >= packed weights + K slices for a split transposed layer; the slices are whole output tensors."""
    b, K, N, h = 4, 512, 512, 8
    o = _out(h, 3, 2, 1, 2)
    desc = _lib.ConvDesc(b, K, N, h, h, o, o, 3, 3, 2, 1, 2, 2)
    lib = _lib.load()
    slices = lib.gc_conv2d_bf16x3_splitk_bytes(desc)
    per_slice = b * N * o * o * 4
    assert slices > 0 and slices % per_slice == 0 and 2 <= slices // per_slice <= K // 64
    assert lib.gc_conv2d_bf16x3_workspace(desc) >= lib.gc_conv2d_bf16x3_packed_bytes(desc) + slices


# ---- weight gradients (gc_conv2d_wgrad_variant_name: the same no-launch probe through the launchers of gc_conv2d_wgrad_* / gc_conv2d_wgrad_samples_*) ----

def _wprobe(b, K, N, h, k, down, pad, samples=False, mode='bf16x3', w=None):
    w = h if w is None else w
    geom = ConvGeom(k, k, 1, down, pad, pad, (h + 2 * pad - k) // down + 1, (w + 2 * pad - k) // down + 1)
    return wgrad_variant(geom, N, b, K, mode, (h, w), samples)


def _kernel(name):
    """A variant name without its split plan: the code that runs."""
    return name.split('|plan:')[0]


# (batch, K, N, plane, taps, down, pad, per-sample form) -> kernel name prefix, split-bf16 arithmetic at B = 4 and B = 8.  In order: the 3x3 stride-1 layers of
# G and D (G's also in the per-sample form its first-order backward takes) and D's 513 -> 512 layer; D's stride-2 3x3 layers with their 1x1 stride-2 skips; the
# transposed layers of G, whose weight gradient is the stride-2 one with the operands swapped; ToRGB at every resolution and FromRGB.  Names derived from the
# built library, then frozen.
STEP_WGRAD_SHAPES = [
    ((4, 512, 512, 4, 3, 1, 1, False), 'wgrad_f32_small_kernel<1,1>|down1,k3'),
    ((8, 512, 512, 4, 3, 1, 1, False), 'wgrad_f32_small_kernel<1,1>|down1,k3'),
    ((4, 512, 512, 4, 3, 1, 1, True), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3|samples'),
    ((8, 512, 512, 4, 3, 1, 1, True), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3|samples'),
    ((4, 512, 512, 8, 3, 1, 1, False), 'wgrad_f32_small_kernel<1,2>|down1,k3'),
    ((8, 512, 512, 8, 3, 1, 1, False), 'wgrad_f32_small_kernel<1,2>|down1,k3'),
    ((4, 512, 512, 8, 3, 1, 1, True), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3|samples'),
    ((8, 512, 512, 8, 3, 1, 1, True), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3|samples'),
    ((4, 512, 512, 16, 3, 1, 1, False), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3'),
    ((8, 512, 512, 16, 3, 1, 1, False), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3'),
    ((4, 512, 512, 16, 3, 1, 1, True), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3|samples'),
    ((8, 512, 512, 16, 3, 1, 1, True), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3|samples'),
    ((4, 512, 512, 32, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((8, 512, 512, 32, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((4, 512, 512, 32, 3, 1, 1, True), 'wgrad_bf16x3_kernel<2,2,1,2,3>|down1,k3|samples'),
    ((8, 512, 512, 32, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((4, 512, 512, 64, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((8, 512, 512, 64, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((4, 512, 512, 64, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((8, 512, 512, 64, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((4, 256, 256, 128, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((8, 256, 256, 128, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((4, 256, 256, 128, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((8, 256, 256, 128, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((4, 128, 128, 256, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((8, 128, 128, 256, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((4, 128, 128, 256, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((8, 128, 128, 256, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((4, 64, 64, 512, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((8, 64, 64, 512, 3, 1, 1, False), 'wgrad_bf16x3_ws2_kernel|down1,k3'),
    ((4, 64, 64, 512, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((8, 64, 64, 512, 3, 1, 1, True), 'wgrad_bf16x3_ws2_kernel|down1,k3|samples'),
    ((4, 32, 32, 1024, 3, 1, 1, False), 'wgrad_bf16x3_kernel<1,1,4,6,3>|down1,k3'),
    ((8, 32, 32, 1024, 3, 1, 1, False), 'wgrad_bf16x3_kernel<1,1,4,6,3>|down1,k3'),
    ((4, 32, 32, 1024, 3, 1, 1, True), 'wgrad_bf16x3_kernel<1,1,4,6,3>|down1,k3|samples'),
    ((8, 32, 32, 1024, 3, 1, 1, True), 'wgrad_bf16x3_kernel<1,1,4,6,3>|down1,k3|samples'),
    ((4, 513, 512, 4, 3, 1, 1, False), 'wgrad_f32_small_kernel<1,1>|down1,k3'),
    ((8, 513, 512, 4, 3, 1, 1, False), 'wgrad_f32_small_kernel<1,1>|down1,k3'),
    ((4, 32, 64, 1025, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<2,3,1>|down2,k3'),
    ((8, 32, 64, 1025, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<2,3,1>|down2,k3'),
    ((4, 32, 64, 1024, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<2,1,1>|down2,k1'),
    ((8, 32, 64, 1024, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<2,1,1>|down2,k1'),
    ((4, 64, 128, 513, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 64, 128, 513, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 64, 128, 512, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((8, 64, 128, 512, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((4, 128, 256, 257, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 128, 256, 257, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 128, 256, 256, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((8, 128, 256, 256, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((4, 256, 512, 129, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 256, 512, 129, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 256, 512, 128, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((8, 256, 512, 128, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((4, 512, 512, 65, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 512, 512, 65, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 512, 512, 64, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((8, 512, 512, 64, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((4, 512, 512, 33, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 512, 512, 33, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 512, 512, 32, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((8, 512, 512, 32, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((4, 512, 512, 17, 3, 2, 0, False), 'wgrad_f32_small_kernel<2,5>|down2,k3'),
    ((8, 512, 512, 17, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 512, 512, 16, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((8, 512, 512, 16, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((4, 512, 512, 9, 3, 2, 0, False), 'wgrad_f32_small_kernel<2,2>|down2,k3'),
    ((8, 512, 512, 9, 3, 2, 0, False), 'wgrad_f32_small_kernel<2,2>|down2,k3'),
    ((4, 512, 512, 8, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((8, 512, 512, 8, 1, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,1,1,4>|down2,k1'),
    ((4, 64, 32, 1025, 3, 2, 0, False), 'wgrad_mfma_kernel<2,1,2,2,2,3>|down2,k3'),
    ((8, 64, 32, 1025, 3, 2, 0, False), 'wgrad_mfma_kernel<2,1,2,2,2,3>|down2,k3'),
    ((4, 128, 64, 513, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,2>|down2,k3'),
    ((8, 128, 64, 513, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,2>|down2,k3'),
    ((4, 128, 64, 513, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,2>|down2,k3|samples'),
    ((8, 128, 64, 513, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,2>|down2,k3|samples'),
    ((4, 256, 128, 257, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 256, 128, 257, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 256, 128, 257, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((8, 256, 128, 257, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((4, 512, 256, 129, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 512, 256, 129, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 512, 256, 129, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((8, 512, 256, 129, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((4, 512, 512, 65, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 512, 512, 65, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 512, 512, 65, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((8, 512, 512, 65, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((4, 512, 512, 33, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((8, 512, 512, 33, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 512, 512, 33, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((8, 512, 512, 33, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((4, 512, 512, 17, 3, 2, 0, False), 'wgrad_f32_small_kernel<2,5>|down2,k3'),
    ((8, 512, 512, 17, 3, 2, 0, False), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3'),
    ((4, 512, 512, 17, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((8, 512, 512, 17, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((4, 512, 512, 9, 3, 2, 0, False), 'wgrad_f32_small_kernel<2,2>|down2,k3'),
    ((8, 512, 512, 9, 3, 2, 0, False), 'wgrad_f32_small_kernel<2,2>|down2,k3'),
    ((4, 512, 512, 9, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((8, 512, 512, 9, 3, 2, 0, True), 'wgrad_bf16x3_s2_kernel<1,3,1,4>|down2,k3|samples'),
    ((4, 512, 3, 4, 1, 1, 0, False), 'wgrad_mfma_kernel<2,1,2,2,1,1>|down1,k1'),
    ((8, 512, 3, 4, 1, 1, 0, False), 'wgrad_mfma_kernel<2,1,2,2,1,1>|down1,k1'),
    ((4, 512, 3, 8, 1, 1, 0, False), 'wgrad_mfma_kernel<2,1,2,2,1,1>|down1,k1'),
    ((8, 512, 3, 8, 1, 1, 0, False), 'wgrad_mfma_kernel<2,1,2,2,1,1>|down1,k1'),
    ((4, 512, 3, 16, 1, 1, 0, False), 'wgrad_mfma_kernel<2,1,2,2,1,1>|down1,k1'),
    ((8, 512, 3, 16, 1, 1, 0, False), 'wgrad_mfma_kernel<2,1,2,2,1,1>|down1,k1'),
    ((4, 512, 3, 32, 1, 1, 0, False), 'wgrad_mfma_kernel<2,1,2,2,1,1>|down1,k1'),
    ((8, 512, 3, 32, 1, 1, 0, False), 'wgrad_mfma_kernel<2,1,2,2,1,1>|down1,k1'),
    ((4, 512, 3, 64, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((8, 512, 3, 64, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((4, 512, 3, 64, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((8, 512, 3, 64, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((4, 256, 3, 128, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((8, 256, 3, 128, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((4, 256, 3, 128, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((8, 256, 3, 128, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((4, 128, 3, 256, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((8, 128, 3, 256, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((4, 128, 3, 256, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((8, 128, 3, 256, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((4, 64, 3, 512, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((8, 64, 3, 512, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((4, 64, 3, 512, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((8, 64, 3, 512, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((4, 32, 3, 1024, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((8, 32, 3, 1024, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_dy|down1,k1'),
    ((4, 32, 3, 1024, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((8, 32, 3, 1024, 1, 1, 0, True), 'pw_wgrad_kernel<true>|thin_dy|down1,k1|samples'),
    ((4, 3, 32, 1024, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_x|down1,k1'),
    ((8, 3, 32, 1024, 1, 1, 0, False), 'pw_wgrad_kernel<true>|thin_x|down1,k1'),
]


@pytest.mark.parametrize('shape,prefix', STEP_WGRAD_SHAPES)
def test_step_wgrad_shapes_reach_their_kernels(shape, prefix):
    name = _wprobe(*shape)
    assert name.startswith(prefix), (shape, name)


def test_wgrad_probe_plans_and_modes():
    """The plan suffix carries what a kernel name alone does not: splits, tiles per split, the band count of the wave-specialised kernel, a direct write."""
    assert _wprobe(4, 512, 512, 64, 3, 1, 1) == 'wgrad_bf16x3_ws2_kernel|down1,k3|plan:splits=4,tiles_per_split=64,bands=4'
    assert _wprobe(8, 512, 512, 32, 3, 1, 1, samples=True) == 'wgrad_bf16x3_ws2_kernel|down1,k3|samples|plan:splits=8,tiles_per_split=16,bands=2'
    assert _wprobe(1, 64, 64, 2, 1, 1, 0, w=8) == 'wgrad_bf16x3_kernel<2,2,1,2,1>|down1,k1|plan:splits=1,tiles_per_split=1,direct'
    assert _wprobe(4, 512, 512, 64, 3, 1, 1, mode='bf16') == _wprobe(4, 512, 512, 64, 3, 1, 1)       # the plain-bf16 build of the same kernels
    assert _wprobe(4, 512, 512, 64, 3, 1, 1, mode='f32').startswith('wgrad_mfma_kernel<2,2,1,1,1,3>|down1,k3|plan:splits=')
    assert _wprobe(4, 512, 512, 8, 3, 1, 1, mode='f32') == _wprobe(4, 512, 512, 8, 3, 1, 1) == 'wgrad_f32_small_kernel<1,2>|down1,k3|plan:groups=1,direct'
    with pytest.raises(RuntimeError):            # fp32 arithmetic has a per-sample form for the thin 1x1 shapes only
        _wprobe(4, 512, 512, 64, 3, 1, 1, samples=True, mode='f32')


def test_every_step_wgrad_variant_has_a_kernel_case():
    """Every weight-gradient kernel the step launches is also compared with fp64 on its own, at kernel level (tests/test_ops_gpu.py)."""
    import test_ops_gpu as ops
    step = {_kernel(_wprobe(*shape)) for shape, _ in STEP_WGRAD_SHAPES}
    cases = set()
    for (b, K, N, h, w, k, down, pad, _), fast, _ in ops.WGRAD_VARIANT_CASES:
        name = _kernel(_wprobe(b, K, N, h, k, down, pad, w=w))
        assert name == _kernel(fast), 'the case list pins the name it reaches'
        cases.add(name)
    for b, K, N, h, w, k, down, pad, _, variant in ops.SAMPLE_WGRAD_CASES:
        name = _kernel(_wprobe(b, K, N, h, k, down, pad, samples=True, w=w))
        assert name == _kernel(variant)
        cases.add(name)
    assert step <= cases, sorted(step - cases)


def test_every_step_conv_variant_has_a_kernel_case():
    """... and so is every forward kernel of STEP_SHAPES by a case of BF16_CASES."""
    import test_ops_gpu as ops
    step = {_probe(*shape)[0] for shape, _, _ in STEP_SHAPES}
    cases = set()
    for b, K, N, h, w, k, up, down, pad in ops.BF16_CASES:
        oh, ow = _out(h, k, up, down, pad), _out(w, k, up, down, pad)
        cases.add(conv_variant(ConvGeom(k, k, up, down, pad, pad, oh, ow), N, b, K, 'bf16x3', (h, w)))
    assert step <= cases, sorted(step - cases)


_MODE_IDS = {'f32': 0, 'bf16x3': 1, 'bf16': 2}


def _frozen_names(column):
    """The kernel names (split plan stripped) of one probe column of tests/golden/dispatch_table.json over all its geometry groups; rc* cells (no kernel) skipped."""
    import json
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import dispatch_table
    with open(dispatch_table.GOLDEN) as f:
        frozen = json.load(f)
    return {n for group, g in frozen.items() if group.split('|', 1)[1] == column for n in g.get('names', {}) if not n.startswith('rc')}


def _conv_name(case, mode):
    b, K, N, h, w, k, up, down, pad = case
    return _kernel(conv_variant(ConvGeom(k, k, up, down, pad, pad, _out(h, k, up, down, pad), _out(w, k, up, down, pad)), N, b, K, mode, (h, w)))


@pytest.mark.parametrize('mode', ['f32', 'bf16x3', 'bf16'])
def test_every_frozen_variant_has_a_kernel_case(mode):
    """Every kernel variant of the frozen decision table is compared with fp64 at kernel level (tests/test_ops_gpu.py) in each arithmetic: the forward
    variants by the forward lists (test_conv2d_kernel, test_conv2d_bf16x3_kernel, test_conv2d_bf16_kernel, test_conv2d_variants) and again by the fused
    epilogue's, the weight-gradient variants by WGRAD_VARIANT_CASES, the per-sample ones by SAMPLE_WGRAD_CASES.  test_dispatch_table_matches_the_frozen_digest
    ties the table to the built library, so a new variant cannot ship without a case."""
    import test_ops_gpu as ops
    forward = {'f32': ops.CONV_CASES + ops.SMALL_CASES, 'bf16x3': ops.BF16_CASES, 'bf16': ops.BF16_CASES[::3]}[mode] + [c[0] for c in ops.CONV_VARIANT_CASES]
    conv = _frozen_names('conv_variant[mode=%d]' % _MODE_IDS[mode])
    wgrad = {_kernel(_wprobe(b, K, N, h, k, down, pad, mode=mode, w=w)) for (b, K, N, h, w, k, down, pad, _), _, _ in ops.WGRAD_VARIANT_CASES}
    samples = set()
    for b, K, N, h, w, k, down, pad, _, _ in ops.SAMPLE_WGRAD_CASES:
        try:
            samples.add(_kernel(_wprobe(b, K, N, h, k, down, pad, samples=True, mode=mode, w=w)))
        except RuntimeError:
            assert mode == 'f32', 'the split-bf16 arithmetics have a per-sample form for every shape of the list'
    missing = {
        'forward lists': conv - {_conv_name(c, mode) for c in forward},
        'EPILOGUE_CASES': conv - {_conv_name(c, mode) for c in ops.EPILOGUE_CASES},
        'WGRAD_VARIANT_CASES': _frozen_names('wgrad_variant[mode=%d,samples=0]' % _MODE_IDS[mode]) - wgrad,
        'SAMPLE_WGRAD_CASES': _frozen_names('wgrad_variant[mode=%d,samples=1]' % _MODE_IDS[mode]) - samples,
    }
    assert not any(missing.values()), 'variants of the frozen table no %s case reaches: %s' % (mode, {k: sorted(v) for k, v in missing.items() if v})


@pytest.mark.parametrize('out_h,out_w,prefix', [(40, 33, 'conv_bf16x3_kernel<1,4,2,1>|up1,down2'), (33, 33, 'conv_s2ws_bf16x3_kernel<1>'),
                                                (33, 40, 'conv_bf16x3_kernel<1,4,2,1>|up1,down2')])
def test_unmasked_stride2_kernel_takes_only_outputs_that_read_inside_the_plane(out_h, out_w, prefix):
    """conv_s2ws_bf16x3_kernel masks nothing: a descriptor whose output extent exceeds (in - 3) / 2 + 1 on either axis (legal: those pixels read zeros) stays
    on the masked one-role kernel.  67 x 67 -> 33 x 33 is the consistent geometry; 20 samples reach the kernel's 192-workgroup threshold."""
    geom = ConvGeom(3, 3, 1, 2, 0, 0, out_h, out_w)
    assert conv_variant(geom, 64, 20, 32, 'bf16x3', (67, 67)).startswith(prefix)


# ---- upfirdn2d (gc_upfirdn2d_variant_name: the plan the FIR launcher follows; HipBackend routes and times by the same answer) ----

def _fir_probe(planes, out_h, out_w, k, up, down):
    import ctypes
    buf = ctypes.create_string_buffer(128)
    rc = _lib.load().gc_upfirdn2d_variant_name(planes, out_h, out_w, k, k, up, down, buf, 128)
    return buf.value.decode() if rc == 0 else rc


# (planes, out_h, out_w, taps, up, down) -> kernel, FFHQ-1024 step at B = 4
STEP_FIR_SHAPES = [
    # the Blur behind a transposed convolution of G (and its adjoint): the tile kernel from 64 x 64 up, whole planes in LDS below
    ((4 * 32, 1024, 1024, 4, 1, 1), 'fir44_tile_kernel'),
    ((4 * 64, 512, 512, 4, 1, 1), 'fir44_tile_kernel'),
    ((4 * 512, 64, 64, 4, 1, 1), 'fir44_tile_kernel'),
    ((4 * 512, 32, 32, 4, 1, 1), 'fir44_small_kernel'),
    ((4 * 512, 8, 8, 4, 1, 1), 'fir44_small_kernel'),
    # the Blur in front of a stride-2 convolution of D, (H + 1) wide, and its adjoint, (H + 3) wide
    ((4 * 32, 1025, 1025, 4, 1, 1), 'fir44_tile_kernel'),
    ((4 * 512, 65, 65, 4, 1, 1), 'fir44_tile_kernel'),
    ((4 * 512, 33, 33, 4, 1, 1), 'fir44_small_kernel'),
    ((4 * 512, 35, 35, 4, 1, 1), 'upfirdn2d_generic_kernel'),      # the adjoint at 32 x 32: too large for LDS, too low for a tile
    ((4 * 512, 5, 5, 4, 1, 1), 'fir44_small_kernel'),
    # Upsample of the RGB skip (3 channels) and its adjoint
    ((4 * 3, 1024, 1024, 4, 2, 1), 'fir44_up2_kernel'),
    ((4 * 3, 32, 32, 4, 2, 1), 'fir44_up2_kernel'),
    ((4 * 3, 16, 16, 4, 2, 1), 'upfirdn2d_generic_kernel'),
    ((4 * 3, 512, 512, 4, 1, 2), 'fir44_down2_kernel'),
    # the decimating FIR of D's ResBlock skip path and its adjoint
    ((4 * 32, 512, 512, 4, 1, 2), 'fir44_down2_kernel'),
    ((4 * 512, 32, 32, 4, 1, 2), 'fir44_down2_kernel'),
    ((4 * 512, 16, 16, 4, 1, 2), 'upfirdn2d_generic_kernel'),
    ((4 * 32, 1024, 1024, 4, 2, 1), 'fir44_up2_kernel'),
    # ADA: 12 x 12 sym6 taps, 1036 -> 2061 up, 2061 -> 1025 down, and the adjoint of the first
    ((4 * 3, 2061, 2061, 12, 2, 1), 'firK_tile_kernel<12>'),
    ((4 * 3, 1025, 1025, 12, 1, 2), 'firK_tile_kernel<12>'),
    ((4 * 3, 1036, 1036, 12, 1, 2), 'firK_tile_kernel<12>'),
]


@pytest.mark.parametrize('shape,kernel', STEP_FIR_SHAPES)
def test_step_fir_shapes_reach_their_kernels(shape, kernel):
    assert _fir_probe(*shape) == kernel, shape


def test_fir_probe_refuses_what_no_kernel_takes():
    assert _fir_probe(1, 16, 64, 33, 1, 1) == -2          # 1089 taps: more than the generic kernel's 1024
    assert _fir_probe(1, 16, 64, 32, 1, 1) == 'upfirdn2d_generic_kernel'
    assert _fir_probe(1, 0, 64, 4, 1, 1) == -1 and _fir_probe(-1, 16, 64, 4, 1, 1) == -1 and _fir_probe(1, 16, 64, 4, 0, 1) == -1


# ---- the whole decision table (tools/dispatch_table.py): every probe and every size / pitch query over a fixed descriptor grid, frozen as a digest ----

def test_dispatch_table_matches_the_frozen_digest():
    """Host-side dispatch work must not move a decision: the digest of the table equals tests/golden/dispatch_table.json.  A deliberate change regenerates
    the file (`python tools/dispatch_table.py --write`) and says in its commit which rows moved."""
    import json
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import dispatch_table
    with open(dispatch_table.GOLDEN) as f:
        frozen = json.load(f)
    now = dispatch_table.digest()
    moved = sorted(g for g in set(frozen) | set(now) if frozen.get(g) != now.get(g))
    assert not moved, ('these (geometry | column) groups of the decision table moved: %s -- run `python tools/dispatch_table.py --dump` on the parent build and '
                       'on this one and diff the two outputs to see the rows' % moved)
