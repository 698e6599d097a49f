"""The gradient of a fused (noise +) bias + leaky-ReLU layer with respect to its NOISE MAP, on gc_bias_act_bwd_noise_f32.

Every StyledConv injects its noise inside a fused kernel (modulated_conv._ModConvAct, upfirdn2d._UpFirDn2dAct).  Training never asks for
d/d(noise); image projection does: it optimises the noise maps.  The quantity is ``noise_w * sum_c g_pre[b, c, h, w]`` with ``g_pre`` the
gradient at the pre-activation, and it is taken in the pass that makes ``g_pre`` (``masked``), or from a ``g_pre`` that the reduce pass has made
already because bias / noise-strength gradients are wanted too (``pixel_sums``).

The launches go through ``_backend.get()._launch``; on a backend that is not the HIP one (the emulation the tests install) the same quantity is
computed with the torch expression of fused_act._BiasAct.backward.
"""
import torch          # every device allocation below goes through this name (torch.empty): tests swap it for a guard-banded allocator
from torch.autograd import Function

from ... import _lib
from . import _backend
from ._backend import HipBackend          # noqa: F401  (the launch path of this module: _backend.get()._launch)

ENTRY = 'gc_bias_act_bwd_noise_f32'


def _extents(t):
    b, c = t.shape[0], t.shape[1]
    return b, c, t.numel() // max(b * c, 1)


def masked(gy, y_ref, noise_w, slope, gain):
    """(g_pre, gnoise): g_pre = gy * (y_ref > 0 ? gain : gain * slope) -- the bits of bias_act_bwd -- and gnoise [B, 1, *] = noise_w * sum_c g_pre,
    from one read of gy and y_ref."""
    be = _backend.get()
    if getattr(be, 'name', None) != 'hip':
        g_pre = be.bias_act_bwd(gy, y_ref, slope, gain)
        return g_pre, g_pre.sum(1, keepdim=True) * noise_w
    gy, y_ref = gy.contiguous(), y_ref.contiguous()
    dev = _lib.require_cuda_f32(gy, y_ref, noise_w)
    b, c, inner = _extents(gy)
    g_pre = torch.empty(tuple(gy.shape), dtype=torch.float32, device=dev)
    gn = torch.empty((b, 1) + tuple(gy.shape[2:]), dtype=torch.float32, device=dev)
    if gy.numel():
        be._launch(dev, ENTRY, _lib.ptr(gy), _lib.ptr(y_ref), _lib.ptr(noise_w), _lib.ptr(g_pre), _lib.ptr(gn), b, c, inner,
                   float(slope), float(gain), _lib.stream_of(gy))
    return g_pre, gn


def pixel_sums(g_pre, noise_w):
    """gnoise [B, 1, *] = noise_w * sum_c g_pre[b, c, *] of a pre-activation gradient that exists already."""
    be = _backend.get()
    if getattr(be, 'name', None) != 'hip':
        return g_pre.sum(1, keepdim=True) * noise_w
    g_pre = g_pre.contiguous()
    dev = _lib.require_cuda_f32(g_pre, noise_w)
    b, c, inner = _extents(g_pre)
    gn = torch.empty((b, 1) + tuple(g_pre.shape[2:]), dtype=torch.float32, device=dev)
    if g_pre.numel():
        be._launch(dev, ENTRY, _lib.ptr(g_pre), None, _lib.ptr(noise_w), None, _lib.ptr(gn), b, c, inner, 1.0, 1.0, _lib.stream_of(g_pre))
    return gn


class _PixelSumsOnce(Function):
    """pixel_sums inside a backward pass that is itself recorded (create_graph=True): g_pre stays differentiable for everybody else, the
    noise-map gradient is a first derivative only."""

    @staticmethod
    def forward(ctx, g_pre, noise_w):
        return pixel_sums(g_pre, noise_w)

    @staticmethod
    def backward(ctx, gg):
        raise RuntimeError('gan_control_amd: the noise-map gradient of a fused StyledConv layer cannot be differentiated again '
                           '(image projection takes first derivatives of the noise maps only)')


def pixel_sums_once(g_pre, noise_w):
    return _backend.call(_PixelSumsOnce, g_pre, noise_w)
