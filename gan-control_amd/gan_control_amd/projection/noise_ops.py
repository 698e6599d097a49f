"""noise_regularize and noise_normalize_ of image projection (reference: projection/projection.py:126-154) over a whole list of noise maps.

A list of CUDA maps takes the HIP path (csrc/noise_reg.hip): ONE call of gc_noise_reg_fwd_f32 (three kernel launches: the 2 x 2-mean pyramids
of every map, the wrapped products per chunk, the fixed-order finish), ONE call of gc_noise_reg_bwd_f32 for the gradient of every map (a
gather from the stored pyramids; the upstream cotangent is read on the device) and ONE call of gc_noise_normalize_f32 (three launches) --
whatever the length of the list and the depth of the pyramids, where the reference's loops make ~900 ATen launches each way for the 17 maps of
the 1024^2 generator.  A shape the kernels do not take raises ValueError naming it; there is no fallback.

A list of CPU maps takes ``noise_regularize_reference`` / ``noise_normalize_reference_``: plain torch ops written from the formulas.  They are
the documented semantics, the oracle of the tests and the path under an emulated backend.
"""
import ctypes

import torch          # every device allocation below goes through this name (torch.empty): tests swap it for a guard-banded allocator
import torch.nn.functional as F
from torch.autograd import Function

from .. import _lib
from ..models.op import _backend
from ..models.op._backend import HipBackend          # noqa: F401  (the launch path of this module: _backend.get()._launch)

REG_FWD, REG_BWD, NORMALIZE = 'gc_noise_reg_fwd_f32', 'gc_noise_reg_bwd_f32', 'gc_noise_normalize_f32'
MAX_MAPS, MAX_SIZE = 32, 1024


def noise_regularize_reference(noises):
    """sum over maps and pyramid levels of mean(n * roll(n, 1, x))^2 + mean(n * roll(n, 1, y))^2; the means run over the whole tensor (batch
    included); the next level is the 2 x 2 mean; the loop computes the terms, stops if size <= 8 and halves otherwise."""
    loss = 0
    for n in noises:
        while True:
            loss = loss + (n * torch.roll(n, 1, 3)).mean().pow(2) + (n * torch.roll(n, 1, 2)).mean().pow(2)
            if n.shape[2] <= 8:
                break
            n = F.avg_pool2d(n, 2)
    return loss


def noise_normalize_reference_(noises):
    """Every map becomes (n - mean) / std in place, mean and the unbiased standard deviation over the whole tensor."""
    with torch.no_grad():
        for n in noises:
            mean, std = n.mean(), n.std()
            n.data.sub_(mean).div_(std)


def _hip_backend():
    hip = _backend.get()
    if getattr(hip, 'name', None) != 'hip':
        raise RuntimeError('gan_control_amd: the projection kernels run on the HIP backend only (active: %r); there is no fallback' % getattr(hip, 'name', hip))
    return hip


def _check_list(noises, what):
    noises = list(noises)
    if not noises or not all(torch.is_tensor(n) for n in noises):
        raise ValueError('%s: a non-empty list of tensors is expected' % what)
    if len({n.is_cuda for n in noises}) != 1 or len({n.device for n in noises}) != 1:
        raise ValueError('%s: the maps are on different devices: %s' % (what, sorted({str(n.device) for n in noises})))
    return noises


def _check_device_maps(noises, what, square):
    if len(noises) > MAX_MAPS:
        raise ValueError('%s: %d maps; the kernels take at most %d' % (what, len(noises), MAX_MAPS))
    for i, n in enumerate(noises):
        if n.dtype != torch.float32:
            raise ValueError('%s: map %d is %s; the kernels take float32' % (what, i, n.dtype))
        if square:
            s = n.shape[-1] if n.dim() == 4 else 0
            if n.dim() != 4 or n.shape[1] != 1 or n.shape[2] != s or s < 4 or s > MAX_SIZE or s & (s - 1) or n.shape[0] < 1:
                raise ValueError('%s: map %d has shape %s; the kernels take [B, 1, S, S] with S a power of two in [4, %d]' % (what, i, tuple(n.shape), MAX_SIZE))
        elif n.numel() < 2:
            raise ValueError('%s: map %d has shape %s; a standard deviation needs two elements' % (what, i, tuple(n.shape)))


class _Tables:
    """The host-side argument arrays of one list (pointers, extents, workspace size): the same tensors come back every step."""
    __slots__ = ('ptrs', 'sizes', 'batches', 'counts', 'reg_bytes', 'norm_bytes')


_tables = {}


def _tables_of(maps, square):
    key = (square,) + tuple((m.data_ptr(), tuple(m.shape)) for m in maps)
    t = _tables.get(key)
    if t is None:
        if len(_tables) > 64:
            _tables.clear()
        n, lib = len(maps), _lib.load()
        t = _tables[key] = _Tables()
        t.ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps])
        t.reg_bytes = t.norm_bytes = 0
        if square:
            t.sizes = (ctypes.c_int32 * n)(*[m.shape[-1] for m in maps])
            t.batches = (ctypes.c_int32 * n)(*[m.shape[0] for m in maps])
            t.reg_bytes = lib.gc_noise_reg_workspace(t.sizes, t.batches, n)
        else:
            t.counts = (ctypes.c_int64 * n)(*[m.numel() for m in maps])
            t.norm_bytes = lib.gc_noise_normalize_workspace(t.counts, n)
    return t


class _NoiseRegularize(Function):
    @staticmethod
    def forward(ctx, *noises):
        hip = _hip_backend()
        maps = [n.contiguous() for n in noises]
        dev = maps[0].device
        t = _tables_of(maps, True)
        ws = torch.empty(max(t.reg_bytes // 4, 1), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        hip._launch(dev, REG_FWD, t.ptrs, t.sizes, t.batches, len(maps), _lib.ptr(loss), _lib.ptr(ws), t.reg_bytes, _lib.stream_of(maps[0]))
        ctx.save_for_backward(ws, *maps)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        if torch.is_grad_enabled():
            raise RuntimeError('gan_control_amd: noise_regularize on the HIP path is differentiable once')
        ws, *maps = ctx.saved_tensors
        hip = _hip_backend()
        dev = maps[0].device
        t = _tables_of(maps, True)
        grads = [torch.empty(tuple(m.shape), dtype=torch.float32, device=dev) for m in maps]
        gptrs = (ctypes.c_void_p * len(maps))(*[g.data_ptr() for g in grads])
        gout = gout.to(torch.float32).reshape(1).contiguous()
        hip._launch(dev, REG_BWD, t.ptrs, t.sizes, t.batches, len(maps), _lib.ptr(gout), gptrs, _lib.ptr(ws), t.reg_bytes, _lib.stream_of(maps[0]))
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad))


def noise_regularize(noises):
    """The reference's noise_regularize (projection.py:126-146): a 0-dim tensor, differentiable with respect to every map.  The caller
    multiplies it by its weight (1e5 in the reference's use)."""
    noises = _check_list(noises, 'noise_regularize')
    if not noises[0].is_cuda:
        return noise_regularize_reference(noises)
    _check_device_maps(noises, 'noise_regularize', True)
    return _NoiseRegularize.apply(*noises)


def noise_normalize_(noises):
    """The reference's noise_normalize_ (projection.py:149-154): every map to mean 0 and (unbiased) standard deviation 1, in place."""
    noises = _check_list(noises, 'noise_normalize_')
    if not noises[0].is_cuda:
        return noise_normalize_reference_(noises)
    _check_device_maps(noises, 'noise_normalize_', False)
    hip = _hip_backend()
    maps = [n.data for n in noises]
    for i, m in enumerate(maps):
        if not m.is_contiguous():
            raise ValueError('noise_normalize_: map %d of shape %s is not contiguous; it cannot be normalised in place' % (i, tuple(m.shape)))
    dev = maps[0].device
    t = _tables_of(maps, False)
    ws = torch.empty(max(t.norm_bytes // 4, 1), dtype=torch.float32, device=dev)
    hip._launch(dev, NORMALIZE, t.ptrs, t.counts, len(maps), _lib.ptr(ws), t.norm_bytes, _lib.stream_of(maps[0]))
