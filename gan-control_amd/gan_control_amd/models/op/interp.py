"""The blends of group interpolation (Inference.interpolate_by_group; reference: evaluation/inference_class.py:125-185).

``interpolate_latents(fixed, z_from, z_to, lo, hi, wa, wb, interpolation)`` returns the z of EVERY frame of one interpolation segment, for both
films, as ``[2, P, B, L]``: with S = [0, lo), G = [lo, hi) (the group) and E = [hi, L),

    out[0, f] = [ blend_f(z_from, z_to) on S | fixed on G | blend_f(z_from, z_to) on E ]          the group is frozen
    out[1, f] = [ fixed on S | blend_f(z_from, z_to) on G | fixed on E ]                          only the group moves

``blend_f(x, y) = wa[f] * x + wb[f] * y`` for ``'linear'`` and for the reference's third branch (any other name: the weights are square
roots, see ``interpolation_weights``); for ``'slerp'`` it is the reference's ``slerp`` (inference_class.py:197-203) applied to each slice on its
own with ``sin(wa[f] * omega) / sin(omega)`` and ``sin(wb[f] * omega) / sin(omega)`` as the coefficients.  Nothing is clamped: parallel slices
are as undefined as in the reference.  ``blend_noise(a, b, wa, wb, out=None)`` is ``wa * a[m] + wb * b[m]`` over a list of equal-shaped maps.

The dispatch rule.  CUDA tensors under the HIP backend with no gradient wanted take the kernels of csrc/interp.hip: ONE
``gc_latent_interp_f32`` call per segment (the weights travel in the kernel arguments; linear and sqrt blends are bit for bit the torch
expression, the slerp coefficients are computed in float64 from float64 row sums) and ONE ``gc_noise_blend_f32`` call per list.  A device
shape the kernels do not take raises ``ValueError`` naming it -- a dtype other than float32, more than 64 frames, rows whose elements are not
adjacent, more than 32 maps, maps that are not dense, an output that overlaps an input -- there is no fallback.  No size threshold: neither
kernel is slower than the torch expressions at any shape measured (profiles/interpolation.md).  CPU tensors, the emulated backend of the tests
and a wanted gradient take ``interpolate_latents_reference`` / ``blend_noise_reference``: the torch formulas, which are the documented
semantics and the oracle of the tests.
"""
import ctypes

import numpy as np
import torch          # every device allocation below goes through this name: tests swap it for a guard-banded allocator

from ... import _lib
from . import _backend
# part of this module's interface: the guard-banded allocator of the tests (guarded(module)) reaches the launch path as module.HipBackend._launch
from ._backend import HipBackend          # noqa: F401

LATENT_ENTRY = 'gc_latent_interp_f32'
NOISE_ENTRY = 'gc_noise_blend_f32'
MODES = {'linear': 0, 'slerp': 1}          # GC_INTERP_LINEAR / GC_INTERP_SLERP; every other name: GC_INTERP_SQRT (include/gancontrol_hip.h)
MODE_SQRT = 2
MAX_FRAMES, MAX_MAPS = 64, 32


def interpolation_weights(pics, interpolation):
    """(wa, wb): the float32 weights of the ``pics`` frames of a segment.  p = linspace(0, 1, pics) in float64; ``'linear'`` and ``'slerp'``:
    1 - p and p; anything else (the reference's third branch): sqrt(1 - p) and sqrt(p).  Rounded to float32 LAST: torch rounds a Python
    scalar to the tensor's dtype, so ``(1 - p) * x`` is ``float32(1 - p) * x`` bit for bit."""
    p = np.linspace(0, 1, int(pics))
    if interpolation in MODES:
        wa, wb = 1 - p, p
    else:
        wa, wb = np.sqrt(1 - p), np.sqrt(p)
    return wa.astype(np.float32), wb.astype(np.float32)


def _slerp(wa, wb, low, high):
    """Inference.slerp with the two weights given: the reference's ``1.0 - val`` and ``val``."""
    low_norm = low / torch.norm(low, dim=1, keepdim=True)
    high_norm = high / torch.norm(high, dim=1, keepdim=True)
    omega = torch.acos((low_norm * high_norm).sum(1))
    so = torch.sin(omega)
    return (torch.sin(wa * omega) / so).unsqueeze(1) * low + (torch.sin(wb * omega) / so).unsqueeze(1) * high


def _check_latents(fixed, z_from, z_to, lo, hi, wa, wb):
    for t in (fixed, z_from, z_to):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape != fixed.shape or t.shape[0] < 1:
            raise ValueError('interpolate_latents: three [B, L] tensors of one shape expected, got %s'
                             % [tuple(t.shape) if torch.is_tensor(t) else type(t).__name__ for t in (fixed, z_from, z_to)])
    lo, hi = int(lo), int(hi)
    if not 0 <= lo < hi <= fixed.shape[1]:
        raise ValueError('interpolate_latents: group [%d, %d) of a latent of %d: 0 <= lo < hi <= L' % (lo, hi, fixed.shape[1]))
    wa, wb = np.ascontiguousarray(wa, dtype=np.float32).reshape(-1), np.ascontiguousarray(wb, dtype=np.float32).reshape(-1)
    if wa.shape[0] < 1 or wa.shape != wb.shape:
        raise ValueError('interpolate_latents: %d and %d weights: one pair per frame, at least one frame' % (wa.shape[0], wb.shape[0]))
    return lo, hi, wa, wb


def interpolate_latents_reference(fixed, z_from, z_to, lo, hi, wa, wb, interpolation):
    """The torch formula (reference lines 153-169 per frame: slice, blend, ``torch.cat``) -> [2, P, B, L]."""
    lo, hi, wa, wb = _check_latents(fixed, z_from, z_to, lo, hi, wa, wb)
    frozen, moving = [], []
    for a, b in zip(wa.tolist(), wb.tolist()):
        if interpolation == 'slerp':
            start = _slerp(a, b, z_from[:, :lo], z_to[:, :lo])
            end = _slerp(a, b, z_from[:, hi:], z_to[:, hi:])
            group = _slerp(a, b, z_from[:, lo:hi], z_to[:, lo:hi])
        else:
            start = a * z_from[:, :lo] + b * z_to[:, :lo]
            end = a * z_from[:, hi:] + b * z_to[:, hi:]
            group = a * z_from[:, lo:hi] + b * z_to[:, lo:hi]
        frozen.append(torch.cat([start, fixed[:, lo:hi], end], dim=1))
        moving.append(torch.cat([fixed[:, :lo], group, fixed[:, hi:]], dim=1))
    return torch.stack([torch.stack(frozen, 0), torch.stack(moving, 0)], 0)


def _device_path(tensors):
    """Whether these tensors belong to the kernels: all on one CUDA device under the HIP backend, and no gradient wanted."""
    if getattr(_backend.get(), 'name', None) != 'hip' or not all(t.is_cuda and t.device == tensors[0].device for t in tensors):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


def _row_stride(t, what):
    """The row stride (elements) the kernel reads ``t`` [B, L] with: 0 for an expanded row, else at least L."""
    b, width = t.shape
    if width > 1 and t.stride(1) != 1:
        raise ValueError('interpolate_latents: %s has strides %s; the kernel reads rows of adjacent elements' % (what, tuple(t.stride())))
    stride = t.stride(0) if b > 1 else width          # (a single row may report any stride, and none is used)
    if stride != 0 and stride < width:
        raise ValueError('interpolate_latents: %s has row stride %d, shorter than its rows (%d)' % (what, stride, width))
    return stride


def interpolate_latents(fixed, z_from, z_to, lo, hi, wa, wb, interpolation):
    """[2, P, B, L] (module docstring).  ``fixed``, ``z_from``, ``z_to``: [B, L]; an expanded single row (row stride 0) is read in place."""
    lo, hi, wa, wb = _check_latents(fixed, z_from, z_to, lo, hi, wa, wb)
    tensors = (fixed, z_from, z_to)
    if not _device_path(tensors):
        return interpolate_latents_reference(fixed, z_from, z_to, lo, hi, wa, wb, interpolation)
    for t, what in zip(tensors, ('fixed', 'z_from', 'z_to')):
        if t.dtype != torch.float32:
            raise ValueError('interpolate_latents: %s is %s; the kernel takes float32' % (what, t.dtype))
    frames = wa.shape[0]
    if frames > MAX_FRAMES:
        raise ValueError('interpolate_latents: %d frames; the kernel takes at most %d per call' % (frames, MAX_FRAMES))
    strides = [_row_stride(t, what) for t, what in zip(tensors, ('fixed', 'z_from', 'z_to'))]
    batch, latent = fixed.shape
    dev = fixed.device
    out = torch.empty((2, frames, batch, latent), dtype=torch.float32, device=dev)
    _backend.get()._launch(dev, LATENT_ENTRY, _lib.ptr(fixed), strides[0], _lib.ptr(z_from), strides[1], _lib.ptr(z_to), strides[2], batch, latent,
                           lo, hi, wa.ctypes.data, wb.ctypes.data, frames, MODES.get(interpolation, MODE_SQRT), _lib.ptr(out), _lib.stream_of(out))
    return out


def _check_maps(a, b, what):
    a, b = list(a), list(b)
    if not a or len(a) != len(b) or not all(torch.is_tensor(t) for t in a + b):
        raise ValueError('%s: two non-empty lists of tensors of one length expected' % what)
    for m, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape or x.numel() < 1:
            raise ValueError('%s: map %d has shapes %s and %s; equal shapes of at least one element expected' % (what, m, tuple(x.shape), tuple(y.shape)))
    return a, b


def blend_noise_reference(a, b, wa, wb):
    """[wa * a[m] + wb * b[m]]: the reference's ``(1 - p) * noise1[i] + p * noise2[i]`` (inference_class.py:154) with the weights given."""
    a, b = _check_maps(a, b, 'blend_noise')
    wa, wb = float(wa), float(wb)
    return [wa * x + wb * y for x, y in zip(a, b)]


class _Table:
    """The host-side argument arrays of one (a, b, out) triple of lists: a caller blends the same lists frame after frame."""
    __slots__ = ('a', 'b', 'out', 'counts')


_tables = {}


def _overlaps(p, pn, q, qn):
    return p < q + 4 * qn and q < p + 4 * pn


def _table_of(a, b, out):
    key = tuple((x.data_ptr(), y.data_ptr(), o.data_ptr(), o.numel()) for x, y, o in zip(a, b, out))
    t = _tables.get(key)
    if t is None:
        n = len(out)
        for m in range(n):
            for k in range(n):
                if (_overlaps(key[m][2], key[m][3], key[k][0], key[k][3]) or _overlaps(key[m][2], key[m][3], key[k][1], key[k][3])
                        or (k != m and _overlaps(key[m][2], key[m][3], key[k][2], key[k][3]))):
                    raise ValueError('blend_noise: out[%d] overlaps map %d of the inputs or of out; the kernel does not blend in place' % (m, k))
        if len(_tables) > 64:
            _tables.clear()
        t = _tables[key] = _Table()
        t.a = (ctypes.c_void_p * n)(*[k[0] for k in key])
        t.b = (ctypes.c_void_p * n)(*[k[1] for k in key])
        t.out = (ctypes.c_void_p * n)(*[k[2] for k in key])
        t.counts = (ctypes.c_int64 * n)(*[k[3] for k in key])
    return t


def blend_noise(a, b, wa, wb, out=None):
    """``out[m] = wa * a[m] + wb * b[m]`` over two lists of equal-shaped maps; ``a is b`` is fine (the reference evaluates the blend of a map
    with itself too, which is not the map bit for bit).  ``out``: a list of tensors like ``a`` to write into, which a caller reuses across
    frames; it is returned.  On the device path: one launch for the whole list."""
    a, b = _check_maps(a, b, 'blend_noise')
    if out is not None:
        out = list(out)
        if len(out) != len(a) or any(not torch.is_tensor(o) or o.shape != x.shape or o.dtype != x.dtype or o.device != x.device for o, x in zip(out, a)):
            raise ValueError('blend_noise: out must be a list of %d tensors with the shapes, dtype and device of the inputs' % len(a))
    if not _device_path(a + b):
        res = blend_noise_reference(a, b, wa, wb)
        if out is None:
            return res
        for o, r in zip(out, res):
            o.copy_(r)
        return out
    if len(a) > MAX_MAPS:
        raise ValueError('blend_noise: %d maps; the kernel takes at most %d per call' % (len(a), MAX_MAPS))
    for m, (x, y) in enumerate(zip(a, b)):
        for t in (x, y):
            if t.dtype != torch.float32:
                raise ValueError('blend_noise: map %d is %s; the kernel takes float32' % (m, t.dtype))
            if not t.is_contiguous():
                raise ValueError('blend_noise: map %d of shape %s has strides %s; the kernel takes dense maps' % (m, tuple(t.shape), tuple(t.stride())))
    dev = a[0].device
    if out is None:
        out = [torch.empty(tuple(x.shape), dtype=torch.float32, device=dev) for x in a]
    elif any(not o.is_contiguous() for o in out):
        raise ValueError('blend_noise: out must be dense maps')
    t = _table_of(a, b, out)
    _backend.get()._launch(dev, NOISE_ENTRY, t.a, t.b, t.out, t.counts, len(a), float(wa), float(wb), _lib.stream_of(a[0]))
    return out
