"""Decoded images to a training batch, on the device: uint8 [B, H, W, 3] -> float32 [B, 3, size, size] in [-1, 1].

The reference does this on the host, per image, in DataLoader workers (ffhq_dataset.py:56-64, afhq_dataset.py:50-59, metfaces_dataset.py:48-57):
``transforms.Resize`` / ``RandomResizedCrop`` on the PIL image, ``RandomHorizontalFlip``, ``ToTensor``, ``Normalize(0.5, 0.5)``.  Here the three
entries of csrc/image_input.hip do it with the same bits:

* the resize is PIL's 8-bit bilinear resample -- per axis a table of fixed-point coefficients (``resample_tables``, built on the host in
  doubles), a horizontal pass, a uint8 intermediate, a vertical pass; a pass runs only where the extent changes.  A crop only offsets the reads:
  the taps are clamped at the crop's edges, as ``crop`` followed by ``resize`` clamps them;
* ``ToTensor`` + ``Normalize`` is a 256-entry table (``normalize_table``) filled once by the reference's own float32 operation sequence
  ``v.float().div(255).sub(0.5).div(0.5)``.  The fused ``v * (2 / 255) - 1`` differs from it by one ulp on 111 of the 256 bytes;
* the flip mirrors the columns while they are stored.

Launches per batch: 1 without a resize, 2 with one (horizontal uint8 pass, then the vertical pass fused with table, flip and planar store).
The tables are validated by the library against their HOST copies before anything is launched, and the kernels clamp the device copies.
There is no fallback: a CPU tensor or a backend other than the HIP one is an error.
"""
import functools

import numpy as np
import torch          # every device allocation below goes through this name (torch.empty): tests swap it for a guard-banded allocator

from .. import _lib
from ..models.op import _backend
from ..models.op._backend import HipBackend          # noqa: F401  (the launch path of this module: _backend.get()._launch)

PRECISION_BITS = 22          # PIL: 32 - 8 - 2


def resample_tables(in_extent, out, offset=0):
    """The per-axis tables of PIL's bilinear resample from ``in_extent`` pixels (a crop of that many, starting at ``offset``) to ``out``:
    ``coeff`` int32 [out, kmax] fixed-point weights (zero past each count) and ``bounds`` int32 [out, 2] = (first input index, offset
    included; number of taps)."""
    coeff, bounds = _tables(int(in_extent), int(out))
    if offset:
        bounds = bounds.copy()
        bounds[:, 0] += int(offset)
    return coeff, bounds


@functools.lru_cache(maxsize=256)
def _tables(n, out):
    if n < 1 or out < 1:
        raise ValueError('resample_tables: extents must be positive, got %d -> %d' % (n, out))
    scale = n / out
    fs = max(scale, 1.0)
    support = fs                                   # the triangle filter's support (1.0) times the filter scale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    count = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n) - xmin
    w = np.zeros((out, ksize), np.float64)
    total = np.zeros(out, np.float64)
    for x in range(ksize):                         # the weights are summed in tap order, as the C loop does
        v = np.maximum(0.0, 1.0 - np.abs((x + xmin - center + 0.5) * ss))
        v[x >= count] = 0.0
        w[:, x] = v
        total = total + v
    w = w / np.where(total != 0.0, total, 1.0)[:, None]
    coeff = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
    bounds = np.stack([xmin, count], 1).astype(np.int32)
    coeff.setflags(write=False)
    bounds.setflags(write=False)
    return coeff, bounds


def resample_tables_batched(extents, out, offsets):
    """``resample_tables`` per sample: coeff [B, out, kmax] (kmax: the widest sample's, zero-padded) and bounds [B, out, 2]."""
    per = [resample_tables(n, out, o) for n, o in zip(extents, offsets)]
    kmax = max(c.shape[1] for c, _ in per)
    coeff = np.zeros((len(per), out, kmax), np.int32)
    for i, (c, _) in enumerate(per):
        coeff[i, :, :c.shape[1]] = c
    return coeff, np.stack([b for _, b in per])


def resample_pass(img, coeff, bounds, axis):
    """One pass on the host in numpy: img uint8 [H, W, 3], resampled along ``axis`` (0 rows -> vertical, 1 columns -> horizontal).  What the
    kernels compute; the fixture generator and the tests compare it with PIL."""
    src = np.moveaxis(np.asarray(img), axis, 0).astype(np.int32)
    out = np.empty((coeff.shape[0],) + src.shape[1:], np.uint8)
    for o in range(coeff.shape[0]):
        first, count = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coeff[o, :count], src[first:first + count], 1)
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_reference(img, size, box=None):
    """crop(box) + bilinear resize to (size_h, size_w) of one uint8 [H, W, 3] image on the host, with this module's tables: horizontal pass,
    uint8 intermediate, vertical pass, each only where the extent changes.  box = (left, top, right, bottom)."""
    h, w = img.shape[:2]
    left, top, right, bottom = box if box is not None else (0, 0, w, h)
    out_h, out_w = size
    img = np.asarray(img)[top:bottom, left:right]
    if right - left != out_w:
        img = resample_pass(img, *resample_tables(right - left, out_w), axis=1)
    if bottom - top != out_h:
        img = resample_pass(img, *resample_tables(bottom - top, out_h), axis=0)
    return np.ascontiguousarray(img)


def normalize_table():
    """byte -> float32 of ToTensor + Normalize(0.5, 0.5), by the reference's own operations (ffhq_dataset.py:62-63) on the host."""
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).to(torch.float32).div(255).sub(0.5).div(0.5)


_lut_cache = {}        # device -> the table on it


def _to_device(host, dev, dtype):
    t = torch.empty(tuple(host.shape), dtype=dtype, device=dev)
    t.copy_(host if torch.is_tensor(host) else torch.from_numpy(np.array(host, copy=True)))          # (the cached tables are read-only arrays)
    return t


def device_table(dev):
    """normalize_table() on ``dev``, uploaded once."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    t = _lut_cache.get(key)
    if t is None:
        t = _lut_cache[key] = _to_device(normalize_table(), dev, torch.float32)
    return t


def _backend_and_device(u8):
    hip = _backend.get()
    if getattr(hip, 'name', None) != 'hip':
        raise RuntimeError('gan_control_amd: the image input path runs on the HIP backend only (active: %r); there is no fallback' % getattr(hip, 'name', hip))
    if not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
        raise RuntimeError('gan_control_amd: images must be a uint8 tensor [B, H, W, 3], got %s' % (tuple(u8.shape) if torch.is_tensor(u8) else type(u8),))
    if not u8.is_cuda:
        raise RuntimeError('gan_control_amd: the image input path needs the uint8 batch on a GPU (got %s); there is no CPU fallback' % u8.device)
    if u8.stride(3) != 1 or u8.stride(2) != 3 or u8.stride(1) < 3 * u8.shape[2] or u8.stride(0) < 0:
        raise RuntimeError('gan_control_amd: images must be interleaved rows (strides %s)' % (tuple(u8.stride()),))
    return hip, u8.device


def _flip_on_device(flip, batch, dev):
    if flip is None:
        host = torch.zeros(batch, dtype=torch.int32)
    elif torch.is_tensor(flip):
        if flip.is_cuda and flip.dtype == torch.int32 and flip.is_contiguous() and flip.numel() == batch:
            return flip
        host = flip.detach().to('cpu').to(torch.int32).reshape(-1)
    else:
        host = torch.tensor([int(bool(f)) for f in flip], dtype=torch.int32)
    if host.numel() != batch:
        raise ValueError('flip needs one flag per sample: %d for a batch of %d' % (host.numel(), batch))
    return _to_device(host, dev, torch.int32)


def u8_to_f32(u8, flip=None, lut=None):
    """gc_image_u8_to_f32: y[b, c, i, j] = lut[u8[b, i, jj, c]], mirrored where flip[b]; one launch."""
    hip, dev = _backend_and_device(u8)
    b, h, w, _ = u8.shape
    lut = device_table(dev) if lut is None else lut
    flip = _flip_on_device(flip, b, dev)
    y = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
    hip._launch(dev, 'gc_image_u8_to_f32', _lib.ptr(u8), u8.stride(1), u8.stride(0), _lib.ptr(lut), _lib.ptr(flip), _lib.ptr(y), b, h, w,
                _lib.stream_of(u8))
    return y


class DeviceTables:
    """The tables of one pass on the host (what the library validates) and on the device (what the kernel reads).  Build once and pass as
    ``coeff`` to resample_u8 / resample_v_u8_to_f32 where the same tables serve many batches."""

    def __init__(self, coeff, bounds, other, dev):
        coeff, bounds = np.ascontiguousarray(coeff, np.int32), np.ascontiguousarray(bounds, np.int32)
        if coeff.ndim == 2:
            coeff, bounds = coeff[None], bounds[None]
        self.samples, self.out, self.kmax = coeff.shape if coeff.ndim == 3 else (0, 0, 0)
        if coeff.ndim != 3 or bounds.shape != (self.samples, self.out, 2):
            raise ValueError('resample tables: coeff [S, out, kmax] and bounds [S, out, 2] expected, got %s and %s' % (coeff.shape, bounds.shape))
        self.bounds_host = bounds
        self.other_host = None if other is None else np.ascontiguousarray(other, np.int32).reshape(self.samples, 2)
        self.coeff = _to_device(coeff, dev, torch.int32)
        self.bounds = _to_device(bounds, dev, torch.int32)
        self.other = None if other is None else _to_device(self.other_host, dev, torch.int32)

    def args(self, batch):
        if self.samples not in (1, batch):
            raise ValueError('resample tables for %d samples and a batch of %d' % (self.samples, batch))
        return (_lib.ptr(self.coeff), _lib.ptr(self.bounds), self.bounds_host.ctypes.data, self.kmax, 0 if self.samples == 1 else 1,
                _lib.ptr(self.other), None if self.other_host is None else self.other_host.ctypes.data)


def resample_u8(u8, out_h, out_w, axis, coeff, bounds=None, other=None):
    """gc_image_resample_u8: one pass along ``axis`` (0 horizontal, 1 vertical), uint8 -> dense uint8 [B, out_h, out_w, 3].  other [S, 2]:
    (offset, count) along the axis that is not resampled."""
    hip, dev = _backend_and_device(u8)
    b, h, w, _ = u8.shape
    t = coeff if isinstance(coeff, DeviceTables) else DeviceTables(coeff, bounds, other, dev)
    y = torch.empty((b, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    c, bd, bdh, kmax, ts, ot, oth = t.args(b)
    hip._launch(dev, 'gc_image_resample_u8', _lib.ptr(u8), u8.stride(1), u8.stride(0), h, w, _lib.ptr(y), b, out_h, out_w, axis,
                c, bd, bdh, kmax, ts, ot, oth, _lib.stream_of(u8))
    return y


def resample_v_u8_to_f32(u8, out_h, out_w, coeff, bounds=None, other=None, flip=None, lut=None):
    """gc_image_resample_v_u8_to_f32: the vertical pass, the table lookup, the flip and the planar store in one launch."""
    hip, dev = _backend_and_device(u8)
    b, h, w, _ = u8.shape
    lut = device_table(dev) if lut is None else lut
    flip = _flip_on_device(flip, b, dev)
    t = coeff if isinstance(coeff, DeviceTables) else DeviceTables(coeff, bounds, other, dev)
    y = torch.empty((b, 3, out_h, out_w), dtype=torch.float32, device=dev)
    c, bd, bdh, kmax, ts, ot, oth = t.args(b)
    hip._launch(dev, 'gc_image_resample_v_u8_to_f32', _lib.ptr(u8), u8.stride(1), u8.stride(0), h, w, _lib.ptr(lut), _lib.ptr(flip), _lib.ptr(y),
                b, out_h, out_w, c, bd, bdh, kmax, ts, ot, oth, _lib.stream_of(u8))
    return y


def images_to_device_batch(u8, size=None, boxes=None, flip=None):
    """uint8 [B, H, W, 3] on the device -> float32 [B, 3, size, size] in [-1, 1] (size: an int or (height, width); None keeps H x W).

    boxes: per-sample (left, top, right, bottom) integer crops, resized to ``size`` each (``resized_crop``); flip: per-sample flags.
    """
    _, dev = _backend_and_device(u8)
    b, h, w, _ = u8.shape
    out_h, out_w = (h, w) if size is None else ((size, size) if isinstance(size, int) else tuple(size))
    if boxes is None:
        if (out_h, out_w) == (h, w):
            return u8_to_f32(u8, flip)
        boxes_l, shared = [(0, 0, w, h)], True
    else:
        boxes_l, shared = [tuple(int(v) for v in bx) for bx in boxes], False
        if len(boxes_l) != b:
            raise ValueError('boxes needs one box per sample: %d for a batch of %d' % (len(boxes_l), b))
    for left, top, right, bottom in boxes_l:
        if not (0 <= left < right <= w and 0 <= top < bottom <= h):
            raise ValueError('box %s outside the %d x %d image' % ((left, top, right, bottom), w, h))
    need_h = any(r - l != out_w for l, _, r, _ in boxes_l)
    need_v = any(bt - t != out_h for _, t, _, bt in boxes_l)
    rows = [(t, bt - t) for _, t, _, bt in boxes_l]
    cols = [(l, r - l) for l, _, r, _ in boxes_l]
    if need_h:
        # horizontal pass into a uint8 intermediate that holds each sample's crop rows from row 0 on
        if shared:
            hc, hb = resample_tables(cols[0][1], out_w, cols[0][0])
        else:
            hc, hb = resample_tables_batched([c[1] for c in cols], out_w, [c[0] for c in cols])
        mid_h = max(n for _, n in rows)
        mid = resample_u8(u8, mid_h, out_w, 0, hc, hb, other=None if shared and rows[0] == (0, mid_h) else rows)
        if not need_v:
            return u8_to_f32(mid, flip)
        u8, rows, cols = mid, [(0, n) for _, n in rows], None
    elif not need_v:
        # a pure crop (every box already has the output size): the vertical pass with identity weights places it
        need_v = True
    if shared:
        vc, vb = resample_tables(rows[0][1], out_h, rows[0][0])
    else:
        vc, vb = resample_tables_batched([r[1] for r in rows], out_h, [r[0] for r in rows])
    other = None if cols is None or (shared and cols[0] == (0, out_w)) else cols
    return resample_v_u8_to_f32(u8, out_h, out_w, vc, vb, other=other, flip=flip)
