"""Generated images to something a person can look at: float32 [B, 3, h, w] in [-1, 1] -> a uint8 image grid -> a PIL image.

The reference does this on the host (evaluation/generation.py:14-22, :87-94): ``t.mul(0.5).add(0.5).clamp(min=0., max=1.).cpu()``,
``torchvision.utils.make_grid``, ``transforms.ToPILImage`` (``mul(255).byte()``) and, for the large matrices, ``transforms.Resize`` on the PIL
image.  Here a batch on the device takes ONE launch of csrc/image_output.hip (gc_image_f32_to_u8_grid) that reads the planes once and writes
the byte grid, the two uint8 resample passes of the input path (datasets/image_ops.py) where a downsample is asked for, and one copy of the
final bytes to the host.  The bytes are the reference's:

* the quantisation is the float32 operation sequence ``x * 0.5``, ``+ 0.5``, ``clamp(0, 1)``, ``* 255``, truncate -- each step rounded on its
  own (``quantize_reference``).  ``x * 127.5 + 127.5`` is another function: it differs on 223 of the 510 floats next to a byte boundary.
  +-inf follow the clamp; NaN gives byte 0 (the reference leaves it to the C cast);
* the geometry is make_grid's (``make_grid_reference``): ``xmaps = min(nrow, B)``, ``ymaps = ceil(B / xmaps)``, tiles ``padding`` apart and from
  the border, empty tiles of a ragged last row and every band filled with ``pad_value``; a single image comes back bare, as from make_grid;
* the resize is PIL's 8-bit bilinear resample (``image_ops.resize_reference``), including the reference's quirk of handing ``Resize`` the pair
  (width // d, height // d) where it reads (height, width).

``quantize_reference`` and ``make_grid_reference`` are the documented semantics, the oracle of the tests and the path of CPU tensors.  Which path
runs is decided by the tensor's device alone: a CUDA tensor on another backend than the HIP one is an error, never a detour over the host.
"""
import numpy as np
import torch          # every device allocation below goes through this name (torch.empty): tests swap it for a guard-banded allocator

from .. import _lib
from ..datasets import image_ops
from ..models.op import _backend
from ..models.op._backend import HipBackend          # noqa: F401  (the launch path of this module: _backend.get()._launch)


def quantize_reference(x):
    """float -> uint8 of the same shape on the host, by the reference's own float32 operations; NaN -> 0."""
    v = torch.as_tensor(x).detach().to('cpu', torch.float32)
    v = v.mul(0.5).add(0.5).clamp(min=0., max=1.).mul(255)
    return torch.where(torch.isnan(v), torch.zeros_like(v), v).to(torch.uint8)


def grid_geometry(batch, h, w, nrow, padding):
    """(xmaps, ymaps, grid_h, grid_w) of torchvision.utils.make_grid."""
    xmaps = min(int(nrow), int(batch))
    ymaps = -(-int(batch) // xmaps)
    return xmaps, ymaps, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def make_grid_reference(u8, nrow, padding=2, pad_value=0):
    """uint8 [B, 3, h, w] -> uint8 [grid_h, grid_w, 3] in numpy: tile k at row (k // xmaps) * (h + padding) + padding, column (k % xmaps) *
    (w + padding) + padding; everything else is ``pad_value``.  (The single-image special case belongs to ``to_u8_grid``.)"""
    u8 = np.asarray(u8)
    b, c, h, w = u8.shape
    xmaps, ymaps, grid_h, grid_w = grid_geometry(b, h, w, nrow, padding)
    out = np.full((grid_h, grid_w, c), pad_value, np.uint8)
    for k in range(b):
        top, left = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        out[top:top + h, left:left + w] = u8[k].transpose(1, 2, 0)
    return out


def _check(x, nrow, padding, pad_value):
    if not torch.is_tensor(x) or x.dim() not in (3, 4) or not x.dtype.is_floating_point:
        raise RuntimeError('gan_control_amd: images must be a float tensor [B, 3, h, w], got %s' % (tuple(x.shape) if torch.is_tensor(x) else type(x),))
    x = x.detach()
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.shape[1] != 3:
        raise RuntimeError('gan_control_amd: image grids are built from 3-channel images, got %d channels' % x.shape[1])
    if min(x.shape) < 1 or int(nrow) < 1 or int(padding) < 0 or not 0 <= int(pad_value) <= 255:
        raise ValueError('to_u8_grid: shape %s, nrow %s, padding %s, pad_value %s' % (tuple(x.shape), nrow, padding, pad_value))
    return x


def _dense_enough(x):
    """What gc_image_f32_to_u8_grid reads in place: unit column stride and strides at least dense (a batch slice, rows with a pitch)."""
    b, _, h, w = x.shape
    ss, sp, sr, sc = x.stride()
    span = (h - 1) * sr + w
    return sc == 1 and sr >= w and sp >= span and (ss >= 2 * sp + span or b == 1)


def to_u8_grid(x, nrow=8, padding=2, pad_value=0, out=None):
    """float32 [B, 3, h, w] -> uint8 [grid_h, grid_w, 3] on x's device.  A CUDA tensor: one launch of gc_image_f32_to_u8_grid (``out``: a
    uint8 view [grid_h, grid_w, 3] with unit strides inside a row to write into, any row stride and byte offset); a CPU tensor:
    ``quantize_reference`` + ``make_grid_reference``.  One image comes back without padding, as make_grid returns it."""
    x = _check(x, nrow, padding, pad_value)
    b, _, h, w = x.shape
    if b == 1:
        padding = 0
    nrow, padding, pad_value = int(nrow), int(padding), int(pad_value)
    _, _, grid_h, grid_w = grid_geometry(b, h, w, nrow, padding)
    if not x.is_cuda:
        if out is not None:
            raise ValueError('to_u8_grid: out= belongs to the device path')
        return torch.from_numpy(make_grid_reference(quantize_reference(x).numpy(), nrow, padding, pad_value))
    hip = _backend.get()
    if getattr(hip, 'name', None) != 'hip':
        raise RuntimeError('gan_control_amd: the image output path runs on the HIP backend only (active: %r); there is no fallback' % getattr(hip, 'name', hip))
    if x.dtype != torch.float32:
        x = x.float()
    if not _dense_enough(x):
        x = x.contiguous()
    dev = x.device
    if out is None:
        out = torch.empty((grid_h, grid_w, 3), dtype=torch.uint8, device=dev)
    elif (not out.is_cuda or out.device != dev or out.dtype != torch.uint8 or tuple(out.shape) != (grid_h, grid_w, 3) or out.stride(2) != 1
          or out.stride(1) != 3 or (out.stride(0) < 3 * grid_w and grid_h > 1)):
        raise RuntimeError('gan_control_amd: out must be a uint8 [%d, %d, 3] view of interleaved rows on %s' % (grid_h, grid_w, dev))
    ss = x.stride(0) if b > 1 else max(x.stride(0), 3 * x.stride(1))          # (the sample stride of a single sample is never used)
    hip._launch(dev, 'gc_image_f32_to_u8_grid', _lib.ptr(x), x.stride(2), x.stride(1), ss, _lib.ptr(out), max(out.stride(0), 3 * grid_w),
                b, h, w, nrow, padding, pad_value, grid_h, grid_w, _lib.stream_of(x))
    return out


def downsampled_size(grid_h, grid_w, downsample):
    """(out_h, out_w) of the reference's ``transforms.Resize((width // d, height // d))``: Resize reads the pair as (h, w), so the output HEIGHT
    comes from the grid's width and the output WIDTH from its height (every grid the reference makes is square)."""
    out_h, out_w = grid_w // downsample, grid_h // downsample
    if out_h < 1 or out_w < 1:
        raise ValueError('grid_image: a %d x %d grid cannot be downsampled by %d' % (grid_h, grid_w, downsample))
    return out_h, out_w


def grid_image(x, nrow, downsample=None, padding=2, pad_value=0):
    """The PIL image the reference's gen_grid / gen_matrix return for the float images ``x``: ``to_u8_grid`` and, with ``downsample``, PIL's
    bilinear resize to ``downsampled_size``.  On the device: the grid launch, a horizontal and a vertical uint8 resample pass (each only where
    the extent changes), one copy to the host."""
    from PIL import Image
    grid = to_u8_grid(x, nrow=nrow, padding=padding, pad_value=pad_value)
    grid_h, grid_w = grid.shape[:2]
    if downsample is not None:
        out_h, out_w = downsampled_size(grid_h, grid_w, int(downsample))
        if not grid.is_cuda:
            grid = torch.from_numpy(image_ops.resize_reference(grid.numpy(), (out_h, out_w)))
        else:
            u8 = grid.unsqueeze(0)
            if out_w != grid_w:
                u8 = image_ops.resample_u8(u8, grid_h, out_w, 0, *image_ops.resample_tables(grid_w, out_w))
            if out_h != grid_h:
                u8 = image_ops.resample_u8(u8, out_h, out_w, 1, *image_ops.resample_tables(grid_h, out_h))
            grid = u8[0]
    return Image.fromarray(np.ascontiguousarray(grid.cpu().numpy()), 'RGB')
