#!/usr/bin/env python
"""Writes tests/golden/image_output.npz: what the reference's host chain gives for the cases of tests/test_image_output*.py.

torchvision is NOT installed where this project is developed.  What the reference's gen_grid / gen_matrix compute is nevertheless fixed by
two libraries that are: ``mul(0.5).add(0.5).clamp(min=0., max=1.)`` and ToPILImage's ``mul(255).byte()`` are torch operations on float32,
and ``transforms.Resize(size, BILINEAR)`` on a PIL image is ``Image.resize((size[1], size[0]), BILINEAR)``.  This script records their results:

    edges/x, edges/byte      for k = 1 .. 255 the smallest float32 that torch's five operations turn into byte k, and the float just below it
                             (byte k - 1): 510 floats, found by bisection over the float32 bit patterns, and their bytes
    <case>/tiles             uint8 [B, 3, h, w]: the quantised images of a grid
    <case>/grid              uint8 [grid_h, grid_w, 3]: make_grid of them (the geometry is written out here in numpy)
    <case>/nrow, /downsample the grid's images per row and the reference's ``downsample`` argument d
    <case>/out               PIL's BILINEAR resize of the grid to HEIGHT grid_w // d and WIDTH grid_h // d -- the reference hands Resize the
                             pair (width // d, height // d), which Resize reads as (h, w)

Before writing, it asserts that the package's host functions (evaluation/image_grid.py, datasets/image_ops.py: resize_reference) reproduce
every recorded array with 0 differing bytes.  Run from the repository root: ``python tools/make_image_output_golden.py``.
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'gan-control_amd'))

from gan_control_amd.datasets import image_ops  # noqa: E402
from gan_control_amd.evaluation import image_grid  # noqa: E402

# name: (batch, h, w, nrow, downsample)
CASES = {
    'g6x16_d4': (6, 16, 16, 3, 4),            # 38 x 56 -> 14 x 9
    'g2x28x42_d2': (2, 28, 42, 2, 2),         # 32 x 90 -> 45 x 16: the height grows
    'g4x18_d3': (4, 18, 18, 2, 3),            # 42 x 42 -> 14 x 14
    'g36x32_d4': (36, 32, 32, 6, 4),          # 206 x 206 -> 51 x 51: the shape of the training matrices
}
PADDING = 2


def torch_bytes(x):
    """The reference's operations, by torch itself."""
    return x.mul(0.5).add(0.5).clamp(min=0., max=1.).mul(255).byte()


def edge_floats():
    """For k = 1 .. 255: (the float just below, the smallest float giving byte k)."""
    def byte_of_bits(bits):
        return int(torch_bytes(torch.tensor([bits], dtype=torch.int32).view(torch.float32))[0])

    def key(bits):          # a monotone map from float32 bit patterns to integers
        return bits if bits >= 0 else -(bits & 0x7FFFFFFF)

    def bits_of_key(k):
        return k if k >= 0 else -k - 2 ** 31

    lo_all = key(int(np.float32(-1.0).view(np.int32)))
    hi_all = key(int(np.float32(1.0).view(np.int32)))
    xs = []
    for k in range(1, 256):
        lo, hi = lo_all, hi_all          # byte(lo) < k <= byte(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if byte_of_bits(bits_of_key(mid)) >= k:
                hi = mid
            else:
                lo = mid
        xs += [bits_of_key(lo), bits_of_key(hi)]
    x = torch.tensor(xs, dtype=torch.int64).to(torch.int32).view(torch.float32)
    return x, torch_bytes(x)


def make_tiles(b, h, w, rng):
    if b * h * w > 64 * 64:          # a large case compresses: ramps with a block checkerboard on top instead of noise
        k, c, i, j = np.meshgrid(np.arange(b), np.arange(3), np.arange(h), np.arange(w), indexing='ij')
        return ((k * 7 + i * 3 + j * 5 + c * 40 + (((i // 4) + (j // 4)) & 1) * 90) % 256).astype(np.uint8)
    return rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)


def main():
    rng = np.random.default_rng(20240917)
    out = {}
    x, by = edge_floats()
    assert x.numel() == 510 and by.tolist() == [v for k in range(1, 256) for v in (k - 1, k)]
    assert torch.equal(image_grid.quantize_reference(x), by)
    closed = (x * 127.5 + 127.5).clamp(0, 255).byte()
    print('edges: x * 127.5 + 127.5 differs on %d of %d' % (int((closed != by).sum()), x.numel()))
    out['edges/x'], out['edges/byte'] = x.numpy(), by.numpy()
    for name, (b, h, w, nrow, d) in CASES.items():
        tiles = make_tiles(b, h, w, rng)
        xmaps = min(nrow, b)
        ymaps = -(-b // xmaps)
        grid = np.zeros((ymaps * (h + PADDING) + PADDING, xmaps * (w + PADDING) + PADDING, 3), np.uint8)
        for k in range(b):
            top, left = (k // xmaps) * (h + PADDING) + PADDING, (k % xmaps) * (w + PADDING) + PADDING
            grid[top:top + h, left:left + w] = tiles[k].transpose(1, 2, 0)
        assert np.array_equal(image_grid.make_grid_reference(tiles, nrow, PADDING, 0), grid), name
        gh, gw = grid.shape[:2]
        out_h, out_w = gw // d, gh // d
        want = np.asarray(Image.fromarray(grid, 'RGB').resize((out_w, out_h), Image.BILINEAR))
        assert want.shape == (out_h, out_w, 3)
        assert np.array_equal(image_ops.resize_reference(grid, (out_h, out_w)), want), name
        out[name + '/tiles'], out[name + '/grid'], out[name + '/out'] = tiles, grid, want
        out[name + '/nrow'], out[name + '/downsample'] = np.int32(nrow), np.int32(d)
        print('%s: %d x %d -> %d x %d' % (name, gh, gw, out_h, out_w))
    path = os.path.join(REPO, 'tests', 'golden', 'image_output.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
