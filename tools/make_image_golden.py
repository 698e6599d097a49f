#!/usr/bin/env python
"""Writes tests/golden/image_input.npz: what the reference's host transform chain gives for the cases of tests/test_image_input*.py.

torchvision is NOT installed where this project is developed, so the reference's dataset modules cannot be imported.  What they compute
is nevertheless fixed by two libraries that are: ``transforms.Resize`` / ``RandomResizedCrop`` on a PIL image call ``Image.resize(...,
BILINEAR)`` (after ``Image.crop(box)`` for a crop), and ``ToTensor`` + ``Normalize(0.5, 0.5)`` are torch's ``div(255)``, ``sub(0.5)``,
``div(0.5)`` on float32.  PIL's ``resize`` / ``crop`` and those three torch operations ARE the reference chain's arithmetic; this script
records their results:

    <case>/in        seeded uint8 input [H, W, 3]
    <case>/out       PIL's resize to the case's output size, uint8 [out_h, out_w, 3]
    <case>/box<i>    a crop box (left, top, right, bottom);  <case>/out<i>: PIL's crop(box).resize(...) for it
    lut              the 256 floats of torch's div / sub / div on every byte

Before writing, it asserts that the package's own table builder (datasets/image_ops.py: resample_tables) with a numpy pass reproduces PIL
on every case with 0 differing bytes.  Run from the repository root: ``python tools/make_image_golden.py``.
"""
import os
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'gan-control_amd'))

from gan_control_amd.datasets import image_ops  # noqa: E402

BOXES = [(3, 5, 60, 59), (10, 0, 70, 66), (0, 7, 57, 64)]
# name: (in_h, in_w, [(out_h, out_w), ...], boxes)
RESIZE = {
    'r64to32': (64, 64, [(32, 32)], []),             # exact 2x: 5 taps
    'r33x47to32': (33, 47, [(32, 32)], []),          # both passes, no integer ratio
    'r20to32': (20, 20, [(32, 32)], []),             # upscale: 3 taps
    'r64x32to32': (64, 32, [(32, 32)], []),          # vertical pass only
    'r32x64to32': (32, 64, [(32, 32)], []),          # horizontal pass only
    'r256to128': (256, 256, [(128, 128)], []),
    'c64': (64, 64, [(32, 32), (48, 48)], [BOXES[0], BOXES[2]]),           # (10, 0, 70, 66) does not fit a 64 x 64 image
    'c80x70': (80, 70, [(32, 32), (48, 48)], BOXES),
}


def make_input(name, h, w, rng):
    if h * w > 128 * 128:        # a large case compresses: ramps with a block checkerboard on top instead of noise
        i, j, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing='ij')
        return ((i * 3 + j * 5 + c * 40 + (((i // 8) + (j // 8)) & 1) * 90) % 256).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def pil_resize(img, size, box=None):
    im = Image.fromarray(img, 'RGB')
    if box is not None:
        im = im.crop(box)
    return np.asarray(im.resize((size[1], size[0]), Image.BILINEAR))


def main():
    rng = np.random.default_rng(20240607)
    out = {}
    for name, (h, w, sizes, boxes) in RESIZE.items():
        img = make_input(name, h, w, rng)
        out[name + '/in'] = img
        for size in sizes:
            tag = '' if len(sizes) == 1 else '_%d' % size[0]
            if not boxes:
                want = pil_resize(img, size)
                assert np.array_equal(image_ops.resize_reference(img, size), want), (name, size)
                out[name + '/out' + tag] = want
            for i, box in enumerate(boxes):
                want = pil_resize(img, size, box)
                assert np.array_equal(image_ops.resize_reference(img, size, box), want), (name, size, box)
                out['%s/box%d' % (name, i)] = np.asarray(box, np.int32)
                out['%s/out%d%s' % (name, i, tag)] = want
    out['lut'] = image_ops.normalize_table().numpy()
    path = os.path.join(REPO, 'tests', 'golden', 'image_input.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
