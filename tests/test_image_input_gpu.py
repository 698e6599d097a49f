"""The three image-input entries on the GPU (csrc/image_input.hip through datasets/image_ops.py) and the stream that feeds the trainer.

Every expectation is the PIL / torch fixture (tests/golden/image_input.npz, tools/make_image_golden.py) or a table gather done by torch on the
CPU; results are compared as float BITS, with no tolerance anywhere.  Each case runs plainly and on poisoned, guard-banded allocations
(tests/guarded_alloc.py swaps the ``torch`` of image_ops: outputs, the uint8 intermediate and the device tables all come from it)."""
import numpy as np
import pytest
import torch

import guarded_alloc
from conftest import load_golden

from gan_control_amd import _lib
from gan_control_amd.datasets import image_folder, image_ops
from gan_control_amd.models.op import _backend

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GOLD = load_golden('image_input')
LUT = torch.from_numpy(GOLD['lut'])
CVT, H, VF = 'gc_image_u8_to_f32', 'gc_image_resample_u8', 'gc_image_resample_v_u8_to_f32'


def expected(u8, flip):
    """float32 [B, 3, H, W] on the CPU: the table gather and the mirror, by torch."""
    out = LUT[torch.as_tensor(u8).long()].permute(0, 3, 1, 2)
    return torch.stack([o.flip(2) if f else o for o, f in zip(out, flip)]).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def strided_view(x, pad, shift):
    """x uint8 [B, H, W, 3] as a device view: rows ``pad`` bytes apart beyond their own, the first byte ``shift`` bytes past a 512-byte boundary."""
    b, h, w, _ = x.shape
    rs = 3 * w + pad
    backing = torch.full((b * h * rs + 1024,), 0xEE, dtype=torch.uint8, device=DEV)
    first = (-backing.data_ptr()) % 512 + shift
    view = torch.as_strided(backing, (b, h, w, 3), (h * rs, rs, 3, 1), first)
    view.copy_(x.to(DEV))
    return view


class Case:
    def __init__(self, name, x, want, entries, size=None, boxes=None, flip=(1, 0, 1), place=None):
        self.name, self.x, self.want, self.entries, self.size, self.boxes, self.flip = name, torch.as_tensor(x), want, entries, size, boxes, list(flip)
        self.place = place or (lambda x: x.to(DEV))

    def run(self, x_dev=None):
        x_dev = self.place(self.x) if x_dev is None else x_dev
        return image_ops.images_to_device_batch(x_dev, size=self.size, boxes=self.boxes, flip=self.flip)


def convert_cases():
    rng = np.random.default_rng(7)
    out = []
    x = rng.integers(0, 256, (3, 5, 13, 3), dtype=np.uint8)
    out.append(Case('cvt-3x5x13', x, expected(x, (1, 0, 1)), [CVT]))
    x = rng.permutation(np.arange(3 * 4 * 16 * 3) % 256).astype(np.uint8).reshape(3, 4, 16, 3)          # every byte value, on the 16-pixel path
    assert len(np.unique(x)) == 256
    out.append(Case('cvt-3x4x16-all-bytes', x, expected(x, (1, 0, 1)), [CVT]))
    x = rng.integers(0, 256, (3, 7, 36, 3), dtype=np.uint8)
    for shift in (1, 2, 3):
        out.append(Case('cvt-3x7x36-view+%d' % shift, x, expected(x, (1, 0, 1)), [CVT], place=lambda x, s=shift: strided_view(x, 17, s)))
    x = rng.integers(0, 256, (1, 1, 1, 3), dtype=np.uint8)
    out.append(Case('cvt-1x1x1', x, expected(x, (1,)), [CVT], flip=(1,)))
    return out


def resize_cases():
    out = []
    launches = {'r64to32': [H, VF], 'r33x47to32': [H, VF], 'r20to32': [H, VF], 'r64x32to32': [VF], 'r32x64to32': [H, CVT], 'r256to128': [H, VF]}
    for name, entries in launches.items():
        want = GOLD[name + '/out']
        x = np.stack([GOLD[name + '/in']] * 3)
        out.append(Case(name, x, expected(np.stack([want] * 3), (1, 0, 1)), entries, size=tuple(want.shape[:2])))
    for name, ids, flip in (('c64', (0, 1), (1, 0)), ('c80x70', (0, 1, 2), (1, 0, 1))):
        for size in (32, 48):
            boxes = [tuple(int(v) for v in GOLD['%s/box%d' % (name, i)]) for i in ids]
            want = np.stack([GOLD['%s/out%d_%d' % (name, i, size)] for i in ids])
            x = np.stack([GOLD[name + '/in']] * len(ids))
            out.append(Case('%s-boxes-%d' % (name, size), x, expected(want, flip), [H, VF], size=size, boxes=boxes, flip=flip))
    return out


CASES = convert_cases() + resize_cases()


def test_the_boxes_are_the_fixtures():
    boxes = {b for c in CASES if c.boxes for b in c.boxes}
    assert boxes == {(3, 5, 60, 59), (10, 0, 70, 66), (0, 7, 57, 64)}


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_bits_and_guard_bands(case):
    """Plain, then on NaN-poisoned and on 1e30-poisoned guard-banded buffers: the guards untouched, every output finite, and three times the
    bits of the fixture; the launches are the ones the path promises (1 without a resize, at most 2 with one)."""
    results = [case.run()]
    for poison in ('nan', 'big'):
        with guarded_alloc.guarded(image_ops, poison=poison) as guard:
            results.append(case.run())
            violations = guard.check()
        assert not violations, violations
        assert guard.entries == case.entries
    want = bits(case.want)
    for y in results:
        assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == tuple(case.want.shape)
        assert bool(torch.isfinite(y).all())
        assert int((bits(y) != want).sum()) == 0


def hostile_u8(x, fill, pad, shift=0):
    """x uint8 [B, H, W, 3] as a device view between 64 KiB of ``fill`` bytes on each side, the ``pad`` bytes behind every row (but the last) filled
    alike, ``shift`` bytes past a 512-byte boundary.  -> (view, backing buffer, its expected content)."""
    b, h, w, _ = x.shape
    rs, guard = 3 * w + pad, 64 << 10
    span = (b * h - 1) * rs + 3 * w
    backing = torch.full((guard + 512 + shift + span + guard,), fill, dtype=torch.uint8, device=DEV)
    first = (-(backing.data_ptr() + guard)) % 512 + guard + shift
    view = torch.as_strided(backing, (b, h, w, 3), (h * rs, rs, 3, 1), first)
    view.copy_(x.to(DEV))
    return view, backing, backing.clone()


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_hostile_inputs(case, monkeypatch):
    """The input between 0xFF bytes, then between 0x00 bytes (row padding included), and every coefficient slot past its bounds count set to
    0x7FFFFFFF: the same bits, and not one byte of the input buffer written."""
    def poisoned(fn):
        def build(*a, **k):
            coeff, bounds = fn(*a, **k)
            coeff = np.array(coeff, copy=True)
            slots = np.arange(coeff.shape[-1])
            coeff[slots >= bounds[..., 1:2]] = 0x7FFFFFFF
            return coeff, bounds
        return build

    monkeypatch.setattr(image_ops, 'resample_tables_batched', poisoned(image_ops.resample_tables_batched))
    monkeypatch.setattr(image_ops, 'resample_tables', poisoned(image_ops.resample_tables))
    want = bits(case.want)
    for fill, pad, shift in ((0xFF, 5, 0), (0x00, 5, 3), (0xFF, 0, 2)):
        view, backing, before = hostile_u8(case.x, fill, pad, shift)
        y = case.run(view)
        assert int((bits(y) != want).sum()) == 0, (fill, pad, shift)
        assert torch.equal(backing, before)


def test_refusals_launch_nothing():
    hip, dev = _backend.get(), torch.device(DEV)
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    lut, flip = image_ops.device_table(dev), torch.zeros(1, dtype=torch.int32, device=DEV)
    y8 = torch.full((1, 8, 4, 3), 0x5A, dtype=torch.uint8, device=DEV)
    yf = torch.full((1, 3, 8, 8), 7.0, device=DEV)
    coeff, bounds = image_ops.resample_tables(8, 4)
    tables = image_ops.DeviceTables(coeff, bounds, None, dev)
    c, bd, bdh, kmax, ts, ot, oth = tables.args(1)
    stream = _lib.stream_of(x)
    with pytest.raises(RuntimeError, match='gc_image_u8_to_f32 failed.*null'):
        hip._launch(dev, 'gc_image_u8_to_f32', _lib.ptr(x), 24, 192, None, _lib.ptr(flip), _lib.ptr(yf), 1, 8, 8, stream)
    with pytest.raises(RuntimeError, match='gc_image_u8_to_f32 failed.*row stride'):
        hip._launch(dev, 'gc_image_u8_to_f32', _lib.ptr(x), 23, 192, _lib.ptr(lut), _lib.ptr(flip), _lib.ptr(yf), 1, 8, 8, stream)
    with pytest.raises(RuntimeError, match='gc_image_resample_u8 failed.*kmax'):
        hip._launch(dev, 'gc_image_resample_u8', _lib.ptr(x), 24, 192, 8, 8, _lib.ptr(y8), 1, 8, 4, 0, c, bd, bdh, 0, ts, ot, oth, stream)
    with pytest.raises(RuntimeError, match='gc_image_resample_u8 failed.*null'):
        hip._launch(dev, 'gc_image_resample_u8', _lib.ptr(x), 24, 192, 8, 8, _lib.ptr(y8), 1, 8, 4, 0, None, bd, bdh, kmax, ts, ot, oth, stream)
    with pytest.raises(RuntimeError, match='gc_image_resample_v_u8_to_f32 failed.*null'):
        hip._launch(dev, 'gc_image_resample_v_u8_to_f32', _lib.ptr(x), 24, 192, 8, 8, None, _lib.ptr(flip), _lib.ptr(yf), 1, 8, 8, c, bd, bdh, kmax, ts,
                    ot, oth, stream)
    outside = np.array(bounds, copy=True)
    outside[3, 0] += 1          # the last output's taps end one pixel past the crop
    with pytest.raises(RuntimeError, match='gc_image_resample_u8 failed.*reads outside'):
        image_ops.resample_u8(x, 8, 4, 0, coeff, outside)
    with pytest.raises(RuntimeError, match='gc_image_resample_v_u8_to_f32 failed.*reads outside'):
        image_ops.resample_v_u8_to_f32(x, 4, 8, coeff, outside)
    with pytest.raises(RuntimeError, match='gc_image_resample_u8 failed.*other'):
        image_ops.resample_u8(x, 8, 4, 0, coeff, bounds, other=[(1, 8)])          # rows 1 .. 8 of an 8-row image
    torch.cuda.synchronize()
    assert bool((y8 == 0x5A).all()) and bool((yf == 7.0).all())


def _write_pngs(root, n, size):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(3)
    (root / 'faces').mkdir(parents=True)
    images = {}
    for i in range(n):
        arr = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
        path = root / 'faces' / ('%03d.png' % i)
        Image.fromarray(arr, 'RGB').save(path)
        images[str(path)] = arr
    return images


def test_stream_prefetch_and_training(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    images = _write_pngs(tmp_path / 'ds', 16, 32)
    ds = image_folder.ImageFolderU8(str(tmp_path / 'ds'))
    stream = image_folder.DeviceImageStream(ds, 4, size=32, training=True, device=DEV, seed=2, num_workers=0)
    flips = 0
    for _ in range(6):          # four batches per epoch: the prefetch crosses the epoch boundary
        img, meta = next(stream)
        want = expected(np.stack([images[p] for p in meta['paths']]), meta['flip'].tolist())
        assert int((bits(img) != bits(want)).sum()) == 0
        flips += int(meta['flip'].sum())
    assert 0 < flips < 24 and stream.epoch >= 1
    # ... the same folder through the resize path (32 -> 16), against PIL itself
    small = image_folder.DeviceImageStream(ds, 4, size=16, training=True, device=DEV, seed=4, num_workers=0)
    for _ in range(2):
        img, meta = next(small)
        pil = np.stack([np.asarray(Image.fromarray(images[p], 'RGB').resize((16, 16), Image.BILINEAR)) for p in meta['paths']])
        assert int((bits(img) != bits(expected(pil, meta['flip'].tolist()))).sum()) == 0
    # ... and into the training loop
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    tr = GeneratorTrainer(default_config(32, 4), device=DEV, seed=0)
    feed = image_folder.get_ffhq_data_loader({'path': str(tmp_path / 'ds'), 'workers': 0}, batch_size=tr.local_batch, size=32, device=DEV, seed=1)
    assert tr.train(data=feed.images(), iters=2) == 2
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.as_tensor(tr.stats['d_loss'])).all())
    via_trainer = tr.make_data_stream({'data_set_name': 'ffhq', 'path': str(tmp_path / 'ds'), 'workers': 0})
    assert next(via_trainer)[0].shape == (4, 3, 32, 32)
