"""The host side of the real-image input path (no GPU): resample tables against the PIL fixture, the byte -> float table, the random-box
sampler, the folder data set with its stream, and the real-statistics pickle.  tests/golden/image_input.npz is written by
tools/make_image_golden.py from PIL and torch alone; nothing here compares the package with itself."""
import math
import pickle

import numpy as np
import pytest
import torch

from conftest import load_golden

from gan_control_amd.datasets import image_folder, image_ops

GOLD = load_golden('image_input')
# fixture case -> output sizes it holds; cases with boxes store one output per box
PLAIN = ['r64to32', 'r33x47to32', 'r20to32', 'r64x32to32', 'r32x64to32', 'r256to128']
CROPPED = {'c64': 2, 'c80x70': 3}


def cases():
    """(id, input, (out_h, out_w), box or None, expected bytes) for everything in the fixture."""
    out = []
    for name in PLAIN:
        want = GOLD[name + '/out']
        out.append((name, GOLD[name + '/in'], want.shape[:2], None, want))
    for name, n in CROPPED.items():
        for size in (32, 48):
            for i in range(n):
                out.append(('%s-box%d-%d' % (name, i, size), GOLD[name + '/in'], (size, size), tuple(int(v) for v in GOLD['%s/box%d' % (name, i)]),
                            GOLD['%s/out%d_%d' % (name, i, size)]))
    return out


CASES = cases()


def test_fixture_holds_the_cases_the_issue_names():
    assert len(CASES) == 6 + (2 + 3) * 2
    boxes = {c[3] for c in CASES if c[3]}
    assert boxes == {(3, 5, 60, 59), (10, 0, 70, 66), (0, 7, 57, 64)}
    assert GOLD['c80x70/in'].shape == (80, 70, 3) and GOLD['r33x47to32/in'].shape == (33, 47, 3)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_tables_and_numpy_pass_reproduce_the_fixture(case):
    _, img, size, box, want = case
    got = image_ops.resize_reference(img, size, box)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize('shape', [(48, 80, 32, 32), (17, 129, 8, 64), (96, 96, 37, 41)])
def test_tables_and_numpy_pass_reproduce_live_pil(shape):
    Image = pytest.importorskip('PIL.Image')
    h, w, oh, ow = shape
    img = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img, 'RGB').resize((ow, oh), Image.BILINEAR))
    assert int((image_ops.resize_reference(img, (oh, ow)) != want).sum()) == 0
    box = (2, 3, w - 1, h - 4)
    want = np.asarray(Image.fromarray(img, 'RGB').crop(box).resize((ow, oh), Image.BILINEAR))
    assert int((image_ops.resize_reference(img, (oh, ow), box) != want).sum()) == 0


def test_table_layout_and_offsets():
    coeff, bounds = image_ops.resample_tables(64, 32)
    assert coeff.shape == (32, 5) and bounds.shape == (32, 2) and coeff.dtype == bounds.dtype == np.int32
    assert image_ops.resample_tables(20, 32)[0].shape[1] == 3
    # every row sums to 2^22 within the rounding of its taps; slots past the count are zero
    assert np.all(np.abs(coeff.sum(1) - (1 << 22)) <= coeff.shape[1] / 2)          # each tap is rounded by at most a half
    for o in range(32):
        assert not coeff[o, bounds[o, 1]:].any() and 0 <= bounds[o, 0] and bounds[o, 0] + bounds[o, 1] <= 64
    shifted = image_ops.resample_tables(64, 32, offset=7)[1]
    assert np.array_equal(shifted[:, 0], bounds[:, 0] + 7) and np.array_equal(shifted[:, 1], bounds[:, 1])
    # an unchanged extent is the identity: one tap of weight 2^22
    ident, ib = image_ops.resample_tables(16, 16, offset=3)
    assert np.all(ident[:, 0] == 1 << 22) and not ident[:, 1:].any() and np.array_equal(ib[:, 0], np.arange(16) + 3)
    bc, bb = image_ops.resample_tables_batched([64, 20], 32, [0, 5])
    assert bc.shape == (2, 32, 5) and bb.shape == (2, 32, 2) and not bc[1, :, 3:].any() and bb[1, 0, 0] == 5


def test_normalize_table_is_the_reference_sequence_not_the_fused_form():
    lut = image_ops.normalize_table()
    assert lut.dtype == torch.float32 and lut.shape == (256,)
    assert np.array_equal(lut.numpy().view(np.int32), GOLD['lut'].view(np.int32))
    v = torch.arange(256, dtype=torch.float32)
    assert torch.equal(lut, ((v / 255) - 0.5) / 0.5)
    fused = v * (2.0 / 255.0) - 1.0
    assert int((fused != lut).sum()) == 111          # one ulp apart on these bytes: the table must not be "simplified"
    assert lut[0] == -1.0 and lut[255] == 1.0


def test_random_boxes():
    h, w = 96, 120
    gen = torch.Generator().manual_seed(5)
    boxes = image_folder.sample_boxes(2000, h, w, gen)
    full = sum(b == (0, 0, w, h) for b in boxes)
    assert 800 < full < 1200          # the 0.5 coin: both branches, about evenly
    for left, top, right, bottom in boxes:
        assert 0 <= left < right <= w and 0 <= top < bottom <= h
        if (left, top, right, bottom) == (0, 0, w, h):
            continue
        bw, bh = right - left, bottom - top
        # w = round(sqrt(area * aspect)), h = round(sqrt(area / aspect)) with area in [0.8, 1] * h * w and aspect in [0.9, 1.1]: each side is
        # within half a pixel of its real value, so the products and quotients below are checked with both sides moved by one pixel
        assert (bw - 1) * (bh - 1) <= 1.0 * h * w and (bw + 1) * (bh + 1) >= 0.8 * h * w
        assert (bw - 1) / (bh + 1) <= 1.1 and (bw + 1) / (bh - 1) >= 0.9
    again = image_folder.sample_boxes(2000, h, w, torch.Generator().manual_seed(5))
    assert again == boxes
    assert image_folder.sample_boxes(50, h, w, torch.Generator().manual_seed(6)) != boxes[:50]
    # a box that can never fit falls back to the centred one of the nearest allowed aspect
    left, top, right, bottom = image_folder.random_resized_box(10, 100, torch.Generator().manual_seed(0))
    assert (top, bottom) == (0, 10) and right - left == 11 and left == (100 - 11) // 2


def _numpy_convert(u8, size=None, boxes=None, flip=None):
    """Stand-in for image_ops.images_to_device_batch on the host: table lookup and flip only (the folders below need no resize)."""
    assert size in (None, u8.shape[1]) and boxes is None
    out = GOLD['lut'][u8.numpy()].transpose(0, 3, 1, 2)
    out = np.stack([o[:, :, ::-1] if f else o for o, f in zip(out, flip.tolist())])
    return torch.from_numpy(np.ascontiguousarray(out))


def _write_folder(root, n, size=16, start=0):
    Image = pytest.importorskip('PIL.Image')
    paths = []
    for i in range(n):
        # names that sort differently from their creation order, in two class directories
        d = root / ('b' if i % 2 else 'a')
        d.mkdir(parents=True, exist_ok=True)
        arr = np.full((size, size, 3), start + i, np.uint8)
        arr[0, :, 1] = np.arange(size)
        p = d / ('img_%02d.png' % ((7 * i) % n))
        Image.fromarray(arr, 'RGB').save(p)
        paths.append(str(p))
    return sorted(paths)


def test_folder_dataset_and_stream(tmp_path):
    pytest.importorskip('PIL')
    paths = _write_folder(tmp_path / 'ds', 8)
    ds = image_folder.ImageFolderU8(str(tmp_path / 'ds'))
    assert ds.samples == paths and len(ds) == 8 and (ds.height, ds.width) == (16, 16)
    img, path = ds[3]
    assert img.dtype == torch.uint8 and img.shape == (16, 16, 3) and path == paths[3]
    stream = image_folder.DeviceImageStream(ds, 4, size=16, training=True, device='cpu', seed=3, convert=_numpy_convert)
    seen = []
    for _ in range(5):          # two batches per epoch: the fifth one is in the third epoch
        img, meta = next(stream)
        assert img.shape == (4, 3, 16, 16) and img.dtype == torch.float32 and len(meta['paths']) == 4 and meta['boxes'] is None
        for k, p in enumerate(meta['paths']):
            value = ds[paths.index(p)][0]
            want = GOLD['lut'][value.numpy()].transpose(2, 0, 1)
            assert np.array_equal(img[k].numpy(), want[:, :, ::-1] if meta['flip'][k] else want)
        seen.append(meta['paths'])
    assert stream.epoch == 2
    assert sorted(seen[0] + seen[1]) == paths and sorted(seen[2] + seen[3]) == paths          # every epoch is a permutation
    assert next(stream.images()).shape == (4, 3, 16, 16)
    # evaluation order: sequential, no flips
    ev = image_folder.DeviceImageStream(ds, 4, training=False, device='cpu', convert=_numpy_convert)
    img, meta = next(ev)
    assert meta['paths'] == paths[:4] and not meta['flip'].any()


def test_size_intruder_is_named(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    _write_folder(tmp_path / 'ds', 8)
    bad = tmp_path / 'ds' / 'b' / 'zz_intruder.png'
    Image.fromarray(np.zeros((16, 15, 3), np.uint8), 'RGB').save(bad)          # 15 wide, 16 high
    ds = image_folder.ImageFolderU8(str(tmp_path / 'ds'))
    with pytest.raises(ValueError, match='zz_intruder.png'):
        ds[len(ds) - 1]


def test_two_ranks_see_disjoint_halves(tmp_path):
    pytest.importorskip('PIL')
    paths = _write_folder(tmp_path / 'ds', 8)
    ds = image_folder.ImageFolderU8(str(tmp_path / 'ds'))
    per_rank = []
    for rank in range(2):
        s = image_folder.DeviceImageStream(ds, 2, training=True, device='cpu', seed=11, rank=rank, world=2, convert=_numpy_convert)
        first = next(s)[1]['paths'] + next(s)[1]['paths']
        second = next(s)[1]['paths'] + next(s)[1]['paths']
        assert s.epoch == 1
        per_rank.append((first, second))
    for epoch in range(2):
        a, b = per_rank[0][epoch], per_rank[1][epoch]
        assert not set(a) & set(b) and sorted(a + b) == paths
    assert per_rank[0][0] != per_rank[0][1]          # the epoch advances the shuffle


def test_afhq_walk_and_loaders(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    root = tmp_path / 'afhq'
    want = []
    for split, names in (('train', ['d2.png', 'd0.jpg']), ('val', ['d1.png'])):
        (root / split / 'dog').mkdir(parents=True)
        (root / split / 'cat').mkdir(parents=True)
        Image.fromarray(np.zeros((16, 16, 3), np.uint8), 'RGB').save(root / split / 'cat' / 'c.png')
        for n in names:
            Image.fromarray(np.zeros((16, 16, 3), np.uint8), 'RGB').save(root / split / 'dog' / n)
            want.append(str(root / split / 'dog' / n))
    ds = image_folder.ImageFolderU8(str(root), 'afhq')
    assert ds.samples == sorted(want)
    s = image_folder.get_afhq_data_loader({'path': str(root), 'workers': 0}, batch_size=2, size=16, device='cpu', seed=1,
                                          convert=lambda u8, size=None, boxes=None, flip=None: (u8, boxes))
    (u8, boxes), meta = next(s)
    assert u8.shape == (2, 16, 16, 3) and len(boxes) == 2 and meta['boxes'] == boxes
    with pytest.raises(ValueError, match='not valid'):
        from gan_control_amd.trainers.generator_trainer import GeneratorTrainer
        GeneratorTrainer.make_data_stream(None, {'data_set_name': 'nope'})


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        image_ops.images_to_device_batch(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='uint8'):
        image_ops.images_to_device_batch(torch.zeros(1, 4, 4, 3))


def test_emulated_backend_is_refused(emu_backend):
    with pytest.raises(RuntimeError, match='HIP backend only'):
        image_ops.images_to_device_batch(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


def test_argument_validation_launches_nothing():
    """The refusals of the three entries need no GPU: they return before any launch (bad pointers are never dereferenced)."""
    from gan_control_amd import _lib
    lib = _lib.load()
    assert lib.gc_image_u8_to_f32(None, 12, 48, 1, 1, 1, 1, 4, 4, None) == -1 and b'null' in lib.gc_last_error()
    assert lib.gc_image_u8_to_f32(1, 11, 48, 1, 1, 1, 1, 4, 4, None) == -1 and b'row stride' in lib.gc_last_error()
    coeff, bounds = image_ops.resample_tables(8, 4)
    bh = np.ascontiguousarray(bounds)
    args = lambda kmax, host: (1, 24, 192, 8, 8, 1, 1, 8, 4, 0, 1, 1, host.ctypes.data, kmax, 0, None, None, None)
    assert lib.gc_image_resample_u8(*args(0, bh)) == -1 and b'kmax' in lib.gc_last_error()
    outside = bh.copy()
    outside[3, 0] += 1          # the last output's taps now end one pixel past the input
    assert lib.gc_image_resample_u8(*args(coeff.shape[1], outside)) == -1 and b'reads outside' in lib.gc_last_error()
    assert lib.gc_image_resample_u8(1, 24, 192, 8, 8, 1, 1, 8, 4, 0, 1, 1, None, 5, 0, None, None, None) == -1 and b'null' in lib.gc_last_error()
    assert lib.gc_image_resample_v_u8_to_f32(1, 24, 192, 8, 8, None, 1, 1, 1, 4, 8, 1, 1, bh.ctypes.data, 5, 0, None, None, None) == -1


def test_real_statistics_round_trip(tmp_path, monkeypatch):
    from gan_control_amd.fid_utils import fid, real_stats
    rng = np.random.default_rng(0)
    feats = torch.from_numpy(rng.standard_normal((24, 6)).astype(np.float32))

    class Stream:
        training = False

        def __init__(self):
            self.at = 0

        def __next__(self):
            img = feats[self.at:self.at + 5].reshape(-1, 6, 1, 1)
            self.at += 5
            return img, {}

    got = real_stats.extract_real_features(Stream(), lambda img: [img * 1.0], 18)
    assert torch.equal(got, feats[:18])
    train_stream = Stream()
    train_stream.training = True
    with pytest.raises(ValueError, match='training=False'):
        real_stats.extract_real_features(train_stream, lambda img: [img], 4)
    path = tmp_path / 'real.pkl'
    real_stats.save_real_statistics(str(path), got)
    with open(path, 'rb') as f:
        stored = pickle.load(f)
    ref = got.double().numpy()
    assert np.array_equal(stored['mean'], np.mean(ref, 0)) and np.array_equal(stored['cov'], np.cov(ref, rowvar=False))
    # ... and fid.evaluate_fid reads exactly this file
    monkeypatch.setattr(fid, 'sample_features', lambda *a, **k: got)

    class Gen:
        def eval(self):
            return self

    value = fid.evaluate_fid(Gen(), object(), 4, 18, 'cpu', str(path))
    assert math.isfinite(value)
