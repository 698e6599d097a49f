"""Real images for the training loop: folders of image files -> an endless stream of float32 [B, 3, size, size] batches on the device.

The reference's loaders (ffhq_dataset.py:56-79, afhq_dataset.py:50-72, metfaces_dataset.py:48-70) decode AND transform in DataLoader workers and
move float32 batches to the device.  Here the decode is PIL in workers and everything after it is HIP: a worker hands over the decoded
``uint8 [H, W, 3]``, the collated ``uint8 [B, H, W, 3]`` crosses to the device through pinned memory (a quarter of the float32 bytes), and
``image_ops.images_to_device_batch`` resizes, crops, flips and normalises there with the bits of the reference's chain.  The random decisions
of the chain (flip, AFHQ's random resized crop) are drawn per sample on the host from one seeded generator and passed along as arguments.
"""
import math
import os

import numpy as np
import torch
from torch.utils import data

from . import image_ops

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')          # what torchvision's ImageFolder accepts
AFHQ_EXTENSIONS = ('.png', '.jpg', '.jpeg', '.JPG')          # afhq_dataset.py:25-28 (case-sensitive there too)


def _class_walk(root):
    """Files in ImageFolder's order: class directories sorted, each walked top-down with sorted names."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError('no class directories under %s' % root)
    out = []
    for cls in classes:
        for base, _, names in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
            out += [os.path.join(base, n) for n in sorted(names) if n.lower().endswith(EXTENSIONS)]
    return out


def _afhq_walk(root):
    """train/dog and val/dog, every file with one of the four suffixes, sorted as one list (afhq_dataset.py:31-36)."""
    out = []
    for split in ('train', 'val'):
        for base, _, names in os.walk(os.path.join(root, split, 'dog')):
            out += [os.path.join(base, n) for n in names if n.endswith(AFHQ_EXTENSIONS)]
    return sorted(out)


class ImageFolderU8(data.Dataset):
    """item -> (uint8 [H, W, 3] tensor, path): PIL decode and convert('RGB'), nothing else.  pattern: 'classes' (the sorted class-directory
    walk of ImageFolder: FFHQ, MetFaces) or 'afhq'.  Every image must have the size of the first one."""

    def __init__(self, root, pattern='classes'):
        if pattern not in ('classes', 'afhq'):
            raise ValueError("pattern must be 'classes' or 'afhq', got %r" % (pattern,))
        self.root, self.pattern = root, pattern
        self.samples = _class_walk(root) if pattern == 'classes' else _afhq_walk(root)
        if not self.samples:
            raise FileNotFoundError('no image files under %s' % root)
        from PIL import Image
        with Image.open(self.samples[0]) as im:
            self.width, self.height = im.size

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        from PIL import Image
        path = self.samples[index]
        with Image.open(path) as im:
            if im.size != (self.width, self.height):
                raise ValueError('%s is %d x %d; every image of this data set must be %d x %d like %s'
                                 % (path, im.size[0], im.size[1], self.width, self.height, self.samples[0]))
            arr = np.array(im.convert('RGB'), dtype=np.uint8)
        return torch.from_numpy(arr), path


# ---- the random resized crop of AFHQ (afhq_dataset.py:51-52), as integer boxes ---------------------------------------------------------
def _uniform(gen, lo, hi):
    return lo + (hi - lo) * float(torch.rand((), generator=gen, dtype=torch.float64))


def random_resized_box(height, width, gen, scale=(0.8, 1.0), ratio=(0.9, 1.1)):
    """(left, top, right, bottom): area fraction uniform in ``scale``, aspect ratio (w / h) log-uniform in ``ratio``, placed uniformly; up to ten
    attempts for a box that fits, then the centred box of the nearest allowed aspect."""
    area = height * width
    for _ in range(10):
        target = area * _uniform(gen, scale[0], scale[1])
        aspect = math.exp(_uniform(gen, math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < w <= width and 0 < h <= height:
            top = int(torch.randint(0, height - h + 1, (), generator=gen))
            left = int(torch.randint(0, width - w + 1, (), generator=gen))
            return left, top, left + w, top + h
    w, h = width, height
    if width / height < min(ratio):
        h = int(round(width / min(ratio)))
    elif width / height > max(ratio):
        w = int(round(height * max(ratio)))
    top, left = (height - h) // 2, (width - w) // 2
    return left, top, left + w, top + h


def sample_boxes(batch, height, width, gen, prob=0.5):
    """Per sample: with probability ``prob`` a random resized box, else the full image."""
    return [random_resized_box(height, width, gen) if float(torch.rand((), generator=gen)) < prob else (0, 0, width, height)
            for _ in range(batch)]


class DeviceImageStream:
    """Endless iterator over ``(real_img, meta)``: real_img float32 [B, 3, size, size] on ``device``, meta = {'paths', 'flip', 'boxes'}.

    On a GPU the next batch is always in flight: its pinned uint8 copy, the H2D transfer and the kernels are issued on a side stream
    before the current batch is handed over, so they overlap the training step that consumes it.  Ordering is by events only: the consumer's
    stream waits on the event recorded behind the producer's kernels, and the batch is marked as used on the consumer's stream.
    """

    def __init__(self, dataset, batch_size, size=None, training=True, device='cuda', seed=0, rank=0, world=1, num_workers=0,
                 crop_prob=0.0, convert=None, prefetch=True):
        self.dataset, self.batch_size, self.size, self.training = dataset, batch_size, size, training
        self.device = torch.device(device)
        self.crop_prob = crop_prob if training else 0.0
        self.convert = image_ops.images_to_device_batch if convert is None else convert
        self.prefetch = prefetch
        self.gen = torch.Generator().manual_seed(seed + rank)          # flips and crop boxes
        if world == 1:
            order = torch.Generator().manual_seed(seed)
            self.sampler = data.RandomSampler(dataset, generator=order) if training else data.SequentialSampler(dataset)
        else:
            self.sampler = data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=training, seed=seed)
        if len(self.sampler) < batch_size:
            raise ValueError('%d images for this rank cannot fill a batch of %d (drop_last)' % (len(self.sampler), batch_size))
        self.loader = data.DataLoader(dataset, batch_size=batch_size, sampler=self.sampler, drop_last=True, num_workers=num_workers)
        self.epoch = 0
        self._host = self._host_batches()
        self._on_gpu = self.device.type == 'cuda'
        self._side = None
        self._pending = None

    def _host_batches(self):
        while True:
            if hasattr(self.sampler, 'set_epoch'):
                self.sampler.set_epoch(self.epoch)
            for batch in self.loader:
                yield batch
            self.epoch += 1

    def _draw(self, batch, height, width):
        flip = (torch.rand(batch, generator=self.gen) < 0.5).to(torch.int32) if self.training else torch.zeros(batch, dtype=torch.int32)
        boxes = sample_boxes(batch, height, width, self.gen, self.crop_prob) if self.crop_prob > 0 else None
        return flip, boxes

    def _produce(self):
        u8, paths = next(self._host)
        flip, boxes = self._draw(u8.shape[0], u8.shape[1], u8.shape[2])
        meta = {'paths': list(paths), 'flip': flip, 'boxes': boxes}
        if not self._on_gpu:
            return self.convert(u8, size=self.size, boxes=boxes, flip=flip), meta, None
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        with torch.cuda.stream(self._side):
            # pinned blocks come from the caching host allocator, which hands one out again only after the copy that read it has finished
            dev_u8 = u8.pin_memory().to(self.device, non_blocking=True)
            img = self.convert(dev_u8, size=self.size, boxes=boxes, flip=flip)
            ready = torch.cuda.Event()
            ready.record(self._side)
        return img, meta, ready

    def __iter__(self):
        return self

    def __next__(self):
        if self._pending is None:
            self._pending = self._produce()
        img, meta, ready = self._pending
        self._pending = self._produce() if (self.prefetch and self._on_gpu) else None          # batch n + 1 is issued before batch n is used
        if ready is not None:
            consumer = torch.cuda.current_stream(self.device)
            consumer.wait_event(ready)
            img.record_stream(consumer)
        return img, meta

    def images(self):
        """The batches alone: what ``GeneratorTrainer.train(data=...)`` takes."""
        while True:
            yield next(self)[0]


def _stream(data_config, pattern, batch_size, size, training, device, seed, rank, world, crop_prob=0.0, square=False, **kw):
    ds = ImageFolderU8(data_config['path'], pattern)
    if square and ds.width != ds.height:
        raise ValueError('%s: %d x %d images; Resize(%d) keeps the aspect ratio and only square batches are supported' % (data_config['path'], ds.width, ds.height, size))
    workers = min(int(data_config.get('workers', 0)), 8)          # decode only; the workers never touch the GPU
    return DeviceImageStream(ds, batch_size, size=size, training=training, device=device, seed=seed, rank=rank, world=world,
                             num_workers=workers, crop_prob=crop_prob, **kw)


def get_ffhq_data_loader(data_config, batch_size=4, size=1024, training=True, device='cuda', seed=0, rank=0, world=1, **kw):
    """ffhq_dataset.py:56-79: Resize(size) where the images are not that size already, flip when training."""
    return _stream(data_config, 'classes', batch_size, size, training, device, seed, rank, world, square=True, **kw)


def get_afhq_data_loader(data_config, batch_size=4, size=512, training=True, device='cuda', seed=0, rank=0, world=1, prob=0.5, **kw):
    """afhq_dataset.py:50-72: when training, a random resized crop with probability ``prob`` per image; Resize([size, size]); flip."""
    return _stream(data_config, 'afhq', batch_size, size, training, device, seed, rank, world, crop_prob=prob, **kw)


def get_metfaces_data_loader(data_config, batch_size=4, size=512, training=True, device='cuda', seed=0, rank=0, world=1, **kw):
    """metfaces_dataset.py:48-70: Resize([size, size]), flip when training."""
    return _stream(data_config, 'classes', batch_size, size, training, device, seed, rank, world, **kw)
