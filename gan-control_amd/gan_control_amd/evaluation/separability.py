"""Separability of a controllable generator (the reference's evaluation/separability.py): how far images that share a sub-latent sit from
images that do not, in a predictor's feature space.

``num_of_samples`` latents are drawn; every odd row copies the ``same_chunk`` columns of the even row before it, so rows (2i, 2i + 1) share
the attribute (and, with ``same_noise_for_same_id``, the injection noise).  The images are generated in batches of 20 under ``no_grad``,
their predictor features regrouped as the reference does -- the even half, then the odd half -- and ``LossModelClass.calc_same_not_same_list``
splits the all-pairs distances of the two halves (pids ``range(n / 2)`` on both sides) into 'same', 'not_same' (per query the closest
signature of another pid) and 'all_not_same'.

Additions to and deviations from the reference, all on purpose:

* ``seed=None``: with a seed the latents and the injection noise come from one ``torch.Generator``, so a run is reproducible;
* the features stay on the generator's device instead of going to the host after every batch, and with ``last_layer_separability_only`` the
  levels that calc_same_not_same_list would skip are dropped as they are produced (layer 1 of ArcFace is 1.6 GB per 2000 samples, held
  for nothing).  The dropped levels come back as ``None`` in the list ``compute_half_same_ids_embeddings_from_generator`` returns;
* with ``return_images`` the images are kept as uint8 [h, w, 3] arrays of at most 256 x 256 each (evaluation.image_grid: the reference's
  quantisation, PIL's bilinear downsample), even half then odd half, not as full-size PIL images;
* with ``save_path`` one ``<save_path>_layer_<i>.json`` per level takes the place of the matplotlib histogram: for 'same',
  'not_same_2nd_best' and 'all_not_same' the count, the mean, the 0.2 / 0.5 / 0.8 percentiles that ``plot_hist`` marks, and a 100-bin
  histogram over the common range of the three;
* no DataParallel wrapper, and a generator batch of ``num_of_samples`` when fewer than 20 samples are asked for (the reference divides by
  zero there); ``num_of_samples`` must be even.
"""
import json
import logging

import numpy as np
import torch

from . import image_grid
from .generation import _make_noise, _model_device, _randn

_log = logging.getLogger(__name__)

BATCH = 20
MAX_IMAGE = 256
LABELS = ('same', 'not_same_2nd_best', 'all_not_same')


def re_arrange_inject_noise(noises):
    """In place: every odd sample of every layer's noise becomes a copy of the even sample before it."""
    for j in range(len(noises)):
        noises[j][1::2] = noises[j][0:noises[j].shape[0] - noises[j].shape[0] % 2:2].detach()
    return noises


def _u8_images(images):
    """float [B, 3, h, w] -> list of uint8 [h', w', 3] host arrays, h', w' <= 256 (one grid_image per sample: a bare image, no padding)."""
    b, _, h, w = images.shape
    down = max(1, -(-max(h, w) // MAX_IMAGE))
    return [np.asarray(image_grid.grid_image(images[i:i + 1], nrow=1, downsample=down if down > 1 else None)) for i in range(b)]


def compute_half_same_ids_embeddings_from_generator(generator, loss_model_class, num_of_samples, same_noise_for_same_id=False, return_images=False,
                                                    same_chunk=(256, 512), seed=None, last_layer_separability_only=False):
    """-> (features per level [num_of_samples, ...] on the generator's device: rows 0 .. n/2 the even samples, the rest the odd ones; images).
    See the module docstring."""
    if num_of_samples < 2 or num_of_samples % 2:
        raise ValueError('separability needs an even number of samples (pairs that share the sub-latent), got %d' % num_of_samples)
    device = _model_device(generator)
    gen = None if seed is None else torch.Generator().manual_seed(int(seed))
    latent_size = getattr(getattr(generator, 'module', generator), 'style_dim', 512)
    latents = _randn((num_of_samples, latent_size), 'cpu', gen)
    latents[1::2, same_chunk[0]:same_chunk[1]] = latents[0::2, same_chunk[0]:same_chunk[1]]
    levels, images_list = None, []
    with torch.no_grad():
        for at in range(0, num_of_samples, BATCH):
            z = latents[at:at + BATCH].to(device)
            inject_noise = None
            if same_noise_for_same_id:
                inject_noise = re_arrange_inject_noise(_make_noise(generator, device, gen, batch_size=z.shape[0]))
            fake_images, _ = generator([z], noise=inject_noise)
            if return_images:
                images_list += _u8_images(fake_images)
            features = list(loss_model_class.calc_features(fake_images))
            if last_layer_separability_only:
                features = [None] * (len(features) - 1) + features[-1:]
            if levels is None:
                levels = [[] for _ in features]
            for level, f in zip(levels, features):
                level.append(f)
    _log.info('extracted %d embeddings', num_of_samples)
    embeddings = []
    for level in levels:
        if level[0] is None:
            embeddings.append(None)
            continue
        f = torch.cat(level, dim=0)
        embeddings.append(torch.cat([f[0::2], f[1::2]], dim=0))
    if return_images:
        images_list = images_list[0::2] + images_list[1::2]
    return embeddings, images_list


def summarize(arrays, bins=100, percentiles=(0.2, 0.5, 0.8)):
    """What the reference's plot_hist draws, as numbers: per array count / mean / percentiles, and ``bins``-bin histograms over the common range."""
    arrays = [np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays]
    lo = min(float(a.min()) for a in arrays if a.size)
    hi = max(float(a.max()) for a in arrays if a.size)
    if hi <= lo:
        hi = lo + 1.0
    out = {'range': [lo, hi], 'bins': int(bins)}
    for label, a in zip(LABELS, arrays):
        hist, _ = np.histogram(a, bins=bins, range=(lo, hi))
        out[label] = {'count': int(a.size), 'mean': float(a.mean()) if a.size else None,
                      'percentiles': {str(p): (float(np.quantile(a, p)) if a.size else None) for p in percentiles},
                      'hist': [int(v) for v in hist]}
    return out


def calc_separability(generator, loss_model_class, same_noise_for_same_id=False, num_of_samples=2000, save_path=None, title=None, return_images=False,
                      same_chunk=(256, 512), last_layer_separability_only=False, seed=None):
    """-> (same_not_same_list, images_list): the reference's calc_separability (separability.py:75-119) on device features."""
    embeddings, images_list = compute_half_same_ids_embeddings_from_generator(
        generator, loss_model_class, num_of_samples, same_noise_for_same_id=same_noise_for_same_id, return_images=return_images,
        same_chunk=same_chunk, seed=seed, last_layer_separability_only=last_layer_separability_only)
    half = num_of_samples // 2
    signatures_embs = [None if e is None else e[:half] for e in embeddings]
    queries_embs = [None if e is None else e[half:] for e in embeddings]
    pids = np.arange(half)
    same_not_same_list = loss_model_class.calc_same_not_same_list(signatures_embs, queries_embs, pids, pids.copy(),
                                                                  last_layer_separability_only=last_layer_separability_only)
    if save_path is not None:
        for i, level in enumerate(same_not_same_list):
            summary = summarize([level['same'], level['not_same'], level['all_not_same']])
            summary['title'] = None if title is None else '%s layer %d' % (title, i)
            with open('%s_layer_%d.json' % (save_path, i), 'w') as f:
                json.dump(summary, f)
    return same_not_same_list, images_list
