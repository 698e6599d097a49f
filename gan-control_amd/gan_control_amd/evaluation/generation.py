"""Sample grids and id x pose matrices of a generator, with the reference's names and signatures (evaluation/generation.py).

Differences from the reference, all of them on purpose:

* ``device`` defaults to the model's own device instead of a literal ``'cuda'``, and an optional ``generator`` (a ``torch.Generator``) makes
  every ``randn`` draw reproducible;
* ``gen_matrix`` runs the generator once per ROW of the matrix (``ids_in_row`` images) instead of once per image; a shared batch-1 injection
  noise is expanded along the batch as ``Inference.expend_noise`` does, so every image sees the values it saw in the reference;
* in the ``same_noise_per_id`` branch the reference indexes ``injection_noises[pic_num]``, which raises ``IndexError`` at the second row (only
  ``ids_in_row`` noises exist).  The running ``injection_num`` it keeps next to it is evidently what was meant, and what is used here;
* ``make_noise_id_pose_matrix`` draws ``max(ids_in_row, pose_in_col)`` latents, so that a matrix with more rows than columns works too (the
  reference draws ``ids_in_row`` and indexes them by row);
* the float -> byte -> grid -> resize chain runs on the images' device (evaluation/image_grid.py) and only the final bytes reach the host.
"""
import logging

import torch

from .image_grid import grid_image

_log = logging.getLogger(__name__)


def _unwrap(model):
    return getattr(model, 'module', model)


def _model_device(model):
    return next(_unwrap(model).parameters()).device


def _randn(shape, device, generator):
    if generator is None:
        return torch.randn(*shape, device=device)
    return torch.randn(*shape, device=generator.device, generator=generator).to(device)


def _make_noise(model, device, generator=None, batch_size=1):
    """Generator.make_noise, drawn from ``generator`` when one is given."""
    m = _unwrap(model)
    if generator is None:
        return m.make_noise(batch_size=batch_size, device=device)
    noises = [_randn((batch_size, 1, 4, 4), device, generator)]
    for i in range(3, m.log_size + 1):
        noises += [_randn((batch_size, 1, 2 ** i, 2 ** i), device, generator) for _ in range(2)]
    return noises


def _expand_noise(noise, batch, device):
    """Per-layer noise for a batch: a batch-1 map is repeated along the batch (Inference.expend_noise), a per-sample one is used as it is."""
    out = []
    for n in noise:
        n = n.to(device)
        if n.shape[0] == 1 and batch > 1:
            n = n.repeat(batch, 1, 1, 1)
        elif n.shape[0] != batch:
            raise ValueError('injection noise for %d samples and a batch of %d' % (n.shape[0], batch))
        out.append(n)
    return out


def gen_grid(model, latent, injection_noise=None, nrow=4, downsample=None):
    """The PIL grid of ``model([latent], noise=injection_noise)``, ``nrow`` images per row."""
    with torch.no_grad():
        output_tensor, _ = model([latent], noise=injection_noise)
    return grid_image(output_tensor, nrow=nrow, downsample=downsample)


def make_noise_id_pose_matrix(model, ids_in_row=6, pose_in_col=6, device=None, id_chunk=(256, 512), generator=None):
    """Latents of an id x pose matrix, row-major: image (row, col) carries the ``id_chunk`` slice of sample ``row`` and the rest of the latent
    of sample ``col``; plus ``ids_in_row`` (at least ``pose_in_col``) batch-1 injection noises.  -> (list of [1, latent] tensors, list of noises)."""
    device = _model_device(model) if device is None else device
    latent_size = getattr(_unwrap(model), 'style_dim', 512)
    inside = list(range(id_chunk[0], id_chunk[1]))
    outside = list(range(id_chunk[0])) + list(range(id_chunk[1], latent_size))
    n = max(ids_in_row, pose_in_col)
    samples = [_randn((1, latent_size), device, generator) for _ in range(n)]
    latents = []
    for row in range(pose_in_col):
        for col in range(ids_in_row):
            z = torch.zeros_like(samples[0])
            z[:, inside] = samples[row][:, inside]
            z[:, outside] = samples[col][:, outside]
            latents.append(z)
    noises = [_make_noise(model, device, generator) for _ in range(n)]
    return latents, noises


@torch.no_grad()
def gen_matrix(model, ids_in_row=6, pose_in_col=6, latents=None, injection_noises=None, device=None, same_noise_per_id=False, downsample=None,
               return_list=False, same_chunk=(256, 512), same_noise_for_all=False, generator=None):
    """The id x pose matrix of ``model``: ``pose_in_col`` rows of ``ids_in_row`` images, one generator call per row.

    same_noise_for_all: every image gets ``injection_noises[0]``; same_noise_per_id: every row gets the next of ``injection_noises`` (with
    both set the rows still change noise, as in the reference); neither: the model draws its own noise.  ``return_list=True`` returns the
    float images [rows * cols, 3, h, w] on the host, otherwise the PIL image of ``grid_image(total, nrow=ids_in_row, downsample=downsample)``."""
    if same_noise_per_id and same_noise_for_all:
        _log.warning('same_noise_per_id and same_noise_for_all are both set: the noise still changes with every row')
    device = _model_device(model) if device is None else torch.device(device)
    if latents is None or injection_noises is None:
        made_latents, made_noises = make_noise_id_pose_matrix(model, ids_in_row=ids_in_row, pose_in_col=pose_in_col, device='cpu',
                                                               id_chunk=same_chunk, generator=generator)
        latents = made_latents if latents is None else latents
        injection_noises = made_noises if injection_noises is None else injection_noises
    injection_noise, injection_num = None, 0
    rows = []
    for row in range(pose_in_col):
        if (row == 0 and (same_noise_per_id or same_noise_for_all)) or (row > 0 and same_noise_per_id):
            injection_noise = _expand_noise(injection_noises[injection_num], ids_in_row, device)
            injection_num += 1
        z = torch.cat([latents[row * ids_in_row + col].reshape(1, -1) for col in range(ids_in_row)], 0).to(device)
        sample, _ = model([z], noise=injection_noise)
        rows.append(sample)
    total_sample = torch.cat(rows, 0)
    if return_list:
        return total_sample.cpu()
    return grid_image(total_sample, nrow=ids_in_row, downsample=downsample)


class IterableModel:
    """A generator as a source of random batches (what the reference's histogram evaluations iterate over)."""

    def __init__(self, model, same_noise_for_same_id=False, batch_size=20):
        self.model = model
        self.same_noise_for_same_id = same_noise_for_same_id
        self.batch_size = batch_size

    def gen_random(self):
        m = _unwrap(self.model)
        random_latent = torch.randn(self.batch_size, getattr(m, 'style_dim', 512), device=_model_device(self.model))
        output, _ = self.model([random_latent], noise=None)
        return output
