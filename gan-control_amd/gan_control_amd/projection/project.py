"""Image projection: the reference's helpers (projection/projection.py: get_lr, latent_noise, make_image, get_avg_latent, merge_group_latents,
load_source_images -- same names and signatures) and ``project``, the optimisation loop they exist for.

The reference ships the helpers only; ``project`` is this package's own loop (StyleGAN2's projector: Adam over the latent and the per-layer
noise maps from the mean latent, a learning-rate ramp, latent noise that fades out, the noise regulariser, noise maps re-normalised after every
step), so nothing about it is a parity claim.  It needs the generator to be differentiable with respect to its noise maps: see
models/op/noise_grad.py.
"""
import math

import numpy as np
import torch
from torch import nn

from ..datasets import image_ops
from ..evaluation import image_grid
from .noise_ops import noise_normalize_, noise_regularize
from .pca import GroupPCA, model_places


def get_lr(t, initial_lr, rampdown=0.25, rampup=0.05):
    """initial_lr * (cosine ramp down over the last ``rampdown`` of t in [0, 1]) * (linear ramp up over the first ``rampup``)."""
    ramp = min(1, (1 - t) / rampdown)
    ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
    return initial_lr * ramp * min(1, t / rampup)


def latent_noise(latent, strength, generator=None):
    """latent + strength * N(0, 1).  ``generator`` (not in the reference) makes the draw reproducible without the global seed."""
    if generator is None:
        return latent + torch.randn_like(latent) * strength
    draw = torch.randn(latent.shape, dtype=latent.dtype, device=generator.device, generator=generator)
    return latent + draw.to(latent.device) * strength


def make_image(tensor):
    """float [B, 3, h, w] in [-1, 1] -> numpy uint8 [B, h, w, 3]: the bytes of ``to_u8_grid(x, nrow=1, padding=0)`` (one kernel launch for a
    CUDA tensor).  ``clamp(0.5 * x + 0.5, 0, 1)`` there and the reference's ``(clamp(x, -1, 1) + 1) / 2`` are the same float32 function.
    Unlike the reference, whose ``clamp_`` on a detached view clamps the caller's tensor in place, the argument is left untouched."""
    x = tensor.detach()
    b, _, h, w = x.shape
    return image_grid.to_u8_grid(x, nrow=1, padding=0).reshape(b, h, w, 3).cpu().numpy()


def get_avg_latent(model, n_mean_latent, device):
    """(mean, std) of the mapping network's output over ``n_mean_latent`` draws, as numpy: mean [style_dim], std = sqrt(sum of squared
    deviations over all coordinates / n_mean_latent), a scalar."""
    if isinstance(model, nn.DataParallel):
        model = model.module
    with torch.no_grad():
        latent_out = model.style(torch.randn(n_mean_latent, 512, device=device))
        latent_mean = latent_out.mean(0)
        latent_std = ((latent_out - latent_mean).pow(2).sum() / n_mean_latent) ** 0.5
    return latent_mean.cpu().numpy(), latent_std.cpu().numpy()


def merge_group_latents(controller, group, latent_in):
    """Replace the ``group`` slice of every sample's latent by its mean over dim 1, in place.  ``controller``: any object with
    ``get_group_w_latent(latent, group)`` and ``insert_group_w_latent(latent, group_latent, group)``."""
    group_latent = controller.get_group_w_latent(latent_in.data, group)
    controller.insert_group_w_latent(latent_in.data, group_latent.data.mean(dim=1).unsqueeze(1), group)


def load_source_images(images, res=256, device=None):
    """Image files -> float32 [N, 3, res, res] in [-1, 1]: RGB decode, the shorter side resized to ``res`` (PIL bilinear), centre crop,
    then byte -> float by the table of the input pipeline (ToTensor + Normalize(0.5, 0.5)).  device: where the result lives; a CUDA device
    takes gc_image_u8_to_f32 for the last step."""
    from PIL import Image
    batch = []
    for name in images:
        img = Image.open(name).convert('RGB')
        w, h = img.size
        if (w <= h and w != res) or (h <= w and h != res):
            size = (res, int(res * h / w)) if w <= h else (int(res * w / h), res)
            img = img.resize(size, Image.BILINEAR)
        w, h = img.size
        left, top = int(round((w - res) / 2.0)), int(round((h - res) / 2.0))
        batch.append(np.asarray(img.crop((left, top, left + res, top + res)), dtype=np.uint8))
    u8 = torch.from_numpy(np.stack(batch))
    if device is not None and torch.device(device).type == 'cuda':
        return image_ops.u8_to_f32(u8.to(device))
    return image_ops.normalize_table()[u8.long()].permute(0, 3, 1, 2).contiguous()


def project(model, target, /, *, steps=1000, lr=0.1, noise=0.05, noise_ramp=0.75, noise_regularize_weight=1e5, mse_weight=0.0, percept=None,
            w_plus=False, n_mean_latent=10000, optimize_noise=True, generator=None, on_step=None, pca=None):
    """Optimise a latent and the per-layer noise maps until ``model`` (a Generator; positional) reproduces ``target`` [B, 3, size, size].

    Every step i of ``steps`` (t = i / steps): Adam's learning rate is ``get_lr(t, lr)``; the latent is perturbed by ``latent_noise`` of
    strength ``latent_std * noise * max(0, 1 - t / noise_ramp) ** 2``; the loss is ``percept(img, target).sum() + noise_regularize_weight *
    noise_regularize(noises) + mse_weight * mse(img, target)``; after the optimiser step the maps are re-normalised (``noise_normalize_``).
    percept: any callable (img, target) -> tensor (an LPIPS network stays external); None with mse_weight == 0 is an error.  w_plus: one
    latent per layer.  optimize_noise=False keeps the drawn maps fixed.  generator: a torch.Generator for every draw made here.
    on_step(i, info): called after each step with the tensors of that step (loss, mse, percept, noise_loss, lr, latent, noises).
    pca: None, a ``GroupPCA`` (projection/pca.py) or a float variance share -- then a ``GroupPCA`` is fitted on the ``n_mean_latent`` draws
    made here, over the groups of the model's fc_config when the mapping network is split and over the whole row otherwise.  When given,
    ``pca.project_(latent)`` keeps the latent in the retained per-group subspaces after every optimiser step (before the noise maps are
    re-normalised), so the returned latent is projected.  ``pca=None`` launches exactly what the loop launched before the option existed.

    The model's parameters get requires_grad_(False) for the duration and their flags back afterwards.
    -> (latent, noises, image, history): the optimised latent [B, style_dim] ([B, n_latent, style_dim] with w_plus), the noise maps, the
    image they give without latent noise, and one dict of floats per step."""
    if percept is None and not mse_weight:
        raise ValueError('project: percept is None and mse_weight is 0: there is nothing to optimise')
    if target.dim() != 4 or target.shape[1] != 3:
        raise ValueError('project: target must be [B, 3, size, size], got %s' % (tuple(target.shape),))
    dev, batch = target.device, target.shape[0]
    rng_dev = generator.device if generator is not None else dev

    def randn(*shape):
        return torch.randn(*shape, device=rng_dev, generator=generator).to(dev)

    params = list(model.parameters())
    flags = [p.requires_grad for p in params]
    try:
        for p in params:
            p.requires_grad_(False)
        with torch.no_grad():
            latent_out = model.style(randn(n_mean_latent, model.style_dim))
            latent_mean = latent_out.mean(0)
            latent_std = ((latent_out - latent_mean).pow(2).sum() / n_mean_latent) ** 0.5
            noises = [randn(*n.shape) for n in model.make_noise(batch, device=dev)]
            if pca is not None and not isinstance(pca, GroupPCA):
                pca = GroupPCA.fit(latent_out, model_places(model), float(pca))
        if pca is not None and pca.mean.device != latent_out.device:
            raise ValueError('project: the GroupPCA lives on %s, the latent on %s; fit it on the target\'s device' % (pca.mean.device, latent_out.device))
        latent_in = latent_mean.detach().clone().unsqueeze(0).repeat(batch, 1)
        if w_plus:
            latent_in = latent_in.unsqueeze(1).repeat(1, model.n_latent, 1)
        latent_in.requires_grad_(True)
        for n in noises:
            n.requires_grad_(bool(optimize_noise))
        optimizer = torch.optim.Adam([latent_in] + (noises if optimize_noise else []), lr=lr)
        zero = torch.zeros((), device=dev)
        records = []
        for i in range(steps):
            t = i / steps
            step_lr = get_lr(t, lr)
            optimizer.param_groups[0]['lr'] = step_lr
            strength = latent_std * noise * max(0, 1 - t / noise_ramp) ** 2
            img, _ = model([latent_noise(latent_in, strength, generator)], input_is_latent=True, noise=noises)
            p_loss = percept(img, target).sum() if percept is not None else zero
            n_loss = noise_regularize(noises) if optimize_noise else zero
            mse = (img - target).pow(2).mean()
            loss = p_loss + noise_regularize_weight * n_loss + mse_weight * mse
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            if pca is not None:
                pca.project_(latent_in)
            if optimize_noise:
                noise_normalize_(noises)
            rec = {'loss': loss.detach(), 'mse': mse.detach(), 'percept': p_loss.detach(), 'noise_loss': n_loss.detach(), 'lr': step_lr}
            records.append(rec)
            if on_step is not None:
                on_step(i, dict(rec, latent=latent_in, noises=noises))
        with torch.no_grad():
            image, _ = model([latent_in], input_is_latent=True, noise=noises)
        history = [{k: float(v) for k, v in rec.items()} for rec in records]          # one trip to the host, at the end
        return latent_in.detach(), [n.detach() for n in noises], image, history
    finally:
        for p, flag in zip(params, flags):
            p.requires_grad_(flag)
