"""Generation from a trained model directory (reference: inference/inference.py::Inference, same names and argument lists).

A model directory holds ``args.json`` (``model_config`` / ``training_config``) and ``checkpoint/<iter>.pt`` with the key ``g_ema``;
``trainers.utils.save_args`` and the trainers' checkpoints write that layout.  Differences from the reference ("Inference API"):
``device=None`` picks CUDA when there is one, else the CPU; there is no DataParallel wrapper, ``.model`` is the Generator; z -> w is ONE
``fc_stacks_forward`` call (models/op/fc_stack.py) and the generator then runs on ``[latent_w]`` with ``input_is_latent=True``.
"""
import json
import os

import torch
from torch import nn

from ..models.gan_model import Generator, MultiFcStack, PixelNorm
from ..models.op.fc_stack import fc_stacks_forward
from ..utils.mini_batch_utils import MiniBatchUtils


class Config:
    """args.json as an object: every top-level key an attribute (``model_config``, ``training_config``, ...)."""

    def __init__(self, fields):
        self.__dict__.update(fields)


def read_config(path):
    with open(path) as f:
        return Config(json.load(f))


def last_checkpoint(directory):
    """(path, iteration string) of the last file under ``directory``/checkpoint in sorted order."""
    folder = os.path.join(directory, 'checkpoint')
    names = sorted(os.listdir(folder))
    if not names:
        raise FileNotFoundError('no checkpoint under %s' % folder)
    return os.path.join(folder, names[-1]), names[-1].split('.')[0]


def pick_device(device):
    if device is not None:
        return torch.device(device)
    return torch.device('cuda' if torch.cuda.is_available() else 'cpu')


class Inference:
    def __init__(self, model_dir, device=None):
        self.device = pick_device(device)
        self.model_dir = model_dir
        self.model, self.batch_utils, self.config, self.ckpt_iter = self.retrieve_model(model_dir, self.device)
        self.noise = None
        self.reset_noise()
        self.mean_w_latent = None
        self.mean_w_latents = None

    def _dtype(self):
        return self.model.input.input.dtype          # what latents and noise maps are drawn in (float32 unless the model was converted)

    # -- w space ----------------------------------------------------------------------------------------------------------------------
    def style(self, latent_z):
        """``model.style(latent_z)`` as one ``fc_stacks_forward`` call: every group's mapping stack reads its slice of z and writes its
        slice of w (no cat); the plain 512-wide stack of a vanilla model is one stack over whole rows."""
        style = self.model.style
        if isinstance(style, MultiFcStack):
            names = style.fc_config.in_order_group_names
            stacks = [getattr(style, n) for n in names]
            slices = [tuple(style.fc_config.groups[n]['latent_place']) for n in names]
        elif isinstance(style, nn.Sequential) and len(style) > 1 and isinstance(style[0], PixelNorm):
            stacks, slices = [style], [None]
        else:
            return style(latent_z)                     # marge_fc: two stages, left to the modules
        latent_w = torch.empty(latent_z.shape[0], self.model.style_dim, dtype=latent_z.dtype, device=latent_z.device)
        return fc_stacks_forward(stacks, latent_z, slices, latent_w, slices)

    def _places(self):
        """{group: (lo, hi)} of the w latent; a vanilla model is one nameless group over the whole row."""
        if self.batch_utils is None:
            return {None: (0, self.model.style_dim)}
        return {k: tuple(v) for k, v in self.batch_utils.place_in_latent_dict.items()}

    @torch.no_grad()
    def calc_mean_w_latents(self, n_rounds=100, n_per_round=1000):
        """mean_w_latent: the mean over ``n_rounds`` of the per-round mean w of ``n_per_round`` normal draws; mean_w_latents: its group slices."""
        size = self.config.model_config['latent_size']
        means = []
        for _ in range(n_rounds):
            latent_w = self.style(torch.randn(n_per_round, size, device=self.device, dtype=self._dtype())).cpu()
            means.append(latent_w.mean(dim=0).unsqueeze(0))
        self.mean_w_latent = torch.cat(means, dim=0).mean(0)
        self.mean_w_latents = {key: self.mean_w_latent[lo:hi] for key, (lo, hi) in self._places().items()}

    # -- noise ------------------------------------------------------------------------------------------------------------------------
    def reset_noise(self):
        self.noise = [n.to(self._dtype()) for n in self.model.make_noise(device=self.device)]

    @staticmethod
    def expend_noise(noise, batch_size):
        """Every [1, 1, h, w] map repeated ``batch_size`` times along dim 0 (the reference's spelling of the name is kept)."""
        return [torch.cat([n.clone() for _ in range(batch_size)], dim=0) for n in noise]

    # -- generation -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def gen_batch(self, batch_size=1, normalize=True, latent=None, input_is_latent=False, static_noise=True, truncation=1, **kwargs):
        """-> (images, latent, latents): ``latent`` is the z that was drawn or given -- the w that entered the generator when a w was given
        or truncation applied -- and ``latents`` the [B, n_latent, 512] tensor the generator returns.  kwargs: ``group='random'`` with a
        given w latent redraws that group's slice.  The caller's tensor is never written."""
        if truncation < 1 and self.mean_w_latents is None:
            self.calc_mean_w_latents()
        size = self.config.model_config['latent_size']
        if latent is None:
            latent = torch.randn(batch_size, size, device=self.device, dtype=self._dtype())
        elif input_is_latent:
            latent = latent.to(self.device)
            for group_key, value in kwargs.items():
                self.check_valid_group(group_key)
                if isinstance(value, str) and value == 'random':
                    lo, hi = self.batch_utils.place_in_latent_dict[group_key]
                    drawn = self.style(torch.randn(latent.shape[0], size, device=self.device, dtype=self._dtype()))
                    latent = latent.clone()
                    latent[..., lo:hi] = drawn[:, lo:hi] if latent.ndim == 2 else drawn[:, None, lo:hi]
        else:
            latent = latent.to(self.device)
        injection_noise = None
        if static_noise:
            self.reset_noise()
            injection_noise = self.noise           # [1, 1, h, w] maps: StyledConv broadcasts them over the batch, bit for bit expend_noise
        latent_w = latent if input_is_latent else self.style(latent)
        if truncation < 1:
            latent_w = latent_w.clone() if input_is_latent else latent_w
            for key, (lo, hi) in self._places().items():
                mean = self.mean_w_latents[key].to(latent_w.device, latent_w.dtype)
                latent_w[..., lo:hi] = truncation * (latent_w[..., lo:hi] - mean) + mean
            latent = latent_w
        tensor, latents = self.model([latent_w], return_latents=True, input_is_latent=True, noise=injection_noise)
        if normalize:
            tensor = tensor.mul(0.5).add(0.5).clamp(min=0., max=1.).cpu()
        return tensor, latent, latents

    def check_valid_group(self, group):
        names = [] if self.batch_utils is None else self.batch_utils.sub_group_names
        if group not in names:
            raise ValueError('group: %s not in valid group names for this model\nValid group names are:\n%s' % (group, str(names)))

    @staticmethod
    def make_resized_grid_image(image_tensors, resize=None, nrow=8):
        """The PIL grid of images in [0, 1] (what ``normalize=True`` returns), ``nrow`` per row; ``resize``: an int (the shorter side) or
        (h, w), PIL bilinear.  Built on evaluation.image_grid.grid_image, which takes [-1, 1]."""
        from PIL import Image
        from ..evaluation.image_grid import grid_image
        image = grid_image(torch.as_tensor(image_tensors).float() * 2 - 1, nrow)
        if resize is not None:
            w, h = image.size
            if isinstance(resize, int):
                short = min(w, h)
                size = (resize, int(resize * h / w)) if w == short else (int(resize * w / h), resize)
            else:
                size = (int(resize[1]), int(resize[0]))
            image = image.resize(size, Image.BILINEAR)
        return image

    @staticmethod
    def retrieve_model(model_dir, device=None):
        """-> (Generator in eval mode on ``device``, MiniBatchUtils or None for a vanilla model, config, iteration string)."""
        device = pick_device(device)
        config = read_config(os.path.join(model_dir, 'args.json'))
        ckpt_path, ckpt_iter = last_checkpoint(model_dir)
        ckpt = torch.load(ckpt_path, map_location='cpu')
        mc = config.model_config
        batch_utils = None
        if not mc['vanilla']:
            tc = config.training_config
            batch_utils = MiniBatchUtils(tc['mini_batch'], tc['sub_groups_dict'], total_batch=tc['batch'])
        model = Generator(mc['size'], mc['latent_size'], mc['n_mlp'], channel_multiplier=mc['channel_multiplier'],
                          out_channels=mc['img_channels'], split_fc=mc['split_fc'],
                          fc_config=None if mc['vanilla'] else batch_utils.get_fc_config(),
                          conv_transpose=mc['conv_transpose'], noise_mode=mc['g_noise_mode'])
        model.load_state_dict(ckpt['g_ema'])
        return model.to(device).eval(), batch_utils, config, ckpt_iter
