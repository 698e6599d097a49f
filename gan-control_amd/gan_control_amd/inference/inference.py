"""Generation from a trained model directory (reference: inference/inference.py::Inference, same names and argument lists).

A model directory holds ``args.json`` (``model_config`` / ``training_config``) and ``checkpoint/<iter>.pt`` with the key ``g_ema``;
``trainers.utils.save_args`` and the trainers' checkpoints write that layout.  Differences from the reference ("Inference API"):
``device=None`` picks CUDA when there is one, else the CPU; there is no DataParallel wrapper, ``.model`` is the Generator; z -> w is ONE
``fc_stacks_forward`` call (models/op/fc_stack.py) and the generator then runs on ``[latent_w]`` with ``input_is_latent=True``.

The group matrices and interpolation films of the reference's second ``Inference`` class (evaluation/inference_class.py:115-212) are methods
of this one: ``generate_matrix_by_group``, ``interpolate_by_group``, ``slerp``, ``gen_grid_image_from_latent``, ``make_interpolation_gif``,
``create_gif``; the blends of a film run on the kernels of models/op/interp.py.
"""
import json
import os

import numpy as np
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
    def style(self, latent_z, out=None):
        """``model.style(latent_z)`` as one ``fc_stacks_forward`` call: every group's mapping stack reads its slice of z and writes its
        slice of w (no cat); the plain 512-wide stack of a vanilla model is one stack over whole rows.  ``out``: a [B, style_dim] tensor
        (rows of adjacent elements, e.g. a row range of a larger buffer) to write w into; it is returned."""
        style = self.model.style
        if isinstance(style, MultiFcStack):
            names = style.fc_config.in_order_group_names
            stacks = [getattr(style, n) for n in names]
            slices = [tuple(style.fc_config.groups[n]['latent_place']) for n in names]
        elif isinstance(style, nn.Sequential) and len(style) > 1 and isinstance(style[0], PixelNorm):
            stacks, slices = [style], [None]
        else:
            w = style(latent_z)                        # marge_fc: two stages, left to the modules
            return w if out is None else out.copy_(w)
        latent_w = out if out is not None else torch.empty(latent_z.shape[0], self.model.style_dim, dtype=latent_z.dtype, device=latent_z.device)
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
    def reset_noise(self, generator=None):
        """Fresh [1, 1, h, w] noise maps; drawn from ``generator`` (a ``torch.Generator``) when one is given."""
        if generator is None:
            self.noise = [n.to(self._dtype()) for n in self.model.make_noise(device=self.device)]
        else:
            from ..evaluation.generation import _make_noise
            self.noise = [n.to(self._dtype()) for n in _make_noise(self.model, self.device, generator)]

    @staticmethod
    def expend_noise(noise, batch_size):
        """Every [1, 1, h, w] map repeated ``batch_size`` times along dim 0 (the reference's spelling of the name is kept)."""
        return [torch.cat([n.clone() for _ in range(batch_size)], dim=0) for n in noise]

    # -- generation -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def gen_batch(self, batch_size=1, normalize=True, latent=None, input_is_latent=False, static_noise=True, truncation=1, generator=None,
                  **kwargs):
        """-> (images, latent, latents): ``latent`` is the z that was drawn or given -- the w that entered the generator when a w was given
        or truncation applied -- and ``latents`` the [B, n_latent, 512] tensor the generator returns.  kwargs: ``group='random'`` with a
        given w latent redraws that group's slice.  The caller's tensor is never written.  ``generator``: a ``torch.Generator`` the drawn
        latent and the static noise maps come from, which makes a call repeatable (as in ``interpolate_by_group``)."""
        if truncation < 1 and self.mean_w_latents is None:
            self.calc_mean_w_latents()
        size = self.config.model_config['latent_size']
        if latent is None:
            latent = torch.randn(batch_size, size, device=self.device, dtype=self._dtype()) if generator is None else \
                torch.randn(batch_size, size, device=generator.device, generator=generator).to(self.device, self._dtype())
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
            self.reset_noise(generator)
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

    # -- group matrices and interpolation films (reference: evaluation/inference_class.py:115-212) ----------------------------------------
    @staticmethod
    def slerp(val, low, high):
        """Spherical interpolation of the rows of ``low`` and ``high`` at ``val`` in [0, 1], the reference's formula (nothing is clamped)."""
        low_norm = low / torch.norm(low, dim=1, keepdim=True)
        high_norm = high / torch.norm(high, dim=1, keepdim=True)
        omega = torch.acos((low_norm * high_norm).sum(1))
        so = torch.sin(omega)
        return (torch.sin((1.0 - val) * omega) / so).unsqueeze(1) * low + (torch.sin(val * omega) / so).unsqueeze(1) * high

    def gen_grid_image_from_latent(self, latent, noise=None, nrow=4, downsample=None, input_is_latent=False):
        """The PIL grid of ``self.model([latent], noise=noise)`` (a z latent; a w latent with ``input_is_latent=True``), ``nrow`` images per
        row."""
        from ..evaluation.image_grid import grid_image
        with torch.no_grad():
            sample, _ = self.model([latent.to(self.device)], noise=noise, input_is_latent=input_is_latent)
        return grid_image(sample, nrow=nrow, downsample=downsample)

    @torch.no_grad()
    def generate_matrix_by_pca(self, group, pca, n_components=6, sigmas=(-2, -1, 0, 1, 2), latent=None, save_path=None, downsample=None,
                               generator=None):
        """The per-group traversal picture of a ``GroupPCA`` (projection/pca.py): image (k, c) renders the w latent with ``group``'s slice
        moved by ``sigmas[c] * sqrt(explained_variance[k]) * components[k]``, for the first ``n_components`` retained components (fewer
        where fewer were kept).  ``latent``: a w latent [D] or [1, D]; None draws z (from ``generator`` when one is given) and maps it.  One
        static noise for every image; all rows go through ONE ``gen_grid_image_from_latent`` call, ``len(sigmas)`` images per row; saved to
        ``'%s.jpg' % save_path`` when a path is given.  -> the PIL image."""
        from ..evaluation.generation import _randn
        if group not in pca.components:
            raise ValueError('generate_matrix_by_pca: group %r is not in the fit (groups: %s)' % (group, list(pca.components)))
        lo, hi = pca.places[group]
        comps = pca.components[group]
        rows = min(int(n_components), comps.shape[0])
        if latent is None:
            latent = self.style(_randn((1, self.config.model_config['latent_size']), self.device, generator).to(self._dtype()))
        w = latent.to(self.device, self._dtype()).reshape(1, -1)
        ev = pca.explained_variance[group]
        steps = torch.tensor([[float(s) * float(np.sqrt(ev[k])) for s in sigmas] for k in range(rows)], dtype=w.dtype, device=self.device)
        moved = w.repeat(rows * len(sigmas), 1)
        moved[:, lo:hi] += (steps[:, :, None] * comps[:rows, None, :].to(w.dtype)).reshape(-1, hi - lo)          # row k * len(sigmas) + c
        self.reset_noise(generator)
        image = self.gen_grid_image_from_latent(moved, noise=self.noise, nrow=len(sigmas), downsample=downsample, input_is_latent=True)
        if save_path is not None:
            image.save('%s.jpg' % save_path)
        return image

    def generate_matrix_by_group(self, group, save_path=None, downsample=None, generator=None):
        """The 6 x 6 matrix in which image (row, col) carries ``group``'s slice of sample ``row`` and the rest of sample ``col``, one shared
        noise; saved to ``'%s.jpg' % save_path`` when a path is given.  -> the PIL image."""
        from ..evaluation.generation import gen_matrix
        self.check_valid_group(group)
        same_chunk = self.batch_utils.place_in_latent_dict[group]
        image = gen_matrix(self.model, same_noise_per_id=False, same_chunk=same_chunk, same_noise_for_all=True, downsample=downsample,
                           generator=generator)
        if save_path is not None:
            image.save('%s.jpg' % save_path)
        return image

    def interpolation_latents(self, group, latent_1, latent_from, latent_to, pics_per_interpolation=10, interpolation='slerp'):
        """The z of every frame of one segment, both films: [2, P, B, L] (models/op/interp.py).  [0]: ``group``'s slice stays ``latent_1``'s
        and the rest moves from ``latent_from`` to ``latent_to``; [1]: only ``group``'s slice moves, the rest stays ``latent_1``'s."""
        from ..models.op.interp import interpolate_latents, interpolation_weights
        self.check_valid_group(group)
        lo, hi = self.batch_utils.place_in_latent_dict[group]
        wa, wb = interpolation_weights(pics_per_interpolation, interpolation)
        return interpolate_latents(latent_1, latent_from, latent_to, lo, hi, wa, wb, interpolation)

    @torch.no_grad()
    def interpolate_by_group(self, group, save_path, batch=4, num_of_intermediate_latents=4, pics_per_interpolation=10, interpolation='slerp',
                             same_noise=True, downsample=None, idx=None, generator=None, return_list=False):
        """Two films of ``num_of_intermediate_latents`` segments of ``pics_per_interpolation`` frames each, ``batch`` walks side by side in a
        frame: in the first ``group`` is frozen at ``latent_1``'s and everything else moves, in the second only ``group`` moves.  Frames go to
        ``<save_path>/freeze_group/%06d.jpg`` and ``<save_path>/freeze_not_same_group/%06d.jpg``, the GIFs to
        ``<save_path>/freeze_group_<basename>[%04d idx].gif`` and ``<save_path>/freeze_not_group_<basename>[%04d idx].gif``.  -> the two lists
        of PIL images; with ``return_list=True`` nothing is written and the two float tensors [frames, batch, 3, h, w] of generator outputs
        come back on the host.  ``generator``: a ``torch.Generator`` that makes the call repeatable.

        Per segment ONE interpolate_latents call and ONE ``self.style`` call over the 2 P B rows; per frame ONE blend_noise call into a
        reused list (with ``same_noise`` it blends the noise with itself, as the reference does: that is not the noise bit for bit), two
        generator calls on w and two grid images."""
        from ..evaluation.generation import _make_noise, _randn
        from ..evaluation.image_grid import grid_image
        from ..models.op.interp import blend_noise, interpolation_weights
        self.check_valid_group(group)
        dtype, size = self._dtype(), self.config.model_config['latent_size']
        pics = int(pics_per_interpolation)
        noise = [n.to(dtype).expand(batch, -1, -1, -1).clone() for n in _make_noise(self.model, self.device, generator)]
        latent_1 = _randn((1, size), self.device, generator).to(dtype).expand(batch, -1)
        latent_2 = [_randn((batch, size), self.device, generator).to(dtype) for _ in range(num_of_intermediate_latents)]
        if same_noise:
            noise_2 = [noise for _ in range(num_of_intermediate_latents)]
        else:
            noise_2 = [[n.to(dtype) for n in _make_noise(self.model, self.device, generator, batch_size=batch)] for _ in range(num_of_intermediate_latents)]
        na, nb = interpolation_weights(pics, 'linear')          # the noise is blended linearly whatever the latents' rule
        z1, noise1, frame_noise = latent_1, noise, None
        films = ([], [])
        for z2, noise2 in zip(latent_2, noise_2):
            z = self.interpolation_latents(group, latent_1, z1, z2, pics, interpolation)
            w = self.style(z.reshape(2 * pics * batch, size)).reshape(2, pics, batch, -1)
            for f in range(pics):
                frame_noise = blend_noise(noise1, noise2, na[f], nb[f], out=frame_noise)
                for film in (0, 1):
                    sample, _ = self.model([w[film, f]], input_is_latent=True, noise=frame_noise)
                    films[film].append(sample.cpu() if return_list else grid_image(sample, nrow=batch, downsample=downsample))
            z1, noise1 = z2, noise2
        if return_list:
            return torch.stack(films[0], 0), torch.stack(films[1], 0)
        tail = os.path.split(save_path)[-1] + ('' if idx is None else '%04d' % idx)
        for images, folder, name in ((films[0], 'freeze_group', '../freeze_group_' + tail),
                                     (films[1], 'freeze_not_same_group', '../freeze_not_group_' + tail)):
            os.makedirs(os.path.join(save_path, folder), exist_ok=True)
            self.make_interpolation_gif(images, os.path.join(save_path, folder), name=name)
        return films

    def make_interpolation_gif(self, image_list, save_path, name='sample'):
        """``image_list`` as ``save_path``/%06d.jpg and as the GIF ``save_path``/``name``.gif."""
        for i, image in enumerate(image_list):
            image.save(os.path.join(save_path, '%06d.jpg' % i))
        self.create_gif(save_path, name=name)

    @staticmethod
    def create_gif(save_dir, delay=50, name='sample'):
        """The reference's ``convert -delay 50 -loop 0 -resize 1024x256 *.jpg <name>.gif`` with PIL, no subprocess: every .jpg of ``save_dir``
        in sorted order, scaled to fit inside 1024 x 256 with its aspect ratio kept, ``delay`` hundredths of a second per frame, looping
        forever.  Image.save(save_all=True) folds a frame that repeats its predecessor into it (the last frame of a segment is the first of
        the next), so the frames are encoded one by one, as ``convert`` writes them."""
        from PIL import GifImagePlugin, Image
        frames = []
        for fname in sorted(n for n in os.listdir(save_dir) if n.endswith('.jpg')):
            with Image.open(os.path.join(save_dir, fname)) as im:
                im = im.convert('RGB')
            scale = min(1024 / im.size[0], 256 / im.size[1])
            size = (min(1024, max(1, round(im.size[0] * scale))), min(256, max(1, round(im.size[1] * scale))))
            frames.append((im if size == im.size else im.resize(size, Image.BILINEAR)).convert('P', palette=Image.ADAPTIVE))
        if not frames:
            raise FileNotFoundError('no .jpg frames under %s' % save_dir)
        with open(os.path.normpath(os.path.join(save_dir, name + '.gif')), 'wb') as fp:
            for block in GifImagePlugin.getheader(frames[0], info={'loop': 0, 'duration': 10 * delay})[0]:
                fp.write(block)
            for frame in frames:
                for block in GifImagePlugin.getdata(frame, duration=10 * delay, include_color_table=True):
                    fp.write(block)
            fp.write(b';')

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
