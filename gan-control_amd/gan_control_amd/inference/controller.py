"""Generation by attribute values (reference: inference/controller.py::Controller, same names and argument lists).

A controller directory holds ``generator/`` (a model directory, see inference.py) and one directory per attribute group whose name starts
with the group's name -- ``args.json`` with ``model_config`` {lr_mlp, n_mlp, in_dim, mid_dim} and ``checkpoint/<iter>.pt`` with the key
``controller`` (``ControllerTrainer.save_nets`` + ``trainers.utils.save_args`` write it) -- plus, optionally, ``expression_q*`` for the
quantised 8-column expression control.  ``gen_batch_by_controls`` is two ``fc_stacks_forward`` calls: z -> w, then every driven controller
writing its group's slice of w; the generator runs on the result.  Deviations from the reference: DESIGN.md, "Inference API".
"""
import os

import torch

from ..models.controller_model import FcStack
from ..models.op.fc_stack import fc_stacks_forward
from .inference import Inference, last_checkpoint, read_config


class Controller(Inference):
    def __init__(self, controller_dir, device=None):
        super().__init__(os.path.join(controller_dir, 'generator'), device=device)
        self.fc_controls = {}
        self.config_controls = {}
        for name in list(self.batch_utils.sub_group_names) + ['expression_q']:
            self.fc_controls[name], self.config_controls[name] = self.retrieve_controller(controller_dir, name)

    def _driven(self, group_key, value):
        """(controller, group whose slice it writes, controls on the device as float) of one ``group=value`` argument."""
        self.check_if_group_has_control(group_key)
        name = 'expression_q' if group_key == 'expression' and value.shape[1] == 8 else group_key
        controller = self.fc_controls[name]
        if controller is None:
            raise ValueError('group: %s has no controller directory (%s was not found)' % (group_key, name))
        return controller, 'expression' if name == 'expression_q' else name, value.to(self.device).to(self._dtype())

    def gen_batch_by_controls(self, batch_size=1, latent=None, normalize=True, input_is_latent=False, static_noise=True, **kwargs):
        """-> (images, latent, latent_w): ``latent`` a copy of the z (or w) that was drawn or given, ``latent_w`` the [B, 512] w with the
        slice of every group named in kwargs (``orientation=tensor [B, 3]``, ``age=tensor [B, 1]``, ...) replaced by its controller's output.
        With ``input_is_latent`` the two are one tensor, as in the reference.  Runs without autograd, as the reference does, unless gradients
        are enabled AND the given latent or a control requires one: then every step is a module call and the results carry the graph."""
        wants_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in [latent, *kwargs.values()])
        with torch.enable_grad() if wants_grad else torch.no_grad():
            return self._gen_batch_by_controls(batch_size, latent, normalize, input_is_latent, static_noise, kwargs)

    def _gen_batch_by_controls(self, batch_size, latent, normalize, input_is_latent, static_noise, controls):
        if latent is None:
            latent = torch.randn(batch_size, self.config.model_config['latent_size'], device=self.device, dtype=self._dtype())
        latent = latent.to(self.device).clone()
        latent_w = latent if input_is_latent else self.style(latent)
        driven = [self._driven(k, v) for k, v in controls.items()]
        if driven and latent_w.ndim == 2:
            places = [tuple(self.batch_utils.place_in_latent_dict[g]) for _, g, _ in driven]
            fc_stacks_forward([c for c, _, _ in driven], [v for _, _, v in driven], None, latent_w, places)
        else:
            for controller, group, value in driven:
                latent_w = self.insert_group_w_latent(latent_w, controller(value), group)
        injection_noise = self.noise if static_noise else None          # [1, 1, h, w]: broadcast over the batch, bit for bit expend_noise
        tensor, _ = self.model([latent_w], input_is_latent=True, noise=injection_noise)
        if normalize:
            tensor = tensor.mul(0.5).add(0.5).clamp(min=0., max=1.).cpu()
        return tensor, latent, latent_w

    def generate_group_w_latent(self, group_key: str, value: torch.Tensor):
        controller = self.fc_controls[group_key]
        if controller is None:
            raise ValueError('group: %s has no controller directory' % group_key)
        return controller(value)

    def _place(self, group):
        return self.batch_utils.place_in_latent_dict[group]

    def insert_group_w_latent(self, latent_w, group_w_latent, group):
        """In place: the group's slice of a [B, 512] or [B, n_latent, 512] latent becomes ``group_w_latent`` (same number of dims)."""
        if group_w_latent.ndim != latent_w.ndim:
            raise ValueError(f'group_w_latent.ndim ({group_w_latent.ndim}) must equal latent_w.ndim ({latent_w.ndim})')
        lo, hi = self._place(group)
        latent_w[..., lo:hi] = group_w_latent
        return latent_w

    def get_group_w_latent(self, latent_w: torch.Tensor, group: str):
        lo, hi = self._place(group)
        return latent_w[..., lo:hi]

    @staticmethod
    def get_controller_dir(controller_dir, sub_group_name):
        """The first directory (sorted) whose name starts with the group's name; ``expression`` does not take ``expression_q*``."""
        for name in sorted(os.listdir(controller_dir)):
            if name.startswith(sub_group_name) and not (sub_group_name == 'expression' and name.startswith('expression_q')):
                return os.path.join(controller_dir, name)
        return None

    def retrieve_controller(self, controller_dir, sub_group_name):
        """-> (FcStack in eval mode, config), or (None, None) when the group has no directory."""
        path = self.get_controller_dir(controller_dir, sub_group_name)
        if path is None:
            return None, None
        config = read_config(os.path.join(path, 'args.json'))
        ckpt_path, _ = last_checkpoint(path)
        ckpt = torch.load(ckpt_path, map_location='cpu')
        lo, hi = self._place('expression' if sub_group_name == 'expression_q' else sub_group_name)
        mc = config.model_config
        controller = FcStack(mc['lr_mlp'], mc['n_mlp'], mc['in_dim'], mc['mid_dim'], hi - lo)
        controller.load_state_dict(ckpt['controller'])
        return controller.to(self.device).eval(), config

    def check_if_group_has_control(self, group):
        if group not in self.fc_controls:
            raise ValueError('group: %s has no control' % group)
        return True
