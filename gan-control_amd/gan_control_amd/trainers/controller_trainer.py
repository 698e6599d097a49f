"""Phase-2 controller training step.

Reference: trainers/controller_trainer.py -- model / optimiser set-up :89-125, ``controller_update`` :202-220,
``calc_latent_rec_adv_loss`` :222-229, ``re_arrange_latent`` :248-252.  A controller maps an attribute vector to the
w sub-latent of one attribute group; it is trained with L1 (or MSE) against the w latents of generated samples.
Built: the ``latent_rec`` objective, the ``attribute_rec`` objective (:231-239: splice the predicted sub-latent into w, run the
FROZEN generator on the HIP kernels, read the attribute off a predictor and compare with the controls -- the gradient reaches the
controller through the generator's input gradients), the Adam set-up with the reference's lazy-regularisation ratio and latent
splicing.  The predictor is a ``losses.LossModelClass`` whose pretrained network is supplied by the caller (external weights,
SURVEY 8f-4).

The rest of the reference's trainer is here as well: ``from_generator_dir`` (:89-125: the generator, the working group and its chunk of w from a
trained generator directory), ``train`` (:183-200) over ``datasets.DeviceFrame`` with ``end_iter_update``'s cadence (:254-268), ``evaluate``
(:292-335), ``save_dual_images`` (:364-391) and the directory layout ``inference.Controller`` loads (:64-87).  ``controller_update_fused`` is
the same step in n_layers + 2 launches for the ``latent_rec`` objective (models/op/fc_train.py), with the loss left on the device.
Not built: ``latent_adv`` (dead code in the reference: :222-229 never sets it), tensorboard.
"""
import json
import os
import shutil

import torch
from torch import nn, optim

from ..models.controller_model import FcStack
from ..models.op import fc_train
from ..models.op.fc_stack import fc_stacks_forward


def default_controller_config(in_dim=3, mid_dim=256, n_mlp=8, batch=32):
    """Fields of configs/controller_configs/*.json that the step uses."""
    return {'model_config': {'lr_mlp': 0.01, 'n_mlp': n_mlp, 'in_dim': in_dim, 'mid_dim': mid_dim},
            'training_config': {'batch': batch, 'reg_every': 4, 'lr': 0.002, 'rec_loss': 'l1', 'losses': ['latent_rec'],
                                'attribute_rec_w': 1.0,
                                # configs/controller_configs/ffhq/*.json: the length of a run and the cadence of end_iter_update
                                'iter': 800000, 'start_iter': 0, 'min_evaluate_interval': 5000, 'save_images_interval': 5000,
                                'save_nets_interval': 20000}}


class ControllerTrainer:
    def __init__(self, config, group_chunk, device='cuda', generator=None, seed=None, loss_class=None):
        """group_chunk = (begin, end) of the attribute group inside the w latent (batch_utils.place_in_latent_dict[group]);
        loss_class = the attribute's losses.LossModelClass (predict / controller_criterion), needed by ``attribute_rec``."""
        self.config, self.device = config, torch.device(device)
        self.model_config, self.training_config = config['model_config'], config['training_config']
        self.group_chunk = (int(group_chunk[0]), int(group_chunk[1]))
        if 'latent_adv' in self.training_config['losses']:
            raise NotImplementedError('ControllerTrainer: latent_adv is never computed by the reference either (controller_trainer.py:222-229)')
        if 'attribute_rec' in self.training_config['losses'] and (generator is None or loss_class is None):
            raise ValueError('ControllerTrainer: attribute_rec needs a generator and a loss_class (the attribute predictor)')
        self.loss_class = loss_class
        if seed is not None:
            torch.manual_seed(seed)
        mc, tc = self.model_config, self.training_config
        self.fc_controller = FcStack(mc['lr_mlp'], mc['n_mlp'], mc['in_dim'], mc['mid_dim'], self.group_chunk[1] - self.group_chunk[0]).to(self.device)
        ratio = tc['reg_every'] / (tc['reg_every'] + 1)                      # controller_trainer.py:107-113
        self.fc_optim = optim.Adam(self.fc_controller.parameters(), lr=tc['lr'] * ratio, betas=(0 ** ratio, 0.99 ** ratio))
        self.rec_loss = nn.L1Loss() if tc.get('rec_loss', 'l1') == 'l1' else nn.MSELoss()
        self.generator = generator.eval().to(self.device) if generator is not None else None
        if self.generator is not None:
            for prm in self.generator.parameters():
                prm.requires_grad_(False)
        self.evaluation_dict = {}
        self.eval_loss_list = []
        self.generator_dir = self.working_group = self.batch_utils = self.generator_config = self.ckpt_iter = self.save_dir = None
        self._image_generator = self.eval_frame = None

    @classmethod
    def from_generator_dir(cls, config, generator_dir, device=None, loss_class=None, seed=None):
        """The trainer of the reference's ``init_models_and_optim`` (controller_trainer.py:89-104): the generator of ``generator_dir``
        (``Inference.retrieve_model``), frozen; the working group is the ``same_group_name`` of the generator's own config for
        ``config['model_config']['loss']`` (``gamma_loss`` lives inside ``recon_3d_loss``) and ``group_chunk`` its place in the w latent."""
        from ..inference.inference import Inference, pick_device
        device = pick_device(device)
        generator, batch_utils, generator_config, ckpt_iter = Inference.retrieve_model(generator_dir, device)
        if batch_utils is None:
            raise ValueError('ControllerTrainer: %s holds a vanilla generator: it has no attribute groups to control' % generator_dir)
        loss = config['model_config']['loss']
        tc = generator_config.training_config
        loss_config = tc['recon_3d_loss'][loss] if loss in ('gamma_loss',) else tc[loss]
        working_group = loss_config['same_group_name']
        trainer = cls(config, batch_utils.place_in_latent_dict[working_group], device=device, generator=generator, seed=seed, loss_class=loss_class)
        trainer.generator_dir, trainer.working_group, trainer.batch_utils = generator_dir, working_group, batch_utils
        trainer.generator_config, trainer.ckpt_iter = generator_config, ckpt_iter
        return trainer

    def calc_latent_rec_loss(self, org_latent, pred_latent):
        lo, hi = self.group_chunk
        return self.rec_loss(pred_latent, org_latent[:, lo:hi])

    def controller_update(self, batch):
        """One optimisation step on (controls, w latents); returns the loss value (also in evaluation_dict)."""
        controls = batch[0].to(self.device).float()
        org_latent = batch[1].to(self.device)
        self.fc_controller.train()
        self.fc_controller.zero_grad()
        pred_latent = self.fc_controller(controls.detach())
        tc = self.training_config
        loss = 0.
        if 'latent_rec' in tc['losses']:
            rec = self.calc_latent_rec_loss(org_latent, pred_latent)
            self.evaluation_dict['latent_rec_loss'] = rec.item()
            loss = loss + rec
        if 'attribute_rec' in tc['losses']:
            att = self.calc_attribute_rec_controller_loss(org_latent, pred_latent, controls)
            self.evaluation_dict['attribute_loss'] = att.item()
            loss = loss + att * tc['attribute_rec_w']
        self.evaluation_dict['loss'] = loss.item()
        loss.backward()
        self.fc_optim.step()
        return self.evaluation_dict['loss']

    def controller_update_fused(self, batch):
        """``controller_update`` with the loss left on the device (a 0-dim tensor; nothing synchronises).  For ``losses == ['latent_rec']``
        it is ``fc_train.fused_step``: under that module's dispatch rule n_layers + 2 launches that update the parameters and ``fc_optim``'s own
        state, else the same autograd step as ``controller_update``.  Any other list of losses is ``controller_update`` itself
        (``attribute_rec`` runs the generator, which dominates that step)."""
        if list(self.training_config['losses']) == ['latent_rec']:
            self.fc_controller.train()
            return fc_train.fused_step(self.fc_controller, self.fc_optim, batch[0].to(self.device).float(), batch[1].to(self.device),
                                       self.group_chunk, self.rec_loss)
        return torch.as_tensor(self.controller_update(batch), dtype=torch.float32, device=self.device)

    def calc_attribute_rec_controller_loss(self, org_latent, pred_latent, controls):
        """controller_trainer.py:231-239."""
        latent = self.re_arrange_latent(org_latent, pred_latent)
        fake_img, _ = self.generator([latent], input_is_latent=True)
        pred = self.loss_class.predict(fake_img)
        return self.loss_class.controller_criterion(pred, controls)

    def re_arrange_latent(self, org_latent, group_latent):
        """w latent with the group's slice replaced by the controller output (controller_trainer.py:248-252)."""
        lo, hi = self.group_chunk
        latent = org_latent.clone()
        latent[:, lo:hi] = group_latent
        return latent

    def save_nets(self, i, save_dir):
        """``<save_dir>/checkpoint/<i:06d>.pt`` holding 'controller' (the FcStack's state_dict) and 'fc_optim': with
        ``trainers.utils.save_args(config, save_dir)`` next to it, the directory inference.Controller loads for this group.  -> the path."""
        import os
        path = os.path.join(save_dir, 'checkpoint', '%s.pt' % str(i).zfill(6))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save({'controller': self.fc_controller.state_dict(), 'fc_optim': self.fc_optim.state_dict()}, path)
        return path

    # -- the reference's loop (controller_trainer.py:183-200, :254-336, :364-391) -----------------------------------------------------------------
    @torch.no_grad()
    def evaluate(self, eval_frame, i=None):
        """controller_trainer.py:292-335 on up to 25 batches of 50 rows of ``eval_frame`` (a ``datasets.DeviceFrame`` of the eval split; a
        frame shorter than one batch is one batch of all its rows).  The batches have one size, so the mean of their mean losses is the mean
        over all their rows: the controller runs over all of them in ONE ``fc_stacks_forward`` call and the L1 / MSE is read from the device
        once.  With ``attribute_rec`` the generator runs batch by batch, as in the reference.  -> eval_loss; the history goes to
        ``<save_dir>/graphs/eval_loss.json`` while ``train`` runs."""
        self.fc_controller.eval()
        tc = self.training_config
        lo, hi = self.group_chunk
        size = 50 if len(eval_frame) >= 50 else max(len(eval_frame), 1)
        batches = min(25, len(eval_frame) // size)
        if batches < 1:
            raise ValueError('ControllerTrainer.evaluate: the eval split is empty')
        controls, latent_w = eval_frame.controls[:batches * size], eval_frame.latents_w[:batches * size]
        pred = torch.empty(controls.shape[0], hi - lo, dtype=controls.dtype, device=controls.device)
        fc_stacks_forward([self.fc_controller], controls, None, pred, None)
        rec = att = 0.
        if 'latent_rec' in tc['losses']:
            rec = self.rec_loss(pred, latent_w[:, lo:hi]).item()
        if 'attribute_rec' in tc['losses']:
            for b in range(batches):
                rows = slice(b * size, (b + 1) * size)
                fake_img, _ = self.generator([self.re_arrange_latent(latent_w[rows], pred[rows])], input_is_latent=True)
                att += self.loss_class.controller_criterion(self.loss_class.predict(fake_img), controls[rows]).item()
            att /= batches
        self.evaluation_dict['eval_loss'] = rec + att
        self.evaluation_dict['eval_rec_loss'] = rec
        self.evaluation_dict['attribute_loss'] = att
        self.eval_loss_list.append(self.evaluation_dict['eval_loss'])
        if self.save_dir is not None:
            path = os.path.join(self.save_dir, 'graphs', 'eval_loss.json')
            os.makedirs(os.path.dirname(path), exist_ok=True)
            history = []
            if os.path.exists(path) and len(self.eval_loss_list) > 1:
                with open(path) as f:
                    history = json.load(f)
            history.append({'iter': None if i is None else int(i), 'eval_loss': self.evaluation_dict['eval_loss'],
                            'eval_rec_loss': rec, 'attribute_loss': att})
            with open(path, 'w') as f:
                json.dump(history, f)
        self.fc_controller.train()
        return self.evaluation_dict['eval_loss']

    @torch.no_grad()
    def save_dual_images(self, i, save_dir, eval_frame, generator=None):
        """controller_trainer.py:364-391: 16 random rows of ``eval_frame``; every original and, next to it, its image with the group's slice of
        w replaced by the controller's output, rendered with the same noise, four images (two pairs) per row.  -> the path of
        ``<save_dir>/images/sample/<i:06d>.png``.  ``generator``: a ``torch.Generator`` that makes the rows and the noise repeatable."""
        from ..evaluation.generation import _make_noise
        from ..evaluation.image_grid import grid_image
        if self.generator is None:
            raise RuntimeError('ControllerTrainer.save_dual_images needs a generator')
        self.fc_controller.eval()
        count = 16
        rows = torch.randint(0, len(eval_frame), (count,), generator=generator,
                             device='cpu' if generator is None else generator.device).to(eval_frame.controls.device)
        controls, latent_ws = eval_frame.controls.index_select(0, rows), eval_frame.latents_w.index_select(0, rows)
        noise = [n.to(latent_ws.dtype) for n in _make_noise(self.generator, self.device, generator, batch_size=count)]
        pred_latent_ws = self.re_arrange_latent(latent_ws, self.fc_controller(controls))
        fake_img, _ = self.generator([latent_ws], input_is_latent=True, noise=noise)
        pred_fake_img, _ = self.generator([pred_latent_ws], input_is_latent=True, noise=noise)
        pairs = torch.stack([fake_img, pred_fake_img], dim=1).reshape(2 * count, *fake_img.shape[1:])          # original, controlled, original, ...
        path = os.path.join(save_dir, 'images', 'sample', '%s.png' % str(i).zfill(6))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        grid_image(pairs, nrow=4).save(path)
        self.fc_controller.train()
        return path

    def init_dirs(self, save_dir):
        """controller_trainer.py:64-87: ``save_dir`` is the group's directory; ``generator/`` next to it gets ``args.json`` and the checkpoint
        the generator was loaded from; ``save_dir`` gets ``args.json`` -- what ``inference.Controller(<parent of save_dir>)`` loads."""
        from .utils import save_args
        for sub in ('checkpoint', 'graphs', os.path.join('images', 'sample')):
            os.makedirs(os.path.join(save_dir, sub), exist_ok=True)
        if self.generator_dir is not None:
            target = os.path.join(os.path.split(os.path.abspath(save_dir))[0], 'generator')
            os.makedirs(os.path.join(target, 'checkpoint'), exist_ok=True)
            name = '%s.pt' % self.ckpt_iter
            for rel in ('args.json', os.path.join('checkpoint', name)):
                if os.path.abspath(os.path.join(self.generator_dir, rel)) != os.path.abspath(os.path.join(target, rel)):
                    shutil.copyfile(os.path.join(self.generator_dir, rel), os.path.join(target, rel))
        save_args(self.config, save_dir)
        self.save_dir = save_dir

    def end_iter_update(self, i, eval_frame=None):
        """controller_trainer.py:254-266.  ``eval_frame``: the eval split (``train`` keeps its own as ``self.eval_frame``)."""
        tc = self.training_config
        eval_frame = self.eval_frame if eval_frame is None else eval_frame
        if i % tc['min_evaluate_interval'] == 0:
            self.evaluate(eval_frame, i)
        if i % tc['save_images_interval'] == 0 and self.generator is not None:
            self.save_dual_images(i, self.save_dir, eval_frame, generator=self._image_generator)
        if i % tc['save_nets_interval'] == 0:
            self.save_nets(i, self.save_dir)

    def train(self, frame_or_path, attribute, save_dir, iters=None, log_interval=100, generator=None):
        """controller_trainer.py:183-200: epochs over ``DeviceFrame(frame_or_path, attribute).epoch(batch)`` until step ``iters`` (default
        ``training_config['iter']``), ``controller_update_fused`` per batch and ``end_iter_update`` after it.  The loss is read from the device
        only every ``log_interval`` steps (into ``evaluation_dict['loss']`` and the returned list of (step, loss)).  ``generator``: a
        ``torch.Generator`` for the order of the rows (and, on the same device, the sample images)."""
        from ..datasets import DeviceFrame
        tc = self.training_config
        frame = frame_or_path
        if not hasattr(frame, 'latents_w') and not isinstance(frame, str):
            frame = str(frame)
        train_frame = DeviceFrame(frame, attribute, self.device, train=True)
        eval_frame = DeviceFrame(frame, attribute, self.device, train=False)
        if len(train_frame) < tc['batch']:
            raise ValueError('ControllerTrainer.train: %d training rows are fewer than one batch of %d' % (len(train_frame), tc['batch']))
        self.init_dirs(save_dir)
        self._image_generator, self.eval_frame = generator, eval_frame
        iters = tc['iter'] if iters is None else int(iters)
        i, log = tc.get('start_iter', 0), []
        for prm in self.fc_controller.parameters():
            prm.requires_grad_(True)
        while i < iters:
            for batch in train_frame.epoch(tc['batch'], generator=generator):
                loss = self.controller_update_fused(batch)
                if i % log_interval == 0:
                    self.evaluation_dict['loss'] = float(loss)
                    log.append((i, self.evaluation_dict['loss']))
                self.end_iter_update(i)
                i += 1
                if i >= iters:
                    break
        return log

    @torch.no_grad()
    def generate(self, org_latent, controls):
        """Images of the frozen generator for latents whose group slice comes from the controller."""
        if self.generator is None:
            raise RuntimeError('ControllerTrainer.generate needs a generator')
        self.fc_controller.eval()
        latent = self.re_arrange_latent(org_latent.to(self.device), self.fc_controller(controls.to(self.device).float()))
        return self.generator([latent], input_is_latent=True)[0]
