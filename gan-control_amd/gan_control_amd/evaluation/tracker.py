"""The image and FID subset of the reference's ``Tracker`` (evaluation/tracker.py): fixed sample grids, id x pose matrices, and the FID
history that decides when ``best_fid.pt`` is written.

Separability, the orientation / expression / age matrices (they need the external predictors), the matplotlib plots and tensorboard are out
of scope; the FID history goes to ``<graph_save_path>/fid.json`` instead of a plot.
"""
import json
import os

import numpy as np

from ..fid_utils import fid as fid_module
from .generation import gen_grid, gen_matrix


class Tracker:
    def __init__(self, latent_samples, injection_noise_samples, inception, g_noise_mode, fid_config=None):
        self.latent_samples = latent_samples
        self.injection_noise_samples = injection_noise_samples
        self.inception = inception
        self.fid_config = fid_config if fid_config is not None else {'enabled': False}
        self.same_noise_per_id = g_noise_mode == 'same_for_same_id'
        self.fids = []
        self.evaluation_dict = {}

    @staticmethod
    def _device(model):
        return next(getattr(model, 'module', model).parameters()).device

    def make_samples(self, model, use_sample_noise=True):
        """The grid of the fixed latents (tracker.py:82-87), four images per row."""
        dev = self._device(model)
        noise = [n.detach().to(dev) for n in self.injection_noise_samples] if use_sample_noise else None
        return gen_grid(model, self.latent_samples.detach().to(dev), injection_noise=noise, nrow=4)

    def make_matrix(self, model, downsample=None, same_chunk=(256, 512), same_noise_for_all=False):
        return gen_matrix(model, same_noise_per_id=self.same_noise_per_id, downsample=downsample, same_chunk=same_chunk,
                          same_noise_for_all=same_noise_for_all)

    def evaluate(self, iter, model, debug=False, graph_save_path=None):
        """The FID cadence of tracker.py:132-133: enabled, and every ``fid_interval`` iterations (every 100 in debug), never at iteration 0."""
        cfg = self.fid_config
        if cfg.get('enabled') and ((debug and iter % 100 == 0) or (iter % cfg['fid_interval'] == 0)) and iter != 0:
            self.fid_evaluation(iter, model, graph_save_path=graph_save_path, debug=debug)

    def fid_evaluation(self, iter, model, graph_save_path=None, debug=False):
        cfg = self.fid_config
        fid = float(fid_module.evaluate_fid(model, self.inception, 20, 100 if debug else cfg['num_of_samples'], self._device(model),
                                            cfg.get('inception_stat_path')))
        self.fids.append(fid)
        self.evaluation_dict['fid'] = fid
        if graph_save_path is not None:
            os.makedirs(graph_save_path, exist_ok=True)
            path = os.path.join(graph_save_path, 'fid.json')
            history = []
            if os.path.exists(path):
                with open(path) as f:
                    history = json.load(f)
            history.append({'iter': int(iter), 'fid': fid})
            with open(path, 'w') as f:
                json.dump(history, f)
        return fid

    def is_best_fid(self):
        if len(self.fids) == 0:
            return False
        return bool(np.array(self.fids)[-1] == np.array(self.fids).min())
