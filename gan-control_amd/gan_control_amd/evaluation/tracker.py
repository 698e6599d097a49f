"""The image, FID and separability subset of the reference's ``Tracker`` (evaluation/tracker.py): fixed sample grids, id x pose matrices,
the FID history that decides when ``best_fid.pt`` is written, and the separability evaluation on the same cadence.

The orientation / expression / age matrices and histograms (they need the external predictors), the matplotlib plots and tensorboard are
out of scope; the FID history goes to ``<graph_save_path>/fid.json`` and the separability history to
``<graph_save_path>/separability.json`` instead of plots.  Beyond the reference: with ``fid_config['kid']`` / ``fid_config['precision_recall']``
the FID sample also yields KID and improved precision / recall (fid_utils/kid.py, fid_utils/precision_recall.py), kept in
``<graph_save_path>/quality.json``; without those keys nothing changes.  ``fid_config['streaming']`` and ``fid_config['fid_method']`` are
handed to ``evaluate_fid`` / ``evaluate_quality`` as ``streaming=`` and ``method=`` (device-resident statistics, eigen-form distance);
without these keys the calls are the ones made before.

Separability (tracker.py:134-155, :185-311) runs for the losses that are BOTH listed in ``separability_config['losses']`` and present in the
``loss_models`` handed to ``evaluate``.  Two deliberate deviations from the reference's ``evaluate``: it indexes ``training_config`` for five
losses to build its table of sub-latent chunks and hides the resulting ``KeyError`` -- and every other failure -- behind a bare ``except``
(SURVEY.md); here the caller passes ``same_chunks`` for the configured losses only, and errors surface.  ``save_separability_buckets`` writes
the reference's file names; the text line it draws on each image goes into ``<global_step:08d>_<name>.json`` beside them, and the right half
of a pair is the query's own image (the reference indexes its image list by the query's pid, which is the query's even-row sibling).
"""
import json
import os

import numpy as np

from ..fid_utils import fid as fid_module
from . import separability
from .generation import gen_grid, gen_matrix

# loss name -> (plot title, tag) of separability_evaluation (tracker.py:200-269)
SEPARABILITY_TAGS = {'embedding_loss': ('id separability', 'id'), 'orientation_loss': ('orientation separability', 'orientation'),
                     'expression_loss': ('expression separability', 'expression'), 'age_loss': ('age separability', 'age'),
                     'hair_loss': ('hair separability', 'hair')}


class Tracker:
    def __init__(self, latent_samples, injection_noise_samples, inception, g_noise_mode, fid_config=None, separability_config=None):
        self.latent_samples = latent_samples
        self.injection_noise_samples = injection_noise_samples
        self.inception = inception
        self.fid_config = fid_config if fid_config is not None else {'enabled': False}
        self.separability_config = separability_config if separability_config is not None else {'enabled': False}
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

    def evaluate(self, iter, model, debug=False, graph_save_path=None, buckets_save_path=None, loss_models=None, same_chunks=None):
        """The cadence of tracker.py:132-155: FID when enabled, every ``fid_interval`` iterations (every 100 in debug), never at iteration 0;
        separability under the same rule with ``separability_interval``.  ``loss_models``: {loss name: LossModelClass}; ``same_chunks``:
        {loss name: (lo, hi)}, the latent columns of the loss's ``same_group_name``."""
        cfg = self.fid_config
        if cfg.get('enabled') and ((debug and iter % 100 == 0) or (iter % cfg['fid_interval'] == 0)) and iter != 0:
            self.fid_evaluation(iter, model, graph_save_path=graph_save_path, debug=debug)
        cfg = self.separability_config
        if cfg.get('enabled') and ((debug and iter % 100 == 0) or (iter % cfg['separability_interval'] == 0)) and iter != 0:
            self.separability_evaluation(model, iter, loss_models=loss_models, graph_save_path=graph_save_path, buckets_save_path=buckets_save_path,
                                         debug=debug, same_chunks=same_chunks)

    def fid_evaluation(self, iter, model, graph_save_path=None, debug=False):
        """FID of a fresh sample; with ``fid_config['kid']`` / ``fid_config['precision_recall']`` also KID / precision and recall of the SAME
        sample (fid.evaluate_quality), into ``evaluation_dict`` and ``<graph_save_path>/quality.json``."""
        cfg = self.fid_config
        n_sample = 100 if debug else cfg['num_of_samples']
        extra = [m for m in ('kid', 'precision_recall') if cfg.get(m)]
        # fid_config['streaming'] / ['fid_method'] -> the keywords of the same names; without the keys the calls are made without them
        opts = {kw: cfg[key] for key, kw in (('streaming', 'streaming'), ('fid_method', 'method')) if key in cfg}
        quality = None
        if extra:
            quality = fid_module.evaluate_quality(model, self.inception, 20, n_sample, self._device(model), cfg.get('inception_stat_path'),
                                                  metrics=['fid'] + extra, **opts)
            quality = {k: float(v) for k, v in quality.items()}
            fid = quality['fid']
        else:
            fid = float(fid_module.evaluate_fid(model, self.inception, 20, n_sample, self._device(model), cfg.get('inception_stat_path'), **opts))
        self.fids.append(fid)
        self.evaluation_dict['fid'] = fid
        if graph_save_path is not None:
            self._append_history(os.path.join(graph_save_path, 'fid.json'), {'iter': int(iter), 'fid': fid})
        if quality is not None:
            for key in ('kid', 'precision', 'recall'):
                if key in quality:
                    self.evaluation_dict[key] = quality[key]
            if graph_save_path is not None:
                self._append_history(os.path.join(graph_save_path, 'quality.json'), dict({'iter': int(iter)}, **quality))
        return fid

    @staticmethod
    def _append_history(path, entry):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        history = []
        if os.path.exists(path):
            with open(path) as f:
                history = json.load(f)
        history.append(entry)
        with open(path, 'w') as f:
            json.dump(history, f)

    def is_best_fid(self):
        if len(self.fids) == 0:
            return False
        return bool(np.array(self.fids)[-1] == np.array(self.fids).min())

    # -- separability (tracker.py:185-311) ------------------------------------------------------------------------------------------
    def separability_evaluation(self, model, global_step, loss_models=None, graph_save_path=None, buckets_save_path=None, debug=False,
                                same_chunks=None):
        """One make_separability_for_tag per loss of ``separability_config['losses']`` that ``loss_models`` holds, in the reference's order;
        the averages go to ``evaluation_dict`` and, with a ``graph_save_path``, to ``separability.json``.  -> the tags that ran."""
        cfg = self.separability_config
        loss_models, same_chunks = loss_models or {}, same_chunks or {}
        ran = []
        for name, (title, tag) in SEPARABILITY_TAGS.items():
            if name not in cfg['losses'] or loss_models.get(name) is None:
                continue
            if name not in same_chunks:
                raise KeyError('separability of %s: same_chunks has no latent chunk for it (got %s)' % (name, sorted(same_chunks)))
            self.make_separability_for_tag(model, loss_models[name], title, tag, same_chunks[name],
                                           None if graph_save_path is None else os.path.join(graph_save_path, '%s_separability' % tag),
                                           buckets_save_path, global_step, debug,
                                           last_layer_separability_only=cfg.get('last_layer_separability_only', False))
            ran.append(tag)
        if ran and graph_save_path is not None:
            entry = {'iter': int(global_step)}
            for tag in ran:
                for key in ('same_avg', 'all_not_same_avg', 'not_same_2nd_best_avg'):
                    entry['%s_%s' % (tag, key)] = self.evaluation_dict['%s_%s' % (tag, key)]
            self._append_history(os.path.join(graph_save_path, 'separability.json'), entry)
        return ran

    def make_separability_for_tag(self, model, loss_class, title, tag, same_chunk, save_path, buckets_save_path, global_step, debug,
                                  last_layer_separability_only=False):
        """calc_separability on ``separability_config['num_of_samples']`` samples (100 in debug); ``<tag>_same_avg``, ``<tag>_all_not_same_avg``
        and ``<tag>_not_same_2nd_best_avg`` of the LAST level; the five closest not-same pairs as bucket files."""
        if save_path is not None:
            os.makedirs(os.path.dirname(save_path) or '.', exist_ok=True)
        same_not_same_list, image_list = separability.calc_separability(
            model, loss_class, same_noise_for_same_id=self.same_noise_per_id, num_of_samples=100 if debug else self.separability_config['num_of_samples'],
            title=title, save_path=save_path, return_images=buckets_save_path is not None, same_chunk=tuple(same_chunk),
            last_layer_separability_only=last_layer_separability_only)
        last = same_not_same_list[-1]
        self.evaluation_dict['%s_same_avg' % tag] = float(np.asarray(last['same']).mean())
        self.evaluation_dict['%s_all_not_same_avg' % tag] = float(np.asarray(last['all_not_same']).mean())
        self.evaluation_dict['%s_not_same_2nd_best_avg' % tag] = float(np.asarray(last['not_same']).mean())
        if buckets_save_path is not None:
            self.save_separability_buckets('%s_embedding' % tag, last['pids_2nd_best_pairs_df'], image_list, global_step, buckets_save_path)
        return same_not_same_list

    @staticmethod
    def save_separability_buckets(name, pids_2nd_best_pairs_df, image_list, global_step, buckets_save_path, k=5):
        """``<global_step:08d>_<name>_<i:02d>.jpg``, i < 5: the signature's and the query's image side by side for the ``k`` smallest
        distances of the frame (ties in frame order, as the reference's repeated idxmin), and their text lines in ``<global_step:08d>_<name>.json``.
        ``image_list``: uint8 [h, w, 3] arrays, the signatures' half then the queries' half; pids index a half.  -> the paths written."""
        from PIL import Image
        os.makedirs(buckets_save_path, exist_ok=True)
        sig, que = np.asarray(pids_2nd_best_pairs_df['signature']), np.asarray(pids_2nd_best_pairs_df['queries'])
        dist = np.asarray(pids_2nd_best_pairs_df['distance'])
        half = len(image_list) // 2
        written, lines = [], []
        for i, row in enumerate(np.argsort(dist, kind='stable')[:k]):
            s, q, d = int(sig[row]), int(que[row]), float(dist[row])
            lines.append({'file': '%08d_%s_%02d.jpg' % (global_step, name, i), 'signature': s, 'queries': q, 'distance': d,
                          'message': '%d) Sig: %d, Que: %d, distance:%.4f' % (i, s, q, d)})
            pair = np.concatenate([np.asarray(image_list[s]), np.asarray(image_list[half + q])], axis=1)
            written.append(os.path.join(buckets_save_path, lines[-1]['file']))
            Image.fromarray(np.ascontiguousarray(pair), 'RGB').save(written[-1])
        written.append(os.path.join(buckets_save_path, '%08d_%s.json' % (global_step, name)))
        with open(written[-1], 'w') as f:
            json.dump(lines, f)
        return written
