"""evaluation.Tracker and the trainer's end-of-iteration cadence (end_iter_update, generator_trainer.py:721-733) on the emulated backend."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from gan_control_amd.evaluation import image_grid
from gan_control_amd.evaluation.tracker import Tracker
from gan_control_amd.fid_utils import fid as fid_module

SIZE, BATCH = 16, 4
GROUPS = {'id': {'place_in_latent': [0, 256], 'place_in_mini_batch': [0, 2]},
          'other': {'place_in_latent': [256, 512], 'place_in_mini_batch': [2, 4]}}


def make_trainer(grouped, **training):
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    from gan_control_amd.utils.mini_batch_utils import MiniBatchUtils
    cfg = copy.deepcopy(default_config(SIZE, BATCH))
    cfg['training_config'].update(training)
    cfg['evaluation_config'] = {'fid': {'enabled': True, 'fid_interval': 1, 'num_of_samples': 40, 'inception_stat_path': 'stats.pkl'}}
    tr = GeneratorTrainer(cfg, device='cpu', seed=0, fused_adam=False)
    if grouped:          # the sub-latent groups of a controllable run (their losses need predictors; the images only need the groups)
        tr.training_config['embedding_loss'] = {'same_group_name': 'id'}
        tr.batch_utils = MiniBatchUtils(BATCH, GROUPS, total_batch=BATCH)
    return tr


def fake_fid(monkeypatch, values):
    calls = []
    it = iter(values)

    def evaluate_fid(generator, feature_net, batch, n_sample, device, inception_stat_path, training=False):
        calls.append((batch, n_sample, inception_stat_path))
        return next(it)

    monkeypatch.setattr(fid_module, 'evaluate_fid', evaluate_fid)
    return calls


def test_tracker_fid_history(emu_backend, monkeypatch, tmp_path):
    tr = make_trainer(False)
    calls = fake_fid(monkeypatch, [5.0, 3.0, 4.0, 2.0])
    tracker = Tracker(torch.zeros(4, 512), None, 'inception', 'normal', fid_config={'enabled': True, 'fid_interval': 10, 'num_of_samples': 40,
                                                                                    'inception_stat_path': 'stats.pkl'})
    graphs = str(tmp_path / 'graphs')
    assert not tracker.is_best_fid()
    best = []
    for i in (0, 5, 10, 20, 25, 30):          # never at 0, only on the interval
        tracker.evaluate(i, tr.g_ema, graph_save_path=graphs)
        best.append(tracker.is_best_fid())
    assert tracker.fids == [5.0, 3.0, 4.0] and tracker.evaluation_dict['fid'] == 4.0
    assert best == [False, False, True, True, True, False]
    assert calls == [(20, 40, 'stats.pkl')] * 3
    with open(os.path.join(graphs, 'fid.json')) as f:
        assert json.load(f) == [{'iter': 10, 'fid': 5.0}, {'iter': 20, 'fid': 3.0}, {'iter': 30, 'fid': 4.0}]
    tracker.evaluate(100, tr.g_ema, debug=True)          # the debug rule: every 100 iterations, on 100 samples, no file without a path
    assert calls[-1] == (20, 100, 'stats.pkl') and tracker.is_best_fid()
    off = Tracker(torch.zeros(4, 512), None, None, 'same_for_same_id')
    off.evaluate(10, tr.g_ema)
    assert off.fids == [] and off.same_noise_per_id and not tracker.same_noise_per_id


def test_make_tracker_and_samples(emu_backend):
    tr = make_trainer(False)
    tracker = tr.make_tracker(n_samples=6, seed=3)
    again = tr.make_tracker(n_samples=6, seed=3)
    assert tracker.latent_samples.shape == (6, 512) and torch.equal(tracker.latent_samples, again.latent_samples)
    assert [tuple(n.shape) for n in tracker.injection_noise_samples] == [tuple(n.shape) for n in tr.g_ema.make_noise(batch_size=6)]
    assert tracker.fid_config['fid_interval'] == 1
    img = tracker.make_samples(tr.g_ema)
    with torch.no_grad():
        want, _ = tr.g_ema([tracker.latent_samples], noise=tracker.injection_noise_samples)
    assert img.size == (4 * (SIZE + 2) + 2, 2 * (SIZE + 2) + 2)
    assert np.array_equal(np.asarray(img), np.asarray(image_grid.grid_image(want, nrow=4)))
    assert tracker.make_matrix(tr.g_ema).size == (6 * (SIZE + 2) + 2,) * 2


def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_train_cadence(emu_backend, monkeypatch, tmp_path):
    """Four iterations; FID at every iteration but 0 (5, 3, 4), images every 3, a checkpoint at every one: best_fid.pt is written with the
    checkpoints of iterations 1 and 2 (5, then 3, is the best so far) and with no other (no FID yet at 0; 4 at 3)."""
    from PIL import Image
    calls = fake_fid(monkeypatch, [5.0, 3.0, 4.0])
    tr = make_trainer(True, min_evaluate_interval=1, save_images_interval=3, save_nets_interval=1)
    saved = []
    real_save = tr.save_nets
    monkeypatch.setattr(tr, 'save_nets', lambda i, save_dir, best_fid=False: (saved.append((i, best_fid)), real_save(i, save_dir, best_fid=best_fid))[1])
    tracker = tr.make_tracker(inception='inception', n_samples=4)
    root = str(tmp_path / 'run')
    assert tr.train(save_dir=root, iters=4, tracker=tracker) == 4
    assert tracker.fids == [5.0, 3.0, 4.0] and len(calls) == 3
    assert saved == [(0, False), (1, False), (1, True), (2, False), (2, True), (3, False)]
    matrices = ['matrix', 'matrix_same_noise', 'default_id_matrix', 'default_id_matrix_same_noise', 'default_other_matrix',
                'default_other_matrix_same_noise']
    want = ['checkpoint/%s.pt' % n for n in ('000000', '000001', '000002', '000003', 'best_fid')] + ['graphs/fid.json']
    want += ['images/sample/%06d.png' % i for i in (0, 3)] + ['images/%s/%06d.jpg' % (m, i) for m in matrices for i in (0, 3)]
    assert files_under(root) == sorted(want)
    with open(os.path.join(root, 'graphs', 'fid.json')) as f:
        assert [e['iter'] for e in json.load(f)] == [1, 2, 3]
    assert Image.open(os.path.join(root, 'images', 'sample', '000000.png')).size == (4 * (SIZE + 2) + 2, SIZE + 2 + 2)
    assert Image.open(os.path.join(root, 'images', 'matrix', '000003.jpg')).size == (6 * (SIZE + 2) + 2,) * 2
    best = torch.load(os.path.join(root, 'checkpoint', 'best_fid.pt'), map_location='cpu', weights_only=False)
    at2 = torch.load(os.path.join(root, 'checkpoint', '000002.pt'), map_location='cpu', weights_only=False)
    assert all(torch.equal(best['g_ema'][k], at2['g_ema'][k]) for k in at2['g_ema'])
    # a vanilla run has no groups: the sample grid only
    plain = make_trainer(False)
    assert [os.path.relpath(p, root) for p in plain.save_images(7, root, tracker)] == ['images/sample/000007.png']


def test_train_without_a_tracker_writes_checkpoints_only(emu_backend, tmp_path):
    tr = make_trainer(True, min_evaluate_interval=1, save_images_interval=1, save_nets_interval=1)
    root = str(tmp_path / 'run')
    assert tr.train(save_dir=root, iters=2) == 2
    assert files_under(root) == ['checkpoint/000000.pt', 'checkpoint/000001.pt']
