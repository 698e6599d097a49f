"""The separability evaluation end to end on the GPU: a 64 x 64 generator, the ArcFace IR-SE 50 predictor (the smallest backbone
tests/arcface_checks.py builds) with procedural weights, 40 samples, all five levels.

The kernel path of calc_same_not_same_list is held against the chunked torch path on the SAME features: the closest not-same signature of
every query must be the same row, and every distance within twice the derived bound of tests/test_pairwise_gpu.py (each path is within
(K + 4) * 2^-24 of the exact value, relative to it).
"""
import numpy as np
import pytest
import torch

import arcface_checks as ac

from gan_control_amd.evaluation import separability
from gan_control_amd.losses import ArcFaceSkeleton, Backbone, LossModelClass
from gan_control_amd.models.op import pairwise as pw

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
LEVEL_K = [64 * 56 * 56, 128 * 28 * 28, 256 * 14 * 14, 512 * 7 * 7, 512]


def test_separability_end_to_end(monkeypatch):
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    generator = GeneratorTrainer(default_config(64, 4), device=DEV, seed=0, fused_adam=False).g_ema.eval()
    cfg = dict(ac.FFHQ_EMBEDDING, center_crop=60)
    skeleton = ArcFaceSkeleton(cfg, state_dict=ac.fill_weights(Backbone(50, 0.6, mode='ir_se').state_dict())).to(DEV)
    lm = LossModelClass(cfg, 'embedding_loss', mini_batch_size=4, skeleton_model=skeleton)
    launched = []
    real = pw.HipBackend._launch
    monkeypatch.setattr(pw.HipBackend, '_launch', lambda self, dev, entry, *a, **k: (launched.append(entry), real(self, dev, entry, *a, **k))[1])
    result, images = separability.calc_separability(generator, lm, same_noise_for_same_id=True, num_of_samples=40, return_images=True, seed=0)
    assert launched.count(pw.ENTRY) == 5 and len(result) == 5 and len(images) == 40 and images[0].shape == (64, 64, 3)
    # the same features through both paths
    emb, _ = separability.compute_half_same_ids_embeddings_from_generator(generator, lm, 40, same_noise_for_same_id=True, seed=0)
    assert [e.shape[1:].numel() for e in emb] == LEVEL_K and all(e.is_cuda for e in emb)
    sig, que, pids = [e[:20] for e in emb], [e[20:] for e in emb], np.arange(20)
    del launched[:]
    kernel = lm.calc_same_not_same_list(sig, que, pids, pids)
    assert launched.count(pw.ENTRY) == 5
    monkeypatch.setattr(pw, 'kernel_taken', lambda *a, **k: False)
    del launched[:]
    chunked = lm.calc_same_not_same_list(sig, que, pids, pids)
    assert pw.ENTRY not in launched
    for i, (a, b, k) in enumerate(zip(kernel, chunked, LEVEL_K)):
        assert np.array_equal(np.asarray(a['pids_2nd_best_pairs_df']['signature']), np.asarray(b['pids_2nd_best_pairs_df']['signature'])), i
        assert np.array_equal(np.asarray(a['pids_2nd_best_pairs_df']['queries']), np.asarray(b['pids_2nd_best_pairs_df']['queries']))
        for key in ('same', 'not_same', 'all_not_same'):
            x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
            err = float((np.abs(x - y) / np.maximum(y, 1e-300)).max())
            print('separability level %d %-12s kernel vs chunked: max relative difference %.3e (bound %.3e)' % (i, key, err, 2 * (k + 4) * U))
            assert x.shape == y.shape and bool((np.abs(x - y) <= 2 * (k + 4) * U * np.maximum(x, y)).all()), (i, key, err)
        assert [len(a[key]) for key in ('same', 'not_same', 'all_not_same')] == [20, 20, 380]
    assert [[len(level[key]) for key in ('same', 'not_same', 'all_not_same')] for level in result] == [[20, 20, 380]] * 5
    # pairs that share the identity sub-latent and the injection noise sit closer than strangers, at every level
    for i, level in enumerate(kernel):
        print('separability level %d: same %.5f  2nd best %.5f  all not same %.5f' % (i, np.mean(level['same']), np.mean(level['not_same']), np.mean(level['all_not_same'])))
        assert np.mean(level['same']) < np.mean(level['all_not_same']), i
