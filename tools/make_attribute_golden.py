"""Writes tests/golden/attribute_losses.npz from the reference's own classes (CPU, build machine only; no test reads the reference):

    python tools/make_attribute_golden.py /path/to/gan-control/src

* HairCriterion (``__call__`` and ``predict``, called unbound: its ``__init__`` needs a GPU and they use none of its state), StyleCriterion
  and Face3dmmCriterion on small random inputs;
* LossModelClass.calc_mini_batch_loss with ``no_model=True`` for hair_loss, style_loss and the eight recon names, values and input gradients,
  on a mini-batch of 8 (same block of 4) with one intermediate level, once per focus setting;
* RandomMiniBatchUtils under fixed ``np.random.seed``s: the places after construction and after two more draws, get_sub_group /
  get_not_sub_group of the row numbers, and re_arrange_z on a small z;
* the seven slices of Face3dmmSkeleton.extract_futures_from_vec.

Only inputs and recorded outputs are stored.  Packages the reference imports but these code paths never call are stubbed.
"""
import copy
import json
import os
import sys
from unittest import mock

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'attribute_losses.npz')

LOSS_CFG = {'lower_thres': [0.3], 'upper_thres': [1.2], 'last_lower_thres': 0.2, 'last_upper_thres': 1.3, 'intermediate_layers_weights': [0.5],
            'last_layer_weight': 1.5}
FOCUS = {'a': ['not_same_as_last_layer', 'same_as_last_layer'], 'b': ['same_as_last_layer', 'not_same_as_last_layer']}
RECON = ['recon_3d_loss', 'recon_id_loss', 'recon_ex_loss', 'recon_tex_loss', 'recon_angles_loss', 'recon_gamma_loss', 'recon_xy_loss', 'recon_z_loss']
# last-level row shapes of the mini-batch cases; style thresholds are on the 1e5 scale of its distances
LAST_SHAPES = dict({'hair_loss': (4, 8, 8), 'style_loss': (3, 3)}, **{name: (27,) for name in RECON})
SUB_GROUPS = {'a': {'place_in_latent': [0, 100], 'place_in_mini_batch': [0, 4], 'count_in_mini_bach': [2, 6]},
              'b': {'place_in_latent': [100, 300], 'place_in_mini_batch': [4, 6], 'count_in_mini_bach': [0, 4]},
              'other': {'place_in_latent': [300, 512], 'place_in_mini_batch': [6, 8], 'count_in_mini_bach': [0, 2]}}
SEEDS = (0, 1, 2, 3, 4, 5)


def hair_features(n, gen):
    """[n, 4, 8, 8]: a masked image and a soft mask; row 0 has no hair at all, row 1 less than 1 % of the pixels."""
    img = torch.rand(n, 3, 8, 8, generator=gen) * 2 - 1
    mask = (torch.rand(n, 1, 8, 8, generator=gen) > 0.5).float() * torch.rand(n, 1, 8, 8, generator=gen)
    mask[0] = 0
    mask[1] = 0
    mask[1, 0, 0, 0] = 0.3
    return torch.cat([img * mask, mask], dim=1)


def last_features(name, n, gen):
    if name == 'hair_loss':
        return hair_features(n, gen)
    if name == 'style_loss':
        return torch.randn(n, *LAST_SHAPES[name], generator=gen) * 1e-3
    return torch.randn(n, *LAST_SHAPES[name], generator=gen)


def places_array(places):
    return np.zeros((0, 2), dtype=np.int64) if places is None else np.asarray(places, dtype=np.int64).reshape(-1, 2)


def main(ref_src):
    sys.path.insert(0, ref_src)
    stubs = {name: mock.MagicMock() for name in ('gan_control.evaluation.hair', 'gan_control.losses.face3dmm_recon.models.pytorch_3d_recon_model',
                                                 'gan_control.utils.tensor_transforms', 'yaml', 'torchvision')
             if name not in sys.modules}
    with mock.patch.dict(sys.modules, stubs):
        from gan_control.losses.hair_loss.hair_criterion import HairCriterion
        from gan_control.losses.stayle.style_criterion import StyleCriterion
        from gan_control.losses.face3dmm_recon.face3dmm_criterion import Face3dmmCriterion
        from gan_control.losses.face3dmm_recon.face3dmm_skeleton import Face3dmmSkeleton
        from gan_control.losses.loss_model import LossModelClass
        from gan_control.utils.mini_batch_random_multi_split_utils import RandomMiniBatchUtils
        out = {}
        gen = torch.Generator().manual_seed(2024)

        # -- the three criteria ------------------------------------------------------------------------------------------------------
        hs, hq = hair_features(5, gen), hair_features(4, gen)
        out.update({'hair/signatures': hs, 'hair/queries': hq, 'hair/distances': HairCriterion.__call__(None, hs, hq), 'hair/predict': HairCriterion.predict(hs)})
        ss, sq = torch.randn(4, 3, 3, generator=gen) * 1e-3, torch.randn(3, 3, 3, generator=gen) * 1e-3
        out.update({'style/signatures': ss, 'style/queries': sq, 'style/distances': StyleCriterion()(ss, sq)})
        rs, rq = torch.randn(5, 27, generator=gen), torch.randn(4, 27, generator=gen)
        crit = Face3dmmCriterion('recon_gamma_loss')
        out.update({'recon/signatures': rs, 'recon/queries': rq, 'recon/distances': crit(rs, rq), 'recon/controller': crit.controller_criterion(rs, rs.flip(0))})

        # -- calc_mini_batch_loss per loss name ---------------------------------------------------------------------------------------
        identity = lambda self, *a, **k: self          # noqa: E731  (HairCriterion.__init__ moves three constants to a GPU it never reads)
        with mock.patch.object(torch.Tensor, 'cuda', identity), mock.patch.object(torch.nn.Module, 'cuda', identity):
            for name in ['hair_loss', 'style_loss'] + RECON:
                inter = torch.randn(8, 2, 3, 3, generator=gen).requires_grad_(True)
                last = last_features(name, 8, gen).requires_grad_(True)
                out.update({'loss/%s/inter' % name: inter, 'loss/%s/last' % name: last})
                for tag, focus in FOCUS.items():
                    cfg = dict(copy.deepcopy(LOSS_CFG), focus_on_list=focus)
                    if name == 'style_loss':
                        cfg.update(last_lower_thres=0.1, last_upper_thres=0.3)
                    if name == 'hair_loss':
                        cfg.update(last_lower_thres=0.05, last_upper_thres=0.3)
                    lm = LossModelClass(cfg, loss_name=name, mini_batch_size=8, no_model=True)
                    loss = lm.calc_mini_batch_loss(last_layer_same_features=[inter[:4], last[:4]], last_layer_not_same_features=[inter[4:], last[4:]])
                    g_inter, g_last = torch.autograd.grad(loss, [inter, last])
                    out.update({'loss/%s/%s/value' % (name, tag): loss, 'loss/%s/%s/g_inter' % (name, tag): g_inter, 'loss/%s/%s/g_last' % (name, tag): g_last})
                    out['loss/%s/%s/cfg' % (name, tag)] = np.array(json.dumps(cfg))
                    print('%-18s focus %s  loss %.6f' % (name, tag, float(loss)))

        # -- RandomMiniBatchUtils ---------------------------------------------------------------------------------------------------------
        order = torch.arange(8)
        z0 = torch.randint(-99, 100, (8, 512), generator=gen).float()          # (whole numbers: the copies are exact and the file stays small)
        out['random/z'] = z0
        out['random/sub_groups'] = np.array(json.dumps(SUB_GROUPS))
        for seed in SEEDS:
            np.random.seed(seed)
            utils = RandomMiniBatchUtils(8, copy.deepcopy(SUB_GROUPS), total_batch=8)
            for draw in range(3):
                if draw:
                    utils.randomize_places_in_batch()
                for group in ('a', 'b', 'other'):
                    places = utils.place_in_mini_batch_dict[group]
                    key = 'random/%d/%d/%s' % (seed, draw, group)
                    out[key + '/places'] = places_array(places)
                    if places is not None:
                        out[key + '/sub'] = utils.get_sub_group(order, group)
                        out[key + '/not_sub'] = utils.get_not_sub_group(order, group)
            out['random/%d/z' % seed] = utils.re_arrange_z([z0.clone()], 0)[0]

        # -- the seven slices -----------------------------------------------------------------------------------------------------------
        vec = torch.randn(3, 257, generator=gen)
        out['slices/vec'] = vec
        for i, futures in enumerate(Face3dmmSkeleton.extract_futures_from_vec([vec])):
            assert len(futures) == 1
            out['slices/%d' % i] = futures[0]

    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    arrays = {k: (v.astype(np.int8) if k.startswith('random/') and k.endswith('z') else v) for k, v in arrays.items()}          # |z| < 100, whole
    np.savez_compressed(OUT, **arrays)
    print('%s: %d arrays, %d bytes' % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
