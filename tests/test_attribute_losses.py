"""The attribute-loss stage without a GPU: the hair / style / 3DMM criteria, extract_futures_from_vec, RandomMiniBatchUtils and
calc_mini_batch_loss for the new loss names against recordings of the reference's own classes (tests/golden/attribute_losses.npz, written by
tools/make_attribute_golden.py); the index form of the same / not-same split; the torch path of models.op.pair_hinge and ``fused=True``
bit for bit against today's composition; every refusal of the new entries before a launch; the trainer's recon_3d_loss sub-losses, random
mini-batch mode and the ``fused_attribute_losses`` key on the emulated backend."""
import copy
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

AL = load_golden('attribute_losses')
RECON = ['recon_3d_loss', 'recon_id_loss', 'recon_ex_loss', 'recon_tex_loss', 'recon_angles_loss', 'recon_gamma_loss', 'recon_xy_loss', 'recon_z_loss']
NEW_NAMES = ['hair_loss', 'style_loss'] + RECON
TOL = 1e-5          # float32 rounding of sums of a few hundred terms, relative to the largest value (the tolerance of tests/test_losses.py)


def t(key):
    return torch.from_numpy(AL[key])


# -- golden parity ---------------------------------------------------------------------------------------------------------------------------
def test_new_criteria_match_the_reference():
    from gan_control_amd.losses import CRITERIA, PREDICTORS
    for tag, name in (('hair', 'hair_loss'), ('style', 'style_loss'), ('recon', 'recon_gamma_loss')):
        got = CRITERIA[name](t(tag + '/signatures'), t(tag + '/queries'))
        want = t(tag + '/distances')
        assert got.shape == want.shape and rel_err(got, want) <= TOL, tag
    # rows 0 and 1 of the hair inputs have no / almost no hair: their distances are exactly zero, and predict() zeroes the empty one
    assert bool((CRITERIA['hair_loss'](t('hair/signatures'), t('hair/queries'))[:2] == 0).all())
    assert rel_err(PREDICTORS['hair_loss'][0](t('hair/signatures')), t('hair/predict')) <= TOL
    assert PREDICTORS['recon_gamma_loss'][0] is None
    rs = t('recon/signatures')
    assert rel_err(PREDICTORS['recon_gamma_loss'][1](rs, rs.flip(0)), t('recon/controller')) <= TOL
    assert all(CRITERIA[n] is CRITERIA['recon_3d_loss'] for n in RECON)


def test_extract_futures_from_vec_gives_the_seven_views():
    from gan_control_amd.losses import extract_futures_from_vec
    vec = t('slices/vec')
    futures = extract_futures_from_vec([torch.zeros(3, 4), vec])
    assert len(futures) == 7
    for i, f in enumerate(futures):
        assert isinstance(f, list) and len(f) == 1 and torch.equal(f[0], t('slices/%d' % i))
        assert f[0].untyped_storage().data_ptr() == vec.untyped_storage().data_ptr()          # a view, never a copy
    assert sum(f[0].shape[1] for f in futures) == 257


@pytest.mark.parametrize('name', NEW_NAMES)
def test_calc_mini_batch_loss_matches_the_reference(name):
    from gan_control_amd.losses import LossModelClass
    for tag in ('a', 'b'):
        cfg = json.loads(str(AL['loss/%s/%s/cfg' % (name, tag)]))
        for fused in (False, True):
            inter, last = t('loss/%s/inter' % name).requires_grad_(True), t('loss/%s/last' % name).requires_grad_(True)
            lm = LossModelClass(cfg, name, mini_batch_size=8, no_model=True, fused=fused)
            loss = lm.calc_mini_batch_loss([inter[:4], last[:4]], [inter[4:], last[4:]])
            want = float(AL['loss/%s/%s/value' % (name, tag)])
            assert abs(float(loss) - want) <= TOL * max(1.0, abs(want)), (name, tag, fused)
            g_inter, g_last = torch.autograd.grad(loss, [inter, last])
            assert rel_err(g_inter, t('loss/%s/%s/g_inter' % (name, tag))) <= TOL and rel_err(g_last, t('loss/%s/%s/g_last' % (name, tag))) <= TOL


def test_unknown_loss_name_and_missing_predictor_still_raise():
    from gan_control_amd.losses import LossModelClass
    cfg = json.loads(str(AL['loss/hair_loss/a/cfg']))
    with pytest.raises(ValueError, match='not valid'):
        LossModelClass(cfg, 'classification_loss', no_model=True)
    with pytest.raises(RuntimeError, match='predictor'):
        LossModelClass(cfg, 'hair_loss')
    LossModelClass(cfg, 'hair_loss', skeleton_model=lambda x: [x])


# -- RandomMiniBatchUtils ----------------------------------------------------------------------------------------------------------------------
SUB_GROUPS = json.loads(str(AL['random/sub_groups']))
SEEDS = sorted({int(k.split('/')[1]) for k in AL if k.startswith('random/') and k.split('/')[1].isdigit()})


def places_array(places):
    return np.zeros((0, 2), dtype=np.int64) if places is None else np.asarray(places, dtype=np.int64).reshape(-1, 2)


def test_random_places_follow_the_reference_under_a_seed():
    from gan_control_amd.utils.mini_batch_utils import RandomMiniBatchUtils
    order = torch.arange(8)
    assert len(SEEDS) >= 6
    seen = set()
    for seed in SEEDS:
        np.random.seed(seed)
        utils = RandomMiniBatchUtils(8, copy.deepcopy(SUB_GROUPS), total_batch=8)
        for draw in range(3):
            if draw:
                utils.randomize_places_in_batch()
            for group in ('a', 'b', 'other'):
                key = 'random/%d/%d/%s' % (seed, draw, group)
                places = utils.place_in_mini_batch_dict[group]
                assert np.array_equal(places_array(places), AL[key + '/places']), key
                seen.add(tuple(map(tuple, places_array(places).tolist())))
                if places is not None:
                    assert torch.equal(utils.get_sub_group(order, group), t(key + '/sub')), key
                    assert torch.equal(utils.get_not_sub_group(order, group), t(key + '/not_sub')), key
        z = utils.re_arrange_z([t('random/z').float()], 0)[0]
        assert torch.equal(z, t('random/%d/z' % seed).float()), seed
    assert len(seen) > 6          # (the recording covers merged ranges, several ranges and empty groups)
    assert () in seen and any(len(p) > 1 for p in seen) and any(len(p) == 1 and p[0][1] - p[0][0] > 2 for p in seen)


def test_random_utils_checks_and_own_generator():
    from gan_control_amd.utils.mini_batch_utils import RandomMiniBatchUtils
    with pytest.raises(ValueError, match='mini_batch 8 vs. total_batch 16'):
        RandomMiniBatchUtils(8, copy.deepcopy(SUB_GROUPS), total_batch=16)
    utils = RandomMiniBatchUtils(8, copy.deepcopy(SUB_GROUPS), total_batch=8, rng=np.random.RandomState(3))
    with pytest.raises(ValueError, match='not suppurting mixing'):
        utils.re_arrange_z([torch.zeros(8, 512), torch.zeros(8, 512)], 0)
    state = np.random.get_state()[1].copy()
    twin = RandomMiniBatchUtils(8, copy.deepcopy(SUB_GROUPS), total_batch=8, rng=np.random.RandomState(3))
    assert twin.place_in_mini_batch_dict == utils.place_in_mini_batch_dict
    assert np.array_equal(np.random.get_state()[1], state)          # a generator of its own leaves the global one alone
    utils.place_in_mini_batch_dict['a'] = [[2, 6]]
    noise = [torch.arange(8.).view(8, 1, 1, 1).repeat(1, 1, 2, 2)]
    assert utils.re_arrange_inject_noise(noise, 'a')[0][:, 0, 0, 0].tolist() == [0, 1, 2, 2, 4, 4, 6, 7]


FFHQ_GROUPS = {'id': [0, 4], 'expression': [4, 6], 'orientation': [6, 8], 'gamma': [8, 10], 'age': [10, 12], 'hair': [12, 14], 'other': [14, 16]}


def ffhq_sub_groups():
    lo, out = 0, {}
    for name, rows in FFHQ_GROUPS.items():
        width = 128 if name == 'id' else 64
        out[name] = {'place_in_latent': [lo, lo + width], 'place_in_mini_batch': rows, 'count_in_mini_bach': [2, 12]}
        lo += width
    return out


def test_row_form_agrees_with_the_slices():
    from gan_control_amd.utils.mini_batch_utils import MiniBatchUtils, RandomMiniBatchUtils
    f = [torch.arange(16.).view(16, 1) * torch.ones(1, 5), torch.arange(16 * 6.).view(16, 2, 3)]
    np.random.seed(11)
    for utils in (MiniBatchUtils(16, ffhq_sub_groups(), total_batch=16), RandomMiniBatchUtils(16, ffhq_sub_groups(), total_batch=16)):
        for group in FFHQ_GROUPS:
            same, other = utils.extract_same_not_same_from_list(f, group)
            rows, n_same, n_not_same = utils.same_not_same_rows(group)
            assert all(isinstance(r, int) for r in rows) and (n_same, n_not_same) == (same[0].shape[0], other[0].shape[0])
            for level in range(2):
                assert torch.equal(torch.cat([same[level], other[level]]), f[level][rows])


# -- the torch path ----------------------------------------------------------------------------------------------------------------------------
def composition(feats, n_same, criterion, focus, lower, upper, weight):
    """Today's calc_mini_batch_loss body for one level: cat, criterion, masks, _level_loss."""
    from gan_control_amd.losses import LossModelClass
    same, other = feats[:n_same], feats[n_same:]
    both = torch.cat([same, other], dim=0)
    dist = criterion(both, both)
    masks = LossModelClass.pair_masks(same.shape[0], other.shape[0], device=feats.device)
    return weight * LossModelClass._level_loss(None, dist, masks, focus, lower, upper)


@pytest.mark.parametrize('focus', ['same_as_last_layer', 'not_same_as_last_layer'])
@pytest.mark.parametrize('mode,name,shape', [('abs', 'age_loss', (11,)), ('abs', 'orientation_loss', (3, 7)), ('sq', 'embedding_loss', (13,)),
                                             ('msq', 'style_loss', (4, 4)), ('abs', 'recon_gamma_loss', (27,))])
def test_torch_path_equals_todays_composition_bit_for_bit(mode, name, shape, focus):
    from gan_control_amd.losses import CRITERIA
    from gan_control_amd.models.op import pair_hinge as ph
    gen = torch.Generator().manual_seed(len(name))
    scale = 1e5 if mode == 'msq' else 1.0
    batch = torch.randn(12, *shape, generator=gen) * (3e-3 if mode == 'msq' else 1.0)
    lower, upper = (0.2, 1.4) if mode != 'sq' else (10.0, 30.0)
    for rows, n_same in (([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], 4), ([6, 7, 8, 9, 0, 1, 2, 3, 4, 5, 10, 11], 4), ([4, 5, 9, 0, 1, 3, 11], 3)):
        a, b = batch.clone().requires_grad_(True), batch.clone().requires_grad_(True)
        want = composition(a[rows], n_same, CRITERIA[name], focus, lower, upper, 0.75)
        identity = rows == list(range(12))
        got = ph.pair_hinge_loss(b, n_same, len(rows) - n_same, mode, lower, upper, focus, 0.75, None if identity else rows, None, scale)
        assert got.dim() == 0 and torch.equal(got, want), (rows, float(got), float(want))
        ga, gb = torch.autograd.grad(want, a)[0], torch.autograd.grad(got, b)[0]
        assert torch.equal(ga, gb) and float(ga.abs().max()) > 0
        unused = [r for r in range(12) if r not in rows]
        assert bool((gb[unused] == 0).all())


@pytest.mark.parametrize('focus', ['same_as_last_layer', 'not_same_as_last_layer'])
def test_torch_path_with_row_valid_equals_the_hair_criterion(focus):
    from gan_control_amd.losses import CRITERIA
    from gan_control_amd.losses.loss_model import _hair_colours
    from gan_control_amd.models.op import pair_hinge as ph
    feats = t('loss/hair_loss/last')
    for rows in (list(range(8)), [5, 4, 0, 1, 2, 7]):
        a, b = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
        want = composition(a[rows], 2, CRITERIA['hair_loss'], focus, 0.05, 0.3, 1.5)
        colours, valid = _hair_colours(b)
        assert valid.dtype == torch.bool and not bool(valid[0]) and not bool(valid[1]) and bool(valid[2:].all())
        got = ph.pair_hinge_loss(colours, 2, len(rows) - 2, 'abs', 0.05, 0.3, focus, 1.5, None if rows == list(range(8)) else rows, valid)
        assert torch.equal(got, want)
        assert torch.equal(torch.autograd.grad(want, a)[0], torch.autograd.grad(got, b)[0])


def test_pair_hinge_argument_checks_and_the_empty_set():
    from gan_control_amd.models.op import pair_hinge as ph
    f = torch.randn(6, 5)
    for kw, word in ((dict(mode='l1'), 'mode must be'), (dict(focus='last'), 'focus_on_list entry'), (dict(n_same=2, n_not_same=5), '6 rows for'),
                     (dict(row_index=[0, 1, 2, 3, 4, 4]), 'distinct rows'), (dict(row_index=[0, 1, 2, 3, 4, 6]), 'distinct rows'),
                     (dict(row_index=[0, 1, 2]), 'distinct rows')):
        args = dict(dict(n_same=2, n_not_same=4, mode='abs', lower=0.1, upper=0.5, focus='same_as_last_layer'), **kw)
        with pytest.raises(ValueError, match=word):
            ph.pair_hinge_loss(f, **args)
    assert ph.set_sizes(2, 2, 'same_as_last_layer') == (1, 5) and ph.set_sizes(3, 5, 'not_same_as_last_layer') == (2, 26)
    assert ph.set_sizes(1, 3, 'same_as_last_layer')[0] == 0 and not ph.kernel_taken(f, 1, 5, 'same_as_last_layer')
    assert bool(torch.isnan(ph.pair_hinge_loss(f, 1, 5, 'abs', 0.1, 0.5, 'same_as_last_layer')))          # torch's mean of an empty set, kept


@pytest.mark.parametrize('name,shape', [('embedding_loss', (16,)), ('dog_id_loss', (9,)), ('orientation_loss', (3, 6)), ('expression_loss', (2, 5)),
                                        ('age_loss', (10,)), ('hair_loss', (4, 8, 8)), ('style_loss', (3, 3)), ('recon_z_loss', (1,)), ('recon_id_loss', (80,))])
def test_fused_equals_unfused_bit_for_bit_on_the_cpu(name, shape):
    from gan_control_amd.losses import LossModelClass
    gen = torch.Generator().manual_seed(7)
    base = {'lower_thres': [0.3, 0.2], 'upper_thres': [1.2, 0.9], 'last_lower_thres': 0.2, 'last_upper_thres': 1.3, 'intermediate_layers_weights': [0.5, 0.0],
            'last_layer_weight': 1.5, 'focus_on_list': ['not_same_as_last_layer', 'same_as_last_layer', 'same_as_last_layer']}
    last = t('loss/hair_loss/last')[:8] if name == 'hair_loss' else torch.randn(8, *shape, generator=gen) * (3e-3 if name == 'style_loss' else 1.0)
    feats = [torch.randn(8, 2, 3, 3, generator=gen), torch.randn(8, 3, 2, 2, generator=gen), last]
    rows = [2, 3, 6, 7, 0, 1, 4, 5]
    for as_last in (False, True):
        if as_last and name in ('embedding_loss', 'dog_id_loss', 'style_loss'):
            continue          # (the squared criteria leave [n, n, c, h] on 4-D maps; the style criterion reduces two axes of three)
        cfg = dict(base, intermediate_criterion_as_last_layer=as_last)
        levels = [last.clone(), last.clone() * 0.5, last] if as_last else feats
        results = []
        for fused in (False, True):
            fs = [f.clone().requires_grad_(True) for f in levels]
            lm = LossModelClass(cfg, name, mini_batch_size=8, no_model=True, fused=fused)
            a = lm.calc_mini_batch_loss([f[:3] for f in fs], [f[3:] for f in fs])
            b = lm.calc_mini_batch_loss_rows(fs, rows, 4, 4)
            results.append((a, b, torch.autograd.grad(a, fs, allow_unused=True), torch.autograd.grad(b, fs, allow_unused=True)))
        (a0, b0, ga0, gb0), (a1, b1, ga1, gb1) = results
        assert torch.equal(a0, a1) and torch.equal(b0, b1)
        for x, y in list(zip(ga0, ga1)) + list(zip(gb0, gb1)):
            assert (x is None and y is None) or torch.equal(x, y)
        assert ga0[1] is None and ga0[0] is not None          # the zero-weight level is skipped on both paths
    # a custom criterion always takes the torch path: the fused flag changes nothing, and the op is never asked
    calls = []
    lm = LossModelClass(base, name, no_model=True, fused=True, criterion=lambda s, q: calls.append(1) or (s.flatten(1).unsqueeze(1) - q.flatten(1).unsqueeze(0)).abs().sum(-1))
    lm.calc_mini_batch_loss([f[:4] for f in feats], [f[4:] for f in feats])
    assert calls == [1]


# -- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_without_a_gpu():
    """Every refusal of the pair-hinge entries comes before a launch, so the calls are safe on a host without a GPU (no pointer is read)."""
    import ctypes
    from gan_control_amd import _lib
    lib = _lib.load()
    p = 4096          # any non-null address

    def idx(*rows):
        return (ctypes.c_int32 * len(rows))(*rows)

    def fwd(f=p, stride=8, n_rows=6, index=None, valid=None, n_same=2, n_not=4, k=8, mode=0, scale=1.0, focus=0, loss=p, d=p, c=p, ws=None, nbytes=0):
        rc = lib.gc_pair_hinge_fwd_f32(f, stride, n_rows, index, valid, n_same, n_not, k, mode, scale, focus, 0.1, 0.5, 1.0, loss, d, c, ws, nbytes, None)
        return rc, lib.gc_last_error()

    def bwd(f=p, stride=8, n_rows=6, index=None, valid=None, n=6, k=8, mode=0, c=p, g=p, df=p):
        rc = lib.gc_pair_hinge_bwd_f32(f, stride, n_rows, index, valid, n, k, mode, 1.0, c, g, df, None)
        return rc, lib.gc_last_error()

    long_k = 200704
    need = lib.gc_pair_hinge_workspace(16, long_k)
    cases = [(fwd, dict(f=None), -1, b'null pointer'), (fwd, dict(loss=None), -1, b'null pointer'), (fwd, dict(d=None), -1, b'null pointer'),
             (fwd, dict(c=None), -1, b'null pointer'), (fwd, dict(k=0), -1, b'k at least 1'), (fwd, dict(n_same=-2), -1, b'negative'),
             (fwd, dict(n_same=1, n_not=0, n_rows=1), -1, b'n at least 2'), (fwd, dict(n_rows=5), -1, b'n_rows at least n'),
             (fwd, dict(n_rows=7), -1, b'without a row index'), (fwd, dict(stride=7), -1, b'shorter than the rows'), (fwd, dict(mode=3), -1, b'unknown mode 3'),
             (fwd, dict(focus=2), -1, b'unknown focus 2'), (fwd, dict(n_same=2, n_not=63, n_rows=65), -2, b'at most 64 rows'),
             (fwd, dict(n_same=2 ** 30, n_not=2 ** 30, n_rows=65), -2, b'at most 64 rows'),
             (fwd, dict(n_rows=1025, index=idx(0, 1, 2, 3, 4, 5)), -2, b'at most 1024 rows'),
             (fwd, dict(n_rows=8, index=idx(0, 1, 2, 3, 4, 8)), -1, b'row_index[5] = 8'), (fwd, dict(n_rows=8, index=idx(0, 1, 2, -1, 4, 5)), -1, b'row_index[3] = -1'),
             (fwd, dict(n_rows=8, index=idx(0, 1, 2, 3, 4, 2)), -1, b'row_index[5] = 2'),
             (fwd, dict(n_same=1, n_not=5), -1, b'empty pair set'), (fwd, dict(n_same=5, n_not=1, focus=1), -1, b'empty pair set'),
             (fwd, dict(n_same=2, n_not=0, n_rows=2), -1, b'empty pair set'),
             (fwd, dict(n_same=4, n_not=12, n_rows=16, k=long_k, stride=long_k), -4, b'workspace too small'),
             (fwd, dict(n_same=4, n_not=12, n_rows=16, k=long_k, stride=long_k, ws=p, nbytes=need - 4), -4, b'workspace too small'),
             (bwd, dict(f=None), -1, b'null pointer'), (bwd, dict(c=None), -1, b'null pointer'), (bwd, dict(g=None), -1, b'null pointer'),
             (bwd, dict(df=None), -1, b'null pointer'), (bwd, dict(k=-1), -1, b'k at least 1'), (bwd, dict(n=1, n_rows=1), -1, b'n at least 2'),
             (bwd, dict(n=65, n_rows=65), -2, b'at most 64 rows'), (bwd, dict(stride=3), -1, b'shorter than the rows'), (bwd, dict(mode=-1), -1, b'unknown mode -1'),
             (bwd, dict(n_rows=7), -1, b'without a row index'), (bwd, dict(n_rows=9, index=idx(0, 1, 2, 3, 9, 5)), -1, b'row_index[4] = 9')]
    for call, kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (call.__name__, kw, rc, msg)
    # the workspace is a function of (n, k) alone: nothing while n k <= 8192 (one launch), splits x n x n floats beyond, 0 for refused extents
    ws = lib.gc_pair_hinge_workspace
    assert ws(16, 512) == 0 and ws(64, 128) == 0 and ws(2, 4096) == 0 and ws(16, 101) == 0
    assert ws(16, 513) == 2 * 16 * 16 * 4 and ws(64, 129) == 64 * 64 * 4 and ws(3, 2731) == 10 * 9 * 4
    assert need % (16 * 16 * 4) == 0 and 2 <= need // (16 * 16 * 4) <= 512
    assert ws(65, 8) == 0 and ws(1, 8) == 0 and ws(16, 0) == 0 and ws(-4, 8) == 0


# -- the trainer on the emulated backend ---------------------------------------------------------------------------------------------------------
class StubPredictor(torch.nn.Module):
    """Stands in for a pretrained attribute network: [pooled feature map, a vector of ``dim`` values], frozen."""

    def __init__(self, dim, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.register_buffer('proj', torch.randn(3 * 16, dim, generator=gen) * 0.3)

    def forward(self, img):
        pooled = torch.nn.functional.adaptive_avg_pool2d(img, 4)
        return [pooled, pooled.flatten(1) @ self.proj]


def hinge_cfg(group=None, enabled=True, **kw):
    cfg = dict({'lower_thres': [0.01], 'upper_thres': [0.5], 'last_lower_thres': 0.05, 'last_upper_thres': 3.0, 'intermediate_layers_weights': [0.5],
                'last_layer_weight': 1.0, 'focus_on_list': ['not_same_as_last_layer', 'same_as_last_layer'], 'enabled': enabled}, **kw)
    if group is not None:
        cfg['same_group_name'] = group
    return cfg


def controllable_trainer(device, **training_keys):
    """A 32 x 32 controllable trainer on the FFHQ mini-batch layout with two stub predictors: an embedding and a 3DMM vector [n, 257] whose
    gamma and ex sub-losses are enabled."""
    import op_checks as oc
    from gan_control_amd.losses import LossModelClass
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer
    ref = oc.load_configs()['ffhq']
    cfg = copy.deepcopy({'model_config': ref['model_config'], 'training_config': ref['training_config']})
    cfg['model_config']['size'] = 32
    tc = cfg['training_config']
    tc['embedding_loss'] = hinge_cfg('id')
    sub = {x + '_loss': hinge_cfg(group, enabled=x in ('gamma', 'ex'), intermediate_layers_weights=[], lower_thres=[], upper_thres=[], focus_on_list=['same_as_last_layer'])
           for x, group in (('id', 'id'), ('ex', 'expression'), ('tex', 'id'), ('angles', 'orientation'), ('gamma', 'gamma'), ('xy', 'orientation'), ('z', 'orientation'))}
    tc['recon_3d_loss'] = dict(hinge_cfg(), **sub)
    tc.update(training_keys)
    losses = {'embedding_loss': LossModelClass(tc['embedding_loss'], 'embedding_loss', mini_batch_size=16, skeleton_model=StubPredictor(12, 5).to(device)),
              'recon_3d_loss': LossModelClass(tc['recon_3d_loss'], 'recon_3d_loss', mini_batch_size=16, skeleton_model=StubPredictor(257, 6).to(device))}
    return GeneratorTrainer(cfg, device=device, seed=0, fused_adam=False, loss_models=losses)


def generator_step(tr, device, mini_batches=1):
    import op_checks as oc
    from gan_control_amd.trainers.utils import requires_grad
    requires_grad(tr.generator, True)
    requires_grad(tr.discriminator, False)
    gen = torch.Generator().manual_seed(9)
    zs = [[torch.randn(16, 512, generator=gen).to(device)] for _ in range(mini_batches)]
    tr.generator_step(zs, noise=oc.seeded_noise(32, 16, 3, device))
    return torch.cat([p.grad.reshape(-1) for p in tr.generator.parameters() if p.grad is not None])


def recorded_ops(fn):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    with Recorder() as rec:
        out = fn()
    return out, rec.ops


def test_trainer_recon_sub_losses_and_the_fused_key(emu_backend):
    plain = controllable_trainer('cpu')
    assert sorted(plain.recon_sub_losses) == ['ex', 'gamma'] and not plain.fused_attribute_losses and not plain.random_places
    assert plain.recon_sub_losses['gamma'].loss_name == 'recon_gamma_loss' and plain.recon_sub_losses['gamma'].skeleton_model is None
    g_plain, ops_plain = recorded_ops(lambda: generator_step(plain, 'cpu'))
    for key in ('g_adv_loss', 'g_embedding_loss', 'gamma_loss', 'ex_loss'):
        assert float(plain.stats[key]) > 0, key
    for key in ('id_loss', 'tex_loss', 'angles_loss', 'xy_loss', 'z_loss', 'g_recon_3d_loss', 'g_gamma_loss'):
        assert key not in plain.stats, key
    # the key present and false is the key absent: the same operations in the same order, the same bits
    off = controllable_trainer('cpu', fused_attribute_losses=False)
    g_off, ops_off = recorded_ops(lambda: generator_step(off, 'cpu'))
    assert ops_off == ops_plain and len(ops_plain) > 500 and torch.equal(g_off, g_plain)
    # the key on: every loss model is flagged, the rows go through the index form (one index per level instead of slices and a cat), same values
    on = controllable_trainer('cpu', fused_attribute_losses=True)
    assert on.fused_attribute_losses and all(m.fused for m in on.loss_models.values()) and all(m.fused for m in on.recon_sub_losses.values())
    g_on, ops_on = recorded_ops(lambda: generator_step(on, 'cpu'))
    assert ops_on != ops_plain
    assert rel_err(g_on, g_plain) <= 1e-5
    for key in ('g_embedding_loss', 'gamma_loss', 'ex_loss'):
        assert abs(float(on.stats[key]) - float(plain.stats[key])) <= 1e-6 * abs(float(plain.stats[key])), key


def test_trainer_random_mode_redraws_the_places_per_mini_batch(emu_backend):
    from gan_control_amd.utils.mini_batch_utils import RandomMiniBatchUtils
    np.random.seed(5)
    tr = controllable_trainer('cpu', mini_batch_mode='random', fused_attribute_losses=True)
    assert tr.random_places and isinstance(tr.batch_utils, RandomMiniBatchUtils)
    drawn = []
    redraw = tr.batch_utils.randomize_places_in_batch

    def spy():
        redraw()
        drawn.append(copy.deepcopy(tr.batch_utils.place_in_mini_batch_dict))

    tr.batch_utils.randomize_places_in_batch = spy
    grads = generator_step(tr, 'cpu', mini_batches=2)
    assert len(drawn) == 2 and drawn[0] != drawn[1]
    assert bool(torch.isfinite(grads).all()) and float(tr.stats['gamma_loss']) > 0
