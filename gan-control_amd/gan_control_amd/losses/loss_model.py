"""Same / not-same hinge losses on predictor features: what makes gan-control "controllable".

Mirrors the part of the reference's ``LossModelClass`` (src/gan_control/losses/loss_model.py:18-38, 107-199) that the
generator step calls when ``model_config.vanilla`` is false (generator_trainer.py:407-547): ``calc_features(img)`` runs a
FROZEN predictor network and returns a list of feature tensors (intermediate layers first, the embedding last);
``calc_mini_batch_loss(same, not_same)`` turns the pairwise distances inside the mini-batch into

    weight * ( mean(relu(d_same - lower)) + mean(relu(upper - d_not_same)) )         per feature level,

where the pairs are read off the mini-batch layout: rows (2i, 2i + 1) of the "same" block share the attribute's
sub-latent (MiniBatchUtils.re_arrange_z), every other pair below the diagonal must differ.

The predictor networks themselves (ArcFace IR-SE50, Hopenet, ESR-9, DEX age, hair segmentation, 3DMM; stock CNNs with
pretrained weights the reference downloads, README.md:97-108) are NOT part of this repository: pass any module / callable
with the ``calc_features`` contract as ``skeleton_model``.  The distance functions of the reference's criteria are here
(``CRITERIA``); they are a handful of elementwise / reduction ops on ``[mini_batch, ...]`` tensors.

The evaluation half of the class (loss_model.py:204-321) is here as well: ``calc_distances_list`` / ``calc_distances`` /
``calc_same_not_same_list``, ``L1Expend`` and ``get_same_not_same_list``, which the separability evaluation (evaluation/separability.py) runs
on thousands of samples.  Their all-pairs distances and per-query minima are ``models.op.pairwise.pairwise_distances`` -- one HIP call on
device features under that module's dispatch rule, the reference's chunked formula otherwise.  ``calc_mini_batch_loss`` does not use it: the
mini-batch losses keep their autograd torch formulas by default.

``LossModelClass(..., fused=True)`` sends every level whose criterion is one of ``CRITERIA`` (or ``L1Expend``'s formula) through
``models.op.pair_hinge.pair_hinge_loss``: one HIP call forward and one backward per level under that module's dispatch rule, the same torch
expression otherwise.  The hair criterion's masked colour means stay torch ops under autograd (two reductions of a ``[n, 4, 256, 256]``
tensor); only the hinge on the resulting ``[n, 3]`` colours, with the rows' validity flags, is the fused call.  ``calc_mini_batch_loss_rows``
is the index form: the whole mini-batch's features plus the rows in "same block, then the rest" order, so nothing is sliced or concatenated.
"""
import torch


def _pairwise(fn):
    def dist(signatures, queries):
        return fn(signatures.unsqueeze(1) - queries.unsqueeze(0))
    return dist


CRITERIA = {
    # arc_face_criterion.py:15-21 (squared L2 between embeddings); dogfacenet uses the same form
    'embedding_loss': _pairwise(lambda d: d.pow(2).sum(-1)),
    'dog_id_loss': _pairwise(lambda d: d.pow(2).sum(-1)),
    # hopenet_criterion.py:32-37, esr9_criterion.py:15-20 (mean absolute difference over the last two axes)
    'orientation_loss': _pairwise(lambda d: d.abs().mean((-2, -1))),
    'expression_loss': _pairwise(lambda d: d.abs().mean((-2, -1))),
    # deep_age_criterion.py:17-22 (mean absolute difference over the last axis)
    'age_loss': _pairwise(lambda d: d.abs().mean(-1)),
}


def _hair_colours(features):
    """[n, 4, h, w] (masked image, mask) -> ([n, 3] mean hair colour in [0, 1], [n, 1] bool: more than 1 % of the pixels are hair)
    (hair_criterion.py:17-36).  The mask sum carries no gradient; an empty mask divides by one."""
    h, w = features.shape[-2:]
    mask_sum = torch.sum(features[:, 3:, :, :].detach(), dim=[-2, -1])
    colours = torch.div(torch.sum(features[:, :3, :, :], dim=[-2, -1]), mask_sum + (mask_sum < 0.5).float())
    return colours.mul(0.5).add(0.5), mask_sum > 0.01 * w * h


def _hair_distance(signatures, queries):
    """hair_criterion.py:16-44: mean absolute colour difference, zero where either row has (almost) no hair.  The mini-batch loss hands
    the same tensor in twice: its colours are reduced once (one node in the autograd graph, as on the fused path)."""
    s, s_valid = _hair_colours(signatures)
    q, q_valid = (s, s_valid) if queries is signatures else _hair_colours(queries)
    diff = (s.unsqueeze(1) - q.unsqueeze(0)) * (s_valid.unsqueeze(1) * q_valid.unsqueeze(0))
    return diff.abs().mean(-1)


def _hair_predict(features):
    """hair_criterion.py:46-54: the colour, zeroed where the mask is empty."""
    mask_sum = torch.sum(features[:, 3:, :, :].detach(), dim=[-2, -1])
    preds = torch.div(torch.sum(features[:, :3, :, :], dim=[-2, -1]), mask_sum + (mask_sum < 0.5).float())
    return preds.mul(0.5).add(0.5) * (mask_sum > 0.5)


RECON_LOSS_NAMES = ('recon_3d_loss', 'recon_id_loss', 'recon_ex_loss', 'recon_tex_loss', 'recon_angles_loss', 'recon_gamma_loss', 'recon_xy_loss',
                    'recon_z_loss')
# the 3DMM coefficient vector [n, 257] and the sub-loss that reads each slice (face3dmm_skeleton.py:36-38)
RECON_SLICES = (('id', 0, 80), ('ex', 80, 144), ('tex', 144, 224), ('angles', 224, 227), ('gamma', 227, 254), ('xy', 254, 256), ('z', 256, 257))

CRITERIA['hair_loss'] = _hair_distance
# style_criterion.py:11-16 (mean squared difference of [c, c] Gram matrices, times 1e5)
STYLE_SCALE = 1e5
CRITERIA['style_loss'] = _pairwise(lambda d: d.pow(2).mean((-2, -1)) * STYLE_SCALE)
# face3dmm_criterion.py:14-21 (mean absolute difference over the last axis), one function for the predictor and its seven slices
CRITERIA.update(dict.fromkeys(RECON_LOSS_NAMES, _pairwise(lambda d: d.abs().mean(-1))))


def extract_futures_from_vec(features):
    """The last feature [n, 257] of the 3DMM predictor cut into (id, ex, tex, angles, gamma, xy, z), each a one-element feature list
    (face3dmm_skeleton.py:36-38).  Views, never copies: the fused losses read the slices in place."""
    vec = features[-1]
    return tuple([vec[:, lo:hi]] for _, lo, hi in RECON_SLICES)


def _expected_bin(logits):
    """softmax expectation over the class index: DEX age head (deep_age_criterion.py:24-33)."""
    prob = torch.softmax(logits, dim=-1)
    return (prob * torch.arange(logits.shape[-1], device=logits.device, dtype=prob.dtype)).sum(-1)


# predict(features) and controller_criterion(pred, target) of the reference's criteria, used by the phase-2 controller's
# attribute_rec objective (controller_trainer.py:231-239)
# REPRODUCED REFERENCE QUIRK (not in SURVEY Appendix C): the age criterion's predict() returns [B] (deep_age_criterion.py:25-32) while the
# controller's target is the controls tensor -- [B] in the reference's own call, but [B, 1] when a caller keeps the column axis, and
# `self.mse(pred, target)` (:37-38) then BROADCASTS [B] against [B, 1] to [B, B] (torch only warns).  The criterion below is the same
# unguarded mse_loss on purpose: tests/test_controller.py pins the [B] case against the reference; do not "fix" the shapes here.
PREDICTORS = {
    'age_loss': (_expected_bin, lambda pred, target: torch.nn.functional.mse_loss(pred, target)),
    # hopenet_criterion.py:6-19, 38-43: three 66-bin heads -> degrees; L1 against the controls
    'orientation_loss': (lambda f: _expected_bin(f) * 3 - 99, lambda pred, target: (pred - target).abs().mean()),
    # hair_criterion.py:46-57
    'hair_loss': (_hair_predict, lambda pred, target: torch.nn.functional.mse_loss(pred, target)),
}
# face3dmm_criterion.py:23-24: no predict() in the reference (the controller reads the slice itself)
PREDICTORS.update(dict.fromkeys(RECON_LOSS_NAMES, (None, lambda pred, target: torch.abs(pred - target).mean())))


def _l1_expand(features):
    """Intermediate feature maps [n, c, h, w]: mean absolute difference of every pair (loss_model.py:140-143)."""
    return (features.unsqueeze(1) - features.unsqueeze(0)).abs().mean((2, 3, 4))


class LossModelClass:
    """config keys (configs/ffhq.json:86-160): lower_thres / upper_thres / intermediate_layers_weights per intermediate level,
    last_lower_thres / last_upper_thres / last_layer_weight, focus_on_list (one entry per level incl. the last)."""

    def __init__(self, config, loss_name='embedding_loss', mini_batch_size=4, device='cuda', no_model=False, parallel=True,
                 skeleton_model=None, criterion=None, predict_fn=None, controller_criterion_fn=None, fused=False):
        self.config, self.loss_name = config, loss_name
        self.fused = bool(fused)          # calc_mini_batch_loss through models.op.pair_hinge (module docstring); never with a custom criterion
        if skeleton_model is None and not no_model:
            raise RuntimeError('LossModelClass(%s): the pretrained predictor is not part of this repository; pass skeleton_model=<frozen '
                               'network returning the list of features>, or no_model=True to use the loss on precomputed features' % loss_name)
        self.skeleton_model = skeleton_model
        if criterion is None:
            if loss_name not in CRITERIA:
                raise ValueError('self.loss_name = %s (not valid)' % loss_name)
            criterion = CRITERIA[loss_name]
        self.last_layer_criterion = criterion
        self.lower_thres, self.upper_thres = config['lower_thres'], config['upper_thres']
        self.last_lower_thres, self.last_upper_thres = config['last_lower_thres'], config['last_upper_thres']
        self.weights = list(config['intermediate_layers_weights']) + [config['last_layer_weight']]
        self.focus_on_list = config['focus_on_list']
        self.mini_batch_size = mini_batch_size
        heads = PREDICTORS.get(loss_name, (None, None))
        self._predict_fn = predict_fn or heads[0]
        self._controller_criterion_fn = controller_criterion_fn or heads[1]

    def calc_features(self, batch):
        return self.skeleton_model(batch)

    def predict(self, generator_output_image, features=None):
        """Attribute values read off the predictor's last features (loss_model.py:107-110)."""
        if self._predict_fn is None:
            raise NotImplementedError('LossModelClass(%s).predict: pass predict_fn' % self.loss_name)
        if features is None:
            features = self.calc_features(generator_output_image)[-1]
        return self._predict_fn(features)

    def controller_criterion(self, pred, target):
        if self._controller_criterion_fn is None:
            raise NotImplementedError('LossModelClass(%s).controller_criterion: pass controller_criterion_fn' % self.loss_name)
        return self._controller_criterion_fn(pred, target)

    # -- pair masks (loss_model.py:181-199): strictly-lower-triangular [row, col] pairs --------------------------------
    @staticmethod
    def pair_masks(n_same, n_not_same, device=None):
        """(valid, same_pairs, not_same_pairs) boolean [n, n] masks, n = n_same + n_not_same: consecutive rows (2i, 2i+1) of the
        first block are the pairs that share the attribute; consecutive rows of the second block are the 'not-same block'
        pairs (they share some OTHER attribute)."""
        n = n_same + n_not_same
        idx = torch.arange(n, device=device)
        valid = idx[:, None] > idx[None, :]
        consecutive = (idx[:, None] == idx[None, :] + 1) & (idx[None, :] % 2 == 0)
        same = consecutive & (idx[None, :] < 2 * (n_same // 2))
        not_same = consecutive & (idx[None, :] >= 2 * (n_same // 2)) & (idx[None, :] < 2 * (n_same // 2) + 2 * (n_not_same // 2))
        return valid, same & valid, not_same & valid

    def _level_loss(self, dist, masks, focus, lower, upper):
        valid, same_mask, not_same_mask = masks
        if focus == 'same_as_last_layer':
            same_d, not_same_d = dist[same_mask], dist[~same_mask & valid]
        elif focus == 'not_same_as_last_layer':
            same_d, not_same_d = dist[not_same_mask], dist[~not_same_mask & valid]
        else:
            raise ValueError('focus_on_list entry %r' % (focus,))
        return torch.clamp(same_d - lower, min=0.).mean() + torch.clamp(upper - not_same_d, min=0.).mean()

    def calc_mini_batch_loss(self, last_layer_same_features=None, last_layer_not_same_features=None):
        if last_layer_same_features is None:
            raise ValueError('last_layer_same_features is None')
        if last_layer_not_same_features is None:
            raise ValueError('last_layer_not_same_features is None')
        same, other = last_layer_same_features, last_layer_not_same_features
        if self.fused:
            levels = len(same)
            wanted = [level == levels - 1 or self.weights[level] != 0 for level in range(levels)]
            return self.calc_mini_batch_loss_rows([torch.cat([same[level], other[level]], dim=0) if wanted[level] else None for level in range(levels)],
                                                  None, same[0].shape[0], other[0].shape[0])
        masks = self.pair_masks(same[0].shape[0], other[0].shape[0], device=same[-1].device)
        as_last = bool(self.config.get('intermediate_criterion_as_last_layer'))
        loss = 0
        for level in range(len(same) - 1):
            if self.weights[level] == 0:
                continue
            feats = torch.cat([same[level], other[level]], dim=0)
            dist = self.last_layer_criterion(feats, feats) if as_last else _l1_expand(feats)
            loss = loss + self.weights[level] * self._level_loss(dist, masks, self.focus_on_list[level], self.lower_thres[level], self.upper_thres[level])
        emb = torch.cat([same[-1], other[-1]], dim=0)
        dist = self.last_layer_criterion(emb, emb)
        return loss + self.weights[-1] * self._level_loss(dist, masks, self.focus_on_list[-1], self.last_lower_thres, self.last_upper_thres)

    def calc_mini_batch_loss_rows(self, features_list, rows, n_same, n_not_same):
        """calc_mini_batch_loss on the WHOLE mini-batch's features: ``rows`` lists the rows in "same block, then the rest" order
        (MiniBatchUtils.same_not_same_rows; None: the rows as they are), the first ``n_same`` of them the same block.  With ``fused`` every
        level whose criterion has a kernel form is one pair_hinge_loss call that reads the rows in place; any other level -- and every level
        without ``fused`` -- picks the rows with one index and runs the criterion and _level_loss as calc_mini_batch_loss does."""
        if features_list is None:
            raise ValueError('features_list is None')
        from ..models.op import pair_hinge
        as_last = bool(self.config.get('intermediate_criterion_as_last_layer'))
        levels = len(features_list)
        loss = 0
        for level in range(levels):
            last = level == levels - 1
            if not last and self.weights[level] == 0:
                continue
            feats = features_list[level]
            fn = self.last_layer_criterion if (last or as_last) else None          # None: L1Expend's formula (_l1_expand)
            lower, upper = (self.last_lower_thres, self.last_upper_thres) if last else (self.lower_thres[level], self.upper_thres[level])
            weight, focus = self.weights[-1 if last else level], self.focus_on_list[-1 if last else level]
            form = _hinge_form(fn, feats) if self.fused else None
            if form is None:
                picked = feats if rows is None else feats[list(rows)]
                dist = fn(picked, picked) if fn is not None else _l1_expand(picked)
                level_loss = weight * self._level_loss(dist, self.pair_masks(n_same, n_not_same, device=feats.device), focus, lower, upper)
            elif form[0] == 'hair':
                colours, valid = _hair_colours(feats)
                level_loss = pair_hinge.pair_hinge_loss(colours, n_same, n_not_same, 'abs', lower, upper, focus, weight, rows, valid)
            else:
                level_loss = pair_hinge.pair_hinge_loss(feats, n_same, n_not_same, form[0], lower, upper, focus, weight, rows, None, form[1])
            loss = loss + level_loss
        return loss

    # -- the evaluation half (loss_model.py:204-285): all-pairs distances of two feature sets and their same / not-same split ----------
    def calc_distances_list(self, signatures_list, queries_list, last_layer_separability_only=False):
        """One [signatures, queries] distance matrix per feature level (loss_model.py:238-250): intermediate levels under ``L1Expend`` -- or
        under the last-layer criterion with ``intermediate_criterion_as_last_layer`` -- and skipped altogether when only the last layer is
        wanted; the last level under ``last_layer_criterion``."""
        as_last = bool(self.config.get('intermediate_criterion_as_last_layer'))
        distances_list = []
        for i, (signatures, queries) in enumerate(zip(signatures_list, queries_list)):
            if i + 1 < len(signatures_list):
                if last_layer_separability_only:
                    continue
                distances_list.append(self.calc_distances(signatures, queries, self.last_layer_criterion if as_last else L1Expend()))
            else:
                distances_list.append(self.calc_distances(signatures, queries, self.last_layer_criterion))
        return distances_list

    def calc_distances(self, signatures, queries, distance_fn, batch_size=20):
        """``distance_fn`` over every (signature, query) pair -> a [signatures, queries] tensor on the features' device (the reference hands
        back a numpy array, loss_model.py:252-285).  ``L1Expend`` and the criteria of ``CRITERIA`` on the row shapes they are written for are
        the 'abs' / 'sq' modes of ``models.op.pairwise.pairwise_distances`` (one HIP call under its dispatch rule); any other callable -- and
        a criterion on rows it does not reduce to a matrix -- is evaluated chunk pair by chunk pair, ``batch_size`` rows a side, and must
        give a [chunk, chunk] matrix (ValueError otherwise).  No gradient is recorded, as in the reference."""
        from ..models.op import pairwise
        signatures, queries = _as_tensor(signatures), _as_tensor(queries)
        mode = _mode_of(distance_fn, signatures)
        with torch.no_grad():
            if mode is not None:
                return pairwise.pairwise_distances(signatures, queries, mode, batch_size=batch_size)
            return pairwise.pairwise_distances(signatures, queries, None, criterion=distance_fn, batch_size=batch_size)

    def calc_same_not_same_list(self, signatures_list, queries_list, signature_pids, queries_pids, last_layer_separability_only=False):
        """Per level a dict of 'same' (distances of the pairs with equal pids), 'not_same' (per query the closest signature of ANOTHER pid:
        the "2nd best"), 'all_not_same' and 'pids_2nd_best_pairs_df' (columns signature / queries / distance: the pid pair behind every
        'not_same' entry), in the reference's order (loss_model.py:204-236): query-major, rows in order within a query.  The selections
        are masked reads of the TRANSPOSED matrix and the minima come with the distances (pairwise_distances); there is no per-query loop.
        Values are float32 numpy arrays; the frame is a pandas DataFrame built once from three arrays, or -- without pandas -- a dict of
        them.  A query whose every signature shares its pid raises ValueError (the reference's np.min of an empty row does)."""
        import numpy as np
        from ..models.op import pairwise
        n_levels = len(signatures_list)
        levels = [n_levels - 1] if last_layer_separability_only else list(range(n_levels))
        as_last = bool(self.config.get('intermediate_criterion_as_last_layer'))
        signature_pids, queries_pids = np.asarray(signature_pids).reshape(-1), np.asarray(queries_pids).reshape(-1)
        same_not_same_list = []
        for level in levels:
            signatures, queries = _as_tensor(signatures_list[level]), _as_tensor(queries_list[level])
            fn = self.last_layer_criterion if (level == n_levels - 1 or as_last) else L1Expend()
            mode = _mode_of(fn, signatures)
            with torch.no_grad():
                d, best, best_idx = pairwise.pairwise_distances(signatures, queries, mode, signature_pids, queries_pids,
                                                                criterion=None if mode is not None else fn)
                same_mask = torch.from_numpy(signature_pids[:, None] == queries_pids[None, :]).to(d.device)
                by_query = d.t()
                same = by_query[same_mask.t()].cpu().numpy()
                all_not_same = by_query[~same_mask.t()].cpu().numpy()
                not_same = best.cpu().numpy()
                rows = best_idx.cpu().numpy()
            same_not_same_list.append({'same': same, 'not_same': not_same, 'all_not_same': all_not_same,
                                       'pids_2nd_best_pairs_df': _pairs_frame(signature_pids[rows], queries_pids, not_same)})
        return same_not_same_list


def _as_tensor(features):
    return features if torch.is_tensor(features) else torch.as_tensor(features)


def _pairs_frame(signature, queries, distance):
    columns = {'signature': signature, 'queries': queries, 'distance': distance}
    try:
        import pandas as pd
    except ImportError:
        return columns
    return pd.DataFrame(columns)


class L1Expend(torch.nn.Module):
    """Mean absolute difference of every (signature, query) pair over all trailing axes of [n, c, h, w] maps or [n, k] rows
    (loss_model.py:308-321)."""

    def __call__(self, signatures, queries):
        if signatures.dim() not in (2, 4):
            raise ValueError('L1Expend: [n, c, h, w] maps or [n, k] rows expected, got %s' % (tuple(signatures.shape),))
        d = signatures.unsqueeze(1) - queries.unsqueeze(0)
        return d.abs().mean(tuple(range(2, d.dim())))


# criterion -> (mode of models.op.pairwise, the row ranks on which the criterion reduces every trailing axis): on any other rank the criterion
# itself is called, and what it returns is checked (the squared-L2 criterion leaves [m, n, c, h] on 4-D maps)
_KERNEL_FORMS = [(CRITERIA['embedding_loss'], 'sq', (2,)), (CRITERIA['dog_id_loss'], 'sq', (2,)), (CRITERIA['orientation_loss'], 'abs', (3,)),
                 (CRITERIA['expression_loss'], 'abs', (3,)), (CRITERIA['age_loss'], 'abs', (2,))]


def _hinge_form(criterion, features):
    """(mode of models.op.pair_hinge, scale) of a mini-batch level under ``criterion`` (None: L1Expend's formula), or None where the criterion
    has no kernel form on these rows (a custom callable, a rank the criterion does not reduce to a matrix): the torch path.  ('hair', 1.0):
    the hair criterion, whose colours are computed first."""
    if criterion is None:
        return ('abs', 1.0) if features.dim() == 4 else None
    if criterion is CRITERIA['hair_loss']:
        return ('hair', 1.0) if features.dim() == 4 else None
    if criterion is CRITERIA['style_loss']:
        return ('msq', STYLE_SCALE) if features.dim() == 3 else None
    if criterion is CRITERIA['recon_3d_loss']:
        return ('abs', 1.0) if features.dim() == 2 else None
    for fn, mode, ranks in _KERNEL_FORMS:
        if criterion is fn:
            return (mode, 1.0) if features.dim() in ranks else None
    return None


def _mode_of(distance_fn, signatures):
    if isinstance(distance_fn, L1Expend):
        return 'abs' if signatures.dim() in (2, 4) else None
    for fn, mode, ranks in _KERNEL_FORMS:
        if distance_fn is fn:
            return mode if signatures.dim() in ranks else None
    return None


def get_same_not_same_list(loss_model, features):
    """Rows (2i, 2i + 1) of every level are one pid (loss_model.py:298-305): even rows are the signatures, odd rows the queries, read in
    place (a row stride of two rows)."""
    import numpy as np
    pids = np.arange(0, len(features[0]), 2)
    return loss_model.calc_same_not_same_list([f[::2] for f in features], [f[1::2] for f in features], pids, pids)
