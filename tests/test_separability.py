"""The separability evaluation without a GPU: models/op/pairwise.py on CPU tensors, the evaluation half of LossModelClass, evaluation/separability.py
on a stub generator and a stub predictor, and the Tracker / trainer cadence on the emulated backend.

The formulas are restated here: distances as float64 double loops over the pairs, calc_same_not_same_list as the reference's per-query loop
(loss_model.py:204-236) written in numpy on a given distance matrix.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from gan_control_amd.evaluation import image_grid, separability
from gan_control_amd.evaluation.tracker import Tracker
from gan_control_amd.losses import LossModelClass, L1Expend, get_same_not_same_list
from gan_control_amd.models.op import pairwise as pw

U = 2.0 ** -24
LOSS_CFG = {'lower_thres': [0.1], 'upper_thres': [0.2], 'last_lower_thres': 0.5, 'last_upper_thres': 1.8, 'intermediate_layers_weights': [1.0],
            'last_layer_weight': 0.25, 'focus_on_list': ['not_same_as_last_layer', 'same_as_last_layer'], 'same_group_name': 'id', 'enabled': True}


def loop64(s, q, mode):
    """D64[i, j] pair by pair: mean_k |s_i - q_j| or sum_k (s_i - q_j)^2 over the flattened rows."""
    s, q = s.double().reshape(s.shape[0], -1), q.double().reshape(q.shape[0], -1)
    out = torch.zeros(s.shape[0], q.shape[0], dtype=torch.float64)
    for i in range(s.shape[0]):
        for j in range(q.shape[0]):
            d = s[i] - q[j]
            out[i, j] = d.abs().sum() / d.numel() if mode == 'abs' else (d * d).sum()
    return out


def within_bound(d, ref, k):
    return bool(((d.double() - ref).abs() <= (k + 4) * U * ref).all())


# -- models/op/pairwise.py on CPU tensors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['abs', 'sq'])
def test_pairwise_distances_on_cpu_tensors(mode):
    gen = torch.Generator().manual_seed(1)
    rows = torch.randn(45, 37, generator=gen)
    maps = torch.randn(46, 3, 4, 5, generator=gen)
    for s, q, k in ((rows[:23], rows[23:], 37), (maps[:25], maps[25:], 60), (maps[::2], maps[1::2], 60), (rows[::2], rows[1::2], 37)):
        assert not pw.kernel_taken(s, q)
        d = pw.pairwise_distances(s, q, mode)
        assert d.shape == (s.shape[0], q.shape[0]) and d.dtype == torch.float32
        assert within_bound(d, loop64(s, q, mode), k)
    with pytest.raises(ValueError, match='mode'):
        pw.pairwise_distances(rows[:3], rows[3:6], 'l2')
    with pytest.raises(ValueError, match='go together'):
        pw.pairwise_distances(rows[:3], rows[3:6], 'sq', signature_pids=np.arange(3))
    with pytest.raises(ValueError, match='one row shape'):
        pw.pairwise_distances(rows[:3], maps[:3], 'sq')


def test_rows_of_a_tensor():
    t = torch.zeros(6, 2, 3, 4)
    assert pw._rows(t) == (24, 24) and pw._rows(t[::2]) == (24, 48) and pw._rows(t[:1].expand(6, 2, 3, 4)) is None
    assert pw._rows(t.transpose(1, 2)) is None and pw._rows(t[:, :, :, ::2]) is None and pw._rows(t[:, :1]) == (12, 24)
    assert pw._rows(torch.zeros(5, 9)[:, :8]) == (8, 9) and pw._rows(torch.zeros(1, 8).expand(1, 8)) == (8, 8)


def test_entry_refuses_bad_arguments_without_a_gpu():
    """Every refusal of gc_pairwise_f32 comes before a launch, so the calls are safe on a host without a GPU (the pointers are never read)."""
    from gan_control_amd import _lib
    lib = _lib.load()
    p = 4096          # any non-null address

    def call(s=p, ss=8, q=p, qs=8, m=4, n=4, k=8, mode=0, d=p, sp=None, qp=None, best=None, idx=None, ws=None, nbytes=0):
        rc = lib.gc_pairwise_f32(s, ss, q, qs, m, n, k, mode, d, sp, qp, best, idx, ws, nbytes, None)
        return rc, lib.gc_last_error()

    for kw, code, word in ((dict(s=None), -1, b'null pointer'), (dict(d=None), -1, b'null pointer'), (dict(m=0), -1, b'at least 1'), (dict(n=-3), -1, b'at least 1'),
                           (dict(k=0), -1, b'at least 1'), (dict(ss=7), -1, b'shorter than the rows'), (dict(qs=0), -1, b'shorter than the rows'),
                           (dict(mode=2), -1, b'unknown mode 2'), (dict(sp=p, best=p, idx=p), -1, b'go together'), (dict(qp=p, best=p, idx=p), -1, b'go together'),
                           (dict(sp=p, qp=p, best=p), -1, b'best / best_idx'),
                           (dict(m=20, n=20, k=200704, ss=200704, qs=200704), -4, b'workspace too small'),
                           (dict(m=20, n=20, k=200704, ss=200704, qs=200704, ws=p, nbytes=lib.gc_pairwise_workspace(20, 20, 200704) - 4), -4, b'workspace too small')):
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    # the workspace is a function of the extents alone: nothing for rows too short to split, splits x m x n floats otherwise, 0 for bad extents
    assert lib.gc_pairwise_workspace(1000, 1000, 255) == 0 and lib.gc_pairwise_workspace(0, 5, 512) == 0 and lib.gc_pairwise_workspace(5, 5, -1) == 0
    assert lib.gc_pairwise_workspace(1000, 1000, 512) == 2 * 1000 * 1000 * 4
    assert lib.gc_pairwise_workspace(20, 20, 200704) % (20 * 20 * 4) == 0 and lib.gc_pairwise_workspace(20, 20, 200704) > 20 * 20 * 4


# -- LossModelClass.calc_distances_list -----------------------------------------------------------------------------------------------------
def features(n, seed, integer=False):
    gen = torch.Generator().manual_seed(seed)
    draw = (lambda *s: torch.randint(-1, 2, s, generator=gen).float()) if integer else (lambda *s: torch.randn(*s, generator=gen))
    return [draw(n, 2, 3, 3), draw(n, 4, 2, 2), draw(n, 6)]


def loss_model(**config):
    cfg = dict(LOSS_CFG, lower_thres=[0.1, 0.1], upper_thres=[0.2, 0.2], intermediate_layers_weights=[1.0, 1.0],
               focus_on_list=['not_same_as_last_layer'] * 2 + ['same_as_last_layer'], **config)
    return LossModelClass(cfg, 'embedding_loss', mini_batch_size=4, no_model=True)


def test_calc_distances_list_levels_and_branches():
    sig, que = features(23, 2), features(21, 3)
    lm = loss_model()
    dists = lm.calc_distances_list(sig, que)
    assert [tuple(d.shape) for d in dists] == [(23, 21)] * 3
    assert within_bound(dists[0], loop64(sig[0], que[0], 'abs'), 18) and within_bound(dists[1], loop64(sig[1], que[1], 'abs'), 16)
    assert within_bound(dists[2], loop64(sig[2], que[2], 'sq'), 6)
    only = lm.calc_distances_list(sig, que, last_layer_separability_only=True)
    assert len(only) == 1 and torch.equal(only[0], dists[2])
    # calc_distances is the chunked formula of the reference for any callable, 20 rows a side by default
    calls = []
    custom = lambda a, b: (calls.append((a.shape[0], b.shape[0])), (a.unsqueeze(1) - b.unsqueeze(0)).abs().amax(-1))[1]
    got = lm.calc_distances(sig[2], que[2], custom)
    assert calls == [(12, 11), (11, 11), (12, 10), (11, 10)]          # torch.chunk of 23 and 21 rows into two pieces; queries outermost
    assert torch.equal(got, (sig[2].unsqueeze(1) - que[2].unsqueeze(0)).abs().amax(-1))
    assert torch.equal(lm.calc_distances(sig[0].numpy(), que[0].numpy(), L1Expend()), dists[0])
    # the squared-L2 criterion leaves [m, n, c, h] on 4-D maps: intermediate_criterion_as_last_layer cannot give a matrix there
    as_last = loss_model(intermediate_criterion_as_last_layer=True)
    with pytest.raises(ValueError, match='matrix'):
        as_last.calc_distances_list(sig, que)
    assert len(as_last.calc_distances_list(sig, que, last_layer_separability_only=True)) == 1
    flat = [f.flatten(1) for f in sig], [f.flatten(1) for f in que]
    got = as_last.calc_distances_list(*flat)
    assert within_bound(got[0], loop64(sig[0], que[0], 'sq'), 18) and within_bound(got[1], loop64(sig[1], que[1], 'sq'), 16)
    age = LossModelClass(LOSS_CFG, 'age_loss', no_model=True)
    assert within_bound(age.calc_distances_list([sig[2]], [que[2]])[0], loop64(sig[2], que[2], 'abs'), 6)


# -- calc_same_not_same_list against the reference's per-query loop ------------------------------------------------------------------------
def reference_loop(all_distances, signature_pids, queries_pids):
    """loss_model.py:206-229 on one distance matrix, literally."""
    same_mask = signature_pids[:, None] == queries_pids[None, :]
    signature_pids_v, _ = np.meshgrid(signature_pids, queries_pids, sparse=False, indexing='ij')
    same, not_same, all_not_same, pairs = [], [], [], []
    for qid in np.arange(all_distances.shape[1]):
        same_row_mask = same_mask[:, qid]
        not_same_row_mask = ~same_mask[:, qid]
        same_row = all_distances[same_row_mask, qid]
        not_same_row = all_distances[not_same_row_mask, qid]
        same.extend(same_row)
        distance_2nd_best = np.min(not_same_row)
        index_2nd_best = np.argmin(not_same_row)
        signature = signature_pids_v[not_same_row_mask, qid][index_2nd_best]
        not_same.append(distance_2nd_best)
        all_not_same.extend(not_same_row)
        pairs.append((signature, queries_pids[qid], distance_2nd_best))
    return same, not_same, all_not_same, pairs


def assert_levels_match(got, dists, s_pid, q_pid):
    assert len(got) == len(dists)
    for level, d in zip(got, dists):
        assert list(level) == ['same', 'not_same', 'all_not_same', 'pids_2nd_best_pairs_df']
        same, not_same, all_not_same, pairs = reference_loop(d.numpy(), s_pid, q_pid)
        assert np.array_equal(level['same'], np.array(same, np.float32)) and np.array_equal(level['not_same'], np.array(not_same, np.float32))
        assert np.array_equal(level['all_not_same'], np.array(all_not_same, np.float32))
        df = level['pids_2nd_best_pairs_df']
        assert list(df.columns if hasattr(df, 'columns') else df) == ['signature', 'queries', 'distance']
        assert [int(v) for v in np.asarray(df['signature'])] == [int(p[0]) for p in pairs]
        assert [int(v) for v in np.asarray(df['queries'])] == [int(p[1]) for p in pairs]
        assert np.array_equal(np.asarray(df['distance'], np.float32), np.array([p[2] for p in pairs], np.float32))


@pytest.mark.parametrize('integer', [False, True])
def test_calc_same_not_same_list_matches_the_reference_loop(integer):
    """Repeated pids on the signature side (the mask maps the masked argmin back to a row), unordered pids, and -- on small integers, where
    distances tie exactly -- the first occurrence."""
    sig, que = features(23, 4, integer), features(9, 5, integer)
    s_pid = np.array([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8, 4, 6, 2, 6])
    q_pid = np.array([1, 5, 9, 2, 6, 11, 3, 8, 4])
    lm = loss_model()
    got = lm.calc_same_not_same_list(sig, que, s_pid, q_pid)
    dists = lm.calc_distances_list(sig, que)
    assert_levels_match(got, dists, s_pid, q_pid)
    if integer:          # the property under test is there: some query's minimum is attained more than once
        for d in (t.numpy() for t in dists):
            assert any((d[s_pid != q_pid[j], j] == d[s_pid != q_pid[j], j].min()).sum() > 1 for j in range(9))
    last = lm.calc_same_not_same_list(sig, que, s_pid, q_pid, last_layer_separability_only=True)
    assert_levels_match(last, dists[2:], s_pid, q_pid)
    assert len(got[0]['same']) == int((s_pid[:, None] == q_pid[None, :]).sum()) and len(got[0]['not_same']) == 9
    assert len(got[0]['same']) + len(got[0]['all_not_same']) == 23 * 9


def test_pairs_without_pandas(monkeypatch):
    import builtins
    real_import = builtins.__import__

    def no_pandas(name, *a, **k):
        if name == 'pandas':
            raise ImportError('no pandas here')
        return real_import(name, *a, **k)

    monkeypatch.setattr(builtins, '__import__', no_pandas)
    sig, que = features(6, 6), features(5, 7)
    got = loss_model().calc_same_not_same_list(sig, que, np.arange(6), np.arange(5))
    assert isinstance(got[0]['pids_2nd_best_pairs_df'], dict)
    assert_levels_match(got, loss_model().calc_distances_list(sig, que), np.arange(6), np.arange(5))


def test_query_without_a_not_same_signature_raises():
    sig, que = features(4, 8), features(3, 9)
    with pytest.raises(ValueError, match='query 1'):
        loss_model().calc_same_not_same_list(sig, que, np.array([2, 2, 2, 2]), np.array([0, 2, 1]))
    # ... but one signature of another pid is enough
    got = loss_model().calc_same_not_same_list(sig, que, np.array([2, 2, 5, 2]), np.array([0, 2, 1]))
    assert int(np.asarray(got[0]['pids_2nd_best_pairs_df']['signature'])[1]) == 5


def test_get_same_not_same_list_reads_even_and_odd_rows():
    feats = features(12, 10)
    lm = loss_model()
    got = get_same_not_same_list(lm, feats)
    pids = np.arange(0, 12, 2)
    assert_levels_match(got, lm.calc_distances_list([f[::2] for f in feats], [f[1::2] for f in feats]), pids, pids)
    assert [int(v) for v in np.asarray(got[-1]['pids_2nd_best_pairs_df']['queries'])] == list(pids)


# -- evaluation/separability.py on a stub generator and a stub predictor ---------------------------------------------------------------
class StubGenerator(nn.Module):
    """8 x 8 images that are a fixed function of the latent and the last injection noise; every call is recorded."""
    style_dim, log_size = 512, 3

    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(0.3))
        self.calls = []

    def make_noise(self, batch_size=1, device=None):
        return [torch.randn(batch_size, 1, 4, 4), torch.randn(batch_size, 1, 8, 8), torch.randn(batch_size, 1, 8, 8)]

    def forward(self, styles, noise=None):
        z = styles[0]
        self.calls.append((z.clone(), None if noise is None else [n.clone() for n in noise]))
        img = torch.stack([z[:, 0:64], z[:, 224:288], z[:, 448:512]], 1).reshape(-1, 3, 8, 8) * self.scale
        if noise is not None:
            img = img + 0.1 * noise[-1]
        return img, None


def stub_skeleton(img):
    return [img * 2.0, img.flatten(1)[:, ::4]]


def stub_loss_model():
    return LossModelClass(LOSS_CFG, 'embedding_loss', mini_batch_size=4, skeleton_model=stub_skeleton)


def test_compute_half_same_ids_embeddings(emu_backend):
    g, lm = StubGenerator(), stub_loss_model()
    emb, images = separability.compute_half_same_ids_embeddings_from_generator(g, lm, 50, same_noise_for_same_id=True, return_images=True,
                                                                               same_chunk=(256, 512), seed=3)
    assert [c[0].shape[0] for c in g.calls] == [20, 20, 10]
    z = torch.cat([c[0] for c in g.calls])
    assert torch.equal(z[1::2, 256:], z[0::2, 256:]) and not bool((z[1::2, :256] == z[0::2, :256]).any())          # the latent copy
    for _, noise in g.calls:                                                                                       # the noise pairing
        assert all(torch.equal(n[1::2], n[0::2]) for n in noise) and not torch.equal(noise[-1][0], noise[-1][2])
    with torch.no_grad():
        img = torch.cat([g(c[0:1], noise=c[1])[0] for c in list(g.calls)])
    want = stub_skeleton(img)
    assert [tuple(e.shape) for e in emb] == [(50, 3, 8, 8), (50, 48)]
    for e, w in zip(emb, want):                                                                                    # even half, then odd half
        assert torch.equal(e[:25], w[0::2]) and torch.equal(e[25:], w[1::2])
    assert len(images) == 50 and images[0].shape == (8, 8, 3) and images[0].dtype == np.uint8
    u8 = image_grid.quantize_reference(img).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(images[0], u8[0]) and np.array_equal(images[1], u8[2]) and np.array_equal(images[25], u8[1])
    # the same seed gives the same run, another seed another one; no seed and no shared noise: the generator draws its own
    again, _ = separability.compute_half_same_ids_embeddings_from_generator(StubGenerator(), lm, 50, same_noise_for_same_id=True, seed=3)
    other, _ = separability.compute_half_same_ids_embeddings_from_generator(StubGenerator(), lm, 50, same_noise_for_same_id=True, seed=4)
    assert all(torch.equal(a, b) for a, b in zip(again, emb)) and not torch.equal(other[1], emb[1])
    g2 = StubGenerator()
    emb2, images2 = separability.compute_half_same_ids_embeddings_from_generator(g2, lm, 6, same_chunk=(0, 256), last_layer_separability_only=True)
    assert emb2[0] is None and emb2[1].shape == (6, 48) and images2 == [] and g2.calls[0][1] is None
    assert torch.equal(g2.calls[0][0][1::2, :256], g2.calls[0][0][0::2, :256])
    with pytest.raises(ValueError, match='even'):
        separability.compute_half_same_ids_embeddings_from_generator(g2, lm, 7)


def test_re_arrange_inject_noise():
    noises = [torch.arange(5.).view(5, 1, 1, 1).repeat(1, 1, 2, 2), torch.arange(4.).view(4, 1, 1, 1)]
    out = separability.re_arrange_inject_noise(noises)
    assert out is noises and out[0][:, 0, 0, 0].tolist() == [0, 0, 2, 2, 4] and out[1].flatten().tolist() == [0, 0, 2, 2]


def test_calc_separability_and_its_summary(emu_backend, tmp_path):
    g, lm = StubGenerator(), stub_loss_model()
    prefix = str(tmp_path / 'id_separability')
    result, images = separability.calc_separability(g, lm, same_noise_for_same_id=True, num_of_samples=40, save_path=prefix, title='id separability',
                                                    return_images=True, seed=1)
    emb, _ = separability.compute_half_same_ids_embeddings_from_generator(StubGenerator(), lm, 40, same_noise_for_same_id=True, seed=1)
    pids = np.arange(20)
    assert_levels_match(result, lm.calc_distances_list([e[:20] for e in emb], [e[20:] for e in emb]), pids, pids)
    assert len(images) == 40 and [len(result[-1][k]) for k in ('same', 'not_same', 'all_not_same')] == [20, 20, 380]
    # pairs that share half the latent and all the noise sit closer than strangers
    assert all(np.mean(level['same']) < np.mean(level['all_not_same']) for level in result)
    for i, level in enumerate(result):
        with open('%s_layer_%d.json' % (prefix, i)) as f:
            summary = json.load(f)
        assert summary['title'] == 'id separability layer %d' % i and summary['bins'] == 100
        for label, key in zip(separability.LABELS, ('same', 'not_same', 'all_not_same')):
            a = np.asarray(level[key], np.float64)
            assert summary[label]['count'] == a.size and summary[label]['mean'] == pytest.approx(a.mean())
            assert summary[label]['percentiles'] == {str(p): pytest.approx(np.quantile(a, p)) for p in (0.2, 0.5, 0.8)}
            assert len(summary[label]['hist']) == 100 and sum(summary[label]['hist']) == a.size
        assert summary['range'][0] == pytest.approx(min(np.min(level[k]) for k in ('same', 'not_same', 'all_not_same')))
    only, none = separability.calc_separability(StubGenerator(), lm, same_noise_for_same_id=True, num_of_samples=40, last_layer_separability_only=True, seed=1)
    assert len(only) == 1 and none == [] and np.array_equal(only[0]['not_same'], result[-1]['not_same'])


# -- Tracker and trainer -----------------------------------------------------------------------------------------------------------------------
SEP = {'enabled': True, 'separability_interval': 10, 'num_of_samples': 40, 'losses': ['embedding_loss', 'orientation_loss'],
       'last_layer_separability_only': True}


def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_tracker_separability_cadence(emu_backend, tmp_path):
    g = StubGenerator()
    models = {'embedding_loss': stub_loss_model(), 'age_loss': stub_loss_model()}          # age_loss is not configured, orientation_loss not present
    tracker = Tracker(torch.zeros(4, 512), None, None, 'same_for_same_id', separability_config=SEP)
    graphs, buckets = str(tmp_path / 'graphs'), str(tmp_path / 'buckets')
    ran = []
    for i in (0, 5, 10, 15, 20):          # never at 0, only on the interval
        before = len(g.calls)
        tracker.evaluate(i, g, graph_save_path=graphs, buckets_save_path=buckets, loss_models=models, same_chunks={'embedding_loss': [256, 512]})
        ran.append(sum(c[0].shape[0] for c in g.calls[before:]))
    assert ran == [0, 0, 40, 0, 40]
    assert sorted(tracker.evaluation_dict) == ['id_all_not_same_avg', 'id_not_same_2nd_best_avg', 'id_same_avg']
    assert tracker.evaluation_dict['id_same_avg'] < tracker.evaluation_dict['id_all_not_same_avg']          # (half the latent and all the noise are shared)
    assert tracker.evaluation_dict['id_not_same_2nd_best_avg'] <= tracker.evaluation_dict['id_all_not_same_avg']
    assert all(torch.equal(n[1::2], n[0::2]) for n in g.calls[-1][1])          # g_noise_mode same_for_same_id
    with open(os.path.join(graphs, 'separability.json')) as f:
        history = json.load(f)
    assert [e['iter'] for e in history] == [10, 20] and history[-1]['id_same_avg'] == tracker.evaluation_dict['id_same_avg']
    assert sorted(history[0]) == ['id_all_not_same_avg', 'id_not_same_2nd_best_avg', 'id_same_avg', 'iter']
    want = ['buckets/%08d_id_embedding%s' % (i, s) for i in (10, 20) for s in ['.json'] + ['_%02d.jpg' % k for k in range(5)]]
    assert files_under(str(tmp_path)) == sorted(want + ['graphs/id_separability_layer_0.json', 'graphs/separability.json'])
    from PIL import Image
    assert Image.open(os.path.join(buckets, '00000010_id_embedding_00.jpg')).size == (16, 8)
    with open(os.path.join(buckets, '00000010_id_embedding.json')) as f:
        lines = json.load(f)
    assert [l['distance'] for l in lines] == sorted(l['distance'] for l in lines) and all(l['signature'] != l['queries'] for l in lines)
    assert lines[0]['message'] == '0) Sig: %d, Que: %d, distance:%.4f' % (lines[0]['signature'], lines[0]['queries'], lines[0]['distance'])
    # debug: every 100 iterations, on 100 samples; no path, no file
    before, n_files = len(g.calls), len(files_under(str(tmp_path)))
    tracker.evaluate(100, g, debug=True, loss_models=models, same_chunks={'embedding_loss': [256, 512]})
    tracker.evaluate(155, g, debug=True, loss_models=models, same_chunks={'embedding_loss': [256, 512]})
    assert sum(c[0].shape[0] for c in g.calls[before:]) == 100 and len(files_under(str(tmp_path))) == n_files
    # errors surface: a configured loss model without its chunk
    with pytest.raises(KeyError, match='embedding_loss'):
        tracker.evaluate(10, g, loss_models=models, same_chunks={})
    off = Tracker(torch.zeros(4, 512), None, None, 'normal')
    off.evaluate(10, g, loss_models=models)
    assert off.evaluation_dict == {} and not off.separability_config['enabled']


def test_save_separability_buckets_takes_the_five_closest(tmp_path):
    images = [np.full((4, 4, 3), 10 * i, np.uint8) for i in range(12)]
    pairs = {'signature': np.array([1, 0, 3, 2, 5, 4]), 'queries': np.arange(6), 'distance': np.array([.5, .1, .3, .1, .9, .2], np.float32)}
    written = Tracker.save_separability_buckets('id_embedding', pairs, images, 7, str(tmp_path))
    assert [os.path.basename(p) for p in written] == ['00000007_id_embedding_%02d.jpg' % i for i in range(5)] + ['00000007_id_embedding.json']
    with open(written[-1]) as f:
        lines = json.load(f)
    assert [(l['signature'], l['queries']) for l in lines] == [(0, 1), (2, 3), (4, 5), (3, 2), (1, 0)]          # ties in frame order
    from PIL import Image
    first = np.asarray(Image.open(written[0]))
    assert first.shape == (4, 8, 3) and abs(int(first[0, 0, 0]) - 0) <= 3 and abs(int(first[0, 7, 0]) - 70) <= 3          # image 0 | image 6 + 1


SIZE, BATCH = 16, 4
GROUPS = {'id': {'place_in_latent': [0, 256], 'place_in_mini_batch': [0, 2]},
          'other': {'place_in_latent': [256, 512], 'place_in_mini_batch': [2, 4]}}


def make_trainer(with_section):
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    from gan_control_amd.utils.mini_batch_utils import MiniBatchUtils
    cfg = copy.deepcopy(default_config(SIZE, BATCH))
    cfg['training_config'].update(min_evaluate_interval=1, save_nets_interval=0, save_images_interval=0)
    cfg['evaluation_config'] = {'fid': {'enabled': False}}
    if with_section:
        cfg['evaluation_config']['separability'] = dict(SEP, separability_interval=1, num_of_samples=8)
    tr = GeneratorTrainer(cfg, device='cpu', seed=0, fused_adam=False)
    tr.training_config['embedding_loss'] = dict(LOSS_CFG)
    tr.batch_utils = MiniBatchUtils(BATCH, GROUPS, total_batch=BATCH)
    tr.loss_models = {'embedding_loss': LossModelClass(LOSS_CFG, 'embedding_loss', mini_batch_size=BATCH,
                                                       skeleton_model=lambda img: [img[:, :, ::2, ::2], img.flatten(1)[:, ::16]])}
    return tr


def test_trainer_runs_separability_on_its_cadence(emu_backend, tmp_path):
    tr = make_trainer(True)
    tracker = tr.make_tracker(n_samples=4)
    assert tracker.separability_config['separability_interval'] == 1 and tr._same_chunks() == {'embedding_loss': [0, 256]}
    root = str(tmp_path / 'run')
    assert tr.train(save_dir=root, iters=2, tracker=tracker) == 2          # never at iteration 0
    want = ['buckets/00000001_id_embedding%s' % s for s in ['.json'] + ['_%02d.jpg' % k for k in range(4)]]          # 4 queries: 4 pairs
    assert files_under(root) == sorted(want + ['graphs/id_separability_layer_0.json', 'graphs/separability.json'])
    with open(os.path.join(root, 'graphs', 'separability.json')) as f:
        assert [e['iter'] for e in json.load(f)] == [1]
    assert {'id_same_avg', 'id_all_not_same_avg', 'id_not_same_2nd_best_avg'} <= set(tracker.evaluation_dict)


def test_trainer_without_the_section_writes_nothing_new(emu_backend, tmp_path):
    tr = make_trainer(False)
    tracker = tr.make_tracker(n_samples=4)
    assert tracker.separability_config == {'enabled': False}
    root = str(tmp_path / 'run')
    assert tr.train(save_dir=root, iters=2, tracker=tracker) == 2
    assert files_under(root) == [] and tracker.evaluation_dict == {}
