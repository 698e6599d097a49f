"""KID and precision / recall without a GPU: the torch path of models/op/manifold.py against the float64 restatements of tests/quality_refs.py
on the shapes of the GPU tests, known answers, the index draws of kid, fid.evaluate_quality and the Tracker.

Bounds (u = 2^-24, derived in quality_refs / the GPU test): radii within (F + 4) u relative; a hit decision equals the float64 one unless it
changes inside the band r (1 -+ 3 (F + 4) u), and at most 2 % of a case's decisions may lie in that band; each KID sum within 3 (F + 3) u.
"""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import quality_refs as qr
from quality_refs import U

from gan_control_amd.evaluation.tracker import Tracker
from gan_control_amd.fid_utils import fid as fid_module
from gan_control_amd.fid_utils import kid as kid_module
from gan_control_amd.fid_utils import real_stats
from gan_control_amd.fid_utils.precision_recall import precision_recall
from gan_control_amd.models.op import manifold as mf


def check_radii(got, ref, f):
    err = float(((got.double().cpu() - ref).abs() / ref.clamp_min(1e-300)).max())
    assert bool(((got.double().cpu() - ref).abs() <= (f + 4) * U * ref).all()), err
    return err


def check_hits(got, ref, undecided, name):
    got = got.cpu()
    share = float(undecided.double().mean())
    assert share <= 0.02, (name, share)
    assert bool((got == ref)[~undecided].all()), name
    return share


@pytest.mark.parametrize('n_r,n_f,f,kth,stride', qr.DISTANCE_CASES + qr.STRIP_HITS_CASES + [qr.BIG_TILE_HITS_CASE])
def test_torch_path_against_float64(n_r, n_f, f, kth, stride):
    case = qr.distance_case(n_r, n_f, f, kth)
    real, fake = torch.from_numpy(case['real']), torch.from_numpy(case['fake'])
    assert not mf.kernel_taken(real, fake)
    rr, fr = mf.knn_radii(real, kth), mf.knn_radii(fake, kth)
    e1, e2 = check_radii(rr, case['real_r2'], f), check_radii(fr, case['fake_r2'], f)
    p_hit, r_hit = mf.manifold_hits(real, rr, fake, fr)
    s1 = check_hits(p_hit, case['probe_hit'], case['probe_undecided'], 'probe_hit')
    s2 = check_hits(r_hit, case['ref_hit'], case['ref_undecided'], 'ref_hit')
    only, none = mf.manifold_hits(real, rr, fake)
    assert none is None and torch.equal(only, p_hit)
    precision, recall = float(case['probe_hit'].double().mean()), float(case['ref_hit'].double().mean())
    print('n_r=%d n_f=%d F=%d kth=%d: radii error %.2e %.2e (bound %.2e), undecided %.4f %.4f, float64 precision %.3f recall %.3f'
          % (n_r, n_f, f, kth, e1, e2, (f + 4) * U, s1, s2, precision, recall))
    if (n_r, n_f, f, kth, stride) in qr.DISTANCE_CASES[:6]:          # the listed shapes: not vacuous
        assert 0.39 <= precision <= 1.0 and 0.39 <= recall <= 1.0


@pytest.mark.parametrize('n,f,kth,stride', qr.STRIP_KNN_CASES)
def test_torch_radii_on_a_strip_sized_set(n, f, kth, stride):
    a = qr.feature_set(1, n, 1.0, 0.0, f)
    check_radii(mf.knn_radii(torch.from_numpy(a), kth), qr.radii64(a, kth), f)


@pytest.mark.parametrize('m,subsets,f,stride', qr.MMD_CASES)
def test_torch_kid_sums_against_float64(m, subsets, f, stride):
    case = qr.mmd_case(m, subsets, f)
    got = mf.poly_mmd_sums(torch.from_numpy(case['x']), torch.from_numpy(case['y']), case['idx_x'], case['idx_y']).numpy()
    assert got.dtype == np.float64 and got.shape == (subsets, 3)
    assert (np.abs(got - case['sums']) <= 3 * (f + 3) * U * case['sums']).all()
    a, b = qr.kid_parts64(case['sums'], m)
    assert abs(kid_module.kid_from_sums(got, m) - (a - b)) <= 3 * (f + 3) * U * (a + b)


def test_known_answers():
    real, fake = (torch.from_numpy(a) for a in qr.real_fake(70, 60, 9))
    assert precision_recall(real, real.clone()) == {'precision': 1.0, 'recall': 1.0}          # a set against itself: distance 0 <= any radius
    assert precision_recall(real, fake + 1e3) == {'precision': 0.0, 'recall': 0.0}            # farther apart than any radius
    out = precision_recall(real, fake, kth=2)
    assert 0.0 < out['precision'] <= 1.0 and 0.0 < out['recall'] <= 1.0
    # ties are hits: integer rows, probe rows exactly on the sphere of a ref row
    ref = torch.tensor([[0.0, 0.0], [3.0, 0.0], [50.0, 50.0], [50.0, 54.0]])
    r2 = mf.knn_radii(ref, 1)
    assert r2.tolist() == [9.0, 9.0, 16.0, 16.0]
    hit, _ = mf.manifold_hits(ref, r2, torch.tensor([[0.0, 3.0], [0.0, 3.5], [54.0, 50.0], [20.0, 20.0]]))
    assert hit.tolist() == [True, False, True, False]


def test_argument_errors():
    a = torch.zeros(3, 4)
    with pytest.raises(ValueError, match='kth'):
        mf.knn_radii(a, 3)          # n < kth + 1
    with pytest.raises(ValueError, match='kth'):
        mf.knn_radii(a, 0)
    with pytest.raises(ValueError, match='one width'):
        mf.manifold_hits(a, torch.zeros(3), torch.zeros(3, 5))
    with pytest.raises(ValueError, match='one radius per row'):
        mf.manifold_hits(a, torch.zeros(2), a)
    with pytest.raises(ValueError, match='outside'):
        mf.poly_mmd_sums(a, a, np.array([[0, 3]]), np.array([[0, 1]]))
    with pytest.raises(ValueError, match='at least 2'):
        kid_module.kid(a[:1], a)
    assert mf.knn_radii(torch.arange(9.0).view(9, 1), 8).tolist() == [64.0, 49.0, 36.0, 25.0, 16.0, 25.0, 36.0, 49.0, 64.0]          # kth beyond the kernel's 7


def test_workspace_queries_without_a_gpu():
    """The workspace queries are host arithmetic (the refusals run on real buffers in the GPU tests)."""
    from gan_control_amd import _lib
    lib = _lib.load()
    n, f = 50000, 2048
    sizes = [lib.gc_knn_radius_workspace(n, f, 3), lib.gc_manifold_hits_workspace(n, n, f), lib.gc_poly_mmd_workspace(100, n, f)]
    assert all(0 < s < 256 << 20 for s in sizes), sizes
    for rows in (n, 20 * n, 65535 * 64):          # linear in the rows: at most 32 strips a side
        assert lib.gc_knn_radius_workspace(rows, f, 3) <= 32 * rows * 4 * 4 and lib.gc_manifold_hits_workspace(rows, rows, f) <= 32 * 2 * rows + 16
    assert lib.gc_knn_radius_workspace(n, f, 8) == 0 and lib.gc_manifold_hits_workspace(0, n, f) == 0 and lib.gc_poly_mmd_workspace(0, 10, f) == 0


def test_kid_index_draws_and_symmetry():
    real, fake = (torch.from_numpy(a) for a in qr.real_fake(50, 40, 12))
    idx_x, idx_y = kid_module.subset_indices(50, 40, num_subsets=3, max_subset_size=16, seed=7)
    rs = np.random.RandomState(7)
    for s in range(3):          # per subset: the generated side first, then the real side
        assert (idx_x[s] == rs.choice(40, 16, replace=False)).all() and (idx_y[s] == rs.choice(50, 16, replace=False)).all()
    assert kid_module.subset_indices(50, 40, 2, 1000, 0)[0].shape == (2, 40)          # m = min(n_real, n_fake, max_subset_size)
    value = kid_module.kid(real, fake, num_subsets=3, max_subset_size=16, seed=7)
    sums = qr.mmd_sums64(fake.numpy(), real.numpy(), idx_x, idx_y)
    a, b = qr.kid_parts64(sums, 16)
    assert abs(value - (a - b)) <= 3 * (12 + 3) * U * (a + b)
    # swapping the sets with swapped index draws swaps the first two sums and transposes the third
    fwd = mf.poly_mmd_sums(fake, real, idx_x, idx_y).numpy()
    bwd = mf.poly_mmd_sums(real, fake, idx_y, idx_x).numpy()
    assert np.array_equal(fwd[:, 0], bwd[:, 1]) and np.array_equal(fwd[:, 1], bwd[:, 0])
    assert np.allclose(fwd[:, 2], bwd[:, 2], rtol=1e-12, atol=0)
    assert abs(kid_module.kid_from_sums(fwd, 16) - kid_module.kid_from_sums(bwd, 16)) <= 1e-12 * (a + b)


class _FakeG(torch.nn.Module):
    """Generator stand-in with the reference's call contract: g([z]) -> (img, None)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))

    def forward(self, styles):
        z = styles[0]
        return z[:, :48].reshape(z.shape[0], 3, 4, 4) * self.w, None


def _feature_net(img):
    return (img.reshape(img.shape[0], 6, 8).mean(2)[:, :, None, None],)


def _stats(tmp_path, with_features=True):
    torch.manual_seed(5)
    feats = _feature_net(_FakeG()([torch.randn(64, 512) * 1.1 + 0.1])[0])[0].reshape(64, -1).detach()
    path = str(tmp_path / ('features.pkl' if with_features else 'stats.pkl'))
    (real_stats.save_real_features if with_features else real_stats.save_real_statistics)(path, feats)
    return path, feats


def test_save_real_features_and_evaluate_quality(tmp_path):
    path, feats = _stats(tmp_path)
    plain, _ = _stats(tmp_path, with_features=False)
    with open(path, 'rb') as f, open(plain, 'rb') as g:
        both, stats = pickle.load(f), pickle.load(g)
    assert sorted(both) == ['cov', 'features', 'mean'] and both['features'].dtype == np.float32 and np.array_equal(both['features'], feats.numpy())
    assert np.array_equal(both['mean'], stats['mean']) and np.array_equal(both['cov'], stats['cov'])
    torch.manual_seed(11)
    fid = fid_module.evaluate_fid(_FakeG(), _feature_net, 8, 30, 'cpu', path)
    torch.manual_seed(11)
    out = fid_module.evaluate_quality(_FakeG(), _feature_net, 8, 30, 'cpu', path, num_subsets=4, max_subset_size=20)
    assert sorted(out) == ['fid', 'kid', 'precision', 'recall'] and out['fid'] == fid          # the same sample, the same host formula
    torch.manual_seed(11)
    fake = fid_module.sample_features(_FakeG(), _feature_net, 8, 30, 'cpu', to_host=False)
    assert out['kid'] == kid_module.kid(feats, fake, num_subsets=4, max_subset_size=20)
    pr = precision_recall(feats, fake)
    assert (out['precision'], out['recall']) == (pr['precision'], pr['recall'])
    torch.manual_seed(11)
    assert fid_module.evaluate_quality(_FakeG(), _feature_net, 8, 30, 'cpu', plain, metrics=('fid',)) == {'fid': fid}
    with pytest.raises(ValueError, match=r"stats\.pkl.*save_real_features"):
        fid_module.evaluate_quality(_FakeG(), _feature_net, 8, 30, 'cpu', plain, metrics=('fid', 'kid'))
    with pytest.raises(ValueError, match='metrics'):
        fid_module.evaluate_quality(_FakeG(), _feature_net, 8, 30, 'cpu', path, metrics=('fid', 'is'))


def test_tracker_quality_history(tmp_path):
    path, _ = _stats(tmp_path)
    base = {'enabled': True, 'fid_interval': 10, 'num_of_samples': 40, 'inception_stat_path': path}
    histories = {}
    for name, extra in (('plain', {}), ('off', {'kid': False, 'precision_recall': False}), ('kid', {'kid': True}),
                        ('both', {'kid': True, 'precision_recall': True})):
        tracker = Tracker(torch.zeros(4, 512), None, _feature_net, 'normal', fid_config=dict(base, **extra))
        graphs = str(tmp_path / name)
        torch.manual_seed(3)
        for i in (10, 20):
            tracker.evaluate(i, _FakeG(), graph_save_path=graphs)
        with open(os.path.join(graphs, 'fid.json'), 'rb') as f:
            histories[name] = f.read()
        assert len(tracker.fids) == 2 and tracker.evaluation_dict['fid'] == tracker.fids[-1]
        quality = os.path.join(graphs, 'quality.json')
        if name in ('plain', 'off'):
            assert not os.path.exists(quality) and sorted(tracker.evaluation_dict) == ['fid']
            continue
        with open(quality) as f:
            rows = json.load(f)
        keys = ['fid', 'kid'] + (['precision', 'recall'] if name == 'both' else [])
        assert [sorted(r) for r in rows] == [sorted(['iter'] + keys)] * 2 and [r['iter'] for r in rows] == [10, 20]
        assert [r['fid'] for r in rows] == tracker.fids
        assert sorted(tracker.evaluation_dict) == sorted(keys) and all(tracker.evaluation_dict[k] == rows[-1][k] for k in keys)
        assert tracker.is_best_fid() == (tracker.fids[-1] == min(tracker.fids))
    assert histories['plain'] == histories['off'] == histories['kid'] == histories['both']          # the same RNG state, the same FID bytes
