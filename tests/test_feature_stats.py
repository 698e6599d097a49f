"""Streaming FID statistics without a GPU: FeatureStats on CPU tensors (the float64 formulas of models/op/feature_moments.py), the eigen-form
Frechet distance, evaluate_fid / evaluate_quality / Tracker plumbing, the second header and its binding table, and all_reduce_ over gloo.

Tolerances of the statistics: feature_stats_checks.bounds (derived; include/gancontrol_stats.h).  Tolerances between the two host distance
formulas are MEASURED on this file's own inputs (1, 4 and 16 threads gave the same figures) and allowed 16 x for BLAS / thread-count variation;
the measured value stands next to each constant.
"""
import ctypes
import os
import pickle
import re
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from feature_stats_checks import bounds, fid_tolerance

from gan_control_amd import _lib
from gan_control_amd.evaluation.tracker import Tracker
from gan_control_amd.fid_utils import fid as fid_module
from gan_control_amd.fid_utils import real_stats
from gan_control_amd.fid_utils.feature_stats import FeatureStats
from gan_control_amd.models.op import feature_moments as fm

STATS_HEADER = os.path.join(REPO, 'include', 'gancontrol_stats.h')
MAIN_HEADER = os.path.join(REPO, 'include', 'gancontrol_hip.h')


def rows(n, f, seed):
    return torch.randn(n, f, generator=torch.Generator().manual_seed(seed)) * 1.5 + 0.5


def assert_statistics(stats, x, tag):
    x64 = x.numpy().astype(np.float64)
    _, _, tm, tc = bounds(x64)
    mean, cov = stats.numpy()
    em = np.abs(mean - x64.mean(0))
    ec = np.abs(cov - np.cov(x64, rowvar=False).reshape(cov.shape))
    print('%s: mean error / bound %.3e, cov error / bound %.3e' % (tag, float((em / tm).max()), float((ec / tc).max())))
    assert mean.dtype == cov.dtype == np.float64 and stats.n == x.shape[0]
    assert np.all(em <= tm) and np.all(ec <= tc)
    assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize('f,n', [(1, 2), (16, 100), (64, 37), (70, 200)])
def test_feature_stats_against_two_pass_numpy(f, n):
    x = rows(n, f, 3 * f + n)
    stats = FeatureStats.from_features(x)
    assert not fm.kernel_taken(stats.s1, stats.s2, x)          # CPU tensors take the formulas
    assert_statistics(stats, x, 'one append')
    assert stats.mean().dtype == torch.float64 and stats.cov().shape == (f, f) and stats.mean().device == x.device


@pytest.mark.parametrize('step', [1, 3, 20])
def test_chunked_appends_equal_one_append_within_the_bound(step):
    x = rows(67, 24, step)
    stats = FeatureStats(24, 'cpu')
    for chunk in x.split(step):
        assert stats.append(chunk) is stats
    # both forms are within the raw-moment bound of the exact statistics: each is compared with the two-pass reference under the same tolerance
    assert_statistics(stats, x, 'chunks of %d' % step)
    assert_statistics(FeatureStats.from_features(x), x, 'one append')
    assert_statistics(FeatureStats(24).append(x[::2]).append(x[1::2]), torch.cat([x[::2], x[1::2]]), 'strided views')


def test_merge_empty_batches_and_too_few_rows():
    x = rows(51, 20, 9)
    whole = FeatureStats.from_features(x)
    halves = FeatureStats.from_features(x[:25]).merge_(FeatureStats.from_features(x[25:]))
    assert halves.n == 51
    assert_statistics(halves, x, 'merge of two halves')
    assert np.allclose(halves.numpy()[1], whole.numpy()[1], rtol=0, atol=float(bounds(x.numpy().astype(np.float64))[3].max()))
    before = (whole.n, whole.s1.clone(), whole.s2.clone())
    whole.append(x[:0]).append(torch.zeros(0, 20))          # b = 0: nothing
    assert whole.n == before[0] and torch.equal(whole.s1, before[1]) and torch.equal(whole.s2, before[2])
    one = FeatureStats(20).append(x[:1])
    assert one.n == 1 and torch.equal(one.mean(), x[0].double())
    with pytest.raises(ValueError, match='at least 2'):
        one.cov()
    with pytest.raises(ValueError, match='at least 2'):
        FeatureStats(20).numpy()
    with pytest.raises(ValueError, match='features expected'):
        one.append(torch.zeros(3, 21))
    with pytest.raises(ValueError, match='features'):
        one.merge_(FeatureStats(21))
    assert one.all_reduce_() is one and one.n == 1          # torch.distributed is not initialised: the identity


# ---- the eigen form ----------------------------------------------------------------------------------------------------------------

def pair(f, n1, n2, seed):
    """(m1, c1, m2, c2) of two float32 samples of n1 and n2 rows: one with mixed (correlated) features, one with independent ones."""
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((f, f)) / np.sqrt(f)
    a = (rng.standard_normal((n1, f)) @ mix + 0.3).astype(np.float32).astype(np.float64)
    b = (rng.standard_normal((n2, f)) * 0.8 + 0.1).astype(np.float32).astype(np.float64)
    return fid_module.feature_statistics(a) + fid_module.feature_statistics(b)


# F -> 16 x the measured |frechet_distance - frechet_distance_eigh| on pair(F, 3 F, 4 F, F): measured 1.07e-14 (F = 16), 1.71e-13 (F = 64)
FULL_RANK_TOL = {16: 16 * 1.07e-14, 64: 16 * 1.71e-13}
# 16 x the measured |eigen form - sum sqrt(max(Re eigvals(c1 c2), 0)) form| on pair(64, 32, 37, 164): measured 7.29e-9 (the zero eigenvalues
# of the non-symmetric product come back as +-1e-16-size numbers, whose roots are 1e-8 each: the independent form is the less accurate one)
DEFICIENT_TOL = 16 * 7.29e-9


@pytest.mark.parametrize('f', [16, 64])
def test_eigen_form_equals_sqrtm_on_full_rank_statistics(f):
    m1, c1, m2, c2 = pair(f, 3 * f, 4 * f, f)
    want, got = fid_module.frechet_distance(m1, c1, m2, c2), fid_module.frechet_distance_eigh(m1, c1, m2, c2)
    print('F = %d: sqrtm %.15g, eigh %.15g, difference %.3e (allowed %.3e)' % (f, want, got, abs(want - got), FULL_RANK_TOL[f]))
    assert abs(want - got) <= FULL_RANK_TOL[f]


def test_eigen_form_on_rank_deficient_statistics():
    f = 64
    m1, c1, m2, c2 = pair(f, f // 2, f // 2 + 5, 100 + f)
    assert np.linalg.matrix_rank(c1) < f and np.linalg.matrix_rank(c2) < f
    got = fid_module.frechet_distance_eigh(m1, c1, m2, c2)
    assert isinstance(got, float) or np.isrealobj(got)
    assert np.isfinite(got) and got >= -1e-9 * (np.trace(c1) + np.trace(c2))
    ev = np.linalg.eigvals(c1 @ c2)
    independent = (m1 - m2) @ (m1 - m2) + np.trace(c1) + np.trace(c2) - 2 * np.sqrt(np.maximum(ev.real, 0.0)).sum()
    print('rank-deficient: eigh %.15g, eigvals form %.15g, difference %.3e (allowed %.3e)' % (got, independent, abs(got - independent), DEFICIENT_TOL))
    assert abs(got - independent) <= DEFICIENT_TOL
    # the distance of a singular C to itself, 2 (tr C - tr sqrt(C^2)): zero up to the roots of noise-level eigenvalues (no eps retry is made)
    zero = np.zeros_like(c1)
    assert abs(fid_module.frechet_distance_eigh(m1, c1, m1, c1)) <= fid_tolerance(zero[0], zero, c1, c1, zero[0])
    with pytest.raises(ValueError, match='method'):
        fid_module.evaluate_fid(None, None, 1, 1, 'cpu', 'nowhere', method='cholesky')


# ---- evaluate_fid / evaluate_quality / real statistics ----------------------------------------------------------------------------------

class _FakeG(torch.nn.Module):
    """Generator stand-in with the reference's call contract: g([z]) -> (img, None)."""

    def __init__(self, channels=3):
        super().__init__()
        self.channels, self.calls = channels, []

    def forward(self, styles):
        z = styles[0]
        self.calls.append(z.shape[0])
        return torch.tanh(z[:, :self.channels * 16].reshape(z.shape[0], self.channels, 4, 4)) + 0.25, None


def _feature_net(img):
    return (torch.nn.functional.avg_pool2d(img, 2),)          # [b, 3, 2, 2] -> 12 features per image


@pytest.fixture(scope='module')
def stat_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('fs') / 'real.pkl')
    real_stats.save_real_features(path, torch.randn(80, 12, generator=torch.Generator().manual_seed(5)) * 0.4 + 0.2)
    return path


def test_default_evaluate_fid_keeps_its_bits_and_streaming_its_draws(stat_path):
    with open(stat_path, 'rb') as fh:
        real = pickle.load(fh)
    # the call as it was: features to the host batch by batch, np.cov, sqrtm
    torch.manual_seed(11)
    feats = fid_module.sample_features(_FakeG(), _feature_net, 8, 45, 'cpu').numpy()
    state = torch.get_rng_state()
    mean, cov = fid_module.feature_statistics(feats)
    parent = fid_module.frechet_distance(mean, cov, real['mean'], real['cov'])
    torch.manual_seed(11)
    g = _FakeG()
    assert fid_module.evaluate_fid(g, _feature_net, 8, 45, 'cpu', stat_path) == parent and g.calls == [8] * 5 + [5]
    assert torch.equal(torch.get_rng_state(), state)
    # streaming: the same draws in the same order ...
    torch.manual_seed(11)
    g = _FakeG()
    streamed = fid_module.evaluate_fid(g, _feature_net, 8, 45, 'cpu', stat_path, streaming=True, method='eigh')
    assert g.calls == [8] * 5 + [5] and torch.equal(torch.get_rng_state(), state)
    # ... and a distance that differs from the host statistics' by no more than the moment bound propagates to
    host = fid_module.frechet_distance_eigh(mean, cov, real['mean'], real['cov'])
    _, _, tm, tc = bounds(feats.astype(np.float64))
    tol = fid_tolerance(tm, tc, cov, real['cov'], mean - real['mean'])
    print('streaming %.15g, host statistics %.15g, difference %.3e (propagated bound %.3e)' % (streamed, host, abs(streamed - host), tol))
    assert abs(streamed - host) <= tol
    torch.manual_seed(11)
    assert fid_module.evaluate_fid(_FakeG(), _feature_net, 8, 45, 'cpu', stat_path, method='eigh') == host
    torch.manual_seed(11)
    stats = fid_module.sample_statistics(_FakeG(), _feature_net, 8, 45, 'cpu')
    assert isinstance(stats, FeatureStats) and stats.n == 45 and stats.num_features == 12 and torch.equal(torch.get_rng_state(), state)


def test_evaluate_quality_streams(stat_path, monkeypatch):
    torch.manual_seed(2)
    want = fid_module.evaluate_fid(_FakeG(), _feature_net, 8, 45, 'cpu', stat_path, streaming=True, method='eigh')
    torch.manual_seed(2)
    default = fid_module.evaluate_quality(_FakeG(), _feature_net, 8, 45, 'cpu', stat_path, metrics=('fid',))
    torch.manual_seed(2)
    plain = fid_module.evaluate_fid(_FakeG(), _feature_net, 8, 45, 'cpu', stat_path)
    assert default == {'fid': plain}
    calls = []
    real_sample = fid_module.sample_features
    monkeypatch.setattr(fid_module, 'sample_features', lambda *a, **k: calls.append(k.get('to_host')) or real_sample(*a, **k))
    torch.manual_seed(2)
    only = fid_module.evaluate_quality(_FakeG(), _feature_net, 8, 45, 'cpu', stat_path, metrics=('fid',), streaming=True, method='eigh')
    assert only == {'fid': want} and calls == []          # FID alone streams: no feature matrix is built at all
    torch.manual_seed(2)
    both = fid_module.evaluate_quality(_FakeG(), _feature_net, 8, 45, 'cpu', stat_path, metrics=('fid', 'kid'), num_subsets=3, max_subset_size=20,
                                       streaming=True, method='eigh')
    assert calls == [False] and sorted(both) == ['fid', 'kid']          # the features stay where they are; the statistics come from them
    # one append of 45 rows against six: each within the propagated moment bound of the distance of the host statistics
    torch.manual_seed(2)
    feats = real_sample(_FakeG(), _feature_net, 8, 45, 'cpu').numpy().astype(np.float64)
    with open(stat_path, 'rb') as fh:
        real = pickle.load(fh)
    mean, cov = fid_module.feature_statistics(feats)
    _, _, tm, tc = bounds(feats)
    assert abs(both['fid'] - want) <= 2 * fid_tolerance(tm, tc, cov, real['cov'], mean - real['mean'])


class _Stream:
    training = False

    def __init__(self, batches):
        self.batches = iter(batches)

    def __next__(self):
        return next(self.batches), None


def test_stream_real_statistics_and_save(tmp_path):
    imgs = torch.rand(23, 3, 4, 4, generator=torch.Generator().manual_seed(8))
    stats = real_stats.stream_real_statistics(_Stream(imgs.split(6)), _feature_net, 20)          # 6 + 6 + 6 + 2 of the last batch's 5
    assert isinstance(stats, FeatureStats) and stats.n == 20
    feats = real_stats.extract_real_features(_Stream(imgs.split(6)), _feature_net, 20)
    assert_statistics(stats, feats, 'real statistics')
    mean, cov = real_stats.save_real_statistics(str(tmp_path / 's.pkl'), stats)
    with open(str(tmp_path / 's.pkl'), 'rb') as fh:
        got = pickle.load(fh)
    assert sorted(got) == ['cov', 'mean'] and np.array_equal(got['mean'], mean) and np.array_equal(got['cov'], cov)
    want_mean, want_cov = real_stats.save_real_statistics(str(tmp_path / 'f.pkl'), feats)          # a feature matrix: as before
    assert np.array_equal(want_mean, fid_module.feature_statistics(feats.double().numpy())[0])
    training = _Stream([])
    training.training = True
    with pytest.raises(ValueError, match='training=False'):
        real_stats.stream_real_statistics(training, _feature_net, 4)


# ---- Tracker -------------------------------------------------------------------------------------------------------------------------

def test_tracker_passes_the_new_keys_and_only_them(monkeypatch):
    calls = []

    def evaluate_fid(*args, **kwargs):
        calls.append(('fid', len(args), kwargs))
        return 3.0

    def evaluate_quality(*args, **kwargs):
        calls.append(('quality', len(args), kwargs))
        return {'fid': 2.0, 'kid': 0.1}

    monkeypatch.setattr(fid_module, 'evaluate_fid', evaluate_fid)
    monkeypatch.setattr(fid_module, 'evaluate_quality', evaluate_quality)
    model = torch.nn.Linear(2, 2)
    base = {'enabled': True, 'fid_interval': 1, 'num_of_samples': 40, 'inception_stat_path': 'stats.pkl'}
    Tracker(torch.zeros(4, 512), None, 'inception', 'normal', fid_config=dict(base)).fid_evaluation(1, model)
    Tracker(torch.zeros(4, 512), None, 'inception', 'normal', fid_config=dict(base, kid=True)).fid_evaluation(1, model)
    # without the keys: positional arguments only (and metrics= for the quality call), as before
    assert calls == [('fid', 6, {}), ('quality', 6, {'metrics': ['fid', 'kid']})]
    del calls[:]
    cfg = dict(base, streaming=True, fid_method='eigh')
    assert Tracker(torch.zeros(4, 512), None, 'inception', 'normal', fid_config=dict(cfg)).fid_evaluation(1, model) == 3.0
    Tracker(torch.zeros(4, 512), None, 'inception', 'normal', fid_config=dict(cfg, kid=True)).fid_evaluation(1, model)
    Tracker(torch.zeros(4, 512), None, 'inception', 'normal', fid_config=dict(base, streaming=False)).fid_evaluation(1, model)
    assert calls == [('fid', 6, {'streaming': True, 'method': 'eigh'}), ('quality', 6, {'metrics': ['fid', 'kid'], 'streaming': True, 'method': 'eigh'}),
                     ('fid', 6, {'streaming': False})]


# ---- the second header and its table -------------------------------------------------------------------------------------------------------

def _declarations(path):
    with open(path) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    return {name: args for name, args in re.findall(r'\b(gc_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;', text, flags=re.S)}


def test_stats_header_and_its_table_agree():
    declared = _declarations(STATS_HEADER)
    assert sorted(declared) == sorted(_lib.STATS_SIGNATURES) and len(declared) == 3
    assert sorted(declared) == sorted([fm.ACCUMULATE_ENTRY, fm.FINISH_ENTRY, fm.MERGE_ENTRY])
    # every one of them is streamed: the stream comes last, as a pointer, in the header and in the table alike
    for name, args in declared.items():
        assert re.search(r'\bgc_stream_t\s+\w+\s*$', args), name
        assert _lib.STATS_SIGNATURES[name][1][-1] is ctypes.c_void_p and _lib.STATS_SIGNATURES[name][0] is ctypes.c_int32
        assert len(_lib.STATS_SIGNATURES[name][1]) == len(args.split(','))
    # the main header and its table stay as the tests that pin them expect
    main = _declarations(MAIN_HEADER)
    assert not set(declared) & set(main) and not set(_lib.STATS_SIGNATURES) & set(_lib.SIGNATURES)
    with open(MAIN_HEADER) as f:
        assert 'feature_moments' not in f.read()
    assert _lib.ABI_VERSION == 2


def test_library_exports_and_binds_the_stats_entries():
    path = _lib.library_path()
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(path)
    lib = _lib.load()
    for name, (res, args) in _lib.STATS_SIGNATURES.items():
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    # bad arguments are refused before any launch: safe without a GPU
    assert lib.gc_feature_moments_accumulate_f32(None, 8, 4, 8, None, None, None) == -1 and b'null' in lib.gc_last_error()
    assert lib.gc_feature_moments_accumulate_f32(1, 8, 0, 8, 1, 1, None) == -1 and b'at least 1' in lib.gc_last_error()
    assert lib.gc_feature_moments_accumulate_f32(1, 7, 4, 8, 1, 1, None) == -1
    assert lib.gc_feature_moments_accumulate_f32(1, 4097, 4, 4097, 1, 1, None) == _lib.GC_ERR_UNSUPPORTED and b'4096' in lib.gc_last_error()
    assert lib.gc_feature_moments_accumulate_f32(1, 2 ** 62, 4, 8, 1, 1, None) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_feature_moments_finish_f64(1, 1, 1, 8, 1, 1, None) == -1 and b'at least 2' in lib.gc_last_error()
    assert lib.gc_feature_moments_finish_f64(1, 1, 5, 4097, 1, 1, None) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_feature_moments_merge_f64(1, 1, None, 1, 8, None) == -1
    assert lib.gc_feature_moments_merge_f64(1, 1, 1, 1, 0, None) == -1


def test_a_library_without_the_stats_entries_is_rejected(monkeypatch):
    _lib.load()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'STATS_SIGNATURES', dict(_lib.STATS_SIGNATURES, gc_feature_moments_of_another_build=(ctypes.c_int32, [])))
    with pytest.raises(RuntimeError, match='does not export gc_feature_moments_of_another_build'):
        _lib.load()


def test_makefile_builds_and_hashes_the_new_files():
    with open(os.path.join(REPO, 'gan-control_amd', 'csrc', 'Makefile')) as f:
        text = f.read()
    srcs = re.search(r'^SRCS := (.*)$', text, flags=re.M).group(1).split()
    hashed = re.search(r'^HASHED := (.*)$', text, flags=re.M).group(1)
    assert 'feature_stats.hip' in srcs and '$(INC)/gancontrol_stats.h' in hashed and '$(INC)/gancontrol_hip.h' in hashed


# ---- all_reduce_ over gloo -------------------------------------------------------------------------------------------------------------

def _reduce_worker(rank, world, port, out):
    for p in (REPO, os.path.join(REPO, 'gan-control_amd'), os.path.join(REPO, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from gan_control_amd.fid_utils.feature_stats import FeatureStats as Stats
    x = rows(41, 18, 77)
    mine = Stats(18).append(x[:20] if rank == 0 else x[20:])
    assert mine.all_reduce_() is mine and mine.n == 41
    if rank == 0:
        torch.save({'mean': mine.mean(), 'cov': mine.cov(), 'n': mine.n}, out)
    dist.destroy_process_group()


def test_all_reduce_of_two_halves_equals_the_whole():
    port = 37500 + os.getpid() % 2000
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'r.pt')
        mp.spawn(_reduce_worker, args=(2, port, out), nprocs=2, join=True)
        got = torch.load(out)
    x = rows(41, 18, 77)
    x64 = x.numpy().astype(np.float64)
    _, _, tm, tc = bounds(x64)
    assert got['n'] == 41
    assert np.all(np.abs(got['mean'].numpy() - x64.mean(0)) <= tm) and np.all(np.abs(got['cov'].numpy() - np.cov(x64, rowvar=False)) <= tc)
    merged = FeatureStats.from_features(x[:20]).merge_(FeatureStats.from_features(x[20:]))
    assert torch.equal(got['cov'], merged.cov()) and torch.equal(got['mean'], merged.mean())          # the sum of two halves, whoever adds them
