"""Generator-side FID evaluation.

Reference: fid_utils/fid.py:14-40 (extract_feature_from_samples), :43-66 (calc_fid) and evaluate_fid.py:11-35.
The generator forward is the HIP hot path (gan_control_amd.models.gan_model.Generator); the distance itself is
host-side numpy / scipy exactly as in the reference (it runs once per 10 000 iterations on 2048-dimensional statistics).

Beyond the reference, both opt-in: ``streaming=True`` takes the statistics from float64 moments accumulated on the device batch by batch
(``sample_statistics`` -> fid_utils/feature_stats.py; no feature leaves the device, one copy of mean and covariance at the end), and
``method='eigh'`` evaluates the trace term through two symmetric eigenproblems (``frechet_distance_eigh``), which stays real for the
rank-deficient covariance of fewer images than features.  Without them every call is the code path and the bits of the reference form.
"""
import pickle
import time

import numpy as np
import torch
from scipy import linalg


def _batch_plan(n_sample, batch_size):
    """Full batches followed by one remainder batch (fid.py:22-27)."""
    full, rest = divmod(int(n_sample), int(batch_size))
    return [int(batch_size)] * full + ([rest] if rest else [])


@torch.no_grad()
def sample_features(generator, feature_net, batch_size, n_sample, device='cuda', training=True, latent_dim=512, generator_fn=None, to_host=True):
    """Features of ``n_sample`` generated images, in generation order: on the host, or with ``to_host=False`` on the device that made them.

    ``feature_net(img)[0]`` is flattened per image (fid.py:34); single-channel images are replicated to three channels
    (fid.py:32-33).  ``training`` only silences the progress output in the reference and is accepted for call compatibility.
    """
    feats = []
    for b in _batch_plan(n_sample, batch_size):
        z = torch.randn(b, latent_dim, device=device)
        img = generator([z])[0] if generator_fn is None else generator_fn(z)
        if img.shape[1] == 1:
            img = img.expand(-1, 3, -1, -1)
        f = feature_net(img)[0]
        f = f.reshape(img.shape[0], -1)
        feats.append(f.to('cpu') if to_host else f)
    return torch.cat(feats, 0)


@torch.no_grad()
def sample_statistics(generator, feature_net, batch_size, n_sample, device='cuda', training=True, latent_dim=512, generator_fn=None):
    """``sample_features`` without the features: the same ``torch.randn`` draws in the same order, hence the same images, each batch added to a
    ``FeatureStats`` on the device that made it.  -> the ``FeatureStats`` of the ``n_sample`` images."""
    from .feature_stats import FeatureStats
    stats = None
    for b in _batch_plan(n_sample, batch_size):
        z = torch.randn(b, latent_dim, device=device)
        img = generator([z])[0] if generator_fn is None else generator_fn(z)
        if img.shape[1] == 1:
            img = img.expand(-1, 3, -1, -1)
        f = feature_net(img)[0]
        f = f.reshape(img.shape[0], -1)
        if stats is None:
            stats = FeatureStats(f.shape[1], f.device)
        stats.append(f)
    if stats is None:
        raise ValueError('sample_statistics: no samples asked for (n_sample = %r)' % (n_sample,))
    return stats


def feature_statistics(features):
    """Mean and (unbiased, as np.cov) covariance of a [n, F] feature matrix (evaluate_fid.py:25-26)."""
    f = np.asarray(features, dtype=np.float64) if not isinstance(features, np.ndarray) else features
    return np.mean(f, 0), np.cov(f, rowvar=False)


def frechet_distance(sample_mean, sample_cov, real_mean, real_cov, eps=1e-6):
    """|m1 - m2|^2 + tr(C1) + tr(C2) - 2 tr((C1 C2)^(1/2)), with the reference's handling of a singular product
    (retry with eps on both diagonals) and of a complex square root (imaginary diagonal above 1e-3 is an error)."""
    root, _ = linalg.sqrtm(sample_cov @ real_cov, disp=False)
    if not np.isfinite(root).all():
        print('product of cov matrices is singular')
        ridge = eps * np.eye(sample_cov.shape[0])
        root = linalg.sqrtm((sample_cov + ridge) @ (real_cov + ridge))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError(f'Imaginary component {np.max(np.abs(root.imag))}')
        root = root.real
    delta = sample_mean - real_mean
    return delta @ delta + np.trace(sample_cov) + np.trace(real_cov) - 2 * np.trace(root)


calc_fid = frechet_distance        # the reference's name (fid.py:43)


def frechet_distance_eigh(sample_mean, sample_cov, real_mean, real_cov):
    """The same distance with tr (C1 C2)^(1/2) from two SYMMETRIC eigenproblems, float64 on the host (as projection/pca.py solves its own):
    ``R = V diag(sqrt(max(lambda, 0))) V^T`` from ``eigh(C1)`` is the symmetric root of C1, ``M = R C2 R`` (symmetrised) is similar to
    ``C1 C2`` up to the null space of C1, and the trace term is ``sum sqrt(max(mu, 0))`` over ``eigvalsh(M)``.  Eigenvalues that rounding made
    negative are clipped at zero, so a rank-deficient covariance (fewer images than features) needs no eps retry and gives no complex root."""
    c1, c2 = np.asarray(sample_cov, dtype=np.float64), np.asarray(real_cov, dtype=np.float64)
    lam, vec = np.linalg.eigh(c1)
    root = (vec * np.sqrt(np.maximum(lam, 0.0))) @ vec.T
    m = root @ c2 @ root
    mu = np.linalg.eigvalsh((m + m.T) * 0.5)
    delta = np.asarray(sample_mean, dtype=np.float64) - np.asarray(real_mean, dtype=np.float64)
    return delta @ delta + np.trace(c1) + np.trace(c2) - 2 * np.sqrt(np.maximum(mu, 0.0)).sum()


FID_METHODS = {'sqrtm': frechet_distance, 'eigh': frechet_distance_eigh}


def _distance_fn(method):
    if method not in FID_METHODS:
        raise ValueError('method must be one of %s, got %r' % (sorted(FID_METHODS), method))
    return FID_METHODS[method]


def evaluate_fid(generator, feature_net, batch, n_sample, device, inception_stat_path, training=False, streaming=False, method='sqrtm'):
    """FID of ``n_sample`` generated images against pickled real statistics {'mean', 'cov'} (evaluate_fid.py:11-35).  ``streaming``: the
    statistics come from ``sample_statistics`` (same draws, same images, no feature on the host); ``method``: 'sqrtm' (the reference's) or
    'eigh' (``frechet_distance_eigh``)."""
    distance = _distance_fn(method)
    t0 = time.time()
    generator.eval()
    if hasattr(feature_net, 'eval'):
        feature_net.eval()
    if streaming:
        stats = sample_statistics(generator, feature_net, batch, n_sample, device, training=training)
        print(f'accumulated {stats.n} features')
        mean, cov = stats.numpy()
    else:
        feats = sample_features(generator, feature_net, batch, n_sample, device, training=training).numpy()
        print(f'extracted {feats.shape[0]} features')
        mean, cov = feature_statistics(feats)
    with open(inception_stat_path, 'rb') as f:
        real = pickle.load(f)
    fid = distance(mean, cov, real['mean'], real['cov'])
    print('fid: %.3f, time: %.3f (min)' % (fid, (time.time() - t0) / 60))
    return fid


QUALITY_METRICS = ('fid', 'kid', 'precision_recall')


def evaluate_quality(generator, feature_net, batch, n_sample, device, inception_stat_path, metrics=QUALITY_METRICS, training=False, kth=3,
                     num_subsets=100, max_subset_size=1000, seed=0, streaming=False, method='sqrtm'):
    """The chosen ``metrics`` of ONE sample of ``n_sample`` generated images -> a dict with 'fid', 'kid', 'precision' and 'recall' (those asked for).

    FID is ``evaluate_fid``'s host formula on a host copy of the generated features (the same value for the same RNG state; unlike
    ``evaluate_fid`` the pickle is read and checked BEFORE anything is sampled).  When a metric beside FID is asked for, the features stay
    whole on the device -- n_sample x F floats more at the peak than ``evaluate_fid``, which moves them batch by batch; with
    ``metrics=('fid',)`` they are moved batch by batch here too.  KID (kid.py) and precision / recall (precision_recall.py) compare them on the device with the real features, the
    float32 ``'features'`` array that ``real_stats.save_real_features`` pickles beside {'mean', 'cov'}.

    ``streaming=True``: the FID statistics come from float64 moments on the device -- of the features that stay there for KID / PR
    (``FeatureStats.from_features``: no host copy of them), or accumulated batch by batch with ``metrics=('fid',)`` (``sample_statistics``).
    ``method``: as ``evaluate_fid``."""
    from .feature_stats import FeatureStats
    from .kid import kid
    from .precision_recall import precision_recall
    unknown = [m for m in metrics if m not in QUALITY_METRICS]
    if unknown or not metrics:
        raise ValueError('evaluate_quality: metrics must be some of %s, got %r' % (QUALITY_METRICS, tuple(metrics)))
    distance = _distance_fn(method)
    t0 = time.time()
    generator.eval()
    if hasattr(feature_net, 'eval'):
        feature_net.eval()
    with open(inception_stat_path, 'rb') as f:
        real = pickle.load(f)
    need_features = [m for m in metrics if m != 'fid']
    if need_features and real.get('features') is None:
        raise ValueError("evaluate_quality: %s has no 'features' and %s need the real features themselves: write it with "
                         "fid_utils.real_stats.save_real_features" % (inception_stat_path, ' and '.join(need_features)))
    out = {}
    if streaming and not need_features:
        stats = sample_statistics(generator, feature_net, batch, n_sample, device, training=training)
        print(f'accumulated {stats.n} features')
        mean, cov = stats.numpy()
        out['fid'] = distance(mean, cov, real['mean'], real['cov'])
        print(', '.join('%s: %.4g' % kv for kv in out.items()) + ', time: %.3f (min)' % ((time.time() - t0) / 60))
        return out
    feats = sample_features(generator, feature_net, batch, n_sample, device, training=training, to_host=not need_features)
    print(f'extracted {feats.shape[0]} features')
    if 'fid' in metrics:
        mean, cov = FeatureStats.from_features(feats.float()).numpy() if streaming else feature_statistics(feats.to('cpu').numpy())
        out['fid'] = distance(mean, cov, real['mean'], real['cov'])
    if need_features:
        feats = feats.float()
        real_feats = torch.from_numpy(np.ascontiguousarray(real['features'], dtype=np.float32)).to(feats.device)
        with torch.no_grad():
            if 'kid' in metrics:
                out['kid'] = kid(real_feats, feats, num_subsets=num_subsets, max_subset_size=max_subset_size, seed=seed)
            if 'precision_recall' in metrics:
                out.update(precision_recall(real_feats, feats, kth=kth))
    print(', '.join('%s: %.4g' % kv for kv in out.items()) + ', time: %.3f (min)' % ((time.time() - t0) / 60))
    return out
