"""Generator-side FID evaluation.

Reference: fid_utils/fid.py:14-40 (extract_feature_from_samples), :43-66 (calc_fid) and evaluate_fid.py:11-35.
The generator forward is the HIP hot path (gan_control_amd.models.gan_model.Generator); the distance itself is
host-side numpy / scipy exactly as in the reference (it runs once per 10 000 iterations on 2048-dimensional statistics).
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


def evaluate_fid(generator, feature_net, batch, n_sample, device, inception_stat_path, training=False):
    """FID of ``n_sample`` generated images against pickled real statistics {'mean', 'cov'} (evaluate_fid.py:11-35)."""
    t0 = time.time()
    generator.eval()
    if hasattr(feature_net, 'eval'):
        feature_net.eval()
    feats = sample_features(generator, feature_net, batch, n_sample, device, training=training).numpy()
    print(f'extracted {feats.shape[0]} features')
    mean, cov = feature_statistics(feats)
    with open(inception_stat_path, 'rb') as f:
        real = pickle.load(f)
    fid = frechet_distance(mean, cov, real['mean'], real['cov'])
    print('fid: %.3f, time: %.3f (min)' % (fid, (time.time() - t0) / 60))
    return fid


QUALITY_METRICS = ('fid', 'kid', 'precision_recall')


def evaluate_quality(generator, feature_net, batch, n_sample, device, inception_stat_path, metrics=QUALITY_METRICS, training=False, kth=3,
                     num_subsets=100, max_subset_size=1000, seed=0):
    """The chosen ``metrics`` of ONE sample of ``n_sample`` generated images -> a dict with 'fid', 'kid', 'precision' and 'recall' (those asked for).

    FID is ``evaluate_fid``'s host formula on a host copy of the generated features (the same value for the same RNG state; unlike
    ``evaluate_fid`` the pickle is read and checked BEFORE anything is sampled).  When a metric beside FID is asked for, the features stay
    whole on the device -- n_sample x F floats more at the peak than ``evaluate_fid``, which moves them batch by batch; with
    ``metrics=('fid',)`` they are moved batch by batch here too.  KID (kid.py) and precision / recall (precision_recall.py) compare them on the device with the real features, the
    float32 ``'features'`` array that ``real_stats.save_real_features`` pickles beside {'mean', 'cov'}."""
    from .kid import kid
    from .precision_recall import precision_recall
    unknown = [m for m in metrics if m not in QUALITY_METRICS]
    if unknown or not metrics:
        raise ValueError('evaluate_quality: metrics must be some of %s, got %r' % (QUALITY_METRICS, tuple(metrics)))
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
    feats = sample_features(generator, feature_net, batch, n_sample, device, training=training, to_host=not need_features)
    print(f'extracted {feats.shape[0]} features')
    out = {}
    if 'fid' in metrics:
        mean, cov = feature_statistics(feats.to('cpu').numpy())
        out['fid'] = frechet_distance(mean, cov, real['mean'], real['cov'])
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
