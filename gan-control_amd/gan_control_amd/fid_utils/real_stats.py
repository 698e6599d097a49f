"""Inception statistics of a folder of REAL images: the {'mean', 'cov'} pickle ``fid.evaluate_fid`` compares generated images against, and
with ``save_real_features`` the features themselves for the metrics that need them (``fid.evaluate_quality``: KID, precision / recall).

Reference: fid_utils/calc_inception.py:61-80 (``extract_features``: every batch of the loader through ``inception(img)[0]``, flattened per
image, collected on the host) and its ``__main__`` (mean and ``np.cov`` of the features, pickled).  The batches come from a
``datasets.image_folder.DeviceImageStream`` built with ``training=False``: no flip and no crop, as the reference's transform for this job.
"""
import pickle

import torch

from .feature_stats import FeatureStats
from .fid import feature_statistics


@torch.no_grad()
def extract_real_features(stream, feature_net, n_images):
    """float32 [n_images, F] on the host: ``feature_net(img)[0]`` per batch of ``stream`` (an iterator of ``(img, meta)``), in stream order."""
    if getattr(stream, 'training', False):
        raise ValueError('real statistics are taken without flip or crop: build the stream with training=False')
    feats, have = [], 0
    while have < n_images:
        img, _ = next(stream)
        f = feature_net(img)[0]
        feats.append(f.reshape(img.shape[0], -1).to('cpu'))
        have += img.shape[0]
    return torch.cat(feats, 0)[:n_images]


@torch.no_grad()
def stream_real_statistics(stream, feature_net, n_images):
    """``extract_real_features`` without the features: every batch of ``stream`` goes into a ``FeatureStats`` on the device that made it (the
    last batch trimmed to ``n_images``); nothing is kept and nothing copied to the host.  -> the ``FeatureStats``."""
    if getattr(stream, 'training', False):
        raise ValueError('real statistics are taken without flip or crop: build the stream with training=False')
    stats, have = None, 0
    while have < n_images:
        img, _ = next(stream)
        f = feature_net(img)[0]
        f = f.reshape(img.shape[0], -1)[:n_images - have]
        if stats is None:
            stats = FeatureStats(f.shape[1], f.device)
        stats.append(f)
        have += f.shape[0]
    if stats is None:
        raise ValueError('stream_real_statistics: no images asked for (n_images = %r)' % (n_images,))
    return stats


def save_real_statistics(path, features):
    """Pickle {'mean', 'cov'} of a [n, F] feature matrix -- or of a ``FeatureStats`` (``stream_real_statistics``) -- where
    ``evaluate_fid(..., inception_stat_path=path)`` reads it."""
    if isinstance(features, FeatureStats):
        mean, cov = features.numpy()
    else:
        f = features.double().numpy() if torch.is_tensor(features) else features
        mean, cov = feature_statistics(f)
    with open(path, 'wb') as fh:
        pickle.dump({'mean': mean, 'cov': cov}, fh)
    return mean, cov


def save_real_features(path, features):
    """``save_real_statistics``'s pickle plus ``'features'``: the float32 [n, F] matrix itself, which KID and precision / recall compare
    generated features against (``fid.evaluate_quality``).  ``evaluate_fid`` reads the same file."""
    host = features.detach().cpu() if torch.is_tensor(features) else torch.as_tensor(features)
    f = host.double().numpy()
    mean, cov = feature_statistics(f)
    with open(path, 'wb') as fh:
        pickle.dump({'mean': mean, 'cov': cov, 'features': host.float().numpy()}, fh)
    return mean, cov
