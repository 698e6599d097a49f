"""Improved precision and recall (Kynkaanniemi et al. 2019, "Improved Precision and Recall Metric for Assessing Generative Models") of
generated against real Inception features.

Each set spans a manifold: the union of the balls around its rows whose squared radius is the squared distance to the row's ``kth``
nearest other row (k = 3 in the paper).  Precision is the share of generated rows inside the real manifold, recall the share of real rows
inside the generated one.  Two ``knn_radii`` calls and ONE ``manifold_hits`` call (models/op/manifold.py): the hit pass reads D(real, fake)
once for both figures, and the features stay on the device they are on.
"""
from ..models.op import manifold


def precision_recall(real_features, fake_features, kth=3):
    """{'precision', 'recall'} (floats) of float32 ``[n_real, F]`` and ``[n_fake, F]`` features on one device."""
    real_r2 = manifold.knn_radii(real_features, kth)
    fake_r2 = manifold.knn_radii(fake_features, kth)
    fake_in_real, real_in_fake = manifold.manifold_hits(real_features, real_r2, fake_features, fake_r2)
    return {'precision': float(fake_in_real.double().mean()), 'recall': float(real_in_fake.double().mean())}
