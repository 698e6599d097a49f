"""Kernel Inception Distance (Binkowski et al. 2018, "Demystifying MMD GANs"): the unbiased squared MMD of generated against real Inception
features under the polynomial kernel ``kappa(u, v) = (u . v / F + 1)^3``, averaged over random subsets -- the figure the ADA work reports
for data sets as small as MetFaces, where FID is badly biased.

For subset ``s`` of ``m = min(n_real, n_fake, max_subset_size)`` rows a side, X drawn from the generated and Y from the real features,

    kid = mean_s [ (sum_{i != j} kappa(X_i, X_j) + sum_{i != j} kappa(Y_i, Y_j)) / (m - 1) - 2 sum_{i, j} kappa(X_i, Y_j) / m ] / m

The three sums of every subset come from ONE ``poly_mmd_sums`` call (models/op/manifold.py), which gathers the rows where they lie.
"""
import numpy as np

from ..models.op import manifold


def subset_indices(n_real, n_fake, num_subsets=100, max_subset_size=1000, seed=0):
    """(idx_x [num_subsets, m] into the generated rows, idx_y [num_subsets, m] into the real rows) from ``RandomState(seed)``: per subset
    ``choice(n_fake, m, replace=False)``, then ``choice(n_real, m, replace=False)``."""
    m = min(int(n_real), int(n_fake), int(max_subset_size))
    if m < 2 or num_subsets < 1:
        raise ValueError('kid: subsets of %d rows (%d real, %d generated features, %d subsets): at least 2 rows and 1 subset' % (m, n_real, n_fake, num_subsets))
    rs = np.random.RandomState(seed)
    idx_x, idx_y = np.empty((num_subsets, m), np.int64), np.empty((num_subsets, m), np.int64)
    for s in range(num_subsets):
        idx_x[s] = rs.choice(n_fake, m, replace=False)
        idx_y[s] = rs.choice(n_real, m, replace=False)
    return idx_x, idx_y


def kid_from_sums(sums, m):
    """The value from the float64 ``[subsets, 3]`` sums of ``poly_mmd_sums``."""
    s = np.asarray(sums.cpu() if hasattr(sums, 'cpu') else sums, dtype=np.float64)
    return float(np.mean((s[:, 0] + s[:, 1]) / (m - 1) - 2.0 * s[:, 2] / m) / m)


def kid(real_features, fake_features, num_subsets=100, max_subset_size=1000, seed=0):
    """KID (a float) of float32 ``[n_real, F]`` and ``[n_fake, F]`` features on one device."""
    idx_x, idx_y = subset_indices(real_features.shape[0], fake_features.shape[0], num_subsets, max_subset_size, seed)
    return kid_from_sums(manifold.poly_mmd_sums(fake_features, real_features, idx_x, idx_y), idx_x.shape[1])
