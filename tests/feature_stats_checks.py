"""The derived tolerances the feature-statistics tests share (tests only; the derivation is in include/gancontrol_stats.h and in the module
docstring of tests/test_feature_stats_gpu.py)."""
import numpy as np

U = 2.0 ** -53


def gamma(n):
    return n * U / (1 - n * U)


def bounds(x64):
    """Tolerances (s1, s2, mean, cov) against the float64 formulas / two-pass np.mean, np.cov for the rows x64 [n, F] (float64 numpy): each is
    the bound of the raw-moment form plus the bound of the reference itself."""
    n = x64.shape[0]
    ax = np.abs(x64)
    p, a = ax.T @ ax, ax.sum(0)
    g = gamma(n)
    aa = np.outer(a, a) / n
    cov = ((2 * g + 8 * U) * (p + aa) + (g + 4 * U) * (p + 7 * aa)) / max(n - 1, 1)
    return 2 * g * a, 2 * g * p, 2 * (g + U) * a / n, cov


def fid_tolerance(mean_tol, cov_tol, c1, c2, delta_mean):
    """How far the Frechet distance (eigen form) moves when the sample statistics move by at most ``mean_tol`` / ``cov_tol`` elementwise.

    tr sqrt: the nonzero eigenvalues mu of R C2 R are those of C2^(1/2) C1 C2^(1/2); a perturbation E of C1 moves each by at most
    |C2|_2 |E|_2 (Weyl), and |sqrt(a) - sqrt(b)| <= sqrt|a - b|, so the F roots move by at most F sqrt(|C2|_2 eps) in all.  eps: |E|_2 <= |E|_F <=
    |cov_tol|_F, plus the backward error of the two symmetric eigensolvers, taken as 64 F u |C1|_2 (LAPACK's bound is a modest multiple of
    F u |A|_2).  The traces move by at most tr(cov_tol), |dm|^2 by at most 2 |dm| |mean_tol| + |mean_tol|^2."""
    f = c1.shape[0]
    eps = float(np.linalg.norm(cov_tol)) + 64 * f * U * float(np.linalg.norm(c1, 2))
    roots = 2 * f * np.sqrt(float(np.linalg.norm(c2, 2)) * eps)
    dm, tm = float(np.linalg.norm(delta_mean)), float(np.linalg.norm(mean_tol))
    return roots + float(np.trace(cov_tol)) + 2 * dm * tm + tm * tm
