"""Inputs and float64 references shared by test_quality_metrics.py and test_quality_metrics_gpu.py (no test in here).

Every reference restates a formula of models/op/manifold.py in float64 on the upcast float32 inputs, with numpy / torch on the host; none
calls the code under test.  References are cached per case and must not be modified by a test.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24

# (n_real, n_fake, F, kth, row stride): the listed shapes, then row counts {kth + 1, 7, 63, 64, 65, 129, 257}, F in {1, 3, 4, 5, 31, 32, 33},
# kth in {1, 3, 7} and the three strides
DISTANCE_CASES = [(5, 4, 3, 1, 'k'), (65, 63, 5, 3, 'k+1'), (129, 130, 33, 3, '2k'), (193, 161, 67, 1, 'k'), (257, 300, 131, 3, 'k'),
                  (130, 70, 2048, 3, 'k'), (8, 9, 1, 7, 'k'), (7, 64, 4, 3, 'k+1'), (64, 7, 31, 1, '2k'), (63, 65, 32, 3, 'k'),
                  (4, 129, 33, 3, 'k'), (257, 64, 5, 7, 'k+1'), (2, 63, 3, 1, '2k')]
# more column tiles than one strip holds (32 strips a side): 34 tiles of 64 on the probe side, then on the ref side (one side within 64
# rows: the 64-wide tile), and both sides above 1920 rows: the 128-wide tile of the hit kernel, 17 tiles a side, with 16-byte loads (F = 4)
# and without.  The radii of 4161 rows walk 33 tiles of 128 in strips of 2, on both load paths.
STRIP_HITS_CASES = [(7, 2113, 3, 3, 'k'), (2113, 7, 5, 3, 'k+1'), (2113, 2177, 4, 3, 'k'), (2177, 2113, 3, 1, 'k+1')]
BIG_TILE_HITS_CASE = (4161, 4225, 4, 3, 'k')          # the 128-wide tile AND more tiles than a strip holds on both sides (33 and 34)
STRIP_KNN_CASES = [(4161, 3, 3, 'k'), (4161, 4, 3, 'k')]          # (n, F, kth, stride)

# (m, subsets, F, row stride) of the KID sums; nx = m + 5, ny = m + 9.  The last two walk 33 tiles of 128 in strips of 2 (4-byte and 16-byte loads).
MMD_CASES = [(2, 1, 1, 'k'), (7, 3, 5, 'k+1'), (63, 1, 67, '2k'), (65, 3, 2048, 'k'), (130, 3, 5, 'k'), (130, 1, 2048, '2k'), (7, 3, 2048, 'k+1'),
             (65, 1, 1, 'k'), (2, 3, 67, 'k'), (4161, 1, 1, 'k'), (4161, 1, 4, 'k')]


def feature_set(seed, n, scale, shift, f):
    """Rows near a 6-dimensional subspace of R^F: distances spread, and two sets made this way overlap partly."""
    p = np.random.RandomState(1234).randn(6, f)
    rs = np.random.RandomState(seed)
    latent = rs.randn(n, 6) * scale + shift
    return (latent @ p / np.sqrt(6.0) + 0.05 * rs.randn(n, f)).astype(np.float32)


def real_fake(n_r, n_f, f):
    return feature_set(1, n_r, 1.0, 0.0, f), feature_set(2, n_f, 0.8, 0.4, f)


def sq_dist64(a, b):
    """D64 [m, n] = sum_c (a[i, c] - b[j, c])^2 in float64, a few rows at a time."""
    a64, b64 = torch.from_numpy(np.asarray(a)).double(), torch.from_numpy(np.asarray(b)).double()
    step = max(1, (1 << 23) // (b64.shape[0] * b64.shape[1]))
    rows = []
    for i in range(0, a64.shape[0], step):
        d = a64[i:i + step, None, :] - b64[None, :, :]
        rows.append((d * d).sum(-1))
    return torch.cat(rows, 0)


def radii64(a, kth):
    """The (kth + 1)-th smallest value of every row of D64(a, a)."""
    return sq_dist64(a, a).sort(dim=1).values[:, kth].contiguous()


def hits64(d, ref_r, probe_r, e):
    """(probe_hit, ref_hit, probe undecided, ref undecided): the float64 decisions, and which of them change inside the band r (1 -+ e)."""
    def side(radius, dim):
        lo = (d <= radius * (1 - e)).any(dim)
        hi = (d <= radius * (1 + e)).any(dim)
        return (d <= radius).any(dim), lo != hi
    p_hit, p_und = side(ref_r[:, None], 0)
    r_hit, r_und = side(probe_r[None, :], 1)
    return p_hit, r_hit, p_und, r_und


@functools.lru_cache(maxsize=None)
def distance_case(n_r, n_f, f, kth):
    """real, fake (float32 numpy) and the float64 references of one case."""
    real, fake = real_fake(n_r, n_f, f)
    d = sq_dist64(real, fake)
    rr, fr = radii64(real, kth), radii64(fake, kth)
    e = 3 * (f + 4) * U
    p_hit, r_hit, p_und, r_und = hits64(d, rr, fr, e)
    return {'real': real, 'fake': fake, 'real_r2': rr, 'fake_r2': fr, 'probe_hit': p_hit, 'ref_hit': r_hit, 'probe_undecided': p_und,
            'ref_undecided': r_und}


def mmd_inputs(m, subsets, f):
    """x [m + 5, F], y [m + 9, F] non-negative float32 and the index draws of the case (seed = m)."""
    rs = np.random.RandomState(m)
    x = (np.abs(rs.randn(m + 5, f)) * 0.5).astype(np.float32)
    y = (np.abs(rs.randn(m + 9, f) * 1.1 + 0.1) * 0.5).astype(np.float32)
    idx_x = np.stack([rs.choice(m + 5, m, replace=False) for _ in range(subsets)])
    idx_y = np.stack([rs.choice(m + 9, m, replace=False) for _ in range(subsets)])
    return x, y, idx_x, idx_y


def mmd_sums64(x, y, idx_x, idx_y):
    """float64 [subsets, 3]: the three kernel sums with float64 dot products."""
    f = x.shape[1]
    out = np.zeros((idx_x.shape[0], 3))
    for s in range(idx_x.shape[0]):
        xs, ys = x[idx_x[s]].astype(np.float64), y[idx_y[s]].astype(np.float64)
        kxx, kyy, kxy = ((a @ b.T / f + 1.0) ** 3 for a, b in ((xs, xs), (ys, ys), (xs, ys)))
        out[s] = [kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()]
    return out


def kid_parts64(sums, m):
    """(A, B): the two positive parts of the KID value, kid = A - B."""
    return float(np.mean((sums[:, 0] + sums[:, 1]) / (m - 1)) / m), float(np.mean(2.0 * sums[:, 2] / m) / m)


@functools.lru_cache(maxsize=None)
def mmd_case(m, subsets, f):
    x, y, idx_x, idx_y = mmd_inputs(m, subsets, f)
    return {'x': x, 'y': y, 'idx_x': idx_x, 'idx_y': idx_y, 'sums': mmd_sums64(x, y, idx_x, idx_y)}
