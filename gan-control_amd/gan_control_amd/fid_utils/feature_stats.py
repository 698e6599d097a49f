"""``FeatureStats``: the mean and covariance of a stream of feature batches, from float64 raw moments kept on the features' device.

``append`` adds a batch to ``s1 = sum x`` and the upper triangle of ``s2 = sum x x^T`` (models/op/feature_moments.py: one HIP launch per
batch on the GPU, the float64 torch formula elsewhere); nothing is copied to the host and no feature is kept.  ``mean()`` / ``cov()``
finish the moments on the device (``np.cov``'s divisor, n - 1); ``numpy()`` is the one copy to the host, for the Frechet distance.
Raw moments are additive: ``merge_`` adds another accumulator, ``all_reduce_`` sums the accumulators of a process group, so every rank
of a data-parallel run can contribute its share of ONE FID sample.

The raw-moment form subtracts ``s1 s1^T / n`` from ``s2``: where the mean dominates the spread it loses ``mean^2 / variance`` in relative
accuracy against the two-pass formula, which is why the moments are float64 and their products exact; the elementwise bound is in
include/gancontrol_stats.h.
"""
import torch

from ..models.op import feature_moments as fm


class FeatureStats:
    def __init__(self, num_features, device='cpu'):
        num_features = int(num_features)
        if num_features < 1:
            raise ValueError('FeatureStats: at least one feature, got %d' % num_features)
        self.num_features = num_features
        self.device = torch.device(device)
        self.n = 0
        self.s1, self.s2 = fm.new_accumulator(num_features, self.device)

    @classmethod
    def from_features(cls, x):
        """The statistics of one [n, F] feature matrix, on its device."""
        x = torch.as_tensor(x)
        if x.dim() != 2:
            raise ValueError('FeatureStats.from_features: [n, F] features expected, got %s' % (tuple(x.shape),))
        return cls(x.shape[1], x.device).append(x)

    @torch.no_grad()
    def append(self, features):
        """Add a [b, F] batch (``b = 0``: nothing).  Floating-point features of another dtype than float32 take the formula in float64."""
        x = torch.as_tensor(features)
        if x.dim() != 2 or x.shape[1] != self.num_features:
            raise ValueError('FeatureStats.append: [b, %d] features expected, got %s' % (self.num_features, tuple(x.shape)))
        if x.shape[0] == 0:
            return self
        if x.device != self.device:
            x = x.to(self.device)
        fm.accumulate_(self.s1, self.s2, x)
        self.n += int(x.shape[0])
        return self

    def _finish(self):
        if self.n < 2:
            raise ValueError('FeatureStats: a covariance needs at least 2 rows, %d appended' % self.n)
        return fm.finish(self.s1, self.s2, self.n)

    def mean(self):
        """float64 [F] on the accumulator's device."""
        if self.n < 1:
            raise ValueError('FeatureStats: no rows appended')
        # the finish entry's own formula, without forming a covariance: a true division by a tensor (a Python divisor becomes a multiplication
        # by its reciprocal on the device, another rounding than the entry's)
        return self.s1 / torch.full((), float(self.n), dtype=torch.float64, device=self.device)

    def cov(self):
        """float64 [F, F] on the accumulator's device, exactly symmetric; ``ValueError`` for fewer than 2 rows."""
        return self._finish()[1]

    def numpy(self):
        """(mean, cov) as float64 arrays: the one copy to the host."""
        mean, cov = self._finish()
        return mean.cpu().numpy(), cov.cpu().numpy()

    @torch.no_grad()
    def merge_(self, other):
        """Add the rows of another accumulator of the same width (moved to this device if need be)."""
        if other.num_features != self.num_features:
            raise ValueError('FeatureStats.merge_: %d and %d features' % (self.num_features, other.num_features))
        s1b, s2b = other.s1, other.s2
        if s1b.device != self.device:
            s1b, s2b = s1b.to(self.device), s2b.to(self.device)
        fm.merge_(self.s1, self.s2, s1b, s2b)
        self.n += other.n
        return self

    @torch.no_grad()
    def all_reduce_(self, group=None):
        """Sum ``n``, ``s1`` and ``s2`` over the process group; the identity when ``torch.distributed`` is not initialised.  (``s2`` is summed
        whole: the elements below the diagonal are undefined before and after.)"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        count = torch.tensor([self.n], dtype=torch.int64, device=self.device)
        dist.all_reduce(count, group=group)
        dist.all_reduce(self.s1, group=group)
        dist.all_reduce(self.s2, group=group)
        self.n = int(count.item())
        return self

