"""Streaming raw moments of feature rows (fid_utils/feature_stats.py: FID statistics without a host copy of the features).

The accumulator of F features is ``s1 [F]`` and ``s2 [F, F]``, float64 on the features' device, zeros when fresh:
``s1[i] = sum_k x[k, i]`` and ``s2[i, j] = sum_k x[k, i] x[k, j]`` for ``j >= i``.  ONLY the upper triangle of ``s2`` is defined (the
kernel may leave anything below it inside the 64 x 64 tiles on the diagonal); every function here reads the upper triangle only.

``accumulate_(s1, s2, x)``: adds the rows of ``x [n, F]`` (``n = 0``: nothing).  Formula, ``accumulate_reference_``: ``xd = x.double();
s1 += xd.sum(0); s2 += xd.T @ xd``.
``finish(s1, s2, n) -> (mean [F], cov [F, F])``: ``mean = s1 / n`` and the full symmetric ``cov = (S2 - s1 s1^T / n) / (n - 1)`` (``np.cov``'s
divisor; ``n >= 2``), ``S2`` the upper triangle mirrored.  Formula: ``finish_reference``.
``merge_(s1a, s2a, s1b, s2b)``: ``s1a += s1b``, upper ``s2a += s2b``.  A KERNEL (gc_feature_moments_merge_f64), not torch ops: the torch
expression would add the undefined elements below the diagonal too, or build an F x F mask.  Formula: ``merge_reference_``.

The error bound of the kernels is derived in include/gancontrol_stats.h and tests/test_feature_stats_gpu.py.

The dispatch rule.  A call is ONE launch of its entry when ALL of these hold:

* the HIP backend is active, the accumulator (and ``mean`` / ``cov``) is dense CUDA float64 and ``x`` CUDA float32, all on one device;
* ``x`` has adjacent-element rows at least F apart (``features[::2]`` and a row-pitched buffer are read in place);
* 1 <= F <= MAX_FEATURES; accumulate: 1 <= n <= MAX_ROWS; finish: 2 <= n.

No size threshold: profiles/feature_stats.md has the shapes measured.  Everything else -- CPU tensors, the emulated backend of the
tests, other dtypes, shapes beyond the limits -- takes the formulas.
"""
import torch          # every device allocation below goes through this name: tests swap it for a guard-banded allocator

from ... import _lib
from . import _backend
# part of this module's interface: the guard-banded allocator of the tests (guarded(module)) reaches the launch path as module.HipBackend._launch
from ._backend import HipBackend          # noqa: F401

ACCUMULATE_ENTRY = 'gc_feature_moments_accumulate_f32'
FINISH_ENTRY = 'gc_feature_moments_finish_f64'
MERGE_ENTRY = 'gc_feature_moments_merge_f64'
MAX_FEATURES = 4096                       # GC_STATS_MAX_FEATURES (include/gancontrol_stats.h)
TILE = 64                                 # GC_STATS_TILE: the s2 tile one workgroup owns
MAX_ROWS = 2 ** 31 - 1                    # rows of one call: the entry takes n as an int


def new_accumulator(features, device):
    """A fresh (s1, s2)."""
    return (torch.zeros(features, dtype=torch.float64, device=device), torch.zeros(features, features, dtype=torch.float64, device=device))


def _row_stride(x):
    """The row stride (elements) of a [n, F] tensor whose rows are adjacent-element rows at least F apart, else None."""
    n, f = x.shape
    if f > 1 and x.stride(1) != 1:
        return None
    stride = x.stride(0) if n > 1 else f          # (a single row may report any stride, and none is used)
    return stride if stride >= f else None


def _accumulator_ok(s1, s2):
    return (s1.is_cuda and s2.is_cuda and s1.device == s2.device and s1.dtype == s2.dtype == torch.float64 and s1.is_contiguous()
            and s2.is_contiguous() and 1 <= s1.shape[0] <= MAX_FEATURES)


def _hip():
    return getattr(_backend.get(), 'name', None) == 'hip'


def kernel_taken(s1, s2, x=None, other=None):
    """The dispatch rule (module docstring): ``kernel_taken(s1, s2, x)`` -- accumulate_ --, ``kernel_taken(s1, s2)`` -- finish (for n >= 2) --,
    ``kernel_taken(s1a, s2a, other=(s1b, s2b))`` -- merge_."""
    if not (_hip() and _accumulator_ok(s1, s2)):
        return False
    if other is not None:
        return _accumulator_ok(*other) and other[0].device == s1.device
    if x is None:
        return True
    return x.is_cuda and x.device == s1.device and x.dtype == torch.float32 and 1 <= x.shape[0] <= MAX_ROWS and _row_stride(x) is not None


def _check(s1, s2, what):
    if not (torch.is_tensor(s1) and torch.is_tensor(s2) and s1.dim() == 1 and s1.shape[0] >= 1 and tuple(s2.shape) == (s1.shape[0], s1.shape[0])):
        raise ValueError('%s: an accumulator (s1 [F], s2 [F, F]) expected' % what)


def accumulate_reference_(s1, s2, x):
    xd = x.to(s1.dtype) if x.dtype != s1.dtype else x
    s1 += xd.sum(0)
    s2 += xd.T @ xd
    return s1, s2


def accumulate_(s1, s2, x):
    """In place (module docstring); returns ``(s1, s2)``."""
    _check(s1, s2, 'accumulate_')
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != s1.shape[0]:
        raise ValueError('accumulate_: features [n, %d] expected, got %s' % (s1.shape[0], tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    if x.shape[0] == 0:
        return s1, s2
    x = x.detach()
    if not kernel_taken(s1, s2, x):
        with torch.no_grad():
            return accumulate_reference_(s1, s2, x.to(s1.device))
    _backend.get()._launch(x.device, ACCUMULATE_ENTRY, x.data_ptr(), _row_stride(x), x.shape[0], x.shape[1], _lib.ptr(s1), _lib.ptr(s2), _lib.stream_of(x))
    return s1, s2


def finish_reference(s1, s2, n):
    upper = torch.triu(s2)
    full = upper + torch.triu(s2, 1).T
    return s1 / n, (full - torch.outer(s1, s1) / n) / (n - 1)


def finish(s1, s2, n):
    """(mean, cov) of the ``n`` rows the accumulator holds (module docstring)."""
    _check(s1, s2, 'finish')
    n = int(n)
    if n < 2:
        raise ValueError('finish: a covariance needs at least 2 rows, the accumulator holds %d' % n)
    if not kernel_taken(s1, s2):
        with torch.no_grad():
            return finish_reference(s1, s2, n)
    f = s1.shape[0]
    mean = torch.empty(f, dtype=torch.float64, device=s1.device)
    cov = torch.empty(f, f, dtype=torch.float64, device=s1.device)
    _backend.get()._launch(s1.device, FINISH_ENTRY, _lib.ptr(s1), _lib.ptr(s2), n, f, _lib.ptr(mean), _lib.ptr(cov), _lib.stream_of(s1))
    return mean, cov


def merge_reference_(s1a, s2a, s1b, s2b):
    s1a += s1b.to(s1a.device)
    s2a += torch.triu(s2b.to(s2a.device))
    return s1a, s2a


def merge_(s1a, s2a, s1b, s2b):
    """In place on the first accumulator (module docstring); returns it."""
    _check(s1a, s2a, 'merge_')
    _check(s1b, s2b, 'merge_')
    if s1a.shape != s1b.shape:
        raise ValueError('merge_: accumulators of %d and %d features' % (s1a.shape[0], s1b.shape[0]))
    if not kernel_taken(s1a, s2a, other=(s1b, s2b)):
        with torch.no_grad():
            return merge_reference_(s1a, s2a, s1b, s2b)
    _backend.get()._launch(s1a.device, MERGE_ENTRY, _lib.ptr(s1a), _lib.ptr(s2a), _lib.ptr(s1b), _lib.ptr(s2b), s1a.shape[0], _lib.stream_of(s1a))
    return s1a, s2a
