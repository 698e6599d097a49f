"""The two device passes of per-group latent PCA (projection/pca.py; reference: projection/projection.py::get_pca_groups).

``places`` is ``{group: (lo, hi)}``: group g is the columns [lo, hi) of a latent row (``Inference._places()``; a vanilla model is
``{None: (0, style_dim)}``).

``group_moments(w [N, D], places) -> (mean, cov)``: per group the mean ``[D_g]`` and the covariance ``[D_g, D_g]`` with divisor N - 1
(scikit-learn's ``explained_variance_`` convention), float64, as per-group views of two packed buffers (``group_moments_packed`` returns the
buffers themselves).  The documented formula, ``moments_reference``, is the two-pass float64 one: ``x = w[:, lo:hi].double()``,
``m = x.mean(0)``, ``(x - m).T @ (x - m) / (N - 1)``.  The kernel (``gc_group_moments_f32``) forms raw moments over a fixed split of the rows
(``ROW_SPLIT`` rows each; longer splits where that would make more than ``MAX_SPLITS``, so the workspace never holds more than ``MAX_SPLITS``
partial sets) and adds the partial sums in a second launch of the same call; its error bound is in include/gancontrol_hip.h and
tests/test_group_pca_gpu.py.

``group_project_(x, mean, components, places)``: in place, every row (the last axis is the latent: ``[B, D]`` and ``[B, n_latent, D]``
alike) and group becomes ``m_g + P_g^T (P_g (x_g - m_g))`` with ``m_g = mean[lo:hi]`` and ``P_g = components[group]`` ``[r_g, D_g]``;
columns outside every group keep their bits.  No autograd: a tensor that requires a gradient is updated through ``.data``, as
``noise_normalize_`` does.  ``project_reference_`` is the float32 torch expression.

The dispatch rule.  A call is ONE gc_group_moments_f32 call (two launches) / ONE gc_group_project_f32 launch when ALL of these hold:

* the HIP backend is active and every tensor is a CUDA float32 tensor on one device;
* rows are adjacent-element rows (``w[::2]`` and a row-pitched buffer are read in place); for the projection the leading axes collapse into
  one row stride, and the mean and every component matrix are dense;
* 1 <= groups <= MAX_GROUPS, every group 1 .. MAX_WIDTH wide inside the row, 2 <= N <= MAX_ROWS (moments), 1 <= r_g <= D_g and groups that
  do not overlap (projection).

No size threshold: neither kernel is slower than its torch formula at any shape measured (profiles/pca_groups.md).  Everything else -- CPU
tensors, the emulated backend of the tests, other dtypes, shapes beyond the limits -- takes the formulas.
"""
import ctypes

import torch          # every device allocation below goes through this name: tests swap it for a guard-banded allocator

from ... import _lib
from . import _backend
# part of this module's interface: the guard-banded allocator of the tests (guarded(module)) reaches the launch path as module.HipBackend._launch
from ._backend import HipBackend          # noqa: F401

MOMENTS_ENTRY = 'gc_group_moments_f32'
MOMENTS_WORKSPACE = 'gc_group_moments_workspace'
PROJECT_ENTRY = 'gc_group_project_f32'
MAX_GROUPS, MAX_WIDTH = 16, 512           # GC_GROUP_MAX / GC_GROUP_MAX_WIDTH (include/gancontrol_hip.h)
ROW_SPLIT = 256                           # GC_GROUP_ROW_SPLIT: rows per partial sum of the moments kernel ...
MAX_SPLITS = 64                           # GC_GROUP_MAX_SPLITS: ... while that makes at most this many partial sums; beyond, longer splits
MAX_ROWS = 65535 * ROW_SPLIT              # GC_GROUP_MAX_ROWS


def _table(places):
    """(names, lo int32 array, hi int32 array) of a places dict, in its order."""
    names = list(places)
    lo = (ctypes.c_int32 * len(names))(*[int(places[k][0]) for k in names])
    hi = (ctypes.c_int32 * len(names))(*[int(places[k][1]) for k in names])
    return names, lo, hi


def _check_places(places, width, what):
    if not places:
        raise ValueError('%s: no groups' % what)
    for k, (lo, hi) in places.items():
        if not 0 <= int(lo) < int(hi) <= width:
            raise ValueError('%s: group %r [%s, %s) is empty or outside rows of %d' % (what, k, lo, hi, width))


def _groups_fit(places):
    return len(places) <= MAX_GROUPS and all(int(hi) - int(lo) <= MAX_WIDTH for lo, hi in places.values())


def _row_stride(t):
    """The row stride (elements) of a [N, D] tensor whose rows are adjacent-element rows at least D apart, else None."""
    n, d = t.shape
    if d > 1 and t.stride(1) != 1:
        return None
    stride = t.stride(0) if n > 1 else d          # (a single row may report any stride, and none is used)
    return stride if stride >= d else None


def _offsets(places):
    """(mean offsets, cov offsets, total mean, total cov) of the packed buffers."""
    mo, co, m, c = {}, {}, 0, 0
    for k, (lo, hi) in places.items():
        d = int(hi) - int(lo)
        mo[k], co[k] = m, c
        m, c = m + d, c + d * d
    return mo, co, m, c


def moments_kernel_taken(w, places):
    """The dispatch rule (module docstring) for group_moments."""
    if getattr(_backend.get(), 'name', None) != 'hip' or not (w.is_cuda and w.dtype == torch.float32) or w.dim() != 2:
        return False
    return _row_stride(w) is not None and 2 <= w.shape[0] <= MAX_ROWS and _groups_fit(places)


def moments_reference(w, places):
    """The two-pass float64 formula per group -> packed (mean [sum D_g], cov [sum D_g^2]) on w's device."""
    mo, co, tm, tc = _offsets(places)
    mean = torch.empty(tm, dtype=torch.float64, device=w.device)
    cov = torch.empty(tc, dtype=torch.float64, device=w.device)
    n = w.shape[0]
    for k, (lo, hi) in places.items():
        x = w[:, int(lo):int(hi)].double()
        m = x.mean(0)
        xc = x - m
        d = int(hi) - int(lo)
        mean[mo[k]:mo[k] + d] = m
        cov[co[k]:co[k] + d * d] = (xc.T @ xc / (n - 1)).reshape(-1)
    return mean, cov


def group_moments_packed(w, places):
    """(mean, cov): the two packed float64 buffers, group after group in the order of ``places``."""
    if not torch.is_tensor(w) or w.dim() != 2 or w.shape[0] < 2:
        raise ValueError('group_moments: [N, D] latents with N >= 2 expected, got %s' % (tuple(w.shape) if torch.is_tensor(w) else type(w).__name__,))
    _check_places(places, w.shape[1], 'group_moments')
    if not moments_kernel_taken(w, places):
        with torch.no_grad():
            return moments_reference(w.detach(), places)
    dev, n = w.device, w.shape[0]
    _, _, tm, tc = _offsets(places)
    _, lo, hi = _table(places)
    mean = torch.empty(tm, dtype=torch.float64, device=dev)
    cov = torch.empty(tc, dtype=torch.float64, device=dev)
    nbytes = getattr(_lib.load(), MOMENTS_WORKSPACE)(n, lo, hi, len(places))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    _backend.get()._launch(dev, MOMENTS_ENTRY, _lib.ptr(w), _row_stride(w), n, lo, hi, len(places), _lib.ptr(mean), _lib.ptr(cov), _lib.ptr(ws),
                           nbytes, _lib.stream_of(w))
    return mean, cov


def unpack(mean, cov, places):
    """Per-group views ({group: [D_g]}, {group: [D_g, D_g]}) of the packed buffers."""
    mo, co, _, _ = _offsets(places)
    means, covs = {}, {}
    for k, (lo, hi) in places.items():
        d = int(hi) - int(lo)
        means[k] = mean[mo[k]:mo[k] + d]
        covs[k] = cov[co[k]:co[k] + d * d].view(d, d)
    return means, covs


def group_moments(w, places):
    """({group: mean float64 [D_g]}, {group: cov float64 [D_g, D_g]}) of ``w`` [N, D] (module docstring)."""
    return unpack(*group_moments_packed(w, places), places)


def _rows_view(x):
    """``x`` as [R, D] rows with one row stride (a view), or None."""
    d = x.shape[-1]
    try:
        rows = x.view(-1, d)
    except RuntimeError:
        return None
    return rows if rows.shape[0] >= 1 and _row_stride(rows) is not None else None


def project_kernel_taken(x, mean, components, places):
    """The dispatch rule (module docstring) for group_project_."""
    if getattr(_backend.get(), 'name', None) != 'hip' or x.dim() < 2:
        return False
    tensors = [x, mean] + [components[k] for k in places]
    if not all(t.is_cuda and t.dtype == torch.float32 and t.device == x.device for t in tensors):
        return False
    if not (_groups_fit(places) and mean.is_contiguous() and all(components[k].is_contiguous() for k in places)):
        return False
    spans = sorted((int(lo), int(hi)) for lo, hi in places.values())
    if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        return False
    return _rows_view(x.data) is not None


def kernel_taken(*args):
    """``kernel_taken(w, places)`` -- group_moments -- or ``kernel_taken(x, mean, components, places)`` -- group_project_."""
    return moments_kernel_taken(*args) if len(args) == 2 else project_kernel_taken(*args)


def _check_project(x, mean, components, places):
    if not torch.is_tensor(x) or x.dim() < 2:
        raise ValueError('group_project_: a [..., D] latent with at least two axes expected')
    d = x.shape[-1]
    _check_places(places, d, 'group_project_')
    if tuple(mean.shape) != (d,):
        raise ValueError('group_project_: mean has shape %s, the latent rows are %d wide' % (tuple(mean.shape), d))
    for k, (lo, hi) in places.items():
        p = components[k]
        if p.dim() != 2 or p.shape[1] != int(hi) - int(lo) or not 1 <= p.shape[0] <= p.shape[1]:
            raise ValueError('group_project_: components of group %r have shape %s; [r, %d] with 1 <= r <= %d expected'
                             % (k, tuple(p.shape), int(hi) - int(lo), int(hi) - int(lo)))


def project_reference_(x, mean, components, places):
    """The float32 expression, in place: x[..., lo:hi] = m + ((x[..., lo:hi] - m) @ P^T) @ P per group."""
    with torch.no_grad():
        data = x.data
        for k, (lo, hi) in places.items():
            lo, hi = int(lo), int(hi)
            m, p = mean[lo:hi], components[k]
            data[..., lo:hi] = m + ((data[..., lo:hi] - m) @ p.T) @ p
    return x


def group_project_(x, mean, components, places):
    """In place (module docstring); returns ``x``."""
    _check_project(x, mean, components, places)
    if not project_kernel_taken(x, mean, components, places):
        return project_reference_(x, mean, components, places)
    rows = _rows_view(x.data)
    names, lo, hi = _table(places)
    ptrs = (ctypes.c_void_p * len(names))(*[components[k].data_ptr() for k in names])
    ranks = (ctypes.c_int32 * len(names))(*[components[k].shape[0] for k in names])
    _backend.get()._launch(x.device, PROJECT_ENTRY, rows.data_ptr(), _row_stride(rows), rows.shape[0], _lib.ptr(mean), ptrs, ranks, lo, hi, len(names),
                           _lib.stream_of(x))
    return x
