"""The distance passes of the sample-quality metrics (fid_utils/precision_recall.py, fid_utils/kid.py) on [n, F] feature rows.

* ``knn_radii(features, kth=3)`` -> float32 ``[n]``: the squared distance of every row to its ``kth`` nearest OTHER row, i.e. the
  ``(kth + 1)``-th smallest value of its row of ``D(features, features)``, the own 0 included (``kthvalue(kth + 1)``).
* ``manifold_hits(ref, ref_r2, probe, probe_r2=None)`` -> ``(probe_hit [n] bool, ref_hit [m] bool | None)`` in one pass over
  ``D(ref, probe)``: ``probe_hit[j] = any_i D[i, j] <= ref_r2[i]`` and, with ``probe_r2``, ``ref_hit[i] = any_j D[i, j] <= probe_r2[j]``.
  ``<=``: a tie is a hit.
* ``poly_mmd_sums(x, y, idx_x, idx_y)`` -> float64 ``[subsets, 3]``: with ``X = x[idx_x[s]]``, ``Y = y[idx_y[s]]`` (``idx_*``: host or
  device integer arrays ``[subsets, m]``) and ``kappa(u, v) = (u . v / F + 1)^3`` the sums ``sum_{i != j} kappa(X_i, X_j)``,
  ``sum_{i != j} kappa(Y_i, Y_j)`` and ``sum_{i, j} kappa(X_i, Y_j)``.  The dot product is float32, everything behind it float64.

``D[i, j] = sum_c (a[i, c] - b[j, c])^2`` in float32, the difference itself (never ``|a|^2 + |b|^2 - 2 a . b``).  Inputs are assumed finite.
``n < kth + 1``, ``kth < 1``, sets of different width, empty sets and subset indices outside the sets raise ``ValueError`` before anything
is launched (the indices are checked on the host).

The dispatch rule.  A call is ONE ``gc_knn_radius_f32`` / ``gc_manifold_hits_f32`` / ``gc_poly_mmd_f32`` call (csrc/manifold.hip: a tile
launch whose epilogue keeps the k smallest values / the hit flags / the float64 sums of a strip of tiles, and a finish launch that merges the
strips; no ``m x n`` value is ever stored) when ALL of these hold:

* the HIP backend is active and every feature tensor (and radius) is a CUDA float32 tensor on one device;
* rows are adjacent-element rows at least ``F`` elements apart -- ``features[::2]`` (row stride 2 F) and a row-pitched [n, F + 1] buffer
  are read in place;
* no gradient is wanted (grad mode off, or no tensor requires one);
* ``kth <= 7``, no set has more than 65535 * 64 rows and there are at most 21845 subsets.

No size threshold: the kernel path is not slower than the torch path at any shape measured (profiles/quality_metrics.md).  Everything else
-- CPU tensors, the emulated backend of the tests, other dtypes, a wanted gradient, ``kth`` or row counts beyond the limits -- runs the torch
code below, which is the documented formula: difference-form distances in chunks of at most ``CHUNK_ELEMS`` differences (never an
``n x n`` allocation), a running ``topk`` merged across the column chunks, and float64 kernel sums subset by subset.  A CUDA tensor never
takes a detour over the host on either path.
"""
import numpy as np
import torch          # every device allocation below goes through this name: tests swap it for a guard-banded allocator

from ... import _lib
from . import _backend
# part of this module's interface: the guard-banded allocator of the tests (guarded(module)) reaches the launch path as module.HipBackend._launch
from ._backend import HipBackend          # noqa: F401
from .pairwise import _rows

KNN_ENTRY, KNN_WORKSPACE = 'gc_knn_radius_f32', 'gc_knn_radius_workspace'
HITS_ENTRY, HITS_WORKSPACE = 'gc_manifold_hits_f32', 'gc_manifold_hits_workspace'
MMD_ENTRY, MMD_WORKSPACE = 'gc_poly_mmd_f32', 'gc_poly_mmd_workspace'
MAX_KTH = 7                          # GC_KNN_MAX_KTH (include/gancontrol_hip.h)
MAX_ROWS = 65535 * 64                # the kernels' limit on either side
MAX_SUBSETS = 65535 // 3
CHUNK_ELEMS = 1 << 24                # differences held at once by the torch path (64 MiB of float32)


def kernel_taken(*tensors):
    """The dispatch rule (module docstring) for the feature / radius tensors of one call."""
    if not all(t.is_cuda for t in tensors) or getattr(_backend.get(), 'name', None) != 'hip':
        return False
    width = None
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.float32 and t.device == tensors[0].device):
            return False
        if torch.is_grad_enabled() and t.requires_grad:
            return False
        if t.shape[0] > MAX_ROWS:
            return False
        if t.dim() == 2:
            r = _rows(t)
            if r is None or r[0] >= 2 ** 31 or (width is not None and r[0] != width):
                return False
            width = r[0]
    return True


def _check_sets(name, *sets):
    for t in sets:
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.shape[1] != sets[0].shape[1]:
            raise ValueError('%s: [n, F] feature sets of one width expected, got %s' % (name, ', '.join(str(tuple(s.shape)) for s in sets)))


def _steps(m, n, f):
    """(rows, columns) of a chunk: at most CHUNK_ELEMS differences, columns first."""
    cols = max(1, min(n, CHUNK_ELEMS // f, 1024))
    return max(1, min(m, CHUNK_ELEMS // (f * cols))), cols


def _sq_chunk(a, b):
    d = a.unsqueeze(1) - b.unsqueeze(0)
    return (d * d).sum(-1)


def knn_radii_torch(features, kth=3):
    """The formula of ``knn_radii`` as torch code on the tensor's own device."""
    n, f = features.shape
    rows, cols = _steps(n, n, f)
    out = []
    for i in range(0, n, rows):
        a = features[i:i + rows]
        best = None
        for j in range(0, n, cols):
            d = _sq_chunk(a, features[j:j + cols])
            d = d if best is None else torch.cat([best, d], 1)
            best = d.topk(min(kth + 1, d.shape[1]), dim=1, largest=False).values
        out.append(best[:, kth])
    return torch.cat(out)


def manifold_hits_torch(ref, ref_r2, probe, probe_r2=None):
    """The formula of ``manifold_hits`` as torch code on the tensors' own device."""
    m, f = ref.shape
    n = probe.shape[0]
    rows, cols = _steps(m, n, f)
    probe_hit = torch.zeros(n, dtype=torch.bool, device=ref.device)
    ref_hit = torch.zeros(m, dtype=torch.bool, device=ref.device) if probe_r2 is not None else None
    for i in range(0, m, rows):
        for j in range(0, n, cols):
            d = _sq_chunk(ref[i:i + rows], probe[j:j + cols])
            probe_hit[j:j + cols] |= (d <= ref_r2[i:i + rows, None]).any(0)
            if ref_hit is not None:
                ref_hit[i:i + rows] |= (d <= probe_r2[None, j:j + cols]).any(1)
    return probe_hit, ref_hit


def poly_mmd_sums_torch(x, y, idx_x, idx_y):
    """The formula of ``poly_mmd_sums`` as torch code: float32 dot products, float64 behind them.  idx_*: int64 tensors on x's device."""
    f = x.shape[1]
    out = torch.zeros((idx_x.shape[0], 3), dtype=torch.float64, device=x.device)
    for s in range(idx_x.shape[0]):
        xs, ys = x[idx_x[s]], y[idx_y[s]]
        for w, (a, b) in enumerate(((xs, xs), (ys, ys), (xs, ys))):
            t = (a @ b.t()).double() / f + 1.0
            t = t * t * t
            if w < 2:
                t.diagonal().zero_()
            out[s, w] = t.sum()
    return out


def knn_radii(features, kth=3):
    _check_sets('knn_radii', features)
    kth = int(kth)
    n, f = features.shape
    if kth < 1 or n < kth + 1:
        raise ValueError('knn_radii: %d rows have no neighbour number %d (kth >= 1 and n >= kth + 1)' % (n, kth))
    if kth > MAX_KTH or not kernel_taken(features):
        return knn_radii_torch(features, kth)
    dev = features.device
    stride = _rows(features)[1]
    radius2 = torch.empty(n, dtype=torch.float32, device=dev)
    nbytes = getattr(_lib.load(), KNN_WORKSPACE)(n, f, kth)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _backend.get()._launch(dev, KNN_ENTRY, _lib.ptr(features), stride, n, f, kth, _lib.ptr(radius2), _lib.ptr(ws), nbytes, _lib.stream_of(features))
    return radius2


def manifold_hits(ref, ref_r2, probe, probe_r2=None):
    _check_sets('manifold_hits', ref, probe)
    m, f = ref.shape
    n = probe.shape[0]
    if tuple(ref_r2.shape) != (m,) or (probe_r2 is not None and tuple(probe_r2.shape) != (n,)):
        raise ValueError('manifold_hits: one radius per row expected, got %s for %d ref rows and %s for %d probe rows'
                         % (tuple(ref_r2.shape), m, None if probe_r2 is None else tuple(probe_r2.shape), n))
    given = (ref, ref_r2, probe) + (() if probe_r2 is None else (probe_r2,))
    if not kernel_taken(*given):
        return manifold_hits_torch(ref, ref_r2, probe, probe_r2)
    dev = ref.device
    ref_r2 = ref_r2.contiguous()
    probe_r2 = None if probe_r2 is None else probe_r2.contiguous()
    probe_hit = torch.empty(n, dtype=torch.uint8, device=dev)
    ref_hit = torch.empty(m, dtype=torch.uint8, device=dev) if probe_r2 is not None else None
    nbytes = getattr(_lib.load(), HITS_WORKSPACE)(m, n, f)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _backend.get()._launch(dev, HITS_ENTRY, _lib.ptr(ref), _rows(ref)[1], _lib.ptr(ref_r2), m, _lib.ptr(probe), _rows(probe)[1], _lib.ptr(probe_r2), n, f,
                           _lib.ptr(probe_hit), _lib.ptr(ref_hit), _lib.ptr(ws), nbytes, _lib.stream_of(ref))
    return probe_hit.bool(), None if ref_hit is None else ref_hit.bool()


def _host_indices(name, idx, rows):
    a = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1 or a.dtype.kind not in 'iu':
        raise ValueError('poly_mmd_sums: %s must be an integer array [subsets, m], got %s %s' % (name, a.dtype, a.shape))
    if a.min() < 0 or a.max() >= rows:
        raise ValueError('poly_mmd_sums: %s has values outside [0, %d)' % (name, rows))
    return a


def poly_mmd_sums(x, y, idx_x, idx_y):
    _check_sets('poly_mmd_sums', x, y)
    ix, iy = _host_indices('idx_x', idx_x, x.shape[0]), _host_indices('idx_y', idx_y, y.shape[0])
    if ix.shape != iy.shape:
        raise ValueError('poly_mmd_sums: idx_x %s and idx_y %s differ in shape' % (ix.shape, iy.shape))
    subsets, m = ix.shape
    dev = x.device
    if subsets > MAX_SUBSETS or not kernel_taken(x, y):
        return poly_mmd_sums_torch(x, y, torch.from_numpy(ix.astype(np.int64)).to(dev), torch.from_numpy(iy.astype(np.int64)).to(dev))
    f = x.shape[1]
    dx = torch.from_numpy(np.ascontiguousarray(ix, dtype=np.int32)).to(dev)
    dy = torch.from_numpy(np.ascontiguousarray(iy, dtype=np.int32)).to(dev)
    sums = torch.empty((subsets, 3), dtype=torch.float64, device=dev)
    nbytes = getattr(_lib.load(), MMD_WORKSPACE)(subsets, m, f)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _backend.get()._launch(dev, MMD_ENTRY, _lib.ptr(x), _rows(x)[1], x.shape[0], _lib.ptr(y), _rows(y)[1], y.shape[0], f, _lib.ptr(dx), _lib.ptr(dy),
                           subsets, m, _lib.ptr(sums), _lib.ptr(ws), nbytes, _lib.stream_of(x))
    return sums
