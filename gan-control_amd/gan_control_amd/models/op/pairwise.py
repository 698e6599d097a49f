"""All-pairs feature distances for the separability evaluation (evaluation/separability.py, LossModelClass.calc_distances).

``pairwise_distances(signatures [m, ...], queries [n, ...], mode)`` returns ``D [m, n]`` (signatures x queries, the orientation of the
reference's ``all_distances``) with the trailing axes of a feature map flattened into one row of ``K`` values:

* ``'abs'``: ``D[i, j] = mean_k |S[i, k] - Q[j, k]|`` -- the reference's ``L1Expend`` (loss_model.py:308-321) and the mean-absolute criteria;
* ``'sq'``:  ``D[i, j] = sum_k (S[i, k] - Q[j, k])^2`` -- ``ArcFaceCriterion`` (arc_face_criterion.py:15-21), the difference itself.

With ``signature_pids`` and ``query_pids`` (host arrays of ids) it returns ``(D, best, best_idx)``: per query column the minimum over the
signatures with ANOTHER pid and the lowest row index that attains it -- ``distance_2nd_best`` and (through ``signature_pids``) ``signature``
of calc_same_not_same_list (loss_model.py:218-229).  A query whose every signature shares its pid has no such row; the reference's ``np.min``
raises on the empty row, and so does this: ``ValueError`` naming the query, read off the host pid arrays before anything is launched.
Inputs are assumed finite.

The dispatch rule.  The call is ONE ``gc_pairwise_f32`` call (csrc/pairwise.hip: a tile launch and, where rows are split along K or pids are
given, a second launch that adds the partial sums and takes the minima) when ALL of these hold:

* the HIP backend is active and both tensors are CUDA float32 tensors on the same device;
* rows are adjacent-element rows: the trailing axes are laid out as in a contiguous tensor (they flatten for free) and rows are at least
  ``K`` elements apart -- ``features[::2]`` (row stride 2 K) and a row-pitched [m, K + 1] buffer are read in place;
* no gradient is wanted (grad mode off, or neither tensor requires one);
* no ``criterion=`` callable is given, ``K`` fits an int32 and neither side has more than 65535 * 64 rows.

No size threshold: the kernel path is not slower than the chunked path at any shape measured, the 50 x 50 debug size included
(profiles/separability.md, rows 'debug').  Everything else -- CPU tensors, the emulated backend of the tests, other dtypes, a wanted
gradient, a custom criterion -- runs ``chunked_distances``: the reference's formula, in chunks of 20 signatures x 20 queries
(loss_model.py:252-285), as torch code; a criterion whose chunk result is not ``[chunk m, chunk n]`` raises ``ValueError`` (the reference's
``intermediate_criterion_as_last_layer`` with the squared-L2 criterion on 4-D maps does that).  It is the documented formula and the
baseline of tools/separability_bench.py.  A CUDA tensor never takes a detour over the host on either path.
"""
import numpy as np
import torch          # every device allocation below goes through this name: tests swap it for a guard-banded allocator

from ... import _lib
from . import _backend
# part of this module's interface: the guard-banded allocator of the tests (guarded(module)) reaches the launch path as module.HipBackend._launch
from ._backend import HipBackend          # noqa: F401

ENTRY = 'gc_pairwise_f32'
WORKSPACE = 'gc_pairwise_workspace'
MODES = {'abs': 0, 'sq': 1}          # GC_PAIRWISE_ABS / GC_PAIRWISE_SQ (include/gancontrol_hip.h)
CHUNK = 20                           # the reference's batch_size
MAX_ROWS = 65535 * 64                # the kernel's limit on either side (include/gancontrol_hip.h)


def _mode_fn(mode):
    """The chunk formula of a mode: [a, ...] x [b, ...] -> [a, b] over every trailing axis."""
    def dist(signatures, queries):
        d = signatures.unsqueeze(1) - queries.unsqueeze(0)
        axes = tuple(range(2, d.dim()))
        return d.abs().mean(axes) if mode == 'abs' else d.pow(2).sum(axes)
    return dist


def chunked_distances(signatures, queries, distance_fn, batch_size=CHUNK):
    """The reference's calc_distances (loss_model.py:252-285) on the tensors' own device: ``torch.chunk`` both sides into
    ceil(rows / batch_size) pieces, ``distance_fn(signature chunk, query chunk)`` for every pair, rows concatenated over the signature
    chunks and columns over the query chunks."""
    if signatures.shape[0] < 1 or queries.shape[0] < 1:
        raise ValueError('pairwise distances of %d signatures and %d queries' % (signatures.shape[0], queries.shape[0]))
    s_chunks = torch.chunk(signatures, -(-signatures.shape[0] // batch_size), dim=0)
    q_chunks = torch.chunk(queries, -(-queries.shape[0] // batch_size), dim=0)
    columns = []
    for qc in q_chunks:
        rows = []
        for sc in s_chunks:
            d = distance_fn(sc, qc)
            if not torch.is_tensor(d) or tuple(d.shape) != (sc.shape[0], qc.shape[0]):
                raise ValueError('pairwise distances: the criterion maps %s x %s to %s, not to a [%d, %d] matrix'
                                 % (tuple(sc.shape), tuple(qc.shape), tuple(d.shape) if torch.is_tensor(d) else type(d).__name__, sc.shape[0], qc.shape[0]))
            rows.append(d)
        columns.append(torch.cat(rows, dim=0))
    return torch.cat(columns, dim=1)


def _rows(t):
    """(K, row stride in elements) of a tensor whose rows are adjacent-element rows, else None."""
    k, want = 1, []
    for size in reversed(t.shape[1:]):
        want.append(k)
        k *= size
    want.reverse()
    if k < 1 or any(size > 1 and st != w for size, st, w in zip(t.shape[1:], t.stride()[1:], want)):
        return None
    stride = t.stride(0) if t.shape[0] > 1 else k          # (a single row may report any stride, and none is used)
    return (k, stride) if stride >= k else None


def kernel_taken(signatures, queries, criterion=None):
    """The dispatch rule (module docstring): whether this call is one gc_pairwise_f32 call."""
    if criterion is not None or getattr(_backend.get(), 'name', None) != 'hip':
        return False
    for t in (signatures, queries):
        if not (t.is_cuda and t.dtype == torch.float32 and t.device == signatures.device):
            return False
    if torch.is_grad_enabled() and (signatures.requires_grad or queries.requires_grad):
        return False
    rs, rq = _rows(signatures), _rows(queries)
    return rs is not None and rq is not None and rs[0] == rq[0] and rs[0] < 2 ** 31 and max(signatures.shape[0], queries.shape[0]) <= MAX_ROWS


def pid_codes(signature_pids, query_pids, m, n):
    """(signature codes, query codes): the two host id arrays as int32 codes of their joint set of values (equal ids, equal codes).  Raises
    ValueError for a query whose every signature shares its pid."""
    s = np.asarray(signature_pids.cpu() if torch.is_tensor(signature_pids) else signature_pids).reshape(-1)
    q = np.asarray(query_pids.cpu() if torch.is_tensor(query_pids) else query_pids).reshape(-1)
    if s.shape[0] != m or q.shape[0] != n:
        raise ValueError('pairwise distances: %d signature pids for %d signatures, %d query pids for %d queries' % (s.shape[0], m, q.shape[0], n))
    _, codes = np.unique(np.concatenate([s, q]), return_inverse=True)
    codes = codes.reshape(-1).astype(np.int32)
    sc, qc = codes[:m], codes[m:]
    if sc.min() == sc.max():          # one pid on the signature side: the queries that carry it have no not-same row
        bad = np.nonzero(qc == sc[0])[0]
        if bad.size:
            raise ValueError('pairwise distances: query %d (pid %s) has no signature with another pid (%d signatures, all of that pid)'
                             % (int(bad[0]), q[int(bad[0])], m))
    return sc, qc


def masked_minima(d, s_codes, q_codes):
    """(best [n], best_idx [n] int64) of a distance matrix as the kernel defines them: the minimum of a column over the rows with another pid
    and the LOWEST row that attains it (np.argmin's first occurrence within the masked row, mapped back to the row index)."""
    m = d.shape[0]
    sp = torch.as_tensor(s_codes, device=d.device)
    qp = torch.as_tensor(q_codes, device=d.device)
    masked = torch.where(sp[:, None] != qp[None, :], d, torch.full_like(d, float('inf')))
    best = masked.min(dim=0).values
    rows = torch.arange(m, device=d.device)[:, None].expand_as(masked)
    best_idx = torch.where(masked == best[None, :], rows, torch.full_like(rows, m)).min(dim=0).values
    return best, best_idx


def pairwise_distances(signatures, queries, mode, signature_pids=None, query_pids=None, criterion=None, batch_size=CHUNK):
    """``D [m, n]``, or ``(D, best, best_idx)`` when both pid arrays are given (module docstring).  ``mode``: 'abs' | 'sq' (ignored with
    ``criterion=``, a callable ``(signature chunk, query chunk) -> [a, b]`` that forces the chunked path)."""
    if criterion is None and mode not in MODES:
        raise ValueError('pairwise_distances: mode must be one of %s, got %r' % (sorted(MODES), mode))
    if (signature_pids is None) != (query_pids is None):
        raise ValueError('pairwise_distances: signature_pids and query_pids go together')
    if signatures.dim() < 2 or queries.dim() < 2 or signatures.shape[1:] != queries.shape[1:] or signatures.shape[0] < 1 or queries.shape[0] < 1:
        raise ValueError('pairwise_distances: [m, ...] and [n, ...] features of one row shape expected, got %s and %s' % (tuple(signatures.shape), tuple(queries.shape)))
    m, n = signatures.shape[0], queries.shape[0]
    codes = pid_codes(signature_pids, query_pids, m, n) if signature_pids is not None else None
    if not kernel_taken(signatures, queries, criterion):
        d = chunked_distances(signatures, queries, criterion if criterion is not None else _mode_fn(mode), batch_size)
        return d if codes is None else (d,) + masked_minima(d, *codes)
    dev = signatures.device
    (k, s_stride), (_, q_stride) = _rows(signatures), _rows(queries)
    d = torch.empty((m, n), dtype=torch.float32, device=dev)
    nbytes = getattr(_lib.load(), WORKSPACE)(m, n, k)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
    sp = qp = best = best_idx = None
    if codes is not None:
        sp = torch.from_numpy(codes[0]).to(dev)
        qp = torch.from_numpy(codes[1]).to(dev)
        best = torch.empty(n, dtype=torch.float32, device=dev)
        best_idx = torch.empty(n, dtype=torch.int32, device=dev)
    _backend.get()._launch(dev, ENTRY, _lib.ptr(signatures), s_stride, _lib.ptr(queries), q_stride, m, n, k, MODES[mode], _lib.ptr(d),
                           _lib.ptr(sp), _lib.ptr(qp), _lib.ptr(best), _lib.ptr(best_idx), _lib.ptr(ws), nbytes, _lib.stream_of(d))
    return d if codes is None else (d, best, best_idx.long())
