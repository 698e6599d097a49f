"""The same / not-same hinge loss of one feature level of the attribute stage (losses/loss_model.py), forward and backward.

``pair_hinge_loss(features [N, ...], n_same, n_not_same, mode, lower, upper, focus, weight, row_index, row_valid, scale)`` is

    weight * ( mean over the 'same' pairs of clamp(D - lower, min=0) + mean over the other pairs of clamp(upper - D, min=0) )

of the strictly-lower-triangular distances ``D[i, j]`` between the ``n = n_same + n_not_same`` rows in pair order ("same block, then the
rest": ``row_index``, a host sequence of distinct rows of ``features``; absent: the rows in order).  The trailing axes of a row flatten into
``K`` values:

* ``'abs'``: ``D[i, j] = mean_k |v_i v_j (F[i, k] - F[j, k])|`` -- the mean-absolute criteria, ``L1Expend`` and, with ``row_valid`` (one flag
  per row of ``features``; ``v = 1`` when absent), the hair criterion on its ``[N, 3]`` colours;
* ``'sq'``:  ``D[i, j] = sum_k (F[i, k] - F[j, k])^2`` -- squared L2 between embeddings;
* ``'msq'``: ``D[i, j] = mean_k (F[i, k] - F[j, k])^2 * scale`` -- the style criterion (``scale = 1e5``).

The pair sets are ``LossModelClass.pair_masks`` + ``_level_loss``: ``focus`` 'same_as_last_layer' takes the pairs (2i, 2i + 1) of the first
``n_same`` rows as 'same', 'not_same_as_last_layer' those of the following ``n_not_same`` rows; every other pair below the diagonal is pushed
apart.  The result is a 0-d tensor on the features' device, differentiable ONCE with respect to ``features`` (no double backward).

The dispatch rule.  The call is ONE ``gc_pair_hinge_fwd_f32`` call (csrc/pair_hinge.hip: one launch of one workgroup while ``n K <= 8192``,
every last-layer shape of the shipped configs; a tile launch split along K plus a fixed-order finish launch for longer rows) and, in the
backward pass, ONE ``gc_pair_hinge_bwd_f32`` call (one launch; it writes the gradient of ALL ``N`` rows, zeros where a row is not indexed,
and reads the upstream gradient from the device: no host sync) when ALL of these hold:

* the HIP backend is active and ``features`` (and ``row_valid``, if given) are CUDA tensors on one device, ``features`` float32;
* rows are adjacent-element rows: the trailing axes are laid out as in a contiguous tensor and rows are at least ``K`` elements apart --
  ``features[::2]``, a row-pitched buffer and a column slice ``vec[:, 227:254]`` (4-byte aligned rows) are read in place;
* ``n <= 64``, ``N <= 1024`` and ``K`` fits an int32;
* both pair sets are non-empty.  (An empty set makes torch's ``mean`` return NaN: that case keeps the torch path, and the NaN.)

No size threshold: profiles/attribute_losses.md has the fused and the torch time of every shape of the FFHQ loss set.  Everything else -- CPU
tensors, the emulated backend of the tests, other dtypes, rows that are not adjacent-element rows -- runs ``torch_pair_hinge``: the formula
as torch code under autograd, the SAME expression as ``LossModelClass._level_loss`` on the criterion's distances (bit for bit on the CPU).
"""
import ctypes

import torch          # every device allocation below goes through this name: tests swap it for a guard-banded allocator

from ... import _lib
from . import _backend
# part of this module's interface: the guard-banded allocator of the tests (guarded(module)) reaches the launch path as module.HipBackend._launch
from ._backend import HipBackend          # noqa: F401
from .pairwise import _rows

FWD_ENTRY = 'gc_pair_hinge_fwd_f32'
BWD_ENTRY = 'gc_pair_hinge_bwd_f32'
WORKSPACE = 'gc_pair_hinge_workspace'
MODES = {'abs': 0, 'sq': 1, 'msq': 2}          # GC_PAIR_HINGE_ABS / _SQ / _MSQ (include/gancontrol_hip.h)
FOCUS = {'same_as_last_layer': 0, 'not_same_as_last_layer': 1}          # GC_PAIR_HINGE_FOCUS_SAME / _NOT_SAME
MAX_ROWS = 64                        # GC_PAIR_HINGE_MAX_ROWS
MAX_BATCH_ROWS = 1024                # GC_PAIR_HINGE_MAX_BATCH_ROWS
ONE_LAUNCH_VALUES = 8192             # GC_PAIR_HINGE_ONE_LAUNCH_VALUES: n K up to here is one forward launch


def mode_distances(feats, mode, valid=None, scale=1.0):
    """[n, n] distances of a mode between the rows of ``feats`` and themselves, over every trailing axis (the expressions of CRITERIA)."""
    d = feats.unsqueeze(1) - feats.unsqueeze(0)
    axes = tuple(range(2, d.dim()))
    if mode == 'abs':
        if valid is not None:
            v = valid.reshape(-1)
            d = d * (v.unsqueeze(1) * v.unsqueeze(0)).reshape((v.shape[0], v.shape[0]) + (1,) * len(axes))
        return d.abs().mean(axes)
    if mode == 'sq':
        return d.pow(2).sum(axes)
    return d.pow(2).mean(axes) * scale


def _check(features, n_same, n_not_same, mode, focus, row_index):
    if mode not in MODES:
        raise ValueError('pair_hinge_loss: mode must be one of %s, got %r' % (sorted(MODES), mode))
    if focus not in FOCUS:
        raise ValueError('focus_on_list entry %r' % (focus,))
    n = n_same + n_not_same
    if features.dim() < 2 or n_same < 0 or n_not_same < 0:
        raise ValueError('pair_hinge_loss: [N, ...] features and non-negative counts expected, got %s, %d + %d' % (tuple(features.shape), n_same, n_not_same))
    if row_index is None:
        if features.shape[0] != n:
            raise ValueError('pair_hinge_loss: %d rows for n_same + n_not_same = %d (pass row_index to select rows)' % (features.shape[0], n))
        return None
    rows = [int(r) for r in row_index]
    if len(rows) != n or len(set(rows)) != n or any(r < 0 or r >= features.shape[0] for r in rows):
        raise ValueError('pair_hinge_loss: row_index must hold n_same + n_not_same = %d distinct rows of the %d, got %s' % (n, features.shape[0], rows))
    return rows


def torch_pair_hinge(features, n_same, n_not_same, mode, lower, upper, focus, weight=1.0, row_index=None, row_valid=None, scale=1.0):
    """The torch path: today's cat + criterion + _level_loss composition, with the rows picked by one index instead of slices and a cat."""
    rows = _check(features, n_same, n_not_same, mode, focus, row_index)
    feats = features if rows is None else features[rows]
    valid = None
    if row_valid is not None and mode == 'abs':
        valid = row_valid.reshape(-1) if rows is None else row_valid.reshape(-1)[rows]
    from ...losses.loss_model import LossModelClass
    dist = mode_distances(feats, mode, valid, scale)
    return weight * LossModelClass._level_loss(None, dist, LossModelClass.pair_masks(n_same, n_not_same, device=features.device), focus, lower, upper)


def set_sizes(n_same, n_not_same, focus):
    """(same pairs, other pairs) of a level."""
    same = n_same // 2 if focus == 'same_as_last_layer' else n_not_same // 2
    n = n_same + n_not_same
    return same, n * (n - 1) // 2 - same


def kernel_taken(features, n_same, n_not_same, focus, row_valid=None):
    """The dispatch rule (module docstring): whether this call is one gc_pair_hinge_fwd_f32 call (and one gc_pair_hinge_bwd_f32 call)."""
    if getattr(_backend.get(), 'name', None) != 'hip':
        return False
    if not (features.is_cuda and features.dtype == torch.float32):
        return False
    if row_valid is not None and not (row_valid.is_cuda and row_valid.device == features.device and row_valid.numel() == features.shape[0]):
        return False
    geom = _rows(features)
    n = n_same + n_not_same
    if geom is None or geom[0] >= 2 ** 31 or n > MAX_ROWS or features.shape[0] > MAX_BATCH_ROWS:
        return False
    return min(set_sizes(n_same, n_not_same, focus)) >= 1


def _index_arg(rows):
    return None if rows is None else (ctypes.c_int32 * len(rows))(*rows)


def pair_hinge_forward(features, n_same, n_not_same, mode, lower, upper, focus, weight=1.0, row_index=None, row_valid=None, scale=1.0):
    """The forward entry on its own -> (loss 0-d, D [n, n], C [n, n] = dloss / dD, the float32 row flags or None): what the autograd function
    saves, the tests read and the trainer's statistics can use.  The caller has checked ``kernel_taken``."""
    rows = _check(features, n_same, n_not_same, mode, focus, row_index)
    dev = features.device
    n, n_rows = n_same + n_not_same, features.shape[0]
    k, stride = _rows(features)
    valid = None
    if row_valid is not None and mode == 'abs':
        valid = row_valid.reshape(-1)
        if valid.dtype != torch.float32 or not valid.is_contiguous():
            valid = valid.to(torch.float32).contiguous()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    d = torch.empty((n, n), dtype=torch.float32, device=dev)
    c = torch.empty((n, n), dtype=torch.float32, device=dev)
    nbytes = getattr(_lib.load(), WORKSPACE)(n, k)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
    _backend.get()._launch(dev, 'gc_pair_hinge_fwd_f32', _lib.ptr(features), stride, n_rows, _index_arg(rows), _lib.ptr(valid), n_same, n_not_same, k,
                           MODES[mode], float(scale), FOCUS[focus], float(lower), float(upper), float(weight), _lib.ptr(loss), _lib.ptr(d), _lib.ptr(c),
                           _lib.ptr(ws), nbytes, _lib.stream_of(features))
    return loss, d, c, valid


def pair_hinge_backward(features, c, grad, n, mode, row_index=None, valid=None, scale=1.0):
    """The backward entry on its own -> dF [N, K] dense: ``grad`` (a 0-d or one-element float32 device tensor) times dloss / dF."""
    dev = features.device
    k, stride = _rows(features)
    df = torch.empty((features.shape[0], k), dtype=torch.float32, device=dev)
    _backend.get()._launch(dev, 'gc_pair_hinge_bwd_f32', _lib.ptr(features), stride, features.shape[0], _index_arg(row_index), _lib.ptr(valid), n, k,
                           MODES[mode], float(scale), _lib.ptr(c), _lib.ptr(grad), _lib.ptr(df), _lib.stream_of(features))
    return df


class PairHingeFunction(torch.autograd.Function):
    """The two entries as one differentiable operation (first derivative only)."""

    @staticmethod
    def forward(ctx, features, n_same, n_not_same, mode, lower, upper, focus, weight, rows, row_valid, scale):
        feats = features.detach()
        loss, _, c, valid = pair_hinge_forward(feats, n_same, n_not_same, mode, lower, upper, focus, weight, rows, row_valid, scale)
        ctx.save_for_backward(feats, c, valid)
        ctx.args = (n_same + n_not_same, mode, rows, scale)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        feats, c, valid = ctx.saved_tensors
        n, mode, rows, scale = ctx.args
        if grad.dtype != torch.float32 or not grad.is_contiguous():
            grad = grad.to(torch.float32).contiguous()
        df = pair_hinge_backward(feats, c, grad, n, mode, rows, valid, scale)
        return (df.view(feats.shape),) + (None,) * 10


def pair_hinge_loss(features, n_same, n_not_same, mode, lower, upper, focus, weight=1.0, row_index=None, row_valid=None, scale=1.0):
    """The hinge loss of one level (module docstring) -> a 0-d tensor on the features' device."""
    rows = _check(features, n_same, n_not_same, mode, focus, row_index)
    if not kernel_taken(features, n_same, n_not_same, focus, row_valid):
        return torch_pair_hinge(features, n_same, n_not_same, mode, lower, upper, focus, weight, rows, row_valid, scale)
    return PairHingeFunction.apply(features, n_same, n_not_same, mode, lower, upper, focus, weight, rows, row_valid, scale)
