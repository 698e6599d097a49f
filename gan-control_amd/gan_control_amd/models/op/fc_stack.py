"""Whole EqualLinear stacks in one launch: the w-space part of the inference API (inference/).

``fc_stacks_forward`` evaluates several independent stacks of ``EqualLinear(activation='fused_lrelu')`` layers -- the per-group mapping
networks of ``Generator.style`` (``create_fc_stack``: PixelNorm + n_mlp layers) or the controllers' ``FcStack`` -- each on its own column
slice of an input row and into its own column slice of an output row.

On CUDA float32 tensors under the HIP backend, with no gradient wanted, the call is ONE ``gc_fc_stacks_fwd_f32`` launch per 8 stacks
(csrc/fc_stack.hip): the slices are pointer offsets and row strides, so the ``torch.cat`` of MultiFcStack and the slice-assign of a controller
splice do not exist.  Every other call -- CPU tensors, the emulated backend of the tests, anything autograd must see, a tensor whose rows
share memory (an expanded control, row stride 0) or whose columns are not adjacent, a shape outside the kernel's limits or outside the measured
dispatch rule below -- calls the modules exactly as ``Generator.style`` / ``FcStack.forward`` do and copies
their results into the output slices: the documented formula and the oracle of the tests.  Nothing else in the package calls this module:
``Generator.forward``, ``Generator.style``, ``FcStack.forward`` and the trainers launch what they always launched.
"""
import ctypes

import torch          # every device allocation below goes through this name: tests swap it for a guard-banded allocator
from torch import nn

from ... import _lib
from . import _backend
# not used below, but part of this module's interface: the guard-banded allocator of the tests (guarded(module)) reaches the launch path of
# a launching module as module.HipBackend._launch, as it does for _backend itself and projection/noise_ops.py
from ._backend import HipBackend          # noqa: F401

ENTRY = 'gc_fc_stacks_fwd_f32'
MAX_LAYERS, MAX_WIDTH = 8, 512          # the kernel's limits (include/gancontrol_hip.h)

# The dispatch rule, from the table in profiles/inference.md (wall time per call, kernel against the module path; the kernel is not slower in
# any row measured).  One workgroup owns (stack, 8 rows) and streams ALL the weights of its stack, so the kernel's time grows with the bytes
# of the largest stack and with the number of 8-row tiles, where the module path's is a constant number of launches: the limits are the
# largest batch MEASURED for each class of stack, and anything beyond them takes the module path until somebody measures it.
# rows 'split x7, B = 1 .. 4000' and 'controllers x4' (at most 1.7 MB of weights per stack; B = 4000: 1405 us against 2593 us):
KERNEL_MAX_BATCH = 4000
# rows 'vanilla 512 x 8, B = 1 .. 1000' (8.4 MB per stack, 1.14 - 1.40 x; B = 1000 is a round of calc_mean_w_latents): a stack above
# KERNEL_WIDE_STACK_BYTES is in that class
KERNEL_WIDE_STACK_BYTES = 2 << 20
KERNEL_WIDE_MAX_BATCH = 1000


class _Plan:
    """What one list of stacks contributes to the argument tables: the layers with the parameters and pointers they had when the plan was made
    (compared with what the layers hold NOW on every call: a module that moved to another device, or whose Parameter objects or their
    storage were replaced, gets a new plan) and the per-layer host arrays."""
    __slots__ = ('stacks', 'layers', 'params', 'ptrs', 'pixel_norm', 'in_dim', 'out_dim', 'n_layers', 'w', 'bias', 'layer_out', 'alpha', 'beta',
                 'c_in_dim', 'c_n_layers', 'c_pixel_norm', 'supported', 'max_bytes', 'device')


_plans = {}


def _split(stack):
    """(leading PixelNorm?, [EqualLinear]) of an nn.Sequential built by create_fc_stack, of an FcStack or of a bare list of layers."""
    from ..gan_model import EqualLinear, PixelNorm
    mods = list(stack.fc_stack) if hasattr(stack, 'fc_stack') else list(stack)
    norm = bool(mods) and isinstance(mods[0], PixelNorm)
    layers = mods[1:] if norm else mods
    if not layers or not all(isinstance(m, EqualLinear) for m in layers):
        raise TypeError('fc_stacks_forward: a stack is [PixelNorm,] EqualLinear, ...; got %s' % [type(m).__name__ for m in mods])
    return norm, layers


def _params(layers):
    return [t for m in layers for t in ((m.weight, m.bias) if m.bias is not None else (m.weight,))]


def _current(plan):
    """The layers of the plan still hold the Parameter objects, at the addresses, that its tables were made from."""
    now = _params(plan.layers)
    return len(now) == len(plan.params) and all(t is u and t.data_ptr() == q for t, u, q in zip(now, plan.params, plan.ptrs))


def _plan_of(stacks, pixel_norm):
    key = tuple(id(s) for s in stacks) + (None if pixel_norm is None else tuple(bool(p) for p in pixel_norm),)
    p = _plans.get(key)
    if p is not None and all(a is b for a, b in zip(p.stacks, stacks)) and _current(p):
        return p
    if len(_plans) > 64:
        _plans.clear()
    p = _plans[key] = _Plan()
    p.stacks = list(stacks)          # (keeps the modules alive: an id is never reused while its plan exists)
    split = [_split(s) for s in stacks]
    p.pixel_norm = [n for n, _ in split] if pixel_norm is None else [bool(v) for v in pixel_norm]
    layers = [ls for _, ls in split]
    flat = [m for ls in layers for m in ls]
    p.layers = flat
    p.params = _params(flat)
    p.ptrs = [t.data_ptr() for t in p.params]
    p.in_dim = [ls[0].weight.shape[1] for ls in layers]
    p.out_dim = [ls[-1].weight.shape[0] for ls in layers]
    p.n_layers = [len(ls) for ls in layers]
    p.device = flat[0].weight.device
    p.supported = (all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == p.device for t in p.params)
                   and all(m.activation and m.bias is not None for m in flat)
                   and all(len(ls) <= MAX_LAYERS for ls in layers)
                   and all(1 <= d <= MAX_WIDTH for m in flat for d in m.weight.shape)
                   and all(a.weight.shape[0] == b.weight.shape[1] for ls in layers for a, b in zip(ls[:-1], ls[1:])))
    p.max_bytes = max(sum(m.weight.numel() * 4 for m in ls) for ls in layers)
    n = len(flat)
    p.w = (ctypes.c_void_p * n)(*[m.weight.data_ptr() for m in flat])
    p.bias = (ctypes.c_void_p * n)(*[m.bias.data_ptr() if m.bias is not None else None for m in flat])
    p.layer_out = (ctypes.c_int32 * n)(*[m.weight.shape[0] for m in flat])
    p.alpha = (ctypes.c_float * n)(*[m.scale for m in flat])
    p.beta = (ctypes.c_float * n)(*[m.lr_mul for m in flat])
    s = len(stacks)
    p.c_in_dim = (ctypes.c_int32 * s)(*p.in_dim)
    p.c_n_layers = (ctypes.c_int32 * s)(*p.n_layers)
    p.c_pixel_norm = (ctypes.c_int32 * s)(*[int(v) for v in p.pixel_norm])
    return p


def _per_stack(t, n):
    return list(t) if isinstance(t, (list, tuple)) else [t] * n


def _row_stride(t, width):
    """The distance between rows in elements: the tensor's own (kernel_taken has seen that rows do not overlap); a one-row tensor may
    report any, and none is used."""
    return t.stride(0) if t.shape[0] > 1 else max(width, 1)


def _rows_apart(t):
    """Rows of a [B, width] tensor with unit column stride lie behind each other without sharing memory (an expanded [1, width] tensor,
    row stride 0, does not: the kernel would need a stride shorter than its rows, which it refuses, and an output's rows would collide)."""
    return t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])


def _overlap(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def kernel_taken(plan, xs, outs, batch):
    """The dispatch rule (module docstring): whether this call is one kernel launch per 8 stacks."""
    if not plan.supported or getattr(_backend.get(), 'name', None) != 'hip':
        return False
    if batch < 1 or batch > (KERNEL_MAX_BATCH if plan.max_bytes <= KERNEL_WIDE_STACK_BYTES else min(KERNEL_MAX_BATCH, KERNEL_WIDE_MAX_BATCH)):
        return False
    tensors = xs + outs
    if not all(t.is_cuda and t.dtype == torch.float32 and t.device == plan.device and _rows_apart(t) for t in tensors):
        return False
    if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(t.requires_grad for t in plan.params)):
        return False
    return not any(_overlap(x, o) for x in {id(t): t for t in xs}.values() for o in {id(t): t for t in outs}.values())


def fc_stacks_forward(stacks, x, x_slices, out, out_slices, pixel_norm=None):
    """Stack i maps ``x_i[:, lo:hi]`` ([B, in_dim_i]) to ``out_i[:, lo:hi]`` ([B, out_dim_i]), written in place; returns ``out``.

    stacks: the modules -- ``nn.Sequential(PixelNorm(), EqualLinear, ...)`` as ``Generator.create_fc_stack`` builds them, or ``FcStack``.
    x / out: one 2-D tensor shared by every stack, or a list with one tensor per stack (the controllers: every one has its own controls and
    all of them write into the same w).  x_slices / out_slices: one ``(lo, hi)`` per stack, or None for whole rows.
    pixel_norm: None -- a stack is normalised iff its first module is a PixelNorm -- or one flag per stack (the normalisation is
    x * rsqrt(mean(x^2) + 1e-8) over the stack's own slice, as MultiFcStack applies it).
    An output slice that another stack of the same call reads is not supported (the kernel's workgroups are independent of each other)."""
    stacks = list(stacks)
    n = len(stacks)
    if n == 0:
        return out
    xs, outs = _per_stack(x, n), _per_stack(out, n)
    x_slices = [None] * n if x_slices is None else list(x_slices)
    out_slices = [None] * n if out_slices is None else list(out_slices)
    if not (len(xs) == len(outs) == len(x_slices) == len(out_slices) == n):
        raise ValueError('fc_stacks_forward: %d stacks, but %d inputs, %d input slices, %d outputs, %d output slices' % (n, len(xs), len(x_slices), len(outs), len(out_slices)))
    plan = _plan_of(stacks, pixel_norm)
    batch = xs[0].shape[0]
    x_lo, o_lo = [], []
    for i in range(n):
        xl, xh = x_slices[i] if x_slices[i] is not None else (0, xs[i].shape[1])
        ol, oh = out_slices[i] if out_slices[i] is not None else (0, outs[i].shape[1])
        if xs[i].dim() != 2 or outs[i].dim() != 2 or xs[i].shape[0] != batch or outs[i].shape[0] != batch:
            raise ValueError('fc_stacks_forward: stack %d: [%d, width] tensors expected, got %s and %s' % (i, batch, tuple(xs[i].shape), tuple(outs[i].shape)))
        if not (0 <= xl and xh <= xs[i].shape[1] and xh - xl == plan.in_dim[i]) or not (0 <= ol and oh <= outs[i].shape[1] and oh - ol == plan.out_dim[i]):
            raise ValueError('fc_stacks_forward: stack %d maps %d -> %d columns; slices %s of %d and %s of %d do not fit'
                             % (i, plan.in_dim[i], plan.out_dim[i], (xl, xh), xs[i].shape[1], (ol, oh), outs[i].shape[1]))
        x_lo.append(xl)
        o_lo.append(ol)
    if not kernel_taken(plan, xs, outs, batch):
        return _module_path(stacks, plan, xs, x_lo, outs, o_lo, pixel_norm, out)
    xp = (ctypes.c_void_p * n)(*[t.data_ptr() + 4 * lo for t, lo in zip(xs, x_lo)])
    yp = (ctypes.c_void_p * n)(*[t.data_ptr() + 4 * lo for t, lo in zip(outs, o_lo)])
    xst = (ctypes.c_int64 * n)(*[_row_stride(t, w) for t, w in zip(xs, plan.in_dim)])
    yst = (ctypes.c_int64 * n)(*[_row_stride(t, w) for t, w in zip(outs, plan.out_dim)])
    _backend.get()._launch(plan.device, ENTRY, xp, xst, yp, yst, plan.c_in_dim, plan.c_n_layers, plan.c_pixel_norm,
                           plan.w, plan.bias, plan.layer_out, plan.alpha, plan.beta, n, batch, _lib.stream_of(outs[0]))
    return out


def _module_path(stacks, plan, xs, x_lo, outs, o_lo, pixel_norm, out):
    from ..gan_model import PixelNorm
    for i, stack in enumerate(stacks):
        h = xs[i][:, x_lo[i]:x_lo[i] + plan.in_dim[i]]
        if pixel_norm is None:
            y = stack(h)                                   # exactly what MultiFcStack.forward / FcStack.forward call
        else:
            norm, layers = _split(stack)
            y = nn.Sequential(*layers)(PixelNorm()(h) if plan.pixel_norm[i] else h)
        outs[i][:, o_lo[i]:o_lo[i] + plan.out_dim[i]] = y
    return out
