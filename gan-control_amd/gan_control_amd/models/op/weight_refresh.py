"""One pass per parameter between an optimiser step and the next forward pass (csrc/weight_refresh.hip, gc_weight_refresh_grouped_f32).

``weight_cache`` refills the derived forms of a network level by level -- parameter -> ``w_t``, ``w_t`` -> ``adj(w_t)``, a pack of either,
``wsq`` of the parameter: three grouped re-layouts, three packs and one wsq launch per refresh, each reading what the previous one wrote -- and
``trainers/utils.accumulate`` reads the generator's parameters once more in two foreach passes.  The entry bound here reads every parameter once
and writes the EMA copy and every form from that one read; the values are the bits of the single-purpose kernels.

This module is the runner behind ``weight_cache.refresh_runner``: the cache turns the recipe chains of a parameter group into items (see
``weight_cache._refresh_plan``), ``run`` allocates the outputs, fills the argument table and launches.  The hook is offered only while the HIP
backend is active and ``GANCONTROL_WEIGHT_REFRESH`` is not ``0``; with the knob off the level-by-level refill and the foreach EMA run as before
(same bits: what a same-tree A/B compares).
"""
import ctypes
import os

import torch          # the outputs are allocated through this name: tests swap it for a guard-banded allocator

from ... import _lib
from . import _backend
from . import weight_cache
from ._backend import HipBackend          # noqa: F401  (the launch path the guard-banded allocator of the tests wraps, as in fc_train.py)

ENABLED = os.environ.get('GANCONTROL_WEIGHT_REFRESH', '1') != '0'
ENTRY = 'gc_weight_refresh_grouped_f32'
TAPS = (1, 9)                       # tap counts the kernel is built for
FORMS = ('w_t', 'adj', 'adj2', 'pack_w', 'pack_adj', 'wsq')

_pack_bytes = {}                    # (conv-desc fields, taps, k, n) -> bytes of the hi / lo packs, 0 = not the common pack format
_checked = [False]


def launches():
    """Kernel launches the entry has issued in this process so far (counted where they are issued)."""
    return _lib.load().gc_weight_refresh_launches()


def _check_mirror():
    if not _checked[0]:
        theirs, ours = _lib.load().gc_weight_refresh_item_bytes(), ctypes.sizeof(_lib.WRefreshItem)
        if theirs != ours:
            raise RuntimeError('gan_control_amd: gc_wrefresh_item is %d bytes in the library and %d in the binding; rebuild the library' % (theirs, ours))
        _checked[0] = True


def pack_bytes(fields, taps, k, n):
    """Bytes of the hi / lo packs of a [taps, k, n] weight under the convolution descriptor ``fields`` when they have the format of
    gc_conv2d_pack_weights_bf16x3 (2 * taps * ceil(k / 8) * n units of 16 bytes); 0 for a descriptor of other extents or one that takes no packs."""
    key = (tuple(fields), taps, k, n)
    v = _pack_bytes.get(key)
    if v is None:
        desc = _lib.ConvDesc(*fields)
        v = 0
        if desc.in_ch == k and desc.out_ch == n and desc.kh * desc.kw == taps:
            v = _lib.load().gc_conv2d_bf16x3_packed_bytes(desc)
            if v != 2 * taps * ((k + 7) // 8) * n * 16:
                v = 0
        _pack_bytes[key] = v
    return v


def run(items, flats=()):
    """items: dicts with ``src`` (a contiguous view [n, k, ...] of a parameter), ``taps``, ``k``, ``n``, ``flip``, ``scale``, the forms wanted --
    ``w_t`` / ``adj`` / ``adj2`` (the adjoint layout of ``adj``: the values of ``w_t``): the shape of the output or None, ``pack_w`` / ``pack_adj``:
    bytes or 0, ``wsq``: bool -- and ``ema``: None or (destination with the memory order of ``src``, decay, alpha).  flats: (src, destination, decay, alpha) of parameters that get the EMA only.
    -> one dict {form: fresh tensor} per item.  Raises _lib.UnsupportedError, before anything is launched, for what the kernel does not take."""
    if not items and not flats:
        return []
    _check_mirror()
    first = items[0]['src'] if items else flats[0][0]
    dev = first.device
    table = (_lib.WRefreshItem * (len(items) + len(flats)))()
    outs = []
    for g, it in zip(table, items):
        src, taps, k, n = it['src'], it['taps'], it['k'], it['n']
        _lib.require_cuda_f32(src)
        if taps not in TAPS or src.numel() != taps * k * n:
            raise _lib.UnsupportedError('weight_refresh: a [%d, %d] weight with %d taps (%d elements)' % (n, k, taps, src.numel()))
        out = {}
        if it.get('w_t') is not None:
            out['w_t'] = torch.empty(tuple(it['w_t']), dtype=torch.float32, device=dev)
        for name in ('adj', 'adj2'):
            if it.get(name) is not None:
                out[name] = torch.empty(tuple(it[name]), dtype=torch.float32, device=dev)
        for name, kk, nn in (('pack_w', k, n), ('pack_adj', n, k)):
            if it.get(name):
                if it[name] != 2 * taps * ((kk + 7) // 8) * nn * 16:
                    raise _lib.UnsupportedError('weight_refresh: %s of %d bytes is not the common pack format' % (name, it[name]))
                out[name] = torch.empty(it[name] // 4, dtype=torch.float32, device=dev)
        if it.get('wsq'):
            out['wsq'] = torch.empty((n, k), dtype=torch.float32, device=dev)
        for name in ('w_t', 'adj', 'adj2'):
            if name in out and out[name].numel() != taps * k * n:
                raise _lib.UnsupportedError('weight_refresh: %s of shape %s for %d x %d x %d elements' % (name, tuple(out[name].shape), taps, k, n))
        g.src = src.data_ptr()
        for name in FORMS:
            setattr(g, name, out[name].data_ptr() if name in out else None)
        g.n, g.k, g.taps, g.flip_taps, g.scale = n, k, taps, int(bool(it['flip'])), float(it['scale'])
        if it.get('ema') is not None:
            dst, decay, alpha = it['ema']
            _lib.require_cuda_f32(dst)
            if dst.numel() != src.numel():
                raise _lib.UnsupportedError('weight_refresh: EMA destination of %d elements for a source of %d' % (dst.numel(), src.numel()))
            g.ema, g.decay, g.alpha = dst.data_ptr(), float(decay), float(alpha)
        outs.append(out)
    for g, (src, dst, decay, alpha) in zip(table[len(items):], flats):
        _lib.require_cuda_f32(src, dst)
        if dst.numel() != src.numel() or src.numel() == 0:
            raise _lib.UnsupportedError('weight_refresh: EMA destination of %d elements for a source of %d' % (dst.numel(), src.numel()))
        g.src, g.ema, g.count, g.taps, g.decay, g.alpha = src.data_ptr(), dst.data_ptr(), src.numel(), 0, float(decay), float(alpha)
    _backend.get()._launch(dev, ENTRY, table, len(table), _lib.stream_of(first))
    return outs


def ema_ok(tensors):
    """Whether the EMA over these tensors can run in the kernel: float32, contiguous, on one GPU."""
    dev = None
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() > 0):
            return False
        if dev is None:
            dev = t.device
        elif t.device != dev:
            return False
    return dev is not None


class _Runner:
    pack_bytes = staticmethod(pack_bytes)
    run = staticmethod(run)
    ema_ok = staticmethod(ema_ok)
    taps = TAPS


def _runner():
    return _Runner if (ENABLED and getattr(_backend.get(), 'name', None) == 'hip') else None


weight_cache.refresh_runner = _runner
