"""gc_fc_stacks_fwd_f32 on the GPU (csrc/fc_stack.hip through models/op/fc_stack.py).

Every case runs on fp32 inputs against the documented formula in float64 (PixelNorm + oracle.controller.fc_stack_forward on the upcast inputs).
The tolerance is relative to the existing module path on the same inputs: with e = max|y - y64| / max|y64|, kernel e <= 4 x module-path e (both
round the same fp32 products and differ in the order of the sums; each e is a maximum over ~1e3 elements).  Every call runs on guard-banded,
poisoned outputs and on inputs with hostile surroundings (tests/guarded_alloc.py).  Measured figures: profiles/inference.md.
"""
import ctypes

import pytest
import torch
from torch import nn

import guarded_alloc
import inference_checks as ic

from gan_control_amd import _lib
from gan_control_amd.models.gan_model import EqualLinear, PixelNorm
from gan_control_amd.models.op import _backend
from gan_control_amd.models.op import fc_stack as fcs

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SPLIT64 = [64] + [256] * 7 + [64]
SPLIT128 = [128] + [256] * 7 + [128]
VANILLA = [512] * 9


def controller_widths(in_dim):
    return [in_dim, 512, 512, 512, 64]


def make_stack(widths, norm, seed):
    """EqualLinear draws randn / lr_mul itself; the biases become non-zero."""
    torch.manual_seed(seed)
    layers = [EqualLinear(a, b, lr_mul=0.01, activation='fused_lrelu') for a, b in zip(widths[:-1], widths[1:])]
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in layers:
            m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 10)
    return nn.Sequential(*([PixelNorm()] if norm else []), *layers).to(DEV)


@pytest.fixture
def any_shape(monkeypatch):
    """The measured dispatch rule aside: every shape inside the kernel's limits takes the kernel."""
    monkeypatch.setattr(fcs, 'KERNEL_MAX_BATCH', 1 << 30)
    monkeypatch.setattr(fcs, 'KERNEL_WIDE_MAX_BATCH', 1 << 30)


# name -> (list of (widths, pixel_norm), layout); layouts: 'z' = column slices of one [B, 512] input and of one [B, 512] output (the mapping
# network), 'odd' = slices at odd column offsets of wider rows on both sides, 'own' = one input tensor per stack, outputs sliced from one row
# at odd offsets (the controllers' splice)
CASES = {
    'split7': ([(SPLIT128, True)] + [(SPLIT64, True)] * 6, 'z'),
    'vanilla': ([(VANILLA, True)], 'z'),
    'controllers': ([(controller_widths(k), False) for k in (1, 3, 8, 27)], 'own'),
    'nine': ([([3, 16], False), (controller_widths(3), False), (SPLIT64, True), ([27, 64, 64], False), ([8, 32], True), ([1, 16], False),
              ([128, 256, 128], True), ([3, 16], True), ([64, 256, 64], True)], 'odd'),
    'single': ([([3, 16], False)], 'odd'),
}
RUNS = [('split7', 1), ('split7', 8), ('split7', 9), ('split7', 17), ('vanilla', 1), ('vanilla', 9), ('controllers', 1), ('controllers', 8),
        ('controllers', 17), ('nine', 9), ('nine', 1), ('single', 17), ('single', 8)]


def build(name, batch, zero_row=None):
    specs, layout = CASES[name]
    stacks = [make_stack(w, norm, 10 * i + len(w)) for i, (w, norm) in enumerate(specs)]
    gen = torch.Generator().manual_seed(batch + len(specs))
    ins, outs = [w[0] for w, _ in specs], [w[-1] for w, _ in specs]
    if layout == 'own':
        xs = [torch.randn(batch, k, generator=gen).to(DEV) for k in ins]
        x_slices = [None] * len(specs)
    else:
        lead = 0 if layout == 'z' else 3
        wide = torch.randn(batch, lead + sum(ins) + (0 if layout == 'z' else 2), generator=gen)
        if zero_row is not None:
            wide[zero_row] = 0
        xs, x_slices, at = wide.to(DEV), [], lead
        for k in ins:
            x_slices.append((at, at + k))
            at += k
    lead = 0 if layout == 'z' else 5
    out_slices, at = [], lead
    for k in outs:
        out_slices.append((at, at + k))
        at += k + (0 if layout == 'z' else 1)          # 'odd' / 'own': one untouched column between two slices
    return stacks, xs, x_slices, (batch, at + (0 if layout == 'z' else 2)), out_slices


def x_of(xs, x_slices, i):
    t = xs[i] if isinstance(xs, list) else xs
    return t if x_slices[i] is None else t[:, x_slices[i][0]:x_slices[i][1]]


def run_kernel(stacks, xs, x_slices, out_shape, out_slices, poison='nan', fill=None, shift=0):
    """One fc_stacks_forward call on a guarded, poisoned output and (fill) on hostile copies of the inputs -> (out, launches)."""
    if fill is not None:
        xs = [guarded_alloc.hostile(t, fill, shift) for t in xs] if isinstance(xs, list) else guarded_alloc.hostile(xs, fill, shift)
    with torch.no_grad(), guarded_alloc.guarded(fcs, poison=poison) as guard:
        out = guard.empty(out_shape, dtype=torch.float32, device=DEV)
        got = fcs.fc_stacks_forward(stacks, xs, x_slices, out, out_slices)
        assert got is out
        assert guard.check() == []
    return out, guard.entries


def errors(out, stacks, xs, x_slices, out_slices):
    """(kernel error, module-path error) against the float64 formula, over all stacks of the call."""
    with torch.no_grad():
        mod = [s(x_of(xs, x_slices, i).contiguous()) for i, s in enumerate(stacks)]
    ref = [ic.oracle_stack(s, x_of(xs, x_slices, i)) for i, s in enumerate(stacks)]
    scale = max(float(r.abs().max()) for r in ref)
    e_k = max(float((out[:, lo:hi].double().cpu() - r).abs().max()) for (lo, hi), r in zip(out_slices, ref)) / scale
    e_m = max(float((m.double().cpu() - r).abs().max()) for m, r in zip(mod, ref)) / scale
    return e_k, e_m


@pytest.mark.parametrize('name,batch', RUNS)
def test_kernel_against_the_float64_formula(name, batch, any_shape):
    case = build(name, batch)
    stacks, xs, x_slices, out_shape, out_slices = case
    out, entries = run_kernel(*case)
    assert entries == [fcs.ENTRY]          # one call of the entry (it cuts 9 stacks into two launches itself)
    e_k, e_m = errors(out, stacks, xs, x_slices, out_slices)
    print('fc_stack %-12s B=%-3d kernel %.3e  module path %.3e' % (name, batch, e_k, e_m))
    assert e_k <= 4 * e_m, (e_k, e_m)
    # the same bits again; columns outside the written slices keep the poison; hostile surroundings of the inputs change nothing
    again, _ = run_kernel(*case)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    written = torch.zeros(out_shape[1], dtype=torch.bool)
    for lo, hi in out_slices:
        written[lo:hi] = True
    bits = out.view(torch.int32).cpu()
    assert bool((bits[:, ~written] == guarded_alloc.POISONS['nan']).all()) and not bool(torch.isnan(out[:, written.to(DEV)]).any())
    for poison, fill, shift in (('big', 'nan', 4), ('nan', 'big', 0)):
        other, _ = run_kernel(*case, poison=poison, fill=fill, shift=shift)
        assert torch.equal(other[:, written.to(DEV)], out[:, written.to(DEV)]), (poison, fill)
        assert bool((other.view(torch.int32).cpu()[:, ~written] == guarded_alloc.POISONS[poison]).all())


def test_all_zero_row_under_pixel_norm(any_shape):
    case = build('split7', 8, zero_row=2)
    stacks, xs, x_slices, out_shape, out_slices = case
    out, _ = run_kernel(*case)
    assert bool(torch.isfinite(out).all())
    e_k, e_m = errors(out, stacks, xs, x_slices, out_slices)
    print('fc_stack zero row        kernel %.3e  module path %.3e' % (e_k, e_m))
    assert e_k <= 4 * e_m, (e_k, e_m)
    # the zero row: every layer sees the biases alone
    ref = ic.oracle_stack(stacks[1], torch.zeros(1, 64))
    lo, hi = out_slices[1]
    assert float((out[2:3, lo:hi].double().cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def _raw(widths_per_stack, batch, x, y, w):
    """The entry called with tables that all point at the same buffers (only shapes matter: the refusals come before any launch)."""
    n = len(widths_per_stack)
    layers = sum(len(ws) - 1 for ws in widths_per_stack)
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    args = ((vp * n)(*[x.data_ptr()] * n), (i64 * n)(*[1024] * n), (vp * n)(*[y.data_ptr()] * n), (i64 * n)(*[1024] * n),
            (i32 * n)(*[ws[0] for ws in widths_per_stack]), (i32 * n)(*[len(ws) - 1 for ws in widths_per_stack]), (i32 * n)(*[0] * n),
            (vp * layers)(*[w.data_ptr()] * layers), (vp * layers)(*[w.data_ptr()] * layers),
            (i32 * layers)(*[d for ws in widths_per_stack for d in ws[1:]]), (f32 * layers)(*[1.0] * layers), (f32 * layers)(*[1.0] * layers))
    _backend.get()._launch(x.device, fcs.ENTRY, *args, n, batch, _lib.stream_of(x))


def test_unsupported_shapes_are_refused_before_any_launch():
    x = torch.zeros(4, 1024, device=DEV)
    y = torch.full((4, 1024), 3.0, device=DEV)
    w = torch.zeros(520 * 520, device=DEV)
    for widths, batch, word in (([[513, 16]], 4, 'input width 513'), ([[16, 513]], 4, 'output width 513'), ([[16] * 10], 4, '9 layers'),
                                ([[16, 16]], 0, 'batch 0'), ([[16, 16], [8, 0]], 4, 'output width 0')):
        with pytest.raises(_lib.UnsupportedError, match=word):
            _raw(widths, batch, x, y, w)
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
    _raw([[16, 16, 16]], 4, x, y, w)          # the same tables within the limits run: zero weights and biases give zeros
    torch.cuda.synchronize()
    assert bool((y[:, :16] == 0).all()) and bool((y[:, 16:] == 3.0).all())


def test_operator_dispatch(any_shape):
    """Autograd, another dtype or an overlapping output take the module path: nothing of the new entry is launched."""
    stack = make_stack([8, 32, 8], True, 5)
    x = torch.randn(4, 8, device=DEV)
    calls = []
    real = _backend.HipBackend._launch

    def counting(self, dev, entry, *a, **k):
        calls.append(entry)
        return real(self, dev, entry, *a, **k)

    _backend.HipBackend._launch = counting
    try:
        with torch.no_grad():
            out = fcs.fc_stacks_forward([stack], x, None, torch.empty(4, 8, device=DEV), None)
            assert calls == [fcs.ENTRY]
            del calls[:]
            same = fcs.fc_stacks_forward([stack], x, None, x.clone(), None)
            assert torch.equal(same, out) and calls == [fcs.ENTRY]
            del calls[:]
            wide = torch.randn(4, 16, device=DEV)
            fcs.fc_stacks_forward([stack], wide, [(0, 8)], wide, [(8, 16)])          # output and input share a buffer
            assert fcs.ENTRY not in calls and torch.equal(wide[:, 8:], stack(wide[:, :8]))
            # rows that share memory (an expanded control, row stride 0): the module path, and what it gives on the contiguous copy
            one = torch.randn(1, 8, device=DEV)
            for shared in (one.expand(4, 8), torch.randn(1, 64, device=DEV).expand(4, 64)[:, 8:16]):
                del calls[:]
                got = fcs.fc_stacks_forward([stack], shared, None, torch.empty(4, 8, device=DEV), None)
                assert fcs.ENTRY not in calls and torch.equal(got, stack(shared.contiguous()))
            del calls[:]
            got = fcs.fc_stacks_forward([stack], one.expand(1, 8), None, torch.empty(1, 8, device=DEV), None)          # one row: no stride is used
            assert calls == [fcs.ENTRY] and float((got - stack(one)).abs().max()) <= 1e-5 * float(got.abs().max())
        del calls[:]
        xg = x.clone().requires_grad_(True)
        y = fcs.fc_stacks_forward([stack], xg, None, torch.empty(4, 8, device=DEV), None)
        assert fcs.ENTRY not in calls and torch.equal(y, stack(x))
        y.sum().backward()
        assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    finally:
        _backend.HipBackend._launch = real


def test_dispatch_limits_follow_the_measured_table():
    """Beyond the largest batch measured for its class of stack (profiles/inference.md) a call takes the module path."""
    wide, narrow = make_stack(VANILLA, True, 7), make_stack(SPLIT64, True, 8)
    seen = []
    real = _backend.HipBackend._launch

    def counting(self, dev, entry, *a, **k):
        seen.append(entry)
        return real(self, dev, entry, *a, **k)

    _backend.HipBackend._launch = counting
    try:
        with torch.no_grad():
            for stack, width, batch, fused in ((wide, 512, fcs.KERNEL_WIDE_MAX_BATCH, True), (wide, 512, fcs.KERNEL_WIDE_MAX_BATCH + 1, False),
                                               (narrow, 64, fcs.KERNEL_WIDE_MAX_BATCH + 1, True), (narrow, 64, fcs.KERNEL_MAX_BATCH + 1, False)):
                del seen[:]
                x = torch.randn(batch, width, device=DEV)
                out = fcs.fc_stacks_forward([stack], x, None, torch.empty(batch, width, device=DEV), None)
                assert (seen == [fcs.ENTRY]) == fused and (fcs.ENTRY in seen) == fused, (width, batch, seen[:3])
                assert float((out - stack(x)).abs().max()) <= 1e-5 * float(out.abs().max())
    finally:
        _backend.HipBackend._launch = real
