"""Late-arriving inputs on a side stream: does every launch of a call go to the stream the caller made current?  (tests only)

The last argument of every kernel entry is the stream.  On the default stream a launch that drops it, a second stage that goes to stream 0 or a
wrapper that asks for the wrong stream still gives the right answer, because everything is serialised there.  ``late_run`` makes the order matter:

    plain run on the default stream (the caller's; its outputs are cloned)         -> ``plain``
    the inputs are overwritten in place with NaN (0xFF bytes for integer tensors); a row-pitched view keeps its layout and padding
    on ``side`` (a ``torch.cuda.Stream()``, see ``side_stream``):   delay of D ms | inputs.copy_(held) | restored.record() | the call itself
    ``restored.query()`` is read the moment the call returns on the host

``restored.query()`` must be False then: every launch of the call was issued while the inputs still held NaN and the side stream was still
inside the delay.  That is what makes the run CONCLUSIVE; a run in which it is True proves nothing and is reported as such, never as a pass.
A launch that went to stream 0 -- or to any stream but the current one -- does not wait for the delay (torch's side streams do not synchronise
with the null stream): it runs at once, reads NaN inputs or a workspace its first stage has not written, and the output is NaN or differs from
``plain``.  A correct call cannot fail: stream order guarantees that it sees the restored inputs.

No stale result, no early write.  A buffer the call obtains on the side stream must not hold the correct result of the plain run (the caching
allocator hands the plain run's freed blocks out again), and a stage that WRITES without reading the late inputs -- a ``hipMemsetAsync`` in front
of an accumulating kernel -- must not get away with running early either.  ``filling(modules, entries)`` swaps the module-level ``torch`` of
the launching modules, as ``guarded_alloc.guarded`` does, for a proxy whose ``empty`` / ``empty_like`` fill what they hand out with NaN on the
CURRENT stream, and ``late_run`` runs the call under it: the fill sits in side-stream order behind the delay and the restore and in front of
the launches that write the buffer.  A launch that ran at once on NaN inputs wrote NaN; what a mis-streamed second stage or memset wrote at
once is overwritten by the fill, and the kernel behind it then accumulates into NaN, or nothing writes the buffer again: the output is NaN in
every case.  (A fill issued BEFORE the delay would not do: a memset on stream 0 would clear it unnoticed.)  Outputs and workspaces that a case
owns itself are part of its inputs: they are restored, to NaN, behind the delay in the same way.

The delay is ``torch.cuda._sleep`` (spins on the clock, touches no memory), calibrated once per process with ``torch.cuda.Event`` timing; where
a torch build has no ``_sleep``, a chain of matmuls on private buffers.  Nothing here launches a kernel of the library or provokes a fault:
stream 0 is a legal stream.
"""
import contextlib
import time

import torch as _torch

D_MS = 100.0          # ten times the largest host issue time of a case, capped at 100 ms (profiles/stream_order.md)

_calibration = {}


def _matmul_chain(n, bufs):
    a, b = bufs
    for _ in range(n):
        _torch.mm(a, b, out=a)          # b is a scaled orthogonal matrix: the values stay bounded


def calibrate():
    """-> ('sleep', cycles per ms) or ('matmul', multiplications per ms, (a, b)): measured once on the current device with Event timing."""
    dev = _torch.cuda.current_device()
    if dev in _calibration:
        return _calibration[dev]
    start, stop = _torch.cuda.Event(enable_timing=True), _torch.cuda.Event(enable_timing=True)
    if hasattr(_torch.cuda, '_sleep'):
        cycles = 20_000_000
        _torch.cuda._sleep(1000)          # (the first launch loads the kernel)
        _torch.cuda.synchronize()
        start.record()
        _torch.cuda._sleep(cycles)
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        cal = ('sleep', cycles / max(ms, 1e-3))
    else:
        q, _ = _torch.linalg.qr(_torch.randn(1024, 1024, device='cuda'))
        bufs = (_torch.randn(1024, 1024, device='cuda'), q.contiguous())
        _matmul_chain(8, bufs)
        _torch.cuda.synchronize()
        start.record()
        _matmul_chain(64, bufs)
        stop.record()
        stop.synchronize()
        cal = ('matmul', 64 / max(start.elapsed_time(stop), 1e-3), bufs)
    _calibration[dev] = cal
    return cal


def delay(ms):
    """GPU work of ``ms`` milliseconds on the current stream that touches none of a case's memory."""
    if ms <= 0:
        return
    cal = calibrate()
    if cal[0] == 'sleep':
        left = int(cal[1] * ms)
        while left > 0:                      # (pieces of at most 2^31 - 1 cycles)
            piece = min(left, (1 << 31) - 1)
            _torch.cuda._sleep(piece)
            left -= piece
    else:
        _matmul_chain(max(1, int(cal[1] * ms)), cal[2])


def measure_delay(ms):
    """How long ``delay(ms)`` takes on the device, by Event timing."""
    start, stop = _torch.cuda.Event(enable_timing=True), _torch.cuda.Event(enable_timing=True)
    _torch.cuda.synchronize()
    start.record()
    delay(ms)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


# ---- the tensors of a case ---------------------------------------------------------------------------------------------------------------------------

def leaves(obj, prefix=''):
    """[(name, tensor)] of every tensor in a dict / list / tuple / nn.Module (parameters and buffers) / tensor; anything else has none."""
    if _torch.is_tensor(obj):
        return [(prefix, obj)]
    if isinstance(obj, dict):
        return [p for k, v in obj.items() for p in leaves(v, '%s/%s' % (prefix, k) if prefix else str(k))]
    if isinstance(obj, (list, tuple)):
        return [p for i, v in enumerate(obj) for p in leaves(v, '%s[%d]' % (prefix, i))]
    if isinstance(obj, _torch.nn.Module):
        return [('%s.%s' % (prefix, n), t) for n, t in list(obj.named_parameters()) + list(obj.named_buffers())]
    return []


def _distinct(pairs):
    seen, out = set(), []
    for name, t in pairs:
        if t.is_cuda and id(t) not in seen:
            seen.add(id(t))
            out.append((name, t))
    return out


def snapshot(inputs):
    """{name: (tensor, clone)} of every device tensor among the inputs."""
    return {name: (t, t.detach().clone()) for name, t in _distinct(leaves(inputs))}


def spoil(held):
    """Overwrite every input in place: NaN for floating point, 0xFF bytes for anything else.  Only the logical elements of a view are written."""
    with _torch.no_grad():
        for t, _ in held.values():
            d = t.detach()
            if d.is_floating_point():
                d.fill_(float('nan'))
            elif d.dtype == _torch.bool:
                d.fill_(True)
            else:
                d.fill_(255 if d.dtype == _torch.uint8 else -1)


def restore(held):
    with _torch.no_grad():
        for t, keep in held.values():
            t.detach().copy_(keep)


def clone_outs(outs):
    return [None if o is None else o.detach().clone() for o in outs]


# ---- allocations of the launching modules -------------------------------------------------------------------------------------------------------------

def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _fill(t, zero):
    if t.numel() == 0:
        return t
    if zero:
        t.zero_()
    elif t.is_floating_point():
        t.fill_(float('nan'))
    else:
        t.fill_(True if t.dtype == _torch.bool else (255 if t.dtype == _torch.uint8 else -1))
    return t


class _Allocs:
    """``empty`` / ``empty_like`` / ``zeros`` of a launching module: real allocations, NaN-filled (0xFF bytes for integers; ``zeros``: zeroed) on
    the stream that is current when they are made."""

    @staticmethod
    def empty(*size, dtype=None, device=None, **kw):
        return _fill(_torch.empty(_shape_of(size), dtype=dtype, device=device, **kw), False)

    @staticmethod
    def zeros(*size, dtype=None, device=None, **kw):
        return _torch.zeros(_shape_of(size), dtype=dtype, device=device, **kw)

    @staticmethod
    def empty_like(t, **kw):
        return _fill(_torch.empty_like(t, **kw), False)


class _TorchProxy:
    def __init__(self, allocs):
        object.__setattr__(self, '_allocs', allocs)
        for name in ('empty', 'empty_like', 'zeros'):
            object.__setattr__(self, name, getattr(allocs, name))

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError('the torch proxy of tests/stream_order.py is read-only')


@contextlib.contextmanager
def filling(modules, entries):
    """``module.torch`` of every module is the proxy and ``HipBackend._launch`` records the entry names; both restored on exit."""
    modules = list(modules)
    backend = modules[0].HipBackend
    real_launch = backend._launch
    real = [m.torch for m in modules]

    def recording_launch(self, dev, entry, *args, **kw):
        entries.append(entry)
        return real_launch(self, dev, entry, *args, **kw)

    proxy = _TorchProxy(_Allocs)
    for m in modules:
        m.torch = proxy
    backend._launch = recording_launch
    try:
        yield
    finally:
        for m, t in zip(modules, real):
            m.torch = t
        backend._launch = real_launch


# ---- the late run -----------------------------------------------------------------------------------------------------------------------------------

_side = {}


def side_stream():
    """The side stream of every late run of the process: one stream of torch's pool, probed once -- a delay on it must NOT hold back a launch
    on stream 0.  A stream that the runtime maps to the hardware queue of the null stream executes behind it, and there a mis-streamed launch
    would wait for the delay like a correct one: RuntimeError then, since the method cannot see a mis-streamed launch on such a runtime and no
    test may pass by it.  (With the default stream: two streams per process.)"""
    dev = _torch.cuda.current_device()
    if dev in _side:
        return _side[dev]
    private = _torch.zeros(64, device='cuda')
    s = _torch.cuda.Stream()
    behind, null_done = _torch.cuda.Event(), _torch.cuda.Event()
    _torch.cuda.synchronize()
    with _torch.cuda.stream(s):
        delay(20.0)
        behind.record(s)
    private.fill_(1.0)                       # on the default stream
    null_done.record()
    null_done.synchronize()                  # (at most the 20 ms of the delay)
    concurrent = not behind.query()
    s.synchronize()
    if not concurrent:
        raise RuntimeError('stream_order: the side stream does not run concurrently with stream 0 on this runtime; the late-input method proves nothing here')
    _side[dev] = s
    return s


class LateRun:
    """outs: what the call returned (read after side.synchronize()); conclusive: ``restored.query()`` was False when the call returned on the
    host; entries: the entries it reached; issue_ms: host time from the start of the call to its return."""
    __slots__ = ('outs', 'conclusive', 'entries', 'issue_ms', 'delay_ms')


def late_run(held, call, modules=(), delay_ms=D_MS):
    """The side-stream pass (module docstring).  held: ``snapshot(inputs)`` taken BEFORE the plain run (a call may update an input in place);
    call: issues the launches and returns a list of tensors; modules: the launching modules whose allocations are filled where they are made.
    One process, two streams: the default one and ``side``."""
    spoil(held)
    _torch.cuda.synchronize()
    side = side_stream()
    restored = _torch.cuda.Event()
    run = LateRun()
    run.entries, run.delay_ms = [], delay_ms
    with _torch.cuda.stream(side):
        delay(delay_ms)
        restore(held)
        restored.record(side)
        t0 = time.perf_counter()
        if modules:
            with filling(modules, run.entries):
                outs = call()
        else:
            outs = call()
        run.conclusive = not restored.query()
        run.issue_ms = 1e3 * (time.perf_counter() - t0)
    side.synchronize()
    run.outs = list(outs)
    return run


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(_torch.uint8) if t.numel() else t


def difference(plain, outs):
    """None when every output is finite and has the plain run's bits; else a sentence naming the first output that does not."""
    if len(plain) != len(outs):
        return '%d outputs, the plain run had %d' % (len(outs), len(plain))
    for i, (p, o) in enumerate(zip(plain, outs)):
        if (p is None) != (o is None):
            return 'output %d: None in one run only' % i
        if p is None:
            continue
        if p.shape != o.shape or p.dtype != o.dtype:
            return 'output %d: %s %s, the plain run gave %s %s' % (i, tuple(o.shape), o.dtype, tuple(p.shape), p.dtype)
        if o.is_floating_point():
            bad = int((~_torch.isfinite(o)).sum()) - int((~_torch.isfinite(p)).sum())
            if bad:
                return 'output %d holds %d non-finite elements the plain run does not have' % (i, bad)
        if not _torch.equal(_bits(o), _bits(p)):
            return 'output %d differs from the plain run in %d bytes' % (i, int((_bits(o) != _bits(p)).sum()))
    return None
