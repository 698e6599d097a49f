#!/usr/bin/env python3
"""Dev tool (GPU): host issue time of every stream case of tests/test_stream_order_gpu.py on the default stream -- the second call of each,
from the start of the callable to its return, no synchronisation inside -- per group and the largest twelve; the delay D they give
(ten times the largest, capped at 100 ms: tests/stream_order.py D_MS) and the calibration of the delay.  profiles/stream_order.md."""
import os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'tests'), os.path.join(REPO, 'gan-control_amd'), REPO]
import torch
import conftest  # noqa
import stream_order as so
import test_stream_order_gpu as t
import test_guarded_buffers as tgb
from gan_control_amd.models.op import _backend

hip = _backend.get()
rows = []


def timed(name, group, call):
    call(); torch.cuda.synchronize()
    t0 = time.perf_counter(); call(); t1 = time.perf_counter()
    torch.cuda.synchronize()
    rows.append((1e3 * (t1 - t0), group, name))


for c in tgb.CASES:
    hip.conv_mode = c.mode or 'f32'
    a = c.build('cuda')
    timed(c.name, 'guarded', lambda: c.run(hip, a, None))
    del a
hip.conv_mode = 'f32'
for c in t.OTHER + t.ABI:
    a = c.build()
    timed(c.name, 'abi' if c in t.ABI else 'other', lambda: c.run(a))
hip.conv_mode = 'bf16x3'
a = t._networks()
for name, fn in (('fwd+bwd', t._fwd_bwd), ('r1', t._r1), ('path_length', t._path_length)):
    timed('autograd ' + name, 'autograd', lambda: fn(a))
rows.sort(reverse=True)
for g in ('guarded', 'other', 'abi', 'autograd'):
    sel = [r for r in rows if r[1] == g]
    print('%-9s %4d cases: max %.3f ms (%s), median %.3f ms' % (g, len(sel), sel[0][0], sel[0][2], sel[len(sel) // 2][0]))
print('largest 12:')
for ms, g, n in rows[:12]:
    print('  %8.3f ms  %-9s %s' % (ms, g, n))
print('D = min(100, 10 x %.3f) = %.1f ms' % (rows[0][0], min(100.0, 10 * rows[0][0])))
cal = so.calibrate()
print('calibration: %s, %.5g per ms; delay(100) measured %.2f ms, delay(20) measured %.2f ms' % (cal[0], cal[1], so.measure_delay(100.0), so.measure_delay(20.0)))
so.side_stream()
print('the side stream runs concurrently with stream 0')
