#!/usr/bin/env python3
"""The tables of profiles/separability.md: the all-pairs distances of the separability evaluation on the kernel path of
models/op/pairwise.py (gc_pairwise_f32) against its chunked torch path -- the reference's arithmetic, 20 x 20 rows at a time, on ATen -- on
one GPU, and whole LossModelClass.calc_same_not_same_list calls on both.

    python tools/separability_bench.py [file to write the tables to as well] [--quick]

Shapes: 1000 signatures x 1000 queries with SQ at K = 512 (the shipped configuration: last layer only) and ABS at K = 25088, 50176, 100352,
200704 (the four IR-SE levels, level 4 first), and 50 x 50 (the debug size) for both.  Every call is timed on its own between two device
events after a warm-up; the two paths alternate three times in one process and the median over all samples is printed, with max / min of the
three per-round medians.  pair-elements / s = m n K / time; the ceiling is the derived 39.3 T pair-elements / s (two vector instructions per
pair-element at the 157.3 TF/s fp32 vector peak = 78.6 T lane-operations / s).  Inputs come from a seed; nothing outside the repository is read.
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'gan-control_amd')):
    sys.path.insert(0, p)

from gan_control_amd.losses import LossModelClass          # noqa: E402
from gan_control_amd.models.op import pairwise as pw          # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
QUICK = '--quick' in sys.argv
OUT = ARGS[0] if ARGS else None
CEILING = 157.3e12 / 2 / 2          # pair-elements per second
DEV = 'cuda'
U = 2.0 ** -24
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def spans(fn, warm, reps):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def ab(kernel_fn, torch_fn, reps_k, reps_t):
    """-> (kernel us, torch us, spread kernel, spread torch): medians over three alternating rounds"""
    rounds = {'k': [], 't': []}
    for r in range(3):
        rounds['k'].append(spans(kernel_fn, 3 if r == 0 else 1, reps_k))
        rounds['t'].append(spans(torch_fn, 1, reps_t))
    med = {k: statistics.median(x for r in v for x in r) for k, v in rounds.items()}
    spread = {k: max(statistics.median(r) for r in v) / min(statistics.median(r) for r in v) for k, v in rounds.items()}
    return med['k'], med['t'], spread['k'], spread['t']


def formula64(s, q, mode):
    s64, q64 = s.double(), q.double()
    k = s.shape[1]
    step = max(1, (1 << 24) // (q.shape[0] * k))
    rows = []
    for i in range(0, s.shape[0], step):
        d = s64[i:i + step, None, :] - q64[None, :, :]
        rows.append(d.abs().sum(-1) / k if mode == 'abs' else (d * d).sum(-1))
    return torch.cat(rows, 0)


def distances_table():
    say('| mode | m x n | K | kernel us | torch path us | ratio | T pair-elements / s | of the 39.3 T/s ceiling | spread kernel / torch |')
    say('|---|---|---|---|---|---|---|---|---|')
    gen = torch.Generator().manual_seed(0)
    shapes = [('sq', 1000, 512), ('abs', 1000, 25088), ('abs', 1000, 50176), ('abs', 1000, 100352), ('abs', 1000, 200704), ('sq', 50, 512), ('abs', 50, 25088),
              ('abs', 50, 200704)]
    if QUICK:
        shapes = [('sq', 1000, 512), ('abs', 1000, 25088), ('sq', 50, 512)]
    for mode, m, k in shapes:
        s = torch.randn(m, k, generator=gen).to(DEV)
        q = torch.randn(m, k, generator=gen).to(DEV)
        assert pw.kernel_taken(s, q)
        fn = pw._mode_fn(mode)
        work = float(m) * m * k
        big = work > 1e10
        with torch.no_grad():
            tk, tt, sk, st = ab(lambda: pw.pairwise_distances(s, q, mode), lambda: pw.chunked_distances(s, q, fn), 20 if big else 200, 2 if big else 20)
        rate = work / (tk * 1e-6)
        say('| %s | %d x %d%s | %d | %.1f | %.1f | %.1f x | %.2f | %.1f %% | %.2f / %.2f |'
            % (mode.upper(), m, m, ' (debug)' if m == 50 else '', k, tk, tt, tt / tk, rate / 1e12, 100 * rate / CEILING, sk, st))
        del s, q
        torch.cuda.empty_cache()


def errors_table():
    say('| mode | m x n | K | kernel max error | torch path max error | bound (K + 4) u |')
    say('|---|---|---|---|---|---|')
    gen = torch.Generator().manual_seed(1)
    for mode, m, k in (('sq', 130, 512), ('abs', 130, 25088), ('abs', 20, 200704), ('abs', 130, 33), ('sq', 130, 5)):
        s = torch.randn(m, k, generator=gen).to(DEV)
        q = torch.randn(m, k, generator=gen).to(DEV)
        ref = formula64(s, q, mode)
        with torch.no_grad():
            ek = float(((pw.pairwise_distances(s, q, mode).double() - ref).abs() / ref).max())
            et = float(((pw.chunked_distances(s, q, pw._mode_fn(mode)).double() - ref).abs() / ref).max())
        say('| %s | %d x %d | %d | %.2e | %.2e | %.2e |' % (mode.upper(), m, m, k, ek, et, (k + 4) * U))


def reference_loop(all_distances, signature_pids, queries_pids):
    """The per-query loop of the reference's calc_same_not_same_list on a host matrix (lists instead of the quadratic DataFrame.append)."""
    same_mask = signature_pids[:, None] == queries_pids[None, :]
    same, not_same, all_not_same, pairs = [], [], [], []
    for qid in range(all_distances.shape[1]):
        not_same_row_mask = ~same_mask[:, qid]
        same.extend(all_distances[same_mask[:, qid], qid])
        not_same_row = all_distances[not_same_row_mask, qid]
        index_2nd_best = np.argmin(not_same_row)
        not_same.append(not_same_row[index_2nd_best])
        all_not_same.extend(not_same_row)
        pairs.append((signature_pids[not_same_row_mask][index_2nd_best], queries_pids[qid], not_same_row[index_2nd_best]))
    return same, not_same, all_not_same, pairs


def host(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def whole_calls_table():
    say('| calc_same_not_same_list | kernel path ms | torch path ms | torch path + the per-query host loop ms |')
    say('|---|---|---|---|')
    cfg = {'lower_thres': [0.1], 'upper_thres': [0.2], 'last_lower_thres': 0.5, 'last_upper_thres': 1.8, 'intermediate_layers_weights': [0],
           'last_layer_weight': 0.25, 'focus_on_list': ['not_same_as_last_layer', 'same_as_last_layer']}
    lm = LossModelClass(cfg, 'embedding_loss', no_model=True)
    gen = torch.Generator().manual_seed(2)
    cases = [('2000 samples, last layer only (K = 512)', 1000, [512], True), ('100 samples (debug), last layer only', 50, [512], True),
             ('2000 samples, level 4 and the last layer (K = 25088, 512)', 1000, [25088, 512], False)]
    if QUICK:
        cases = cases[:2]
    real = pw.kernel_taken
    for name, m, ks, last_only in cases:
        sig = [torch.randn(m, k, generator=gen).to(DEV) for k in ks]
        que = [torch.randn(m, k, generator=gen).to(DEV) for k in ks]
        if len(ks) > 1:
            sig[0], que[0] = sig[0].view(m, 512, 7, 7), que[0].view(m, 512, 7, 7)
        if last_only and len(ks) == 1:          # the levels the evaluation dropped are None
            sig, que = [None] + sig, [None] + que
        pids = np.arange(m)
        call = lambda: lm.calc_same_not_same_list(sig, que, pids, pids, last_layer_separability_only=last_only)

        def looped():
            with torch.no_grad():
                dists = [pw.chunked_distances(s, q, pw._mode_fn('sq' if s.dim() == 2 else 'abs')) for s, q in zip(sig, que) if s is not None]
            return [reference_loop(d.cpu().numpy(), pids, pids) for d in dists]

        tk = host(call, 5)
        pw.kernel_taken = lambda *a, **k: False
        try:
            tt = host(call, 3)
        finally:
            pw.kernel_taken = real
        tl = host(looped, 3)
        say('| %s | %.2f | %.2f | %.2f |' % (name, tk, tt, tl))


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'separability_bench.py measures on a GPU'
    say('device: %s' % torch.cuda.get_device_name(0))
    say()
    distances_table()
    say()
    errors_table()
    say()
    whole_calls_table()
