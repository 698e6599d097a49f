#!/usr/bin/env python3
"""The tables of profiles/feature_stats.md: streaming FID statistics (models/op/feature_moments.py, fid_utils/feature_stats.py) on one GPU.

    python tools/feature_stats_bench.py [file to write the tables to as well] [--quick] [--kernels-only] [--size S] [--samples N]

1. ``append`` of a 20 x 2048 batch against the per-batch ``f.to('cpu')`` it replaces: device time between two events over a run of appends,
   and host time of the call (for the copy, the time the host is blocked).  The append is bound by the read-modify-write of the accumulator:
   bytes = 2 x 8 x (64 x 64 per upper tile) + the batch; the rate is quoted against the HBM figures.
2. One call at 50 000 x 2048 against the device formula ``xd = x.double(); xd.sum(0); xd.T @ xd`` and against ``np.cov`` on the host's
   threads.  FLOP = 2 n x (the elements of the upper tiles) for the kernel (what it executes), 2 n F^2 for the formula.
3. ``evaluate_fid`` at the Tracker's batch of 20 (generator of --size, InceptionV3 pool3, --samples images; seeded weights, nothing is read
   from outside the repository): the default call against ``streaming=True, method='eigh'``, and the parts on their own.
4. ``frechet_distance`` against ``frechet_distance_eigh`` at F = 2048 on the host.
Every timed shape is warmed up; medians over the repetitions, with min .. max (whole `evaluate_fid` calls and their parts: three runs after
a warm-up run).
"""
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'gan-control_amd')):
    sys.path.insert(0, p)

from gan_control_amd.fid_utils import fid as fid_module          # noqa: E402
from gan_control_amd.fid_utils.feature_stats import FeatureStats          # noqa: E402
from gan_control_amd.models.op import feature_moments as fm          # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
QUICK = '--quick' in sys.argv


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


OUT = ARGS[0] if ARGS and not ARGS[0].isdigit() else None
SIZE, SAMPLES = option('--size', 256), option('--samples', 1000)
DEV = 'cuda'
F = 2048
HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12          # bytes / s: spec, and the float4 copy rate measured on this part
FP64_MATRIX_PEAK = 78.6e12                        # FLOP / s: the vendor's FP64 matrix figure for the MI355X
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def med(v):
    return '%.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))


def device_ms(fn, warm, reps, inner=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def host_ms(fn, warm, reps, sync_before=True):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        if sync_before:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    torch.cuda.synchronize()
    return out


def upper_tile_elements(f):
    nt = -(-f // fm.TILE)
    return nt * (nt + 1) // 2 * fm.TILE * fm.TILE


def append_table():
    x = torch.randn(20, F, device=DEV) * 0.3 + 0.4
    stats = FeatureStats(F, DEV)
    assert fm.kernel_taken(stats.s1, stats.s2, x)
    nbytes = 2 * 8 * upper_tile_elements(F) + x.numel() * 4 + 2 * 8 * F
    dev = device_ms(lambda: stats.append(x), 5, 9, inner=50)
    host = host_ms(lambda: stats.append(x), 5, 200)
    copy_host = host_ms(lambda: x.to('cpu'), 5, 200)
    copy_dev = device_ms(lambda: x.to('cpu'), 5, 9, inner=50)
    rate = nbytes / (statistics.median(dev) * 1e-3)
    say('| per batch of 20 x 2048 | device ms | host ms of the call |')
    say('|---|---|---|')
    say('| `FeatureStats.append` (one launch, %.1f MB read-modify-write) | %s | %s (enqueue; nothing waits) |' % (nbytes / 1e6, med(dev), med(host)))
    say("| `f.to('cpu')` of the same batch, the features ready | %s | %s (the host is blocked for all of it, and for whatever is still queued in front) |"
        % (med(copy_dev), med(copy_host)))
    say()
    say('append: %.2f TB/s of accumulator traffic = %.0f %% of the %.1f TB/s HBM spec, %.0f %% of the %.2f TB/s copy rate measured on this part '
        '(the 34 MB accumulator fits the 256 MB Infinity Cache, so the figure is not a pure HBM rate)'
        % (rate / 1e12, 100 * rate / HBM_SPEC, HBM_SPEC / 1e12, 100 * rate / HBM_MEASURED, HBM_MEASURED / 1e12))


def big_table():
    n = 10000 if QUICK else 50000
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(n, F, generator=gen, device=DEV) * 0.3 + 0.4

    def kernel():
        s1, s2 = fm.new_accumulator(F, DEV)
        fm.accumulate_(s1, s2, x)
        return s1, s2

    def formula():
        xd = x.double()
        return xd.sum(0), xd.T @ xd

    s1, s2 = fm.new_accumulator(F, DEV)
    acc = device_ms(lambda: fm.accumulate_(s1, s2, x), 1, 5)
    call = device_ms(kernel, 1, 5)
    form = device_ms(formula, 1, 5)
    (k1, k2), (f1, f2) = kernel(), formula()
    rel = float(((torch.triu(k2) - torch.triu(f2)).abs().max() / f2.abs().max()).cpu())
    flop_k, flop_f = 2.0 * n * upper_tile_elements(F), 2.0 * n * F * F
    tk, tf = statistics.median(acc) * 1e-3, statistics.median(form) * 1e-3
    say('| one call, %d x %d | ms | FLOP executed | TFLOP/s | share of the %.1f TF FP64 matrix peak |' % (n, F, FP64_MATRIX_PEAK / 1e12))
    say('|---|---|---|---|---|')
    say('| `accumulate_` into an existing accumulator | %s | %.3g | %.1f | %.0f %% |' % (med(acc), flop_k, flop_k / tk / 1e12, 100 * flop_k / tk / FP64_MATRIX_PEAK))
    say('| fresh accumulator (two memsets) + `accumulate_` | %s | | | |' % med(call))
    say('| device formula `xd = x.double(); xd.sum(0); xd.T @ xd` (%.1f GB widened copy) | %s | %.3g | %.1f | %.0f %% |'
        % (n * F * 8 / 1e9, med(form), flop_f, flop_f / tf / 1e12, 100 * flop_f / tf / FP64_MATRIX_PEAK))
    say()
    say('kernel against the device formula: %.2f x (%.3f ms against %.3f ms); upper triangles agree to %.2e of the largest element'
        % (tf / tk, tk * 1e3, tf * 1e3, rel))
    host = x.cpu().numpy()
    torch.set_num_threads(16)
    t0 = time.perf_counter()
    wide = host.astype(np.float64)
    t1 = time.perf_counter()
    np.cov(wide, rowvar=False)
    t2 = time.perf_counter()
    say('host, %d threads: widening to float64 %.2f s, `np.cov` %.2f s (once each)' % (torch.get_num_threads(), t1 - t0, t2 - t1))
    del wide, host


def fid_table():
    from gan_control_amd.fid_utils.inception import InceptionV3
    from gan_control_amd.models.gan_model import Generator
    from oracle import inception as oracle_inception, networks          # the seeded weight fills of the tests (well-scaled activations)
    g = Generator(SIZE, 512, 8, channel_multiplier=2, conv_transpose=True)
    g.load_state_dict(networks.procedural_fill_(g.state_dict()))
    g = g.to(DEV).eval()
    net = InceptionV3(output_blocks=[3], normalize_input=False)
    net.load_state_dict(oracle_inception.procedural_inception_fill_(net.state_dict()))
    net = net.to(DEV).eval()
    n = 200 if QUICK else SAMPLES
    gen = torch.Generator().manual_seed(2)
    basis = torch.randn(64, F, generator=gen)
    real = (torch.randn(1336, 64, generator=gen) @ basis / 8 + 0.05 * torch.randn(1336, F, generator=gen) + 0.4).double().numpy()
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'real.pkl')
    rm, rc = fid_module.feature_statistics(real)          # 1 336 rows of 2 048 features: a rank-deficient real side
    with open(path, 'wb') as fh:
        pickle.dump({'mean': rm, 'cov': rc}, fh)

    REPS = 3

    def timed(fn, seed=None):
        """-> (the last result, [seconds of REPS runs]) after one warm-up run; the global seed is set before every run when one is given."""
        out, spans = None, []
        for rep in range(REPS + 1):
            if seed is not None:
                torch.manual_seed(seed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rep:
                spans.append(time.perf_counter() - t0)
        return out, spans

    def sec(v):
        return '%.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))

    feats, t_gen = timed(lambda: fid_module.sample_features(g, net, 20, n, DEV, to_host=False), 5)
    _, t_gen_host = timed(lambda: fid_module.sample_features(g, net, 20, n, DEV), 5)
    stats, t_stream = timed(lambda: fid_module.sample_statistics(g, net, 20, n, DEV), 5)
    host_feats = feats.cpu().numpy()
    (mean, cov), t_np = timed(lambda: fid_module.feature_statistics(host_feats))
    (smean, scov), t_finish = timed(stats.numpy)
    d_sqrtm, t_sqrtm = timed(lambda: fid_module.frechet_distance(mean, cov, rm, rc))
    d_eigh, t_eigh = timed(lambda: fid_module.frechet_distance_eigh(mean, cov, rm, rc))
    d_stream = fid_module.frechet_distance_eigh(smean, scov, rm, rc)
    v_default, t_default = timed(lambda: fid_module.evaluate_fid(g, net, 20, n, DEV, path), 5)
    v_stream, t_streaming = timed(lambda: fid_module.evaluate_fid(g, net, 20, n, DEV, path, streaming=True, method='eigh'), 5)
    say('| `evaluate_fid`, %d images of %d x %d in batches of 20, F = 2048, real side of 1 336 images | seconds: median (min .. max) of %d runs after a warm-up run |'
        % (n, SIZE, SIZE, REPS))
    say('|---|---|')
    say('| default call (features to the host per batch, `np.cov`, `sqrtm`) | %s |' % sec(t_default))
    say("| `streaming=True, method='eigh'` | %s |" % sec(t_streaming))
    say('| generator + Inception alone, features left on the device | %s |' % sec(t_gen))
    say("| generator + Inception + per-batch `f.to('cpu')` | %s |" % sec(t_gen_host))
    say('| generator + Inception + per-batch `append` (`sample_statistics`) | %s |' % sec(t_stream))
    say('| host statistics: widening + `np.cov` of %d x 2048 | %s |' % (n, sec(t_np)))
    say('| device statistics: finish + the one copy of mean and covariance | %s |' % sec(t_finish))
    say('| distance at F = 2048, `frechet_distance` (sqrtm) | %s |' % sec(t_sqrtm))
    say('| distance at F = 2048, `frechet_distance_eigh` | %s |' % sec(t_eigh))
    say()
    say('values: default %.9g, streaming + eigh %.9g; on the same host statistics sqrtm %.9g, eigh %.9g; eigh on the streamed statistics %.9g'
        % (v_default, v_stream, d_sqrtm, d_eigh, d_stream))
    say('host threads: %d' % torch.get_num_threads())


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'feature_stats_bench.py measures on a GPU'
    torch.set_num_threads(min(16, torch.get_num_threads()))
    say('device: %s' % torch.cuda.get_device_name(0))
    say()
    append_table()
    say()
    big_table()
    if '--kernels-only' not in sys.argv:
        say()
        fid_table()
