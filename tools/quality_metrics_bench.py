#!/usr/bin/env python3
"""The tables of profiles/quality_metrics.md: improved precision / recall and KID on the kernel path of models/op/manifold.py
(gc_knn_radius_f32, gc_manifold_hits_f32, gc_poly_mmd_f32) against its torch path -- the documented formula in chunks, on ATen -- on one GPU.

    python tools/quality_metrics_bench.py [file to write the tables to as well] [--quick]

Shapes: precision / recall of N real against N generated rows of F = 2048 features (the Inception pool) at N = 1000, 10000 and 50000, k = 3:
two radius passes and one hit pass; KID at its defaults (100 subsets of 1000 rows out of N = 10000 a side).  Every call is timed on its own
between two device events after a warm-up; the two paths alternate (three rounds where a round takes under a second, one where the torch
path alone takes minutes: no spread is printed there, and the torch path runs without a warm-up call from N = 10000 on) and the median
over all samples is printed with max / min of the per-round medians.  A span is a whole operator call: both launches, the allocation of
the outputs and the workspace and, for KID, the index check and upload -- not kernel time.  The radii and hit vectors of the timed calls
of both paths are compared at every shape.  pair-elements / s = m n F / span; the ceiling is the derived 39.3 T pair-elements / s (a subtraction and a fused multiply-add per pair-element at the
157.3 TF/s fp32 vector peak = 78.6 T lane-operations / s); the KID kernel issues one fused multiply-add per pair-element: 78.6 T / s.
Inputs come from a seed (rows near a low-dimensional subspace, as the tests'); nothing outside the repository is read.
"""
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'gan-control_amd')):
    sys.path.insert(0, p)

from gan_control_amd.fid_utils import kid as kid_module          # noqa: E402
from gan_control_amd.models.op import manifold as mf          # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
QUICK = '--quick' in sys.argv
OUT = ARGS[0] if ARGS else None
LANE_OPS = 157.3e12 / 2          # vector lane-operations per second
DEV = 'cuda'
U = 2.0 ** -24
F = 2048
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
        out.append(a.elapsed_time(b))
    return out


def ab(kernel_fn, torch_fn, rounds, reps_k, reps_t, warm_t=1):
    """-> (kernel ms, torch ms, spread kernel, spread torch): medians over alternating rounds"""
    got = {'k': [], 't': []}
    for r in range(rounds):
        got['k'].append(spans(kernel_fn, 2 if r == 0 else 1, reps_k))
        got['t'].append(spans(torch_fn, warm_t if r == 0 else 0, reps_t))
    med = {k: statistics.median(x for r in v for x in r) for k, v in got.items()}
    spread = {k: max(statistics.median(r) for r in v) / min(statistics.median(r) for r in v) for k, v in got.items()}
    return med['k'], med['t'], spread['k'], spread['t']


def feature_set(seed, n, scale, shift):
    p = torch.randn(16, F, generator=torch.Generator(device=DEV).manual_seed(1234), device=DEV)          # one subspace for every set
    gen = torch.Generator(device=DEV).manual_seed(seed)
    latent = torch.randn(n, 16, generator=gen, device=DEV) * scale + shift
    return latent @ p / 4.0 + 0.05 * torch.randn(n, F, generator=gen, device=DEV)


def spread_text(rounds, sk, st):
    return '%.2f / %.2f' % (sk, st) if rounds > 1 else '- (one round)'


def precision_recall_table():
    say('| N real x N generated, F = 2048 | pass | kernel ms | torch path ms | ratio | T pair-elements / s | call span over the 39.3 T/s ceiling | spread kernel / torch |')
    say('|---|---|---|---|---|---|---|---|')
    agreement = []
    for n in ((1000, 10000) if QUICK else (1000, 10000, 50000)):
        real, fake = feature_set(1, n, 1.0, 0.0), feature_set(2, n, 0.8, 0.4)
        assert mf.kernel_taken(real, fake)
        small = n <= 1000
        rounds, reps_k, reps_t, warm_t = (3, 20, 5, 1) if small else (3, 5, 1, 0) if n <= 10000 else (1, 3, 1, 0)
        work = float(n) * n * F
        kept = {}          # the results of the timed calls themselves: what was timed is what is compared

        def keep(name, fn):
            def call():
                kept[name] = fn()
            return call

        with torch.no_grad():
            rr, fr = mf.knn_radii(real), mf.knn_radii(fake)
            total_k = total_t = 0.0
            for name, kf, tf, passes in (('radii (two sets)', keep('rk', lambda: (mf.knn_radii(real), mf.knn_radii(fake))),
                                          keep('rt', lambda: (mf.knn_radii_torch(real), mf.knn_radii_torch(fake))), 2),
                                         ('hits (both directions)', keep('hk', lambda: mf.manifold_hits(real, rr, fake, fr)),
                                          keep('ht', lambda: mf.manifold_hits_torch(real, rr, fake, fr)), 1)):
                tk, tt, sk, st = ab(kf, tf, rounds, reps_k, reps_t, warm_t)
                rate = passes * work / (tk * 1e-3)
                total_k, total_t = total_k + tk, total_t + tt
                say('| %d x %d | %s | %.2f | %.1f | %.1f x | %.2f | %.1f %% | %s |'
                    % (n, n, name, tk, tt, tt / tk, rate / 1e12, 100 * rate / (LANE_OPS / 2), spread_text(rounds, sk, st)))
            p_hit, r_hit = kept['hk']
            say('| %d x %d | precision / recall (the three passes) | %.2f | %.1f | %.1f x | | | precision %.3f, recall %.3f |'
                % (n, n, total_k, total_t, total_t / total_k, float(p_hit.double().mean()), float(r_hit.double().mean())))
            # both paths carry (F + 4) u per radius, so they are within 2 (F + 4) u of each other; a hit decision may differ only where a
            # distance lies within that band of its radius
            rel = max(float(((a.double() - b.double()).abs() / b.double()).max()) for a, b in zip(kept['rk'], kept['rt']))
            assert rel <= 2 * (F + 4) * U, rel
            differ = [int((a != b).sum()) for a, b in zip(kept['hk'], kept['ht'])]
            agreement.append('| %d x %d | %.2e | %.2e | %d of %d | %d of %d | %.3f / %.3f | %.3f / %.3f |'
                             % (n, n, rel, 2 * (F + 4) * U, differ[0], n, differ[1], n, float(p_hit.double().mean()), float(kept['ht'][0].double().mean()),
                                float(r_hit.double().mean()), float(kept['ht'][1].double().mean())))
        del real, fake, kept
        torch.cuda.empty_cache()
    say()
    say('| kernel path against torch path, the timed calls | radii: max relative difference | bound 2 (F + 4) u | probe_hit decisions that differ | ref_hit decisions that differ | precision kernel / torch | recall kernel / torch |')
    say('|---|---|---|---|---|---|---|')
    for line in agreement:
        say(line)


def kid_table():
    say('| KID, F = 2048 | kernel ms | torch path ms | ratio | T pair-elements / s | call span over the 78.6 T/s ceiling | spread kernel / torch | value kernel / torch |')
    say('|---|---|---|---|---|---|---|---|')
    n = 10000
    real, fake = feature_set(1, n, 1.0, 0.0).abs(), feature_set(2, n, 0.8, 0.4).abs()
    for subsets, m in ((100, 1000), (10, 1000)) if not QUICK else ((10, 1000),):
        idx_x, idx_y = kid_module.subset_indices(n, n, subsets, m, 0)
        dx, dy = torch.from_numpy(idx_x).to(DEV), torch.from_numpy(idx_y).to(DEV)
        with torch.no_grad():
            tk, tt, sk, st = ab(lambda: mf.poly_mmd_sums(fake, real, idx_x, idx_y), lambda: mf.poly_mmd_sums_torch(fake, real, dx, dy), 3, 5, 2)
            vk = kid_module.kid_from_sums(mf.poly_mmd_sums(fake, real, idx_x, idx_y), m)
            vt = kid_module.kid_from_sums(mf.poly_mmd_sums_torch(fake, real, dx, dy), m)
        rate = 3.0 * subsets * m * m * F / (tk * 1e-3)
        say('| %d subsets of %d rows%s | %.2f | %.1f | %.1f x | %.2f | %.1f %% | %.2f / %.2f | %.6g / %.6g |'
            % (subsets, m, ' (the defaults)' if subsets == 100 else '', tk, tt, tt / tk, rate / 1e12, 100 * rate / LANE_OPS, sk, st, vk, vt))


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'quality_metrics_bench.py measures on a GPU'
    say('device: %s' % torch.cuda.get_device_name(0))
    say()
    kid_table()
    say()
    precision_recall_table()
