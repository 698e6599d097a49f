#!/usr/bin/env python3
"""The tables of profiles/pca_groups.md: per-group latent PCA on one GPU, every kernel against its torch formula on the same device.

    python tools/pca_bench.py [file to write the tables to as well] [--quick]

1. ``group_moments`` (gc_group_moments_f32: two launches) against ``moments_reference`` on the device (per-group float64 two-pass covariance
   by ATen) at N = 10 000 for the FFHQ layout (128 + 6 x 64), the AFHQ layout (192, 192, 128) and one 512-wide group, and at N = 700.
2. A whole ``get_pca_groups`` call on a split (FFHQ layout) and a vanilla 8-layer mapping network (N = 10 000, n_mlp 8, random weights), with
   the host ``eigh`` share timed on its own; the reference's host route -- the latents copied to the host and a float32 scikit-learn ``PCA``
   per group -- where scikit-learn is installed (the table says so where it is not).
3. ``group_project_`` (gc_group_project_f32: one launch) against ``project_reference_`` (the float32 expression on ATen) at 1 row and 18 rows
   (one w_plus latent), FFHQ layout and one 512-wide group, with the ranks a fit at variance_percent 0.5 keeps.
4. One ``project`` step on the ``--size`` (default 256) split generator with and without ``pca``: device events at every ``on_step``
   call of one ``project`` run (tools/projection_bench.py's method: alternating variants, medians and min - max spread).

Kernel / formula timings: device events around one call after a warm-up; the two paths alternate three times in one process and the median
over all samples is printed, with max / min of the three per-round medians.  Host timings: time.perf_counter around a synchronised call.
Inputs come from seeds; nothing outside the repository is read.
"""
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'gan-control_amd')):
    sys.path.insert(0, p)

from gan_control_amd import projection          # noqa: E402
from gan_control_amd.inference import Inference          # noqa: E402
from gan_control_amd.models.gan_model import Generator          # noqa: E402
from gan_control_amd.models.op import group_pca as gp          # noqa: E402
from gan_control_amd.projection.pca import GroupPCA, get_pca_groups          # noqa: E402
from gan_control_amd.utils.fc_config import FcConfig          # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
QUICK = '--quick' in sys.argv
SIZE = int(next((a.split('=')[1] for a in sys.argv if a.startswith('--size=')), 256))
OUT = ARGS[0] if ARGS else None
DEV = 'cuda'
FFHQ = {'id': (0, 128), 'expression': (128, 192), 'orientation': (192, 256), 'gamma': (256, 320), 'age': (320, 384), 'hair': (384, 448),
        'other': (448, 512)}
AFHQ = {'id': (0, 192), 'orientation': (192, 384), 'other': (384, 512)}
VANILLA = {None: (0, 512)}
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


def ab(kernel_fn, torch_fn, reps):
    """-> (kernel us, torch us, spread kernel, spread torch): medians over three alternating rounds"""
    rounds = {'k': [], 't': []}
    for r in range(3):
        rounds['k'].append(spans(kernel_fn, 3 if r == 0 else 1, reps))
        rounds['t'].append(spans(torch_fn, 3 if r == 0 else 1, reps))
    med = {k: statistics.median(x for r in v for x in r) for k, v in rounds.items()}
    spread = {k: max(statistics.median(r) for r in v) / min(statistics.median(r) for r in v) for k, v in rounds.items()}
    return med['k'], med['t'], spread['k'], spread['t']


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def latents(n, seed):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n, 512, generator=gen)
    return (torch.nn.functional.leaky_relu(z @ (torch.randn(512, 512, generator=gen) / 22.6), 0.2) + 0.3).to(DEV)


def moments_table():
    say('| layout | N | kernel us | torch formula us | ratio | GFLOP (fp64, upper tiles) | spread kernel / torch |')
    say('|---|---|---|---|---|---|---|')
    for n in ((10000, 700) if not QUICK else (10000,)):
        w = latents(n, 0)
        for name, places in (('FFHQ 128 + 6 x 64', FFHQ), ('AFHQ 192, 192, 128', AFHQ), ('vanilla 512', VANILLA)):
            assert gp.kernel_taken(w, places)
            with torch.no_grad():
                tk, tt, sk, st = ab(lambda: gp.group_moments_packed(w, places), lambda: gp.moments_reference(w, places), 20)
            flop = sum(2.0 * n * (hi - lo) * (hi - lo + 1) / 2 for lo, hi in places.values()) / 1e9
            say('| %s | %d | %.1f | %.1f | %.2f x | %.2f | %.2f / %.2f |' % (name, n, tk, tt, tt / tk, flop, sk, st))


def mapping(split):
    fc = FcConfig(list(FFHQ), {k: {'latent_place': list(v), 'latent_size': v[1] - v[0]} for k, v in FFHQ.items()}) if split else None
    torch.manual_seed(0)
    g = Generator(SIZE, 512, 8, channel_multiplier=2, conv_transpose=True, split_fc=split, fc_config=fc).to(DEV).eval()
    inf = Inference.__new__(Inference)          # the generation API on a model that was never saved: style() and _places() need these two
    inf.model = g
    inf.batch_utils = types.SimpleNamespace(place_in_latent_dict=FFHQ) if split else None
    return inf


def whole_call_table():
    try:
        from sklearn.decomposition import PCA
    except ImportError:
        PCA = None
    say('| mapping network | N | get_pca_groups ms | of which host eigh ms | reference host route ms (float32 scikit-learn) | sampling w ms |')
    say('|---|---|---|---|---|---|')
    n = 10000
    for name, split in (('split, FFHQ layout', True), ('vanilla 512', False)):
        inf = mapping(split)
        places = inf._places()
        gen = torch.Generator().manual_seed(1)
        call = lambda: get_pca_groups(inf, torch.zeros(512), n, DEV, generator=torch.Generator().manual_seed(1))          # noqa: E731
        call()
        whole = host_ms(call, 3 if QUICK else 5)
        with torch.no_grad():
            from gan_control_amd.projection.pca import _sample_w
            sample = host_ms(lambda: _sample_w(inf, inf.model, n, torch.device(DEV), gen), 3)
            w = _sample_w(inf, inf.model, n, torch.device(DEV), gen)
            _, cov = gp.unpack(*gp.group_moments_packed(w, places), places)
            covs = {k: v.cpu().numpy() for k, v in cov.items()}
        eig = host_ms(lambda: [GroupPCA.eig(c) for c in covs.values()], 5)

        def host_route():
            x = w.cpu().numpy()
            for lo, hi in places.values():
                p = PCA()
                p.fit(x[:, lo:hi])
                ev = p.explained_variance_
                np.argmax(np.cumsum(ev) / np.sum(ev) > 0.5)
        ref = ('%.1f' % host_ms(host_route, 3)[0]) if PCA is not None else 'not measured: scikit-learn is not installed'
        say('| %s | %d | %.1f (%.1f - %.1f) | %.1f | %s | %.1f |' % (name, n, whole[0], whole[1], whole[2], eig[0], ref, sample[0]))


def project_table():
    say('| layout (ranks at 0.5) | rows | kernel us | torch expression us | ratio | spread kernel / torch |')
    say('|---|---|---|---|---|---|')
    for name, places in (('FFHQ 128 + 6 x 64', FFHQ), ('vanilla 512', VANILLA)):
        fit = GroupPCA.fit(latents(10000, 2), places)
        ranks = ', '.join(str(fit.components[k].shape[0]) for k in places)
        for rows in (1, 18):
            x = latents(rows, 3)
            y = x.clone()
            assert gp.kernel_taken(x, fit.mean, fit.components, places)
            with torch.no_grad():
                tk, tt, sk, st = ab(lambda: gp.group_project_(x.copy_(y), fit.mean, fit.components, places),
                                    lambda: gp.project_reference_(x.copy_(y), fit.mean, fit.components, places), 100)
                tc, _, _, _ = ab(lambda: x.copy_(y), lambda: x.copy_(y), 100)
            say('| %s (%s) | %d | %.1f | %.1f | %.2f x | %.2f / %.2f |' % (name, ranks, rows, tk - tc, tt - tc, (tt - tc) / max(tk - tc, 1e-3), sk, st))
    say('')
    say('(the copy that restores x before every call, %.1f us, is subtracted from both columns)' % tc)


def step_table():
    say('| generator | variant | us per project step (median, min - max) | steps timed |')
    say('|---|---|---|---|')
    inf = mapping(True)
    g = inf.model
    with torch.no_grad():
        target, _ = g([torch.randn(1, 512, generator=torch.Generator().manual_seed(4)).to(DEV)])
    fit = GroupPCA.fit(g.style(torch.randn(10000, 512, generator=torch.Generator().manual_seed(5)).to(DEV)).detach(), FFHQ)
    steps = 12 if QUICK else 30
    samples = {'without pca': [], 'with pca (GroupPCA, FFHQ layout)': []}
    for _ in range(3):
        for name, kw in (('without pca', {}), ('with pca (GroupPCA, FFHQ layout)', {'pca': fit})):
            events = []

            def on_step(i, info):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                events.append(e)
            projection.project(g, target, steps=steps, lr=0.1, mse_weight=1.0, n_mean_latent=1000, generator=torch.Generator().manual_seed(3),
                               on_step=on_step, **kw)
            torch.cuda.synchronize()
            samples[name] += [a.elapsed_time(b) * 1e3 for a, b in zip(events[4:], events[5:])]
    for name, v in samples.items():
        say('| %d x %d, split | %s | %.0f (%.0f - %.0f) | %d |' % (SIZE, SIZE, name, statistics.median(v), min(v), max(v), len(v)))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('pca_bench: needs a GPU; nothing is measured without one')
    say('device: %s' % torch.cuda.get_device_name(0))
    say('')
    say('### group_moments')
    moments_table()
    say('')
    say('### get_pca_groups, whole call')
    whole_call_table()
    say('')
    say('### group_project_')
    project_table()
    say('')
    say('### one project step')
    step_table()


if __name__ == '__main__':
    main()
