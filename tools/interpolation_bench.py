#!/usr/bin/env python3
"""The tables of profiles/interpolation.md: the blends of group interpolation as ATen expressions (the ``*_reference`` functions of
models/op/interp.py on device tensors) against the kernels of csrc/interp.hip, and a whole Inference.interpolate_by_group call against the
same film composed as the reference composes it from the building blocks the project had before (``baseline_film`` below: per frame three
slice-wise blends, two cats, a blend per noise map, two generator calls on z, two grid images).  On one GPU, the legs alternating in one process.

    python tools/interpolation_bench.py [size of the whole-call case, default 512] [file to write the tables to as well] [blends: stop before the whole call]

Per case and path: host issue time per call (a loop without a synchronise), wall time per call (the same loop up to the final synchronise) and
the device span of one call (events around single calls, median); three alternations, medians, and the spread (max / min) of the wall times."""
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'gan-control_amd'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)

import inference_checks as ic          # noqa: E402
from gan_control_amd.evaluation.generation import _make_noise, _randn          # noqa: E402
from gan_control_amd.evaluation.image_grid import grid_image          # noqa: E402
from gan_control_amd.inference import Inference          # noqa: E402
from gan_control_amd.models.op import interp          # noqa: E402

OUT = sys.argv[2] if __name__ == '__main__' and len(sys.argv) > 2 else None
HBM_TBS = 6.29          # MI355X, measured float4 copy
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def measure(fn, reps):
    """(host issue us, wall us per call, device span us of one call: median of events around single calls)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    spans = []
    for _ in range(min(reps, 30)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        spans.append(a.elapsed_time(b) * 1e3)
    return (t1 - t0) / reps * 1e6, (t2 - t0) / reps * 1e6, statistics.median(spans)


def ab(name, aten_fn, kernel_fn, reps, note=lambda k: ''):
    rows = {'aten': [], 'kernel': []}
    for _ in range(3):
        rows['aten'].append(measure(aten_fn, reps))
        rows['kernel'].append(measure(kernel_fn, reps))
    med = {k: [statistics.median(r[i] for r in v) for i in range(3)] for k, v in rows.items()}
    spread = {k: max(r[1] for r in v) / min(r[1] for r in v) for k, v in rows.items()}
    m, k = med['aten'], med['kernel']
    say('| %s | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.2f | %.2f / %.2f | %s |'
        % (name, m[0], m[1], m[2], k[0], k[1], k[2], m[1] / k[1], spread['aten'], spread['kernel'], note(k)))


def noise_list(size, batch):
    log = int(np.log2(size))
    shapes = [(batch, 1, 4, 4)] + [(batch, 1, 2 ** i, 2 ** i) for i in range(3, log + 1) for _ in range(2)]
    return [torch.randn(*s, device='cuda') for s in shapes], [torch.randn(*s, device='cuda') for s in shapes]


@torch.no_grad()
def baseline_film(inf, group, batch, segments, pics, interpolation, downsample=None):
    """interpolate_by_group as the reference composes it (evaluation/inference_class.py:125-185), from what the project had before."""
    noise = [n.expand(batch, -1, -1, -1).clone() for n in _make_noise(inf.model, inf.device, None)]
    lo, hi = inf.batch_utils.place_in_latent_dict[group]
    latent_1 = _randn((1, 512), inf.device, None).expand(batch, -1)
    latent_2 = [_randn((batch, 512), inf.device, None) for _ in range(segments)]
    noise_2 = [[n.clone() for n in noise] for _ in range(segments)]
    z1s, z1e, z1g = latent_1[:, :lo], latent_1[:, hi:], latent_1[:, lo:hi]
    noise1 = noise
    films = ([], [])
    for z2, noise2 in zip(latent_2, noise_2):
        for _, p in zip(range(pics), np.linspace(0, 1, pics)):
            frame_noise = [(1 - p) * noise1[i] + p * noise2[i] for i in range(len(noise1))]
            if interpolation == 'linear':
                start, end, grp = (1 - p) * z1s + p * z2[:, :lo], (1 - p) * z1e + p * z2[:, hi:], (1 - p) * z1g + p * z2[:, lo:hi]
            else:
                start, end, grp = Inference.slerp(p, z1s, z2[:, :lo]), Inference.slerp(p, z1e, z2[:, hi:]), Inference.slerp(p, z1g, z2[:, lo:hi])
            for film, z in enumerate((torch.cat([start, latent_1[:, lo:hi], end], dim=1), torch.cat([latent_1[:, :lo], grp, latent_1[:, hi:]], dim=1))):
                sample, _ = inf.model([z], noise=frame_noise)
                films[film].append(grid_image(sample, nrow=batch, downsample=downsample))
        z1s, z1e, z1g = z2[:, :lo], z2[:, hi:], z2[:, lo:hi]
        noise1 = noise2
    return films


def main():
    if not torch.cuda.is_available():
        sys.exit('tools/interpolation_bench.py measures on a GPU')
    torch.manual_seed(0)
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    say('%s' % torch.cuda.get_device_name(0))
    say('')
    say('| case | ATen: host issue us | ATen: wall us / call | ATen: device span us | kernel: host issue us | kernel: wall us / call | kernel: device span us | wall ATen / kernel | spread (max / min wall) ATen / kernel | note |')
    say('|---|---|---|---|---|---|---|---|---|---|')
    with torch.no_grad():
        # one segment's latents: L = 512, batch 4, P = 10, the age group
        fixed = torch.randn(1, 512, device='cuda').expand(4, -1)
        z1, z2 = torch.randn(4, 512, device='cuda'), torch.randn(4, 512, device='cuda')
        for mode in ('slerp', 'linear'):
            for pics in (10, 64):
                wa, wb = interp.interpolation_weights(pics, mode)
                ab('latents %s, B = 4, P = %d' % (mode, pics), lambda: interp.interpolate_latents_reference(fixed, z1, z2, 320, 384, wa, wb, mode),
                   lambda: interp.interpolate_latents(fixed, z1, z2, 320, 384, wa, wb, mode), 100 if pics == 10 else 30)
        # one frame's noise blend
        for gsize, batch in ((32, 1), (32, 4), (512, 4), (1024, 1), (1024, 4), (1024, 16)):
            a, b = noise_list(gsize, batch)
            out = [torch.empty_like(x) for x in a]
            nbytes = 3 * 4 * sum(x.numel() for x in a)
            ab('noise blend, %d^2 generator (%d maps), B = %d' % (gsize, len(a), batch), lambda: interp.blend_noise_reference(a, b, 0.3, 0.7),
               lambda: interp.blend_noise(a, b, 0.3, 0.7, out=out), 200 if gsize < 512 else 50,
               note=lambda k: '%.1f MB moved, %.2f TB/s over the wall time of back-to-back calls = %.0f %% of %.2f TB/s%s'
               % (nbytes / 1e6, nbytes / k[1] / 1e6, 100 * nbytes / k[1] / 1e6 / HBM_TBS, HBM_TBS, ' (host-bound: a lower limit)' if k[0] > 0.9 * k[1] else ''))
    if len(sys.argv) > 3 and sys.argv[3] == 'blends':
        return
    # the whole call
    root = tempfile.mkdtemp()
    ic.write_model_dir(root, ic.ffhq_config(size))
    inf = Inference(root)
    for mode in ('slerp', 'linear'):
        ab('interpolate_by_group %d^2, defaults (B = 4, 4 x 10 frames), %s, images in memory' % (size, mode),
           lambda: baseline_film(inf, 'age', 4, 4, 10, mode),
           lambda: film_in_memory(inf, root, mode), 2)


def film_in_memory(inf, root, mode):
    """interpolate_by_group with its PIL frames built and no file written: what baseline_film returns."""
    keep = inf.make_interpolation_gif
    inf.make_interpolation_gif = lambda *a, **k: None
    try:
        return inf.interpolate_by_group('age', os.path.join(root, 'film'), interpolation=mode)
    finally:
        inf.make_interpolation_gif = keep


if __name__ == '__main__':
    main()
