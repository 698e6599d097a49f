#!/usr/bin/env python3
"""The tables of profiles/controller_training.md: one controller training step as ``ControllerTrainer.controller_update`` (the module path:
what the parent of this feature ran) against ``controller_update_fused`` (models/op/fc_train.py), on the same device-resident batches, and one
epoch of ``datasets.DeviceFrame.epoch`` against the ``DataLoader`` over the same frame, on one GPU.

    python tools/controller_training_bench.py [file to write the tables to as well]

Per case and path: host issue time (a loop of steps without a synchronise, per step) and wall time per step (the same loop up to the final
synchronise), each window at least 0.6 s long.  The module path reads its loss three times per step, so its two columns nearly coincide.  The two paths alternate three times
in one process; the medians are printed, and the spread of the wall times (max / min over the three rounds).  Both paths really step their own
copy of the same network, so the parameters move while the loop runs, as in training."""
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'gan-control_amd')):
    sys.path.insert(0, p)

from gan_control_amd.datasets import DeviceFrame, get_dataframe_data_loader          # noqa: E402
from gan_control_amd.models.op import fc_train          # noqa: E402
from gan_control_amd.trainers.controller_trainer import ControllerTrainer, default_controller_config          # noqa: E402

OUT = sys.argv[1] if __name__ == '__main__' and len(sys.argv) > 1 else None
lines = []
LATENT = 640          # wider than the widest slice (512 columns from column 64 on)


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, 'w') as f:
            f.write('\n'.join(lines) + '\n')


WINDOW = 0.6          # seconds per timed window: long enough that the clock and the scheduler do not show


def measure(fn, reps=None):
    """(host issue us, wall us) per call, over a window of at least WINDOW seconds (sized from 20 synchronised warm-up calls)"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    reps = max(200, int(WINDOW / ((time.perf_counter() - t0) / 20)) + 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) / reps * 1e6, (t2 - t0) / reps * 1e6


def ab(name, module_fn, fused_fn):
    """alternate the two versions three times; the median of each column"""
    rows = {'module': [], 'fused': []}
    for _ in range(3):
        rows['module'].append(measure(module_fn))
        rows['fused'].append(measure(fused_fn))
    med = {k: [statistics.median(r[i] for r in v) for i in range(2)] for k, v in rows.items()}
    spread = {k: max(r[1] for r in v) / min(r[1] for r in v) for k, v in rows.items()}
    m, k = med['module'], med['fused']
    say('| %s | %.0f | %.0f | %.0f | %.0f | %.2f | %.2f / %.2f |' % (name, m[0], m[1], k[0], k[1], m[1] / k[1], spread['module'], spread['fused']))


def step_case(in_dim, mid, n_mlp, out, batch):
    chunk = (64, 64 + out)
    gen = torch.Generator().manual_seed(batch + in_dim)
    batches = [(torch.randn(batch, in_dim, generator=gen).cuda(), torch.randn(batch, LATENT, generator=gen).cuda()) for _ in range(8)]
    cfg = default_controller_config(in_dim, mid, n_mlp, batch=batch)
    module, fused = ControllerTrainer(cfg, chunk, device='cuda', seed=1), ControllerTrainer(cfg, chunk, device='cuda', seed=1)
    assert fc_train.fused_step_taken(fused.fc_controller, fused.fc_optim, *batches[0], chunk, fused.rec_loss)
    count = [0, 0]

    def module_step():
        count[0] += 1
        module.controller_update(batches[count[0] % 8])

    def fused_step():
        count[1] += 1
        fused.controller_update_fused(batches[count[1] % 8])

    ab('%d -> %d x %d -> %d, B = %d' % (in_dim, mid, n_mlp - 1, out, batch), module_step, fused_step)


def epoch_case(rows, batch, workers):
    rng = np.random.default_rng(0)
    frame = pd.DataFrame({'latents_w': [rng.standard_normal(LATENT).astype(np.float32) for _ in range(rows)],
                          'orientation': [rng.standard_normal(3).astype(np.float32) for _ in range(rows)]})
    t0 = time.perf_counter()
    dev = DeviceFrame(frame, 'orientation', 'cuda')
    torch.cuda.synchronize()
    build = time.perf_counter() - t0
    loader = get_dataframe_data_loader(frame, 'orientation', batch_size=batch, workers=workers)

    def loader_epoch():
        n = 0
        for c, w in loader:
            c, w = c.cuda().float(), w.cuda()
            n += 1
        torch.cuda.synchronize()
        return n

    def device_epoch():
        n = 0
        for c, w in dev.epoch(batch):
            n += 1
        torch.cuda.synchronize()
        return n

    times = {'loader': [], 'device': []}
    for _ in range(3):
        for key, fn in (('loader', loader_epoch), ('device', device_epoch)):
            t0 = time.perf_counter()
            n = fn()
            times[key].append((time.perf_counter() - t0) / n * 1e6)
    a, b = statistics.median(times['loader']), statistics.median(times['device'])
    say('| %d rows, B = %d, %d workers | %.1f | %.2f | %.0f | %.1f |' % (rows, batch, workers, a, b, a / b, build * 1e3))


def main():
    if not torch.cuda.is_available():
        sys.exit('tools/controller_training_bench.py measures on a GPU')
    say('%s' % torch.cuda.get_device_name(0))
    say('')
    say('| stack, batch | module: host issue us | module: wall us / step | fused: host issue us | fused: wall us / step | wall module / fused | spread (max / min wall) module / fused |')
    say('|---|---|---|---|---|---|---|')
    step_case(3, 256, 8, 512, 32)          # the reference configuration's shape
    for in_dim in (1, 27, 64):
        for out in (40, 512):
            for batch in (8, 32, 64):
                step_case(in_dim, 512, 4, out, batch)
    say('')
    say('| frame | DataLoader: us / batch (to the device) | DeviceFrame.epoch: us / batch | ratio | DeviceFrame built in ms |')
    say('|---|---|---|---|---|')
    epoch_case(4000, 32, 0)
    epoch_case(4000, 32, 4)


if __name__ == '__main__':
    main()
