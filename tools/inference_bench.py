#!/usr/bin/env python3
"""The table of profiles/inference.md: the w-space part of an inference call on the module path (Generator.style / FcStack, what the parent of
this feature launched) against the fused calls of models/op/fc_stack.py, on one GPU.

    python tools/inference_bench.py [size, default 512] [file to write the table to as well]

Per case and path: host issue time (a loop of calls without a synchronise, per call), wall time per call (the same loop up to the final
synchronise) and the device span of one call (events around single calls, median).  The two paths alternate three times in one process; the
medians are printed, and the spread of the wall times (max / min over the three rounds).  The dispatch limits of fc_stack.py are lifted: the
table is what they are set from.  Model and controller directories are generated from seeds into a temporary directory."""
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'gan-control_amd'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)

import inference_checks as ic          # noqa: E402
from gan_control_amd.inference import Controller          # noqa: E402
from gan_control_amd.models.op import fc_stack as fcs          # noqa: E402

OUT = sys.argv[2] if __name__ == '__main__' and len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def measure(fn, reps):
    """(host issue us, wall us per call, device span us of one call: median of events around single calls)"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    spans = []
    for _ in range(min(reps, 50)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        spans.append(a.elapsed_time(b) * 1e3)
    return (t1 - t0) / reps * 1e6, (t2 - t0) / reps * 1e6, statistics.median(spans)


def ab(name, module_fn, kernel_fn, reps):
    """alternate the two versions three times; the median of each column"""
    rows = {'module': [], 'kernel': []}
    for _ in range(3):
        rows['module'].append(measure(module_fn, reps))
        rows['kernel'].append(measure(kernel_fn, reps))
    med = {k: [statistics.median(r[i] for r in v) for i in range(3)] for k, v in rows.items()}
    spread = {k: max(r[1] for r in v) / min(r[1] for r in v) for k, v in rows.items()}
    m, k = med['module'], med['kernel']
    say('| %s | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.2f | %.2f / %.2f |' % (name, m[0], m[1], m[2], k[0], k[1], k[2], m[1] / k[1], spread['module'], spread['kernel']))


def main():
    if not torch.cuda.is_available():
        sys.exit('tools/inference_bench.py measures on a GPU')
    torch.manual_seed(0)
    root = tempfile.mkdtemp()
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    cfg = ic.ffhq_config(size)
    ic.write_model_dir(os.path.join(root, 'generator'), cfg)
    places = {k: v['place_in_latent'] for k, v in cfg['training_config']['sub_groups_dict'].items()}
    for i, name in enumerate(('orientation', 'age', 'gamma', 'expression_q')):
        lo, hi = places['expression' if name == 'expression_q' else name]
        ic.write_controller(root, name + '_run', ic.CONTROLS[name], hi - lo, 50 + i)
    ctl = Controller(root)
    fcs.KERNEL_MAX_BATCH = fcs.KERNEL_WIDE_MAX_BATCH = 1 << 30          # the rule is what this table decides
    style = ctl.model.style
    say('size %d, %s' % (size, torch.cuda.get_device_name(0)))
    say('')
    say('| case | module: host issue us | module: wall us / call | module: device span us | kernel: host issue us | kernel: wall us / call | kernel: device span us | wall module / kernel | spread (max / min wall) module / kernel |')
    say('|---|---|---|---|---|---|---|---|---|')
    with torch.no_grad():
        for batch in (1, 8, 64, 256, 1000, 4000):
            z = torch.randn(batch, 512, device='cuda')
            ab('split x7, B = %d' % batch, lambda: style(z), lambda: ctl.style(z), 300 if batch <= 64 else 100)
        from gan_control_amd.models.gan_model import Generator
        vanilla = Generator.create_fc_stack(0.01, 8, 512).cuda()
        for batch in (1, 8, 64, 256, 1000):
            z = torch.randn(batch, 512, device='cuda')
            out = torch.empty(batch, 512, device='cuda')
            ab('vanilla 512 x 8, B = %d' % batch, lambda: vanilla(z), lambda: fcs.fc_stacks_forward([vanilla], z, None, out, None), 300 if batch <= 64 else 100)
        names = ('orientation', 'age', 'gamma', 'expression_q')
        nets = [ctl.fc_controls[n] for n in names]
        slices = [tuple(places['expression' if n == 'expression_q' else n]) for n in names]
        for batch in (1, 8):
            xs = [torch.randn(batch, ic.CONTROLS[n], device='cuda') for n in names]
            w = torch.randn(batch, 512, device='cuda')

            def module_path():
                for net, x, (lo, hi) in zip(nets, xs, slices):
                    w[:, lo:hi] = net(x)

            ab('controllers x4, B = %d' % batch, module_path, lambda: fcs.fc_stacks_forward(nets, xs, None, w, slices), 300)
        # end to end, batch 1
        z = torch.randn(1, 512, device='cuda')
        controls = {'orientation': torch.randn(1, 3), 'age': torch.rand(1, 1) * 60, 'gamma': torch.randn(1, 27), 'expression': torch.eye(8)[:1]}
        controls = {k: v.cuda() for k, v in controls.items()}

        def e2e(max_batch):
            def run():
                fcs.KERNEL_MAX_BATCH = max_batch
                ctl.gen_batch_by_controls(latent=z, normalize=False, **controls)
            return run

        ab('gen_batch_by_controls %d^2, B = 1, 4 controls' % size, e2e(0), e2e(1 << 30), 50)


if __name__ == '__main__':
    main()
