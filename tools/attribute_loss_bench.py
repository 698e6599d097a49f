#!/usr/bin/env python3
"""The tables of profiles/attribute_losses.md: the hinge stage of the attribute losses on the kernel path of models/op/pair_hinge.py
(gc_pair_hinge_fwd_f32 + gc_pair_hinge_bwd_f32) against its torch path -- today's cat / criterion / mask-gather composition on ATen -- on one
GPU, forward plus backward, at mini-batch 16.

    python tools/attribute_loss_bench.py [file to write the tables to as well] [--quick]          the times
    python tools/attribute_loss_bench.py [file] --launches                                         the kernel launches per call, from the profiler

Shapes: the last-layer features of the FFHQ loss set -- 512 (identity, SQ), [3, 66] (orientation), [9, 8] (expression: the nine branches of
ESR-9 x eight emotions), 101 (age), [4, 256, 256] (hair: masked image + mask; the colour means are torch ops on both paths), 257 cut seven
ways (the 3DMM vector) -- each on the rows of its own group of the FFHQ mini-batch layout, one intermediate level of K = 200704
([16, 64, 56, 56] maps under L1Expend's formula), and the whole set in one pass through LossModelClass (fused=True with
calc_mini_batch_loss_rows against fused=False with the slices).  Every call (loss and backward into the features) is timed on its own between
two device events after a warm-up; the two paths alternate three times in one process and the median over all samples is printed, with max /
min of the three per-round medians.  The launch counts come from torch.profiler in a run of their own (--launches): tracing slows the host.
Inputs come from a seed; nothing outside the repository is read.
"""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'gan-control_amd')):
    sys.path.insert(0, p)

from gan_control_amd.losses import LossModelClass          # noqa: E402
from gan_control_amd.losses.loss_model import RECON_SLICES          # noqa: E402
from gan_control_amd.models.op import pair_hinge as ph          # noqa: E402
from gan_control_amd.utils.mini_batch_utils import MiniBatchUtils          # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
QUICK, LAUNCHES = '--quick' in sys.argv, '--launches' in sys.argv
OUT = ARGS[0] if ARGS else None
DEV = 'cuda'
MINI = 16
lines = []

# the FFHQ mini-batch layout (configs/ffhq.json: sub_groups_dict)
GROUPS = {'id': ([0, 128], [0, 4]), 'expression': ([128, 192], [4, 6]), 'orientation': ([192, 256], [6, 8]), 'gamma': ([256, 320], [8, 10]),
          'age': ([320, 384], [10, 12]), 'hair': ([384, 448], [12, 14]), 'other': ([448, 512], [14, 16])}
# loss name -> (last-layer row shape, same group, (lower, upper) so that both hinges are active on unit-variance features)
LOSSES = {'embedding_loss': ((512,), 'id', (900.0, 1100.0)), 'orientation_loss': ((3, 66), 'orientation', (1.0, 1.2)),
          'expression_loss': ((9, 8), 'expression', (1.0, 1.2)), 'age_loss': ((101,), 'age', (1.0, 1.2)), 'hair_loss': ((4, 256, 256), 'hair', (0.005, 0.02))}
RECON_GROUPS = {'id': 'id', 'ex': 'expression', 'tex': 'id', 'angles': 'orientation', 'gamma': 'gamma', 'xy': 'orientation', 'z': 'orientation'}


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


def ab(fused_fn, torch_fn, reps):
    """-> (fused us, torch us, spread fused, spread torch): medians over three alternating rounds"""
    rounds = {'f': [], 't': []}
    for r in range(3):
        rounds['f'].append(spans(fused_fn, 5 if r == 0 else 1, reps))
        rounds['t'].append(spans(torch_fn, 5 if r == 0 else 1, reps))
    med = {k: statistics.median(x for r in v for x in r) for k, v in rounds.items()}
    spread = {k: max(statistics.median(r) for r in v) / min(statistics.median(r) for r in v) for k, v in rounds.items()}
    return med['f'], med['t'], spread['f'], spread['t']


def launches(fn):
    """Device kernels one call starts, counted by the profiler (the call has run before: nothing is loaded or tuned inside the window)."""
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
    return len(kernels)


def batch_utils():
    groups = {n: {'place_in_latent': lat, 'place_in_mini_batch': rows} for n, (lat, rows) in GROUPS.items()}
    return MiniBatchUtils(MINI, groups, total_batch=MINI)


def level_cfg(lower, upper, levels=1):
    return {'lower_thres': [lower] * (levels - 1), 'upper_thres': [upper] * (levels - 1), 'last_lower_thres': lower, 'last_upper_thres': upper,
            'intermediate_layers_weights': [1.0] * (levels - 1), 'last_layer_weight': 1.0, 'focus_on_list': ['same_as_last_layer'] * levels}


def hair_features(gen):
    mask = (torch.rand(MINI, 1, 256, 256, generator=gen) > 0.6).float()
    return torch.cat([(torch.rand(MINI, 3, 256, 256, generator=gen) * 2 - 1) * mask, mask], dim=1)


def cases(gen):
    """name -> (LossModelClass arguments, feature list builder, group)"""
    out = []
    for name, (shape, group, (lower, upper)) in LOSSES.items():
        feats = hair_features(gen) if name == 'hair_loss' else torch.randn(MINI, *shape, generator=gen)
        out.append((name, '%s' % (list(shape),), name, level_cfg(lower, upper), [feats.to(DEV)], group))
    vec = torch.randn(MINI, 257, generator=gen).to(DEV)
    for x, lo, hi in RECON_SLICES:
        out.append(('recon_%s_loss' % x, '257[%d:%d]' % (lo, hi), 'recon_%s_loss' % x, level_cfg(1.0, 1.2), [vec[:, lo:hi]], RECON_GROUPS[x]))
    if not QUICK:
        maps = torch.randn(MINI, 64, 56, 56, generator=gen).to(DEV)
        # an intermediate level alone: the last level gets weight zero and a one-value row
        cfg = dict(level_cfg(1.0, 1.2, levels=2), last_layer_weight=0.0)
        out.append(('intermediate level (L1Expend)', '[64, 56, 56] = 200704', 'age_loss', cfg, [maps, torch.randn(MINI, 1, generator=gen).to(DEV)], 'id'))
    return out


def paths(loss_name, cfg, feats, group, utils):
    """(fused call, torch call): loss and backward into the features' leaves, as the trainer runs them."""
    leaves = [f.clone().requires_grad_(True) if f.is_contiguous() else f.detach().requires_grad_(True) for f in feats]
    fused = LossModelClass(cfg, loss_name, mini_batch_size=MINI, no_model=True, fused=True)
    plain = LossModelClass(cfg, loss_name, mini_batch_size=MINI, no_model=True)
    rows, n_same, n_not_same = utils.same_not_same_rows(group)

    def fused_fn():
        for leaf in leaves:
            leaf.grad = None
        fused.calc_mini_batch_loss_rows(leaves, rows, n_same, n_not_same).backward()

    def torch_fn():
        for leaf in leaves:
            leaf.grad = None
        same, other = utils.extract_same_not_same_from_list(leaves, group)
        plain.calc_mini_batch_loss(last_layer_same_features=same, last_layer_not_same_features=other).backward()

    return fused_fn, torch_fn, leaves


def agree(fused_fn, torch_fn, leaves):
    """The two paths on the same inputs: the largest gradient difference relative to the largest gradient."""
    fused_fn()
    a = [leaf.grad.clone() for leaf in leaves if leaf.grad is not None]
    torch_fn()
    b = [leaf.grad.clone() for leaf in leaves if leaf.grad is not None]
    return max(float((x - y).abs().max()) / max(float(y.abs().max()), 1e-30) for x, y in zip(a, b))


def main():
    assert torch.cuda.is_available(), 'attribute_loss_bench.py measures on a GPU'
    say('device: %s' % torch.cuda.get_device_name(0))
    say()
    gen = torch.Generator().manual_seed(0)
    utils = batch_utils()
    table = cases(gen)
    if LAUNCHES:
        say('| loss | rows | fused launches | torch path launches |')
        say('|---|---|---|---|')
    else:
        say('| loss | rows | fused us | torch path us | ratio | spread fused / torch | largest gradient difference |')
        say('|---|---|---|---|---|---|---|')
    everything = []
    for label, shape, loss_name, cfg, feats, group in table:
        fused_fn, torch_fn, leaves = paths(loss_name, cfg, feats, group, utils)
        assert all(ph.kernel_taken(f, 2, 14, 'same_as_last_layer') for f in feats if f.dim() != 4 or f.shape[1] != 4)
        if not label.startswith('intermediate'):
            everything.append((fused_fn, torch_fn))
        if LAUNCHES:
            say('| %s | %s | %d | %d |' % (label, shape, launches(fused_fn), launches(torch_fn)))
            continue
        err = agree(fused_fn, torch_fn, leaves)
        tf, tt, sf, st = ab(fused_fn, torch_fn, 20 if label.startswith('intermediate') else (50 if QUICK else 200))
        say('| %s | %s | %.1f | %.1f | %.2f x | %.2f / %.2f | %.1e |' % (label, shape, tf, tt, tt / tf, sf, st, err))

    def all_fused():
        for f, _ in everything:
            f()

    def all_torch():
        for _, t in everything:
            t()

    if LAUNCHES:
        say('| the FFHQ loss set, %d losses | last layers | %d | %d |' % (len(everything), launches(all_fused), launches(all_torch)))
    else:
        tf, tt, sf, st = ab(all_fused, all_torch, 20 if QUICK else 100)
        say('| the FFHQ loss set, %d losses | last layers | %.1f | %.1f | %.2f x | %.2f / %.2f | |' % (len(everything), tf, tt, tt / tf, sf, st))


if __name__ == '__main__':
    main()
