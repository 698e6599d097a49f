"""Cost of the projection kernels on one GPU (profiles/projection.md).

    python tools/projection_bench.py [--rounds 10] [--inner 10] [--warmup 3] [--size 1024] [--batch 1]

For the noise list of the ``--size`` generator (17 maps at 1024: 4^2, then two each of 8^2 .. 1024^2), each against the same expressions in
ATen on the same device, the variants ALTERNATING inside every round of one process:
1. ``noise_regularize`` forward + backward (HIP: 3 + 1 kernel launches) against ``noise_regularize_reference`` under autograd;
2. ``noise_normalize_`` (HIP: 3 launches) against the per-map ``mean`` / ``std`` / ``sub_`` / ``div_`` loop;
3. the activation backward of the widest layer, [batch, 32, size, size]: gc_bias_act_bwd_noise_f32 (g_pre and the noise-map gradient in one pass)
   against gc_bias_act_bwd_f32 followed by ``g_pre.sum(1, keepdim=True) * noise_w``, and against gc_bias_act_bwd_f32 alone (what a backward
   pass without noise gradients pays);
4. one generator forward + backward (split-bf16 convolutions, parameters frozen, gradient w.r.t. the latent) with and without noise-map
   gradients.
Timing: device events around ``inner`` back-to-back calls, ``rounds`` windows per variant after ``warmup`` untimed ones; medians and the
min - max spread.  Kernel launches of the ATen variants are counted from one profiled call (torch.profiler device events), in a call of its
own outside the timed windows; "not measured" where the profiler gives no device events.  One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'gan-control_amd'))

from gan_control_amd import projection  # noqa: E402
from gan_control_amd.models.op import _backend, noise_grad  # noqa: E402
from gan_control_amd.projection import noise_ops  # noqa: E402


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner          # us per call


def alternate(variants, rounds, inner, warmup):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(window(fn, inner))
    return out


def device_launches(fn):
    """Kernel launches of one call, from the profiler's device events; None where it records none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n or None
    except Exception:          # noqa: BLE001  (a profiler that does not start is "not measured", never a failed benchmark)
        return None


def report(name, samples, extra=None):
    row = {'name': name, 'us_median': round(statistics.median(samples), 2), 'us_min': round(min(samples), 2), 'us_max': round(max(samples), 2),
           'rounds': len(samples)}
    row.update(extra or {})
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--batch', type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('projection_bench: needs a GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'size': args.size, 'batch': args.batch}), flush=True)
    gen = torch.Generator().manual_seed(0)
    log = args.size.bit_length() - 1
    shapes = [(args.batch, 1, 4, 4)] + [(args.batch, 1, 2 ** i, 2 ** i) for i in range(3, log + 1) for _ in range(2)]
    maps = [torch.randn(s, generator=gen).to(dev).requires_grad_(True) for s in shapes]
    nbytes = 4 * sum(m.numel() for m in maps)

    def reg(fn):
        def run():
            for m in maps:
                m.grad = None
            (fn(maps) * 1e5).backward()
        return run

    variants = {'noise_regularize fwd+bwd, HIP': reg(projection.noise_regularize), 'noise_regularize fwd+bwd, ATen': reg(noise_ops.noise_regularize_reference)}
    launches = {'noise_regularize fwd+bwd, HIP': '3 + 1 (+ ATen: mul by the weight, its backward)', 'noise_regularize fwd+bwd, ATen': device_launches(variants['noise_regularize fwd+bwd, ATen'])}
    for k, v in alternate(variants, args.rounds, args.inner, args.warmup).items():
        report(k, v, {'maps': len(maps), 'map_bytes': nbytes, 'device_launches': launches[k] or 'not measured'})

    plain = [m.detach().clone() for m in maps]
    variants = {'noise_normalize_, HIP': lambda: projection.noise_normalize_(plain), 'noise_normalize_, ATen': lambda: noise_ops.noise_normalize_reference_(plain)}
    launches = {'noise_normalize_, HIP': 3, 'noise_normalize_, ATen': device_launches(variants['noise_normalize_, ATen'])}
    for k, v in alternate(variants, args.rounds, args.inner, args.warmup).items():
        report(k, v, {'maps': len(maps), 'map_bytes': nbytes, 'device_launches': launches[k] or 'not measured'})

    hip = _backend.get()
    gy = torch.randn(args.batch, 32, args.size, args.size, generator=gen).to(dev)
    y = torch.randn(args.batch, 32, args.size, args.size, generator=gen).to(dev)
    nw = torch.tensor([0.3], device=dev)
    variants = {'activation backward + noise-map gradient, one HIP pass': lambda: noise_grad.masked(gy, y, nw, 0.2, 2 ** 0.5),
                'activation backward (HIP) + sum(1) * noise_w (ATen)': lambda: hip.bias_act_bwd(gy, y, 0.2, 2 ** 0.5).sum(1, keepdim=True) * nw,
                'activation backward alone (HIP)': lambda: hip.bias_act_bwd(gy, y, 0.2, 2 ** 0.5)}
    for k, v in alternate(variants, args.rounds, args.inner, args.warmup).items():
        med = statistics.median(v)
        report(k, v, {'shape': list(gy.shape), 'GBps_of_3_tensor_passes': round(3 * 4 * gy.numel() / med * 1e-3, 1)})
    del gy, y

    from gan_control_amd.models.gan_model import Generator
    prev, hip.conv_mode = hip.conv_mode, 'bf16x3'
    try:
        g = Generator(args.size, 512, 8, channel_multiplier=2, conv_transpose=True).to(dev)
        for p in g.parameters():
            p.requires_grad_(False)
        with torch.no_grad():
            for m in g.modules():
                if type(m).__name__ == 'NoiseInjection':
                    m.weight.fill_(0.1)
        w = g.style(torch.randn(args.batch, 512, generator=gen).to(dev)).detach().requires_grad_(True)
        probe = torch.randn(args.batch, 3, args.size, args.size, generator=gen).to(dev)
        noises = [m.detach().clone() for m in maps]

        def step(noise_grads):
            def run():
                for n in noises:
                    n.requires_grad_(noise_grads)
                    n.grad = None
                w.grad = None
                img, _ = g([w], input_is_latent=True, noise=noises)
                (img * probe).sum().backward()
            return run

        variants = {'generator fwd+bwd, latent gradient only': step(False), 'generator fwd+bwd, latent + 17 noise-map gradients': step(True)}
        for k, v in alternate(variants, args.rounds, max(1, args.inner // 5), args.warmup).items():
            report(k, v, {'mode': 'bf16x3'})
    finally:
        hip.conv_mode = prev


if __name__ == '__main__':
    main()
