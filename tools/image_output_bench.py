"""Cost of the image output path on one GPU (profiles/image_output.md).

    python tools/image_output_bench.py [--rounds 10] [--inner 10] [--warmup 3] [--out FILE.json]

1. float32 [36, 3, 1024, 1024], nrow 6 -> the uint8 6152 x 6152 x 3 grid of a training matrix: gc_image_f32_to_u8_grid (one launch) against
   the ATen composition on the same device that produces the same bytes -- ``mul, add, clamp, mul, to(uint8), permute`` and one slice copy
   per tile into a zeroed grid -- measured ALTERNATING in one process.  The gate: the HIP launch is not slower than ATen.
2. The same for [16, 3, 1024, 1024], nrow 4 (the sample grid).
3. Everything gen_matrix(downsample=4) does after the generator calls: grid_image of the 36 images = the grid launch, the two uint8 resample
   passes (6152^2 -> 1538^2), the copy of the 7 MB result to the host and Image.fromarray; a host clock around it (the copy synchronises).
Timing of 1 and 2: device events around ``inner`` back-to-back calls, ``rounds`` windows per variant after ``warmup`` untimed ones, medians
(and the min - max spread).  GB/s = the bytes the algorithm must move (12 B read per pixel, every byte of the grid written once) over the
median.  Prints one JSON line per measurement and names the device.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'gan-control_amd'))

from gan_control_amd.evaluation import image_grid  # noqa: E402


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner          # us per call


def alternate(variants, rounds, inner, warmup):
    """{name: [us per call, one per round]}: the variants take turns inside every round."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(window(fn, inner))
    return out


def report(name, samples, nbytes, extra=None):
    med = statistics.median(samples)
    row = {'name': name, 'us_median': round(med, 2), 'us_min': round(min(samples), 2), 'us_max': round(max(samples), 2), 'rounds': len(samples),
           'bytes': nbytes, 'GBps': round(nbytes / med * 1e-3, 1)}
    row.update(extra or {})
    print(json.dumps(row), flush=True)
    return row


def aten_chain(x, nrow, padding=2):
    """The reference's operations and make_grid's copies, by ATen on x's device: the same bytes as to_u8_grid (no NaN in x)."""
    b, _, h, w = x.shape
    u8 = x.mul(0.5).add(0.5).clamp(min=0., max=1.).mul(255).to(torch.uint8).permute(0, 2, 3, 1)
    xmaps, _, grid_h, grid_w = image_grid.grid_geometry(b, h, w, nrow, padding)
    grid = torch.zeros((grid_h, grid_w, 3), dtype=torch.uint8, device=x.device)
    for k in range(b):
        top, left = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        grid[top:top + h, left:left + w] = u8[k]
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('image_output_bench.py measures on a GPU; none is visible')
    dev = torch.device('cuda:0')
    box = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'hip': torch.version.hip}
    print(json.dumps(box), flush=True)
    rows = [box]
    size = args.size
    x36 = (torch.rand((36, 3, size, size), device=dev) * 2.4 - 1.2)
    gates = []
    for tag, x, nrow in (('36_nrow6', x36, 6), ('16_nrow4', x36[:16], 4)):
        b = x.shape[0]
        _, _, gh, gw = image_grid.grid_geometry(b, size, size, nrow, 2)
        out = torch.empty((gh, gw, 3), dtype=torch.uint8, device=dev)
        differ = int((image_grid.to_u8_grid(x, nrow=nrow) != aten_chain(x, nrow)).sum())
        print(json.dumps({'name': 'bytes_differing_from_aten_chain_' + tag, 'value': differ, 'of': gh * gw * 3}), flush=True)
        nbytes = b * 3 * size * size * 4 + gh * gw * 3
        res = alternate({'hip_grid_' + tag: lambda x=x, nrow=nrow, out=out: image_grid.to_u8_grid(x, nrow=nrow, out=out),
                         'aten_chain_' + tag: lambda x=x, nrow=nrow: aten_chain(x, nrow)}, args.rounds, args.inner, args.warmup)
        for k, v in res.items():
            rows.append(report(k, v, nbytes, {'grid': [gh, gw]}))
        hip, aten = statistics.median(res['hip_grid_' + tag]), statistics.median(res['aten_chain_' + tag])
        gates.append(hip <= aten)
        rows.append({'name': 'aten_over_hip_' + tag, 'value': round(aten / hip, 2), 'differing_bytes': differ})
        print(json.dumps(rows[-1]), flush=True)
    # the whole output side of gen_matrix(downsample=4)
    for _ in range(2):
        image_grid.grid_image(x36, 6, downsample=max(size // 256, 1))
    samples = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = image_grid.grid_image(x36, 6, downsample=max(size // 256, 1))
        samples.append((time.perf_counter() - t0) * 1e6)
    rows.append(report('grid_image_36_nrow6_downsampled_host_clock', samples, 36 * 3 * size * size * 4, {'image': list(img.size)}))
    rows.append({'name': 'gate_grid_launch_not_slower_than_aten', 'value': bool(all(gates))})
    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)
    if not all(gates):
        raise SystemExit('gate failed: the grid launch is slower than the ATen composition')


if __name__ == '__main__':
    main()
