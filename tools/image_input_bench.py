"""Cost of the real-image input path on one GPU (profiles/image_input_r08.md).

    python tools/image_input_bench.py [--rounds 15] [--inner 20] [--warmup 5] [--out FILE.json]

1. No resize, uint8 [4, 1024, 1024, 3] -> float32 [4, 3, 1024, 1024] with two of four samples flipped: gc_image_u8_to_f32 (one launch)
   against the ATen composition on the same device and the same input, ``permute -> float -> div(255) -> sub(0.5) -> div(0.5) -> flip``,
   measured ALTERNATING in one process.  Also timed: the same kernel on rows that start one dword past a 16-byte boundary with 4 bytes of
   padding each, and on a 1020-wide view of the batch.  The gate: the HIP path is not slower than ATen.
2. Resize 1024^2 -> 512^2: the two launches (horizontal uint8 pass, fused vertical pass) with prebuilt device tables.  No GPU reference
   exists for this arithmetic (PIL's 8-bit fixed-point resample): the kernels are reported alone, and once more through
   images_to_device_batch (tables built and uploaded per call).
3. H2D time of the batch as pinned uint8 and as pinned float32.
Timing: device events around ``inner`` back-to-back calls, ``rounds`` windows per variant after ``warmup`` untimed ones, medians (and the
min - max spread).  GB/s = the bytes the algorithm must move (input read once, output written once) over the median.  Prints one JSON line
per measurement and names the device.
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'gan-control_amd'))

from gan_control_amd.datasets import image_ops  # noqa: E402


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


def aten_chain(u8, flags):
    x = u8.permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)
    return torch.where(flags.view(-1, 1, 1, 1), x.flip(3), x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('image_input_bench.py measures on a GPU; none is visible')
    dev = torch.device('cuda:0')
    box = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'hip': torch.version.hip}
    print(json.dumps(box), flush=True)
    rows = [box]
    b, h, w = 4, 1024, 1024
    gen = torch.Generator().manual_seed(0)
    host = torch.randint(0, 256, (b, h, w, 3), dtype=torch.uint8, generator=gen)
    u8 = host.to(dev)
    flip = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=dev)
    flags = flip.bool()
    # the same pixels one dword past the aligned start, rows 3 * w + 4 bytes apart
    backing = torch.empty(b * h * (3 * w + 4) + 64, dtype=torch.uint8, device=dev)
    shifted = torch.as_strided(backing, (b, h, w, 3), (h * (3 * w + 4), 3 * w + 4, 3, 1), 4)
    shifted.copy_(u8)
    odd = u8[:, :, :w - 4]          # rows with unused bytes behind them
    want = aten_chain(u8, flags)
    got = image_ops.u8_to_f32(u8, flip)
    differ = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    print(json.dumps({'name': 'elements_differing_from_aten_chain', 'value': differ, 'of': want.numel(),
                      'note': 'information only: ATen on the device may divide by a scalar as a multiplication by its reciprocal; the tests compare with the host chain'}), flush=True)
    nbytes = b * h * w * 3 * (1 + 4)
    res = alternate({'hip_u8_to_f32': lambda: image_ops.u8_to_f32(u8, flip),
                     'aten_chain': lambda: aten_chain(u8, flags),
                     'hip_u8_to_f32_unaligned_view': lambda: image_ops.u8_to_f32(shifted, flip)}, args.rounds, args.inner, args.warmup)
    for k, v in res.items():
        rows.append(report(k, v, nbytes))
    res4 = alternate({'hip_u8_to_f32_w1020': lambda: image_ops.u8_to_f32(odd, flip)}, args.rounds, args.inner, args.warmup)
    rows.append(report('hip_u8_to_f32_w1020', res4['hip_u8_to_f32_w1020'], b * h * (w - 4) * 15))
    gate = statistics.median(res['hip_u8_to_f32']) <= statistics.median(res['aten_chain'])
    rows.append({'name': 'gate_no_resize_not_slower_than_aten', 'value': bool(gate)})
    print(json.dumps(rows[-1]), flush=True)
    # resize 1024^2 -> 512^2
    size = 512
    hc, hb = image_ops.resample_tables(w, size)
    vc, vb = image_ops.resample_tables(h, size)
    th, tv = image_ops.DeviceTables(hc, hb, None, dev), image_ops.DeviceTables(vc, vb, None, dev)

    def two_launches():
        mid = image_ops.resample_u8(u8, h, size, 0, th)
        return image_ops.resample_v_u8_to_f32(mid, size, size, tv, flip=flip)

    res = alternate({'hip_resize_1024_to_512_kernels': two_launches,
                     'hip_resize_1024_to_512_with_table_upload': lambda: image_ops.images_to_device_batch(u8, size=size, flip=flip),
                     'hip_resize_horizontal_pass_only': lambda: image_ops.resample_u8(u8, h, size, 0, th)}, args.rounds, args.inner, args.warmup)
    moved = {'hip_resize_1024_to_512_kernels': b * (h * w * 3 + 2 * h * size * 3 + size * size * 12),
             'hip_resize_1024_to_512_with_table_upload': b * (h * w * 3 + 2 * h * size * 3 + size * size * 12),
             'hip_resize_horizontal_pass_only': b * (h * w * 3 + h * size * 3)}
    for k, v in res.items():
        rows.append(report(k, v, moved[k], {'note': 'no GPU reference exists for this arithmetic; the kernels alone'}))
    # H2D of the batch, pinned
    pin8, pin32 = host.pin_memory(), torch.empty((b, 3, h, w), dtype=torch.float32).pin_memory()
    d8, d32 = torch.empty_like(u8), torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
    res = alternate({'h2d_uint8_batch': lambda: d8.copy_(pin8, non_blocking=True), 'h2d_float32_batch': lambda: d32.copy_(pin32, non_blocking=True)},
                    args.rounds, max(args.inner // 4, 1), 2)
    rows.append(report('h2d_uint8_batch', res['h2d_uint8_batch'], pin8.numel()))
    rows.append(report('h2d_float32_batch', res['h2d_float32_batch'], pin32.numel() * 4))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)
    if not gate:
        raise SystemExit('gate failed: the no-resize HIP path is slower than the ATen composition')


if __name__ == '__main__':
    main()
