"""The decision table of the convolution and FIR dispatch: every kernel-variant probe and every size / pitch query of the library over a fixed descriptor grid.

No GPU is needed: gc_conv2d_variant_name and gc_conv2d_wgrad_variant_name run the launchers in their no-launch probe mode, gc_upfirdn2d_variant_name reads the
plan the FIR launcher follows, the queries are host code.
tests/golden/dispatch_table.json holds a DIGEST of the table -- per (geometry, column) group the row count, a sha256 over the rows and, for the probe
columns, the histogram of kernel names -- and tests/test_dispatch.py recomputes it from the built library.  When a digest moves, diff the rows of two builds:

    python tools/dispatch_table.py --dump > before.txt          # on the parent build
    python tools/dispatch_table.py --dump > after.txt           # on the changed build
    diff before.txt after.txt

    python tools/dispatch_table.py --write                      # regenerate tests/golden/dispatch_table.json (a deliberate change of a decision)

    python tools/dispatch_table.py --cheapest                   # per probe column and kernel variant: the grid descriptor with the fewest MACs that reaches it
"""
import argparse
import collections
import ctypes
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'dispatch_table.json')
for _p in (os.path.join(REPO, 'gan-control_amd'), os.path.join(REPO, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from gan_control_amd import _lib          # noqa: E402

# (taps, up, down, pad)
GEOMETRIES = [(3, 1, 1, 1), (3, 1, 2, 0), (3, 2, 1, 2), (1, 1, 1, 0), (1, 1, 2, 0), (3, 1, 1, 0), (3, 2, 1, 1), (1, 2, 1, 0)]
BATCHES = [1, 2, 3, 4, 8, 16]
IN_CH = [3, 16, 24, 32, 64, 96, 128, 256, 512, 513]
OUT_CH = [3, 32, 64, 96, 128, 256, 512]
PLANES = [4, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025]
# the tile-count rules differ per axis: (in_h, in_w)
NON_SQUARE = [(16, 64), (64, 16), (33, 129), (129, 33), (8, 512), (512, 8), (65, 257), (40, 72)]


def out_extent(n, k, up, down, pad):
    return (n - 1) * up + k - 2 * (k - 1 - pad) if up > 1 else (n + 2 * pad - k) // down + 1


def _desc(b, K, N, h, w, k, up, down, pad, pitched=False):
    oh, ow = out_extent(h, k, up, down, pad), out_extent(w, k, up, down, pad)
    in_pitch = (w // 32 + 1) * 32 if pitched and down == 2 else 0
    out_pitch = (ow // 32 + 1) * 32 if pitched and up == 2 else 0
    return (b, K, N, h, w, oh, ow, k, k, up, down, pad, pad, in_pitch, out_pitch)


def grid():
    """Every descriptor of the table as a tuple in gc_conv_desc field order."""
    from test_dispatch import STEP_SHAPES, STEP_WGRAD_SHAPES
    descs = []
    for pitched in (False, True):
        for k, up, down, pad in GEOMETRIES:
            if pitched and up == 1 and down == 1:
                continue
            for b in BATCHES:
                for K in IN_CH:
                    for N in OUT_CH:
                        descs += [_desc(b, K, N, h, h, k, up, down, pad, pitched) for h in PLANES]
    for k, up, down, pad in GEOMETRIES:
        for h, w in NON_SQUARE:
            for b, K, N in [(4, 512, 512), (8, 64, 32), (2, 256, 128), (16, 128, 256)]:
                descs.append(_desc(b, K, N, h, w, k, up, down, pad))
    for (b, K, N, h, k, up, down, pad), _, _ in STEP_SHAPES:
        descs.append(_desc(b, K, N, h, h, k, up, down, pad))
    for (b, K, N, h, k, down, pad, _), _ in STEP_WGRAD_SHAPES:
        descs.append(_desc(b, K, N, h, h, k, 1, down, pad))
    return list(dict.fromkeys(descs))


def columns(lib):
    """name -> (function of a ConvDesc returning the cell as a string, applies to transposed descriptors too?)"""
    buf = ctypes.create_string_buffer(128)

    def conv(mode):
        def f(d):
            rc = lib.gc_conv2d_variant_name(d, mode, buf, 128)
            return buf.value.decode() if rc == 0 else 'rc%d' % rc
        return f

    def wgrad(mode, samples):
        def f(d):
            rc = lib.gc_conv2d_wgrad_variant_name(d, mode, samples, buf, 128)
            return buf.value.decode() if rc == 0 else 'rc%d' % rc
        return f

    cols = collections.OrderedDict()
    for mode in (0, 1, 2):
        cols['conv_variant[mode=%d]' % mode] = (conv(mode), True)
    for mode in (0, 1, 2):
        for samples in (0, 1):
            cols['wgrad_variant[mode=%d,samples=%d]' % (mode, samples)] = (wgrad(mode, samples), False)
    for q in ('gc_conv2d_bf16x3_splitk_bytes', 'gc_conv2d_bf16x3_workspace', 'gc_conv2d_bf16x3_packed_bytes', 'gc_conv2d_f32_workspace'):
        cols[q] = ((lambda fn: lambda d: str(fn(d)))(getattr(lib, q)), True)
    for q in ('gc_conv2d_wgrad_workspace', 'gc_conv2d_wgrad_bf16x3_workspace'):
        cols[q] = ((lambda fn: lambda d: str(fn(d)))(getattr(lib, q)), False)
    for mode in (0, 1, 2):
        cols['gc_conv2d_wgrad_samples_workspace[mode=%d]' % mode] = ((lambda m: lambda d: str(lib.gc_conv2d_wgrad_samples_workspace(d, m)))(mode), False)
    cols['gc_conv2d_out_pitch'] = (lambda d: str(lib.gc_conv2d_out_pitch(d, 1)), True)
    for wg in (0, 1):
        cols['gc_conv2d_in_pitch_ok[wgrad=%d]' % wg] = ((lambda g: lambda d: str(lib.gc_conv2d_in_pitch_ok(d, 1, g)))(wg), True)
    return cols


# ---- upfirdn2d (gc_upfirdn2d_variant_name): one column, the kernel plan_fir names ----
FIR_TAPS = [4, 12, 3, 5]                                    # 3 and 5: nothing but the generic kernel
FIR_UP_DOWN = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2)]
FIR_PLANES = [1, 65535, 65536]                              # gridDim.z holds 65535
# both sides of every extent threshold: 16 x 64 (tile kernel), 8 x 32 (down2 / up2 / 12-tap tile kernels), and (out_h + 3) * (out_w + 3) <= 1296 (small-plane kernel:
# 36 * 36 = 18 * 72 = 12 * 108 = 1296; 36 * 37 = 1332)
FIR_OUT = [(h, w) for h in (7, 8, 15, 16, 33, 34) for w in (31, 32, 63, 64)] + [(33, 33), (33, 34), (34, 33), (15, 69), (15, 70), (69, 15), (70, 15), (9, 105), (9, 106),
                                                                                (15, 200), (100, 63), (1024, 1024), (1025, 1025)]


def fir_grid():
    """(planes, out_h, out_w, taps, up, down) of every FIR row; the last row has more taps than any kernel takes."""
    from test_dispatch import STEP_FIR_SHAPES
    shapes = [(planes, oh, ow, k, up, down) for k in FIR_TAPS for up, down in FIR_UP_DOWN for planes in FIR_PLANES for oh, ow in FIR_OUT]
    shapes += [shape for shape, _ in STEP_FIR_SHAPES]
    shapes.append((1, 16, 64, 33, 1, 1))
    return list(dict.fromkeys(shapes))


def fir_rows(lib):
    buf = ctypes.create_string_buffer(128)
    for t in fir_grid():
        planes, oh, ow, k, up, down = t
        rc = lib.gc_upfirdn2d_variant_name(planes, oh, ow, k, k, up, down, buf, 128)
        yield 'fir:%d,%d,%d|fir_variant[name]' % t[3:], ','.join(map(str, t)) + ' -> ' + (buf.value.decode() if rc == 0 else 'rc%d' % rc)


def rows():
    """Yield (group, row text): group = '<taps>,<up>,<down>,<pad>|<column>', row = '<descriptor fields> -> <cell>'; the FIR groups ('fir:<taps>,<up>,<down>|...') follow."""
    lib = _lib.load()
    cols = columns(lib)
    for t in grid():
        d = _lib.ConvDesc(*t)
        geom = '%d,%d,%d,%d' % (t[7], t[9], t[10], t[11])
        key = ','.join(map(str, t))
        for name, (fn, transposed_too) in cols.items():
            if t[9] == 1 or transposed_too:
                yield geom + '|' + name, key + ' -> ' + fn(d)
    yield from fir_rows(lib)


def digest():
    groups = collections.OrderedDict()
    for group, row in rows():
        g = groups.get(group)
        if g is None:
            g = groups[group] = {'rows': 0, 'sha': hashlib.sha256(), 'names': collections.Counter()}
        g['rows'] += 1
        g['sha'].update(row.encode() + b'\n')
        if '_variant[' in group:
            g['names'][row.split(' -> ', 1)[1].split('|plan:')[0]] += 1
    out = collections.OrderedDict()
    for group, g in groups.items():
        out[group] = {'rows': g['rows'], 'sha256': g['sha'].hexdigest()}
        if g['names']:
            out[group]['names'] = dict(sorted(g['names'].items()))
    return out


def macs(t):
    """Multiply-adds of the convolution a descriptor tuple describes: batch * K * N * out pixels * taps."""
    b, K, N, _, _, oh, ow, kh, kw = t[:9]
    return b * K * N * oh * ow * kh * kw


def cheapest():
    """(column, variant) -> (MACs, descriptor tuple) of the grid's cheapest descriptor that reaches the variant (split plan stripped, rc* cells skipped);
    the probe columns only.  How the kernel-level test cases find a shape for a variant."""
    lib = _lib.load()
    probes = [(name, fn, tt) for name, (fn, tt) in columns(lib).items() if '_variant[' in name]
    best = {}
    for t in grid():
        d = _lib.ConvDesc(*t)
        cost = macs(t)
        for name, fn, transposed_too in probes:
            if t[9] != 1 and not transposed_too:
                continue
            cell = fn(d).split('|plan:')[0]
            if cell.startswith('rc'):
                continue
            key = (name, cell)
            if key not in best or cost < best[key][0]:
                best[key] = (cost, t)
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--dump', action='store_true', help='print every row (diff two builds when a digest moves)')
    ap.add_argument('--write', action='store_true', help='write the digest to tests/golden/dispatch_table.json')
    ap.add_argument('--cheapest', action='store_true',
                    help='per probe column and kernel variant, the cheapest grid descriptor reaching it: b,K,N,in_h,in_w,out_h,out_w,kh,kw,up,down,pad_y,pad_x,in_pitch,out_pitch')
    args = ap.parse_args()
    if args.dump:
        for group, row in rows():
            print(group + ' | ' + row)
        return
    if args.cheapest:
        for (name, cell), (cost, t) in sorted(cheapest().items()):
            print('%s | %s | %.3g MAC | %s' % (name, cell, cost, ','.join(map(str, t))))
        return
    text = json.dumps(digest(), indent=1) + '\n'
    if args.write:
        with open(GOLDEN, 'w') as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == '__main__':
    main()
