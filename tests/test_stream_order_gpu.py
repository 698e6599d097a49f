"""Every kernel entry on a side stream behind late-arriving inputs (tests/stream_order.py): the one argument of the C ABI no other test varies.

GPU part (``-m gpu``): every case of the guarded table (tests/test_guarded_buffers.py: every entry ``op/_backend.py`` launches, in each
arithmetic, with the multi-launch forms), one case per entry launched from another module (``OTHER``), the five entries no Python wrapper
calls and the one whose only wrapper blocks the host, through ``_lib`` (``ABI``), a generator / discriminator forward and backward with both
second-order passes, and the harness's own negative controls.

CPU part (no marker): every declaration of include/gancontrol_hip.h that takes a ``gc_stream_t`` is claimed by a case that must be conclusive,
no case claims a name the header does not have, and the list of cases whose wrapper blocks the host by contract is explicit and small.
"""
import ctypes
import os
import re

import pytest
import torch

import stream_order as so
import test_guarded_buffers as tgb
import test_fc_stack_gpu as tfs
import test_fc_train_gpu as tft
import test_group_pca_gpu as tgp
import test_image_input_gpu as tii
import test_image_output_gpu as tio
import test_interpolation_gpu as tin
import test_pair_hinge_gpu as tph
import test_pairwise_gpu as tpw
import test_projection_gpu as tpj
import test_quality_metrics_gpu as tqm
import quality_refs as qr

from gan_control_amd import _lib, projection
from gan_control_amd.datasets import image_ops
from gan_control_amd.evaluation import image_grid
from gan_control_amd.models.op import _backend, fc_stack, fc_train, group_pca, interp, manifold, noise_grad, pair_hinge, pairwise, weight_cache, weight_refresh
from gan_control_amd.projection import noise_ops

DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, 'include', 'gancontrol_hip.h')
SLOPE, GAIN = 0.2, 2 ** 0.5


class Case:
    """name; entries the run must reach; the launching modules, whose allocations are NaN-filled; build() -> the inputs (a dict: tensors, lists of tensors,
    modules, anything else); run(a) -> [tensors] (an input updated in place is returned like any other output); mode: the convolution
    arithmetic."""

    def __init__(self, name, entries, modules, build, run, mode=None):
        self.name, self.entries, self.modules, self.build, self.run, self.mode = name, frozenset(entries), tuple(modules), build, run, mode


OTHER = []


def other(name, entries, modules, mode=None):
    def deco(pair):
        build, run = pair()
        OTHER.append(Case(name, entries, modules, build, run, mode))
        return pair
    return deco


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- op/fc_stack.py, op/fc_train.py -----------------------------------------------------------------------------------------------------------------

@other('fc_stacks_forward', {fc_stack.ENTRY}, [fc_stack])
def _():
    def build():
        stacks, xs, x_slices, out_shape, out_slices = tfs.build('single', 8)          # the smallest run of tests/test_fc_stack_gpu.py
        return {'stacks': stacks, 'xs': xs, 'out': torch.full(out_shape, -3.0, device=DEV), '_slices': (x_slices, out_slices)}

    def run(a):
        with torch.no_grad():
            return [fc_stack.fc_stacks_forward(a['stacks'], a['xs'], a['_slices'][0], a['out'], a['_slices'][1])]
    return build, run


@other('fc_train-fused_step', {fc_train.ENTRY_FWD, fc_train.ENTRY_LOSS, fc_train.ENTRY_BWD}, [fc_train])
def _():
    name = 'odd'          # two layers: the backward entry is launched twice

    def build():
        stack = tft.make_stack(tft.SHAPES[name][1], 5)
        controls, latents = tft.make_data(name)
        opt = tft.adam_for(stack, beta1=0.9)
        tft.seed_state(opt, 11)
        params = list(stack.parameters())
        return {'stack': stack, 'controls': controls, 'latents': latents, '_opt': opt,
                'moments': [opt.state[p][k] for p in params for k in ('exp_avg', 'exp_avg_sq')]}

    def run(a):
        stack, opt = a['stack'], a['_opt']
        fc_train._plans.pop(stack, None)          # a fresh plan: its activation and gradient workspaces are allocated in this run
        for p in stack.parameters():
            opt.state[p]['step'] = torch.tensor(3.0)
        assert fc_train.fused_step_taken(stack, opt, a['controls'], a['latents'], tft.chunk_of(name), 'l1')
        with torch.no_grad():
            loss = fc_train.fused_step(stack, opt, a['controls'], a['latents'], tft.chunk_of(name), 'l1')
        return [loss] + [p.detach() for p in stack.parameters()] + a['moments']
    return build, run


# ---- op/interp.py ------------------------------------------------------------------------------------------------------------------------------------

@other('latent_interp', {interp.LATENT_ENTRY}, [interp])
def _():
    b, l, lo, hi = tin.SHAPES[3]          # (1, 48, 16, 32)

    def build():
        row, z_from, z_to = tin.latent_inputs(b, l, 3)
        return {'row': row, 'from': z_from, 'to': z_to}

    def run(a):
        wa, wb = interp.interpolation_weights(10, 'slerp')
        with torch.no_grad():
            return [interp.interpolate_latents(a['row'].expand(b, l), a['from'], a['to'], lo, hi, wa, wb, 'slerp')]
    return build, run


@other('noise_blend', {interp.NOISE_ENTRY}, [interp])
def _():
    def build():
        x, y = tin.noise_lists('odd')
        return {'a': x, 'b': y}

    def run(a):
        with torch.no_grad():
            return interp.blend_noise(a['a'], a['b'], 0.3, 0.7)
    return build, run


# ---- op/manifold.py, op/pairwise.py, op/pair_hinge.py ---------------------------------------------------------------------------------------------------

_DIST = qr.DISTANCE_CASES[0]          # (5, 4, 3, 1, 'k')


def _manifold_inputs():
    n_r, n_f, f, kth, stride = _DIST
    case = qr.distance_case(n_r, n_f, f, kth)
    return {'real': tqm.strided(case['real'], stride), 'fake': tqm.strided(case['fake'], stride),
            'real_r2': case['real_r2'].float().to(DEV), 'fake_r2': case['fake_r2'].float().to(DEV)}


@other('knn_radii', {manifold.KNN_ENTRY}, [manifold])
def _():
    def run(a):
        with torch.no_grad():
            return [manifold.knn_radii(a['real'], _DIST[3])]
    return _manifold_inputs, run


@other('manifold_hits', {manifold.HITS_ENTRY}, [manifold])
def _():
    def run(a):
        with torch.no_grad():
            return list(manifold.manifold_hits(a['real'], a['real_r2'], a['fake'], a['fake_r2']))
    return _manifold_inputs, run


@other('poly_mmd_sums', {manifold.MMD_ENTRY}, [manifold])
def _():
    m, subsets, f, stride = qr.MMD_CASES[1]          # (7, 3, 5, 'k+1')

    def build():
        x, y, ix, iy = qr.mmd_inputs(m, subsets, f)
        return {'x': tqm.strided(x, stride), 'y': tqm.strided(y, stride), '_idx': (ix, iy)}

    def run(a):
        with torch.no_grad():
            return [manifold.poly_mmd_sums(a['x'], a['y'], *a['_idx'])]
    return build, run


def _pairwise(pids):
    m, n, k, stride = tpw.CASES[1]          # (2, 7, 3, 'k')

    def build():
        gen = _gen(17)
        return {'s': tpw.strided(m, k, stride, gen), 'q': tpw.strided(n, k, stride, gen)}

    def run(a):
        with torch.no_grad():
            if pids:
                return list(pairwise.pairwise_distances(a['s'], a['q'], 'abs', *tpw.pids_of(m, n)))
            return [pairwise.pairwise_distances(a['s'], a['q'], 'abs')]
    return build, run


other('pairwise', {pairwise.ENTRY}, [pairwise])(lambda: _pairwise(False))
other('pairwise-pids', {pairwise.ENTRY}, [pairwise])(lambda: _pairwise(True))


@other('pair_hinge', {'gc_pair_hinge_fwd_f32', 'gc_pair_hinge_bwd_f32'}, [pair_hinge])
def _():
    n_same, n_not_same, k = 2, 2, 3          # PAIRS[0] of tests/test_pair_hinge_gpu.py, rows a float apart ('k+1')

    def build():
        return {'f': tph.make_rows(n_same + n_not_same, k, 'k+1', _gen(23), False), 'g': torch.tensor(0.75, device=DEV)}

    def run(a):
        with torch.no_grad():
            loss, d, c, v32 = pair_hinge.pair_hinge_forward(a['f'], n_same, n_not_same, 'sq', 0.5, 4.0, tph.FOCUS[0], 0.75, None, None, 1.0)
            df = pair_hinge.pair_hinge_backward(a['f'], c, a['g'], n_same + n_not_same, 'sq', None, v32, 1.0)
        return [loss, d, c, df]
    return build, run


# ---- op/group_pca.py ---------------------------------------------------------------------------------------------------------------------------------

@other('group_moments', {group_pca.MOMENTS_ENTRY}, [group_pca])
def _():
    n, groups, d, kind, _ = tgp.MOMENT_CASES[1]          # (3, [(1, 31), (33, 32)], 68, 'd')

    def run(a):
        with torch.no_grad():
            return list(group_pca.group_moments_packed(a['w'], tgp.places_of(groups)))
    return (lambda: {'w': tgp.strided(n, d, kind, _gen(29))}), run


@other('group_project', {group_pca.PROJECT_ENTRY}, [group_pca])
def _():
    rows, groups, d, kind, shape = tgp.PROJECT_CASES[1]          # (2, [(1, 33, 7)], 36, 'd+1')

    def build():
        x, mean, comps, places = tgp.project_case(rows, groups, d, kind, _gen(31), shape)
        return {'x': x, 'mean': mean, 'comps': comps, '_places': places}

    def run(a):
        assert group_pca.project_kernel_taken(a['x'], a['mean'], a['comps'], a['_places'])
        with torch.no_grad():
            return [group_pca.group_project_(a['x'], a['mean'], a['comps'], a['_places'])]
    return build, run


# ---- op/weight_refresh.py, op/noise_grad.py ----------------------------------------------------------------------------------------------------------------

@other('weight_refresh', {weight_refresh.ENTRY}, [weight_refresh])
def _():
    n, k, taps = 32, 32, 9          # CASES[0] of tests/test_weight_refresh_gpu.py
    ks = 3

    def build():
        gen = _gen(n * 1000 + k * 10 + taps)
        return {'w': torch.randn(n, k, ks, ks, generator=gen).to(DEV), 'ema': torch.randn(n, k, ks, ks, generator=gen).to(DEV),
                'flat': torch.randn(77, generator=gen).to(DEV), 'flat_ema': torch.randn(77, generator=gen).to(DEV)}

    def run(a):
        item = {'src': a['w'], 'taps': taps, 'k': k, 'n': n, 'flip': True, 'scale': 0.37, 'w_t': (ks, ks, k, n), 'adj': (ks, ks, n, k), 'adj2': (ks, ks, k, n),
                'pack_w': 2 * taps * ((k + 7) // 8) * n * 16, 'pack_adj': 2 * taps * ((n + 7) // 8) * k * 16, 'wsq': True, 'ema': (a['ema'], 0.999, 0.001)}
        out, = weight_refresh.run([item], [(a['flat'], a['flat_ema'], 0.5, 0.5)])
        return [out[f] for f in ('w_t', 'adj', 'adj2', 'pack_w', 'pack_adj', 'wsq')] + [a['ema'], a['flat_ema']]
    return build, run


@other('noise_grad', {noise_grad.ENTRY}, [noise_grad])
def _():
    def build():
        gy, y, nw = tpj.pixel_inputs(*tpj.GUARDED_PIXEL[0], 37)          # (2, 5, 5, 7)
        return {'gy': gy.to(DEV), 'y': y.to(DEV), 'nw': nw.to(DEV)}

    def run(a):
        g_pre, gn = noise_grad.masked(a['gy'], a['y'], a['nw'], SLOPE, GAIN)
        return [g_pre, gn, noise_grad.pixel_sums(a['gy'], a['nw'])]
    return build, run


# ---- projection/noise_ops.py -----------------------------------------------------------------------------------------------------------------------------

_MAPS = [(2, 16), (1, 4)]          # of SINGLE in tests/test_projection_gpu.py: two pyramid levels and the one-level map


@other('noise_regularize', {noise_ops.REG_FWD, noise_ops.REG_BWD}, [noise_ops])
def _():
    def build():
        return {'maps': [m.to(DEV).requires_grad_(True) for m in tpj.make_maps(_MAPS, 'smooth', 41)], 'cot': torch.tensor(-2.5e4, device=DEV)}

    def run(a):
        for m in a['maps']:
            m.grad = None
        loss = projection.noise_regularize(a['maps'])
        (loss * a['cot']).backward()          # the backward entry is launched from an autograd thread
        return [loss.detach()] + [m.grad for m in a['maps']]
    return build, run


@other('noise_normalize', {noise_ops.NORMALIZE}, [noise_ops])
def _():
    def run(a):
        projection.noise_normalize_(a['maps'])
        return list(a['maps'])
    return (lambda: {'maps': [m.to(DEV) for m in tpj.make_maps(_MAPS, 'white', 43)]}), run


# ---- datasets/image_ops.py, evaluation/image_grid.py -------------------------------------------------------------------------------------------------------
# The tables a caller builds once (DeviceTables, the byte -> float table, the flip flags as an int32 device tensor) are inputs of the per-entry
# cases: uploading them is the builder's work, not the launch's.  'images_to_device_batch' is the call as the input pipeline makes it.

def _image_tables():
    return {'lut': image_ops.device_table(torch.device(DEV, torch.cuda.current_device())).clone(), 'flip': torch.tensor([1, 0, 1], dtype=torch.int32).to(DEV)}


@other('image_u8_to_f32', {'gc_image_u8_to_f32'}, [image_ops])
def _():
    def build():
        return dict(_image_tables(), x=tii.CASES[0].x.to(DEV))          # cvt-3x5x13
    return build, lambda a: [image_ops.u8_to_f32(a['x'], a['flip'], a['lut'])]


@other('image_resample', {'gc_image_resample_u8', 'gc_image_resample_v_u8_to_f32'}, [image_ops])
def _():
    def build():
        case = [c for c in tii.CASES if c.name == 'r20to32'][0]          # the smallest resize fixture: both passes
        a = dict(_image_tables(), x=case.x.to(DEV))
        h, w = case.x.shape[1:3]
        a['_h'] = image_ops.DeviceTables(*image_ops.resample_tables(w, 32), None, a['x'].device)
        a['_v'] = image_ops.DeviceTables(*image_ops.resample_tables(h, 32), None, a['x'].device)
        a['tables'] = [a['_h'].coeff, a['_h'].bounds, a['_v'].coeff, a['_v'].bounds]
        return a

    def run(a):
        mid = image_ops.resample_u8(a['x'], a['x'].shape[1], 32, 0, a['_h'])
        return [mid, image_ops.resample_v_u8_to_f32(mid, 32, 32, a['_v'], flip=a['flip'], lut=a['lut'])]
    return build, run


@other('images_to_device_batch', {'gc_image_resample_u8', 'gc_image_resample_v_u8_to_f32'}, [image_ops])
def _():
    """As DeviceImageStream calls it on its side stream: host flip flags, tables built and uploaded per call (BLOCKS_HOST)."""
    case = [c for c in tii.CASES if c.name == 'r20to32'][0]
    return (lambda: {'x': case.x.to(DEV)}), lambda a: [case.run(a['x'])]


@other('image_f32_to_u8_grid', {'gc_image_f32_to_u8_grid'}, [image_grid])
def _():
    shape, nrow = tio.SHAPES[0]          # ((3, 3, 5, 13), 8)
    return (lambda: {'x': tio.make_input(shape, 47).to(DEV)}), lambda a: [image_grid.to_u8_grid(a['x'], nrow=nrow, padding=2, pad_value=0x5A)]


# ---- the entries no Python wrapper calls: through _lib, as a C caller would ------------------------------------------------------------------------------
# Outputs and workspaces are part of the inputs here (NaN before the plain run, NaN again when the inputs are restored): nothing is allocated
# inside the run.

ABI = []
_ABI_CONV = (2, 64, 64, 40, 70, 3, 1, 1, 1)          # _PACK_SHAPES[0] of the guarded table: takes packed weights, so the unpacked entries pack first


def _call(entry, *args):
    _lib.check(getattr(_lib.load(), entry)(*args), entry)


def _abi_conv(entry, fused, bf16x3):
    c = _ABI_CONV
    b, K, N, h, w, k = c[:6]
    geom = tgb._conv_geom(c)

    def build():
        gen = _gen(53)
        a = {'x': torch.randn(b, K, h, w, generator=gen), 'wt': torch.randn(k, k, K, N, generator=gen), 'si': torch.randn(b, K, generator=gen),
             'so': torch.rand(b, N, generator=gen) + 0.5, 'bias': torch.randn(N, generator=gen), 'y': torch.full((b, N, geom.out_h, geom.out_w), float('nan'))}
        a = {n: t.to(DEV) for n, t in a.items()}
        if bf16x3:
            desc = tgb._conv_desc(c)
            lib = _lib.load()
            nbytes = max(lib.gc_conv2d_bf16x3_workspace(desc), lib.gc_conv2d_bf16x3_packed_bytes(desc) + lib.gc_conv2d_bf16x3_splitk_bytes(desc), 16)
            a['ws'] = torch.full((nbytes // 4 + 4,), float('nan'), device=DEV)
        return a

    def run(a):
        desc = tgb._conv_desc(c)
        ep = _lib.ConvEpilogue(_lib.ptr(a['bias']), None, None, SLOPE, GAIN, 1, None)
        args = [ctypes.byref(desc), _lib.ptr(a['x']), _lib.ptr(a['wt']), _lib.ptr(a['si']), _lib.ptr(a['so'])] + ([ctypes.byref(ep)] if fused else []) + [_lib.ptr(a['y'])]
        if bf16x3:
            args += [_lib.ptr(a['ws']), a['ws'].numel() * 4]
        _call(entry, *args, _lib.stream_of(a['x']))
        return [a['y']]
    ABI.append(Case('abi-' + entry, {entry}, (), build, run))


_abi_conv('gc_conv2d_f32', False, False)
_abi_conv('gc_conv2d_fused_f32', True, False)
_abi_conv('gc_conv2d_bf16x3_f32', False, True)
_abi_conv('gc_conv2d_fused_bf16x3_f32', True, True)


def _abi_reduce():
    shape = (1, 5, 129, 131)          # the plane of the guarded table's bias_act_bwd_reduce case: two chunks, the second ragged

    def build():
        a = tgb._act_inputs(shape, DEV, 'bar')
        chunks = _lib.load().gc_bias_act_bwd_chunks(shape[2] * shape[3])
        a.update(dx=torch.full(shape, float('nan'), device=DEV), psum=torch.full((shape[0], shape[1], chunks), float('nan'), device=DEV),
                 pdot=torch.full((shape[0], shape[1], chunks), float('nan'), device=DEV))
        return a

    def run(a):
        _call('gc_bias_act_bwd_reduce_f32', _lib.ptr(a['dy']), _lib.ptr(a['y']), _lib.ptr(a['nz']), _lib.ptr(a['dx']), _lib.ptr(a['psum']), _lib.ptr(a['pdot']),
              shape[0], shape[1], shape[2] * shape[3], SLOPE, GAIN, _lib.stream_of(a['dy']))
        return [a['dx'], a['psum'], a['pdot']]
    ABI.append(Case('abi-gc_bias_act_bwd_reduce_f32', {'gc_bias_act_bwd_reduce_f32'}, (), build, run))


_abi_reduce()


def _abi_poly_mmd():
    """The wrapper of this entry uploads its host index arrays per call (BLOCKS_HOST); with the indices on the device already, as the wrapper
    passes them on, the entry itself runs conclusively."""
    m, subsets, f, stride = qr.MMD_CASES[1]          # (7, 3, 5, 'k+1')

    def build():
        x, y, ix, iy = qr.mmd_inputs(m, subsets, f)
        nbytes = _lib.load().gc_poly_mmd_workspace(subsets, m, f)
        return {'x': tqm.strided(x, stride), 'y': tqm.strided(y, stride), 'ix': torch.from_numpy(ix.astype('int32')).to(DEV), 'iy': torch.from_numpy(iy.astype('int32')).to(DEV),
                'sums': torch.full((subsets, 3), float('nan'), dtype=torch.float64, device=DEV), 'ws': torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=DEV), '_bytes': nbytes}

    def run(a):
        x, y = a['x'], a['y']
        _call('gc_poly_mmd_f32', _lib.ptr(x), manifold._rows(x)[1], x.shape[0], _lib.ptr(y), manifold._rows(y)[1], y.shape[0], f, _lib.ptr(a['ix']), _lib.ptr(a['iy']),
              subsets, m, _lib.ptr(a['sums']), _lib.ptr(a['ws']), a['_bytes'], _lib.stream_of(x))
        return [a['sums']]
    ABI.append(Case('abi-gc_poly_mmd_f32', {'gc_poly_mmd_f32'}, (), build, run))


_abi_poly_mmd()

# Cases whose wrapper blocks the host BY CONTRACT before it launches: the conclusiveness check cannot hold for them, and they are held to the
# plain run's bits only.  {case name: 'the blocking statement, file:line'}.  No case of the guarded table and none of ABI may be listed, and at
# most one case per entry.
BLOCKS_HOST = {
    # the subset indices are HOST arrays by contract (validated on the host, _host_indices) and uploaded from pageable memory per call
    'poly_mmd_sums': 'dx = torch.from_numpy(np.ascontiguousarray(ix, dtype=np.int32)).to(dev), manifold.py:192',
    # the pid arrays are host arrays by contract (np.unique over them makes the codes); the same entry runs conclusively in 'pairwise'
    'pairwise-pids': 'sp = torch.from_numpy(codes[0]).to(dev), pairwise.py:154',
    # the call as DeviceImageStream makes it: host flip flags and per-call resample tables, uploaded by _to_device; the two entries run
    # conclusively in 'image_resample', on tables built once
    'images_to_device_batch': 't.copy_(host if torch.is_tensor(host) else torch.from_numpy(np.array(host, copy=True))), image_ops.py:114',
}
BLOCKS_HOST_CAP = 3


# ====================================================================================================================================================
# CPU tests
# ====================================================================================================================================================

def stream_entries():
    """Every function declared in include/gancontrol_hip.h with a ``gc_stream_t`` parameter."""
    with open(HEADER) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    return sorted({name for name, args in re.findall(r'\b(gc_\w+)\s*\(([^;{}]*?)\)\s*;', src, flags=re.S) if re.search(r'\bgc_stream_t\b', args)})


def test_header_parser_finds_the_stream_entries():
    names = stream_entries()
    assert len(names) >= 70 and len(names) == len(set(names))
    for must in ('gc_bias_act_f32', 'gc_conv2d_f32', 'gc_weight_refresh_grouped_f32', 'gc_pair_hinge_bwd_f32', 'gc_fc_stack_bwd_adam_f32', 'gc_poly_mmd_f32'):
        assert must in names, must
    for query in ('gc_channel_sum_workspace', 'gc_conv2d_out_pitch', 'gc_abi_version', 'gc_fc_train_launches', 'gc_stream_t'):
        assert query not in names, query
    assert set(names) <= set(_lib.SIGNATURES), sorted(set(names) - set(_lib.SIGNATURES))
    # ... and every one of them takes the stream LAST, as a pointer: what the cases vary
    assert all(_lib.SIGNATURES[n][1][-1] is ctypes.c_void_p for n in names)


def test_every_stream_entry_has_a_stream_case():
    assert tgb._SELECTION_ERROR is None, tgb._SELECTION_ERROR
    names = set(stream_entries())
    claims = {}
    for c in list(tgb.CASES) + OTHER + ABI:
        for e in c.entries:
            claims.setdefault(e, []).append(c.name)
    assert not (names - set(claims)), 'entries that take a stream and have no stream case: %s' % sorted(names - set(claims))
    assert set(claims) <= names, 'cases claim names the header does not declare with a stream: %s' % sorted(set(claims) - names)
    all_names = [c.name for c in list(tgb.CASES) + OTHER + ABI]
    assert len(set(all_names)) == len(all_names)
    # the guarded table claims what op/_backend.py launches and OTHER / ABI the rest: no entry is left to "somebody else's table"
    assert not (set().union(*(c.entries for c in OTHER + ABI)) & set(tgb.launching_entries()))
    # ... and every entry has a case that must be conclusive
    conclusive = set().union(*(c.entries for c in list(tgb.CASES) + OTHER + ABI if c.name not in BLOCKS_HOST))
    assert conclusive == names, sorted(names - conclusive)


def test_blocks_host_is_explicit_and_small():
    others = {c.name: c for c in OTHER}
    assert set(BLOCKS_HOST) <= set(others), 'only cases of OTHER may block the host: %s' % sorted(set(BLOCKS_HOST) - set(others))
    assert not set(BLOCKS_HOST) & ({c.name for c in tgb.CASES} | {c.name for c in ABI})
    assert len(BLOCKS_HOST) <= BLOCKS_HOST_CAP
    per_entry = {}
    for name in BLOCKS_HOST:
        for e in others[name].entries:
            per_entry.setdefault(e, []).append(name)
    assert all(len(v) == 1 for v in per_entry.values()), per_entry
    pkg = os.path.join(REPO, 'gan-control_amd', 'gan_control_amd')
    for name, why in BLOCKS_HOST.items():
        m = re.fullmatch(r'(.+), (\w+\.py):(\d+)', why)
        assert m, (name, why)
        path, = [os.path.join(d, m.group(2)) for d, _, files in os.walk(pkg) if m.group(2) in files]
        with open(path) as f:
            line = f.read().splitlines()[int(m.group(3)) - 1]
        assert line.strip().startswith(m.group(1)), (name, line.strip())


# ====================================================================================================================================================
# GPU tests
# ====================================================================================================================================================

@pytest.fixture(scope='module')
def hip():
    _lib.load()
    assert torch.cuda.is_available() and _backend.get().name == 'hip'
    so.calibrate()
    so.side_stream()
    return _backend.get()


def _late(name, entries, modules, a, call, same=None, blocks_host=False):
    """Plain run, late run, the verdict (module docstring of tests/stream_order.py)."""
    held = so.snapshot(a)
    plain = so.clone_outs(call())
    torch.cuda.synchronize()
    assert any(o is not None for o in plain)
    run = so.late_run(held, call, modules)
    print('%s: entries %s, %s, issued in %.3f ms' % (
        name, sorted(set(run.entries)) if modules else sorted(entries), 'CONCLUSIVE' if run.conclusive else 'inconclusive', run.issue_ms))
    if modules:
        assert entries <= set(run.entries), (sorted(entries - set(run.entries)), sorted(set(run.entries)))
    if not blocks_host:
        assert run.conclusive, ('%s: the inputs were restored before the call returned on the host (delay %.0f ms): the run proves nothing about the '
                                'streams of its launches' % (name, run.delay_ms))
    if same is not None:
        assert same(plain, run.outs), name
        assert all(o is None or bool(torch.isfinite(o).all()) for o in run.outs), name
    else:
        diff = so.difference(plain, run.outs)
        assert diff is None, '%s behind late inputs on a side stream: %s -- a launch did not go to the current stream' % (name, diff)


def _guarded_fault(e, name):
    if 'illegal memory access' in str(e) or 'HIP error' in str(e):          # the context is lost: no later launch should be made
        pytest.exit('GPU fault in case %s: %s' % (name, str(e).splitlines()[0]), returncode=3)


@pytest.mark.gpu
@pytest.mark.parametrize('case', tgb.CASES, ids=[c.name for c in tgb.CASES])
def test_guarded_table_on_a_side_stream(case, hip):
    prev = hip.conv_mode
    hip.conv_mode = case.mode or 'f32'
    try:
        a = case.build(DEV)
        same = None if case.same is None else (lambda plain, outs: case.same(a, plain, outs))
        _late(case.name, case.entries, [_backend], a, lambda: list(case.run(hip, a, None)), same)
    except RuntimeError as e:
        _guarded_fault(e, case.name)
        raise
    finally:
        hip.conv_mode = prev


@pytest.mark.gpu
@pytest.mark.parametrize('case', OTHER + ABI, ids=[c.name for c in OTHER + ABI])
def test_other_entries_on_a_side_stream(case, hip):
    prev = hip.conv_mode
    hip.conv_mode = case.mode or 'f32'
    try:
        a = case.build()
        _late(case.name, case.entries, list(case.modules), a, lambda: list(case.run(a)), blocks_host=case.name in BLOCKS_HOST)
    except RuntimeError as e:
        _guarded_fault(e, case.name)
        raise
    finally:
        hip.conv_mode = prev


# ---- autograd on a side stream ---------------------------------------------------------------------------------------------------------------------------

def _networks():
    from gan_control_amd.models.gan_model import Discriminator, Generator
    torch.manual_seed(0)
    g = Generator(64, 512, 8, channel_multiplier=2, conv_transpose=True).to(DEV)
    d = Discriminator(64, channel_multiplier=2).to(DEV)
    gen = _gen(59)
    a = {'G': g, 'D': d, 'z': torch.randn(2, 512, generator=gen).to(DEV), 'real': (torch.rand(2, 3, 64, 64, generator=gen) * 2 - 1).to(DEV),
         'pl_noise': torch.randn(2, 3, 64, 64, generator=gen).to(DEV)}
    a['noise'] = [torch.randn(n.shape[0] * 2, *n.shape[1:], generator=gen).to(DEV) for n in g.make_noise(1)]
    return a


def _grads(*modules):
    return [p.grad for m in modules for p in m.parameters() if p.grad is not None]


def _clear(*modules):
    weight_cache.clear()          # the weight forms are rebuilt on the stream under test
    for m in modules:
        for p in m.parameters():
            p.grad = None


def _fwd_bwd(a):
    g, d = a['G'], a['D']
    _clear(g, d)
    img, _ = g([a['z']], noise=a['noise'])
    pred, _ = d(img)
    torch.nn.functional.softplus(-pred).mean().backward()
    outs = [img.detach()] + _grads(g, d)
    assert len(outs) > 1 + 20
    return outs


def _r1(a):
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer
    d = a['D']
    _clear(d)
    real = a['real'].detach().requires_grad_(True)
    pred, _ = d(real)
    GeneratorTrainer.d_r1_loss(pred, real).backward()
    outs = _grads(d)
    assert len(outs) > 10
    return outs


def _path_length(a):
    from gan_control_amd.models.gan_model import Generator
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer
    g = a['G']
    _clear(g)
    img, latents = g([a['z']], noise=a['noise'], return_latents=True)
    grad = Generator.g_path_regularize_grad(img, latents, pl_noise=a['pl_noise'])
    GeneratorTrainer.g_path_regularize_grad(grad, 0)[0].backward()
    outs = _grads(g)
    assert len(outs) > 10
    return outs


@pytest.fixture(scope='module')
def networks(hip):
    return _networks()


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['fwd+bwd', 'r1', 'path_length'])
def test_autograd_on_a_side_stream(which, networks, hip):
    """Generator(64) / Discriminator(64), batch 2, split-bf16, no augmentation: the backward nodes run on autograd's worker threads and ask
    ``_lib.stream_of`` there.  The image and every parameter gradient of G forward -> D -> softplus -> backward, every D gradient of the R1 pass
    and every G gradient of the path-length pass (the second-order entries) behind late inputs, bit-identical to the default-stream run.
    The allocations of op/_backend.py are NaN-filled where they are made, as in every late run."""
    a = networks
    fn = {'fwd+bwd': _fwd_bwd, 'r1': _r1, 'path_length': _path_length}[which]
    prev, hip.conv_mode = hip.conv_mode, 'bf16x3'
    try:
        held = so.snapshot(a)
        entries = []
        with so.filling([_backend], entries):
            plain = so.clone_outs(fn(a))
        torch.cuda.synchronize()
        run = so.late_run(held, lambda: fn(a), [_backend])
        print('autograd %s: %d launches of %d entries, %s, issued in %.3f ms, %d outputs' % (
            which, len(run.entries), len(set(run.entries)), 'CONCLUSIVE' if run.conclusive else 'inconclusive', run.issue_ms, len(run.outs)))
        assert run.entries == entries, 'the late run launched other entries than the plain run'
        assert run.conclusive, 'autograd %s: the inputs were restored before the pass returned on the host: the run proves nothing' % which
        diff = so.difference(plain, run.outs)
        assert diff is None, 'autograd %s behind late inputs on a side stream: %s' % (which, diff)
    except RuntimeError as e:
        _guarded_fault(e, 'autograd ' + which)
        raise
    finally:
        hip.conv_mode = prev
        _clear(a['G'], a['D'])


# ---- the harness's own controls ---------------------------------------------------------------------------------------------------------------------------

def _bias_act_inputs():
    a = tgb._act_inputs((1, 5, 33, 31), DEV, 'ba')
    a = {n: a[n] for n in ('x', 'bias', 'nz', 'nw')}
    a['y'] = torch.full((1, 5, 33, 31), float('nan'), device=DEV)
    return a


def _bias_act(a, stream):
    _call('gc_bias_act_f32', _lib.ptr(a['x']), _lib.ptr(a['bias']), _lib.ptr(a['nz']), _lib.ptr(a['nw']), _lib.ptr(a['y']), 1, 5, 33 * 31, SLOPE, GAIN, stream)
    return [a['y']]


def _plane_dot_inputs():
    shape = (3, 2, 70, 161)
    gen = _gen(61)
    chunks = _lib.load().gc_bias_act_bwd_chunks(shape[2] * shape[3])
    return {'a': torch.randn(*shape, generator=gen).to(DEV), 'b': torch.randn(*shape, generator=gen).to(DEV), '_chunks': chunks,
            'partial': torch.full((6, chunks), float('nan'), device=DEV), 'out': torch.full((6,), float('nan'), device=DEV)}


def _plane_dot(a, first, second):
    _call('gc_plane_dot_f32', _lib.ptr(a['a']), _lib.ptr(a['b']), _lib.ptr(a['partial']), 6, 70 * 161, first)
    _call('gc_rows_sum_div_f32', _lib.ptr(a['partial']), None, _lib.ptr(a['out']), 6, a['_chunks'], second)
    return [a['out']]


def _control(a, call, delay_ms=so.D_MS):
    held = so.snapshot(a)
    plain = so.clone_outs(call())
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in plain)
    run = so.late_run(held, call, delay_ms=delay_ms)
    return run, so.difference(plain, run.outs)


@pytest.mark.gpu
def test_harness_catches_a_launch_on_stream_0(hip):
    """gc_bias_act_f32 handed stream handle 0 while the side stream is current and delayed (a legal call): it runs at once, on NaN inputs."""
    a = _bias_act_inputs()
    run, diff = _control(a, lambda: _bias_act(a, None))
    print('bias_act on stream 0: conclusive %s, %s' % (run.conclusive, diff))
    assert run.conclusive and diff is not None
    # the same call on the current stream passes
    run, diff = _control(a, lambda: _bias_act(a, _lib.stream_of(a['x'])))
    print('bias_act on the current stream: conclusive %s, %s' % (run.conclusive, diff))
    assert run.conclusive and diff is None


@pytest.mark.gpu
def test_harness_catches_a_second_stage_on_stream_0(hip):
    """gc_plane_dot_f32 on the current stream, gc_rows_sum_div_f32 on stream 0: the second stage sums partial sums that are not written yet."""
    a = _plane_dot_inputs()
    run, diff = _control(a, lambda: _plane_dot(a, _lib.stream_of(a['a']), None))
    print('second stage on stream 0: conclusive %s, %s' % (run.conclusive, diff))
    assert run.conclusive and diff is not None
    run, diff = _control(a, lambda: _plane_dot(a, _lib.stream_of(a['a']), _lib.stream_of(a['a'])))
    print('both stages on the current stream: conclusive %s, %s' % (run.conclusive, diff))
    assert run.conclusive and diff is None


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['bias_act', 'channel_sum', 'plane_dot'])
def test_harness_catches_a_wrapper_that_asks_for_the_wrong_stream(name, hip, monkeypatch):
    """Cases of the guarded table through HipBackend, with ``_lib.stream_of`` answering stream 0 during the late run only (one launch; two stages
    with a workspace; two entries): the whole path of test_guarded_table_on_a_side_stream reports it."""
    case, = [c for c in tgb.CASES if c.name == name]
    a = case.build(DEV)
    held = so.snapshot(a)
    plain = so.clone_outs(case.run(hip, a, None))
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, 'stream_of', lambda t: None)
    run = so.late_run(held, lambda: list(case.run(hip, a, None)), [_backend])
    monkeypatch.undo()
    diff = so.difference(plain, run.outs)
    print('%s with every launch on stream 0: conclusive %s, %s' % (name, run.conclusive, diff))
    assert run.conclusive and case.entries <= set(run.entries) and diff is not None


def _clear_then_accumulate(a, clear_stream):
    """The shape of the warp adjoint (warp.hip: hipMemsetAsync, then a kernel of atomic adds) with the stream of the clearing stage a
    parameter: the output is allocated as HipBackend allocates, cleared on ``clear_stream``, accumulated into on the current stream."""
    y = _backend.torch.empty(tuple(a['x'].shape), dtype=torch.float32, device=a['x'].device)
    with torch.cuda.stream(clear_stream):
        y.zero_()
    y.add_(a['x'])
    return [y]


@pytest.mark.gpu
def test_harness_catches_a_clearing_stage_on_stream_0(hip):
    """A stage that only WRITES -- it reads none of the late inputs -- and runs at once on stream 0: the accumulation behind the delay must not
    find its zeros.  The fill of the allocation, in side-stream order between the two, is what shows it."""
    a = {'x': torch.randn(3, 5, 7, generator=_gen(67)).to(DEV)}
    held = so.snapshot(a)
    plain = so.clone_outs(_clear_then_accumulate(a, torch.cuda.current_stream()))
    torch.cuda.synchronize()
    run = so.late_run(held, lambda: _clear_then_accumulate(a, torch.cuda.default_stream()), [_backend])
    diff = so.difference(plain, run.outs)
    print('clearing stage on stream 0: conclusive %s, %s' % (run.conclusive, diff))
    assert run.conclusive and diff is not None
    run = so.late_run(held, lambda: _clear_then_accumulate(a, torch.cuda.current_stream()), [_backend])
    diff = so.difference(plain, run.outs)
    print('clearing stage on the current stream: conclusive %s, %s' % (run.conclusive, diff))
    assert run.conclusive and diff is None


@pytest.mark.gpu
def test_harness_reports_a_delay_that_is_too_short_as_inconclusive(hip):
    """No delay, and a host that is still busy when the (correct) launches have run: the values are right and the run must NOT count."""
    a = _bias_act_inputs()

    def slow_host():
        outs = _bias_act(a, _lib.stream_of(a['x']))
        done = torch.cuda.Event()
        done.record()
        done.synchronize()          # (microseconds: nothing is queued in front of the launch)
        return outs
    run, diff = _control(a, slow_host, delay_ms=0.0)
    print('no delay: conclusive %s, %s' % (run.conclusive, diff))
    assert diff is None and not run.conclusive


@pytest.mark.gpu
def test_delay_calibration(hip):
    """delay(D) lasts D on the device within a factor of two either way (Event timing), on the clock it was calibrated with."""
    cal = so.calibrate()
    ms = so.measure_delay(so.D_MS)
    print('delay calibration: %s, %.4g per ms; delay(%.0f ms) measured %.1f ms' % (cal[0], cal[1], so.D_MS, ms))
    assert so.D_MS / 2 <= ms <= so.D_MS * 2
