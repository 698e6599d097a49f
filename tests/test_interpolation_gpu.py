"""gc_latent_interp_f32 and gc_noise_blend_f32 on the GPU (csrc/interp.hip through models/op/interp.py), and Inference.interpolate_by_group on them.

Linear and sqrt blends and the noise blend are compared BIT FOR BIT with the torch formulas of the module on the same device tensors.  Slerp is
compared with the formula in float64 on the upcast inputs: elementwise over ``out``, e = max |value - ref64| / s with s the row's max |value|
over the two blended inputs; the kernel's e must stay within 4 x the e of the float32 torch formula (the margin tests/test_inference_gpu.py
gives a fused kernel over the module path: another summation order in three row sums, device acos / sin a few ulp from torch's), and never
below 2^-23, the rounding of the result itself.  The slerp inputs are conditioned, and the test asserts it: every row slice has |cos omega| <= 0.9
in float64.  Every output is a guard-banded, NaN-poisoned buffer and every input has NaN around it and between its strided rows
(tests/guarded_alloc.py).  Measured errors: profiles/interpolation.md.

Latent shapes (B, L, lo, hi): the id / other / age groups of the ffhq configuration (an empty first slice, an empty last slice, all three), a row
shorter than a workgroup (48) and one that is no multiple of anything (50, slices of 17 / 18 / 15); for the exact modes also (2, 10, 3, 7) and
(1, 5, 0, 5) with both outer slices empty.  Frames: 1, 2, 10 and the limit 64.  ``fixed`` is one expanded row (stride 0), ``from`` has row stride L + 1.
"""
import ctypes

import numpy as np
import pytest
import torch

import guarded_alloc
import inference_checks as ic

from gan_control_amd import _lib
from gan_control_amd.inference import Inference
from gan_control_amd.models.gan_model import NoiseInjection
from gan_control_amd.models.op import _backend
from gan_control_amd.models.op import fc_stack as fcs
from gan_control_amd.models.op import interp

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SHAPES = [(4, 512, 0, 128), (4, 512, 448, 512), (5, 512, 320, 384), (1, 48, 16, 32), (3, 50, 17, 35)]
EXACT_ONLY = [(2, 10, 3, 7), (1, 5, 0, 5)]
FRAMES = [1, 2, 10, 64]


def bits(t):
    return t.contiguous().view(torch.int32)


def latent_inputs(b, l, seed):
    """(row [1, l], from [b, l] with row stride l + 1, to [b, l]) on the device."""
    gen = torch.Generator().manual_seed(seed)
    row = torch.randn(1, l, generator=gen).to(DEV)
    z_from = torch.randn(b, l + 1, generator=gen).to(DEV)[:, :l]
    z_to = torch.randn(b, l, generator=gen).to(DEV)
    return row, z_from, z_to


def run_latents(row, z_from, z_to, lo, hi, wa, wb, mode, fill='nan', poison='nan', shift=0):
    """One interpolate_latents call on a guarded output and hostile copies of the inputs -> the result."""
    b = z_to.shape[0]
    h_row, h_to = guarded_alloc.hostile(row, fill, shift), guarded_alloc.hostile(z_to, fill, shift)
    fixed = h_row.expand(b, -1)
    if z_from is None:          # the first segment of a film: the walk starts at the expanded row itself
        z_from, h_from = row, fixed
    else:
        h_from = guarded_alloc.hostile(z_from, fill, shift)
        assert h_from.stride(0) == z_from.shape[1] + 1 or b == 1
    assert fixed.stride(0) == 0 or b == 1
    with torch.no_grad(), guarded_alloc.guarded(interp, poison=poison) as guard:
        out = interp.interpolate_latents(fixed, h_from, h_to, lo, hi, wa, wb, mode)
        assert guard.check() == []
    assert guard.entries == [interp.LATENT_ENTRY] and len(guard.allocations) == 1
    for h, t in ((h_row, row), (h_from, z_from), (h_to, z_to)):
        assert h is fixed or guarded_alloc.hostile_changes(h, t) is None
    assert out.shape == (2, wa.shape[0], b, z_to.shape[1]) and out.is_contiguous() and bool(torch.isfinite(out).all())
    return out


@pytest.mark.parametrize('frames', FRAMES)
@pytest.mark.parametrize('mode', ['linear', 'sqrt'])
@pytest.mark.parametrize('b,l,lo,hi', SHAPES + EXACT_ONLY)
def test_linear_and_sqrt_latents_equal_the_torch_formula_bit_for_bit(b, l, lo, hi, mode, frames):
    row, z_from, z_to = latent_inputs(b, l, 100 * l + 10 * b + frames)
    wa, wb = interp.interpolation_weights(frames, mode)
    out = run_latents(row, z_from, z_to, lo, hi, wa, wb, mode)
    with torch.no_grad():
        want = interp.interpolate_latents_reference(row.expand(b, -1), z_from, z_to, lo, hi, wa, wb, mode)
    assert torch.equal(bits(out), bits(want))
    # the first segment of a film: the expanded row is also where the walk starts; and another poison, fill and alignment
    out = run_latents(row, None, z_to, lo, hi, wa, wb, mode, fill='big', poison='big', shift=4)
    with torch.no_grad():
        want = interp.interpolate_latents_reference(row.expand(b, -1), row.expand(b, -1), z_to, lo, hi, wa, wb, mode)
    assert torch.equal(bits(out), bits(want))


def slice_cosines(z_from, z_to, lo, hi):
    x, y = z_from.double(), z_to.double()
    cos = []
    for a, e in ((0, lo), (lo, hi), (hi, x.shape[1])):
        if e > a:
            cos.append((x[:, a:e] * y[:, a:e]).sum(1) / (x[:, a:e].norm(dim=1) * y[:, a:e].norm(dim=1)))
    return torch.cat(cos)


@pytest.mark.parametrize('frames', FRAMES)
@pytest.mark.parametrize('b,l,lo,hi', SHAPES)
def test_slerp_latents_against_the_float64_formula(b, l, lo, hi, frames):
    row, z_from, z_to = latent_inputs(b, l, 100 * l + 10 * b + frames)
    assert float(slice_cosines(z_from, z_to, lo, hi).abs().max()) <= 0.9          # the condition on the inputs
    wa, wb = interp.interpolation_weights(frames, 'slerp')
    out = run_latents(row, z_from, z_to, lo, hi, wa, wb, 'slerp')
    fixed = row.expand(b, -1)
    with torch.no_grad():
        ref64 = interp.interpolate_latents_reference(fixed.double(), z_from.double(), z_to.double(), lo, hi, wa, wb, 'slerp')
        ref32 = interp.interpolate_latents_reference(fixed, z_from, z_to, lo, hi, wa, wb, 'slerp')
    s = torch.maximum(z_from.abs().max(dim=1).values, z_to.abs().max(dim=1).values).double().view(1, 1, b, 1)
    e_kernel = float(((out.double() - ref64).abs() / s).max())
    e_torch = float(((ref32.double() - ref64).abs() / s).max())
    print('slerp B=%d L=%-3d group [%d, %d) P=%-2d  e_kernel %.3e  e_torch %.3e' % (b, l, lo, hi, frames, e_kernel, e_torch))
    assert e_kernel <= 4 * max(e_torch, 2.0 ** -23), (e_kernel, e_torch)
    # what is not blended is copied: the frozen group in film 0, everything else in film 1
    assert torch.equal(out[0, :, :, lo:hi], fixed[:, lo:hi].expand(frames, -1, -1))
    assert torch.equal(out[1, :, :, :lo], fixed[:, :lo].expand(frames, -1, -1)) and torch.equal(out[1, :, :, hi:], fixed[:, hi:].expand(frames, -1, -1))
    # the same bits again, on the other poison and fill at another alignment
    again = run_latents(row, z_from, z_to, lo, hi, wa, wb, 'slerp', fill='big', poison='big', shift=4)
    assert torch.equal(bits(out), bits(again))


def noise_lists(name, seed=0):
    gen = torch.Generator().manual_seed(seed)
    if name.startswith('g32'):          # the 7 maps of the 32 x 32 generator
        batch = int(name[4:])
        shapes = [(batch, 1, 4, 4)] + [(batch, 1, 2 ** i, 2 ** i) for i in range(3, 6) for _ in range(2)]
    else:
        shapes = {'one_1024': [(1, 1, 1024, 1024)], 'odd': [(3, 1, 5, 7), (1, 1, 1, 1)], 'many': [(1, 1, 4, 4)] * 32}[name]
    return [torch.randn(*s, generator=gen).to(DEV) for s in shapes], [torch.randn(*s, generator=gen).to(DEV) for s in shapes]


def run_noise(a, b, wa, wb, out=None, fill='nan', shift=0, same=False):
    ha = [guarded_alloc.hostile(t, fill, shift) for t in a]
    hb = ha if same else [guarded_alloc.hostile(t, fill, shift) for t in b]
    with torch.no_grad(), guarded_alloc.guarded(interp) as guard:
        got = interp.blend_noise(ha, hb, wa, wb, out=out)
        assert guard.check() == []
    assert guard.entries == [interp.NOISE_ENTRY] and len(guard.allocations) == (len(a) if out is None else 0)
    for h, t in list(zip(ha, a)) + list(zip(hb, a if same else b)):
        assert guarded_alloc.hostile_changes(h, t) is None
    return got


@pytest.mark.parametrize('mode', ['linear', 'sqrt'])
@pytest.mark.parametrize('name', ['g32_1', 'g32_4', 'one_1024', 'odd', 'many'])
def test_noise_blend_equals_the_torch_formula_bit_for_bit(name, mode):
    a, b = noise_lists(name)
    was, wbs = interp.interpolation_weights(10, mode)
    assert (was[0], wbs[0], was[-1], wbs[-1]) == (1, 0, 0, 1)
    frames = range(10) if name != 'one_1024' else (0, 3, 9)
    out = None
    for k in frames:
        with torch.no_grad():
            want = interp.blend_noise_reference(a, b, was[k], wbs[k])
        shift = 4 * (k % 2)          # odd frames: inputs off the 16-byte boundary, the 4-byte path
        got = run_noise(a, b, was[k], wbs[k], shift=shift)
        assert len(got) == len(a) and all(g.shape == x.shape and torch.equal(bits(g), bits(w)) for g, x, w in zip(got, a, want))
        # a reused out list: the same tensors come back, rewritten
        if out is None:
            out = [torch.full_like(x, float('nan')) for x in a]
        back = run_noise(a, b, was[k], wbs[k], out=out, shift=shift)
        assert all(o is p for o, p in zip(back, out)) and all(torch.equal(bits(o), bits(w)) for o, w in zip(out, want))
        # a is b: the reference evaluates wa * n + wb * n, which is not n bit for bit
        with torch.no_grad():
            want = interp.blend_noise_reference(a, a, was[k], wbs[k])
        got = run_noise(a, a, was[k], wbs[k], same=True, shift=shift)
        assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want))


def test_noise_blend_tails_and_unaligned_outputs():
    """Counts of 1 .. 9 and 4095 .. 4101 elements (the 16-byte words, the 4-byte tail, the 4096-element workgroup), outputs on and off the boundary."""
    gen = torch.Generator().manual_seed(4)
    counts = list(range(1, 10)) + list(range(4095, 4102)) + [8191, 8193]
    a = [torch.randn(c, generator=gen).to(DEV) for c in counts]
    b = [torch.randn(c, generator=gen).to(DEV) for c in counts]
    with torch.no_grad():
        want = interp.blend_noise_reference(a, b, 0.3, 0.7)
    got = run_noise(a, b, 0.3, 0.7)
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want))
    with guarded_alloc.guarded(interp) as guard:
        full = [guard.empty(c + 1, dtype=torch.float32, device=DEV) for c in counts]
        out = [t[1:] for t in full]          # 4 bytes past the boundary
        interp.blend_noise(a, b, 0.3, 0.7, out=out)
        assert guard.check() == []
    assert all(torch.equal(bits(o), bits(w)) for o, w in zip(out, want))
    assert all(bool(torch.isnan(t[0])) for t in full)          # the word in front stays poison


def _latent_rc(lib, fixed, fs, z_from, rs, z_to, ts, batch, latent, lo, hi, wa, wb, frames, mode, out):
    ptr = lambda t: None if t is None else t.data_ptr()
    wp = lambda w: None if w is None else w.ctypes.data
    return lib.gc_latent_interp_f32(ptr(fixed), fs, ptr(z_from), rs, ptr(z_to), ts, batch, latent, lo, hi, wp(wa), wp(wb), frames, mode, ptr(out),
                                    _lib.stream_of(out if out is not None else z_to))


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    x = torch.randn(4, 16, device=DEV)
    out = torch.full((2, 64, 4, 16), 3.0, device=DEV)
    w = np.full(65, 0.5, dtype=np.float32)
    ok = dict(fixed=x, fs=16, z_from=x, rs=16, z_to=x, ts=16, batch=4, latent=16, lo=4, hi=8, wa=w, wb=w, frames=2, mode=0, out=out)
    for code, word, change in ((-1, 'null pointer', dict(fixed=None)), (-1, 'null pointer', dict(out=None)), (-1, 'null pointer', dict(wb=None)),
                               (-1, 'at least 1', dict(frames=0)), (-2, 'at most 64', dict(frames=65)), (-1, 'lo < hi', dict(lo=8, hi=8)),
                               (-1, 'lo < hi', dict(lo=9, hi=8)), (-1, 'lo < hi', dict(hi=17)), (-1, 'lo < hi', dict(lo=-1)),
                               (-1, 'negative stride', dict(rs=-16)), (-1, 'row stride 8', dict(fs=8)), (-1, 'unknown mode 3', dict(mode=3)),
                               (-1, 'at least 1', dict(batch=0))):
        assert _latent_rc(lib, **dict(ok, **change)) == code, change
        assert word in lib.gc_last_error().decode(), (change, lib.gc_last_error())
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert _latent_rc(lib, **dict(ok, fs=0)) == 0          # the same call within the rules (an expanded row) runs
    torch.cuda.synchronize()
    assert bool((out.view(-1)[:2 * 2 * 4 * 16] != 3.0).all()) and bool((out.view(-1)[2 * 2 * 4 * 16:] == 3.0).all())

    maps = [torch.randn(16, device=DEV) for _ in range(33)]
    outs = [torch.full((16,), 3.0, device=DEV) for _ in range(33)]
    table = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    counts = (ctypes.c_int64 * 33)(*([16] * 33))
    stream = _lib.stream_of(maps[0])
    pa, po = table(maps), table(outs)
    zero = (ctypes.c_int64 * 33)(*([16, 0] + [16] * 31))
    nulls = (ctypes.c_void_p * 2)(maps[0].data_ptr(), None)
    for code, word, args in ((-1, 'null pointer', (None, pa, po, counts, 2)), (-1, 'null pointer', (pa, pa, po, None, 2)),
                             (-1, 'null pointer', (pa, nulls, po, counts, 2)), (-1, 'empty list', (pa, pa, po, counts, 0)),
                             (-2, 'at most 32', (pa, pa, po, counts, 33)), (-1, '0 elements', (pa, pa, po, zero, 2)),
                             (-1, 'overlaps', (pa, pa, pa, counts, 2))):
        assert lib.gc_noise_blend_f32(*args, 0.5, 0.5, stream) == code, word
        assert word in lib.gc_last_error().decode(), (word, lib.gc_last_error())
    torch.cuda.synchronize()
    assert all(bool((o == 3.0).all()) for o in outs)
    assert lib.gc_noise_blend_f32(pa, pa, po, counts, 32, 0.5, 0.5, stream) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(o, 0.5 * m + 0.5 * m) for o, m in zip(outs[:32], maps)) and bool((outs[32] == 3.0).all())


def test_shapes_the_kernels_do_not_take_raise_value_errors():
    x = torch.randn(3, 32, device=DEV)
    wa, wb = interp.interpolation_weights(4, 'linear')
    with guarded_alloc.guarded(interp) as guard:
        with pytest.raises(ValueError, match='float64'):
            interp.interpolate_latents(x.double(), x.double(), x.double(), 8, 16, wa, wb, 'linear')
        with pytest.raises(ValueError, match='65 frames'):
            interp.interpolate_latents(x, x, x, 8, 16, *interp.interpolation_weights(65, 'slerp'), 'slerp')
        with pytest.raises(ValueError, match='adjacent'):
            interp.interpolate_latents(x, torch.randn(3, 64, device=DEV)[:, ::2], x, 8, 16, wa, wb, 'linear')
        with pytest.raises(ValueError, match='0 <= lo < hi'):
            interp.interpolate_latents(x, x, x, 16, 16, wa, wb, 'linear')
        maps = [torch.randn(2, 1, 8, 8, device=DEV) for _ in range(3)]
        with pytest.raises(ValueError, match='overlaps'):
            interp.blend_noise(maps, maps, 0.5, 0.5, out=maps)
        with pytest.raises(ValueError, match='overlaps'):
            interp.blend_noise(maps[:2], maps[:2], 0.5, 0.5, out=[maps[2], maps[0][:]])
        with pytest.raises(ValueError, match='float64'):
            interp.blend_noise([m.double() for m in maps], [m.double() for m in maps], 0.5, 0.5)
        with pytest.raises(ValueError, match='dense'):
            interp.blend_noise([maps[0][:, :, ::2]], [maps[1][:, :, ::2]], 0.5, 0.5)
        with pytest.raises(ValueError, match='33 maps'):
            interp.blend_noise(maps * 11, maps * 11, 0.5, 0.5)
    assert guard.entries == [] and guard.allocations == []
    # a wanted gradient takes the torch formula, and gives one
    xg = x.clone().requires_grad_(True)
    with guarded_alloc.guarded(interp) as guard:
        z = interp.interpolate_latents(x, xg, torch.randn(3, 32, device=DEV), 8, 16, wa, wb, 'slerp')
    assert guard.entries == [] and z.requires_grad
    z.sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())


@pytest.fixture(scope='module')
def inf32(tmp_path_factory):
    root = tmp_path_factory.mktemp('interpolation')
    ic.write_model_dir(str(root), ic.ffhq_config(32))
    inf = Inference(str(root))
    with torch.no_grad():          # the noise strengths are zero as constructed: with values, the injected noise reaches the images
        for k, m in enumerate(m for m in inf.model.modules() if isinstance(m, NoiseInjection)):
            m.weight.fill_(0.05 * (k + 1))
    return inf


@pytest.fixture
def launches(monkeypatch):
    """The entry names HipBackend._launch is called with, in order."""
    seen = []
    real = _backend.HipBackend._launch

    def recording(self, dev, entry, *a, **k):
        seen.append(entry)
        return real(self, dev, entry, *a, **k)

    monkeypatch.setattr(_backend.HipBackend, '_launch', recording)
    return seen


def test_interpolate_by_group_end_to_end(inf32, launches, monkeypatch):
    assert inf32.device.type == 'cuda'
    zs, calls = [], []
    real = Inference.interpolation_latents

    def recording(self, *a, **k):
        z = real(self, *a, **k)
        zs.append(z)
        return z

    monkeypatch.setattr(Inference, 'interpolation_latents', recording)
    hook = inf32.model.register_forward_pre_hook(
        lambda m, args, kwargs: calls.append((args[0][0].clone(), [n.clone() for n in kwargs['noise']], kwargs['input_is_latent'])), with_kwargs=True)
    try:
        films = inf32.interpolate_by_group('orientation', None, batch=2, num_of_intermediate_latents=2, pics_per_interpolation=3, interpolation='slerp',
                                           generator=torch.Generator().manual_seed(9), return_list=True)
    finally:
        hook.remove()
    seen = list(launches)
    assert films[0].shape == (6, 2, 3, 32, 32) and films[1].shape == (6, 2, 3, 32, 32) and not films[0].is_cuda
    # per segment one latent entry and one mapping call, per frame one noise blend
    assert seen.count(interp.LATENT_ENTRY) == 2 and seen.count(fcs.ENTRY) == 2 and seen.count(interp.NOISE_ENTRY) == 6
    order = [e for e in seen if e in (interp.LATENT_ENTRY, fcs.ENTRY, interp.NOISE_ENTRY)]
    assert order == ([interp.LATENT_ENTRY, fcs.ENTRY] + [interp.NOISE_ENTRY] * 3) * 2
    assert len(zs) == 2 and len(calls) == 12
    with torch.no_grad():
        for seg, z in enumerate(zs):
            assert z.shape == (2, 3, 2, 512) and z.is_cuda
            w = inf32.style(z.reshape(-1, 512)).reshape(2, 3, 2, 512)
            for f in range(3):
                for film in (0, 1):
                    cw, cn, is_w = calls[6 * seg + 2 * f + film]
                    assert is_w is True and torch.equal(cw, w[film, f])
                    img, _ = inf32.model([cw], input_is_latent=True, noise=cn)
                    assert torch.equal(films[film][3 * seg + f], img.cpu())
                assert all(torch.equal(a, b) for a, b in zip(calls[6 * seg + 2 * f][1], calls[6 * seg + 2 * f + 1][1]))          # one noise per frame
    # repeatable; and the noise of a frame is the blend, not the noise itself
    again = inf32.interpolate_by_group('orientation', None, batch=2, num_of_intermediate_latents=2, pics_per_interpolation=3, interpolation='slerp',
                                       generator=torch.Generator().manual_seed(9), return_list=True)
    assert torch.equal(films[0], again[0]) and torch.equal(films[1], again[1])
    wa, wb = interp.interpolation_weights(3, 'linear')
    n0 = calls[0][1]
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(calls[2][1], interp.blend_noise_reference(n0, n0, wa[1], wb[1])))


def test_existing_callers_launch_what_they_launched(inf32, launches):
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    inf32.gen_batch(batch_size=2)
    assert fcs.ENTRY in launches and interp.LATENT_ENTRY not in launches and interp.NOISE_ENTRY not in launches
    del launches[:]
    tr = GeneratorTrainer(default_config(32, 4), device=DEV, seed=0, fused_adam=False)
    tr.train(iters=1)
    assert len(launches) > 50 and interp.LATENT_ENTRY not in launches and interp.NOISE_ENTRY not in launches
