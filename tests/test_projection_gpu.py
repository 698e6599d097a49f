"""Image projection on the GPU: gc_bias_act_bwd_noise_f32 (models/op/noise_grad.py), the generator's noise-map gradients, the fused noise
regulariser / normaliser (csrc/noise_reg.hip through projection/noise_ops.py), make_image and the projection loop.

Expectations are float64 on the host: the reference's own results (tests/golden/projection.npz) or the documented CPU formulas, which
test_projection.py holds to that fixture at 1e-12.  Kernel cases run plainly, three times for the bits, and on poisoned guard-banded
allocations (tests/guarded_alloc.py) with their inputs between hostile words."""
import numpy as np
import pytest
import torch

import guarded_alloc
import projection_checks as pc
from conftest import group, rel_err

from gan_control_amd import _lib, projection
from gan_control_amd.models.op import _backend, noise_grad
from gan_control_amd.projection import noise_ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GOLD = pc.GOLD
SLOPE, GAIN = 0.2, 2 ** 0.5


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


# ---- the pixel-sum kernel ---------------------------------------------------------------------------------------------------------------
def pixel_inputs(b, c, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    gy, y = torch.randn(b, c, h, w, generator=gen), torch.randn(b, c, h, w, generator=gen)
    y.reshape(-1)[::7] = 0.0                                   # exact zeros take the negative branch, as in gc_bias_act_bwd_f32
    return gy, y, torch.tensor([0.37])


def pixel_expected(gy, y, nw):
    g = gy.double() * torch.where(y > 0, torch.tensor(GAIN, dtype=torch.float64), torch.tensor(GAIN * SLOPE, dtype=torch.float64))
    return g, g.sum(1, keepdim=True) * nw.double()


PLANES = [(4, 4), (5, 7), (33, 31), (64, 64), (129, 129)]


@pytest.mark.parametrize('c', [1, 5, 32, 512])
@pytest.mark.parametrize('plane', PLANES, ids=['%dx%d' % p for p in PLANES])
def test_pixel_sums_both_forms(plane, c):
    hip = _backend.get()
    for b in (1, 2):
        gy, y, nw = pixel_inputs(b, c, *plane, seed=b + 10 * c + plane[0])
        want_g, want_n = pixel_expected(gy, y, nw)
        dgy, dy_, dnw = gy.to(DEV), y.to(DEV), nw.to(DEV)
        g_pre, gn = noise_grad.masked(dgy, dy_, dnw, SLOPE, GAIN)
        assert gn.shape == (b, 1) + plane
        e1, e2 = rel_err(g_pre, want_g), rel_err(gn, want_n)
        print('masked  b %d c %d %s: g_pre %.2e, sums %.2e' % (b, c, plane, e1, e2))
        assert e1 <= 2e-5 and e2 <= 2e-5
        assert torch.equal(bits(g_pre), bits(hip.bias_act_bwd(dgy, dy_, SLOPE, GAIN))), 'dx must be the bits of gc_bias_act_bwd_f32'
        only = noise_grad.pixel_sums(g_pre, dnw)
        e3 = rel_err(only, want_n)
        print('sums    b %d c %d %s: %.2e' % (b, c, plane, e3))
        assert e3 <= 2e-5
        assert torch.equal(bits(only), bits(gn)), 'both forms add the same numbers in the same order'
        for _ in range(2):
            g2, n2 = noise_grad.masked(dgy, dy_, dnw, SLOPE, GAIN)
            assert torch.equal(bits(g2), bits(g_pre)) and torch.equal(bits(n2), bits(gn))
            assert torch.equal(bits(noise_grad.pixel_sums(g_pre, dnw)), bits(only))


GUARDED_PIXEL = [(2, 5, 5, 7), (2, 32, 33, 31), (1, 512, 4, 4), (2, 5, 129, 129)]


@pytest.mark.parametrize('shape', GUARDED_PIXEL, ids=['x'.join(map(str, s)) for s in GUARDED_PIXEL])
def test_pixel_sums_on_guarded_buffers_with_hostile_inputs(shape):
    gy, y, nw = pixel_inputs(*shape, seed=sum(shape))
    dgy, dy_, dnw = gy.to(DEV), y.to(DEV), nw.to(DEV)
    plain_g, plain_n = noise_grad.masked(dgy, dy_, dnw, SLOPE, GAIN)
    for poison, fill, shift in (('nan', 'nan', 0), ('big', 'big', 4), ('nan', 'zero', 4)):          # shift 4: every base 4 bytes off a 16-byte boundary
        hg, hy, hw = (guarded_alloc.hostile(t, fill, shift) for t in (dgy, dy_, dnw))
        assert shift == 0 or hg.data_ptr() % 16 == 4
        with guarded_alloc.guarded(noise_grad, poison=poison) as guard:
            g_pre, gn = noise_grad.masked(hg, hy, hw, SLOPE, GAIN)
            only = noise_grad.pixel_sums(hg, hw)          # the second form reads gy as g_pre
            violations = guard.check()
        assert not violations, violations
        assert guard.entries == [noise_grad.ENTRY] * 2 and len(guard.allocations) == 3
        assert torch.equal(bits(g_pre), bits(plain_g)) and torch.equal(bits(gn), bits(plain_n)), (poison, fill)
        assert torch.equal(bits(only), bits(noise_grad.pixel_sums(dgy, dnw)))
        for h, t in ((hg, dgy), (hy, dy_), (hw, dnw)):
            assert guarded_alloc.hostile_changes(h, t) is None


def test_pixel_sums_refusals_launch_nothing():
    hip, dev = _backend.get(), torch.device(DEV)
    gy, y, nw = (t.to(DEV) for t in pixel_inputs(2, 3, 4, 5, seed=1))
    dx, dn = torch.full_like(gy, 7.0), torch.full((2, 1, 4, 5), 7.0, device=DEV)
    args = dict(dy=_lib.ptr(gy), y=_lib.ptr(y), nw=_lib.ptr(nw), dx=_lib.ptr(dx), dn=_lib.ptr(dn), b=2, c=3, inner=20)
    for kw, text in (({'dy': None}, 'null'), ({'nw': None}, 'null'), ({'dn': None}, 'null'), ({'dx': None}, 'y_ref without dx'), ({'b': 0}, 'extents'),
                     ({'c': -1}, 'extents'), ({'inner': 0}, 'extents'), ({'b': 70000}, '65535')):
        a = dict(args, **kw)
        with pytest.raises(RuntimeError, match='gc_bias_act_bwd_noise_f32 failed.*' + text):
            hip._launch(dev, noise_grad.ENTRY, a['dy'], a['y'], a['nw'], a['dx'], a['dn'], a['b'], a['c'], a['inner'], SLOPE, GAIN, _lib.stream_of(gy))
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all()) and bool((dn == 7.0).all())


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
def check_generator_noise_grads(tol):
    """Per-tensor gradient norms against the reference's float64 gradients, the bar of the network gradients in test_ops_gpu.py."""
    r = group(GOLD, 'gen')
    img, grads, zgrad = pc.generator_noise_grads(DEV)
    assert zgrad is not None and len(grads) == int(r['count'])
    for i, g in enumerate(grads):
        assert g is not None, 'noise map %d has no gradient' % i
        want = r['g%d' % i].double()
        norm_err = abs(float(g.double().norm().cpu()) - float(want.norm())) / float(want.norm())
        diff = float((g.double().cpu() - want).norm() / want.norm())
        print('noise map %d %s: norm err %.3e, |difference| / |reference| %.3e' % (i, tuple(g.shape), norm_err, diff))
        # (the norm bar alone admits an error orthogonal to the gradient of up to sqrt(2 tol) of its length: hold the difference to that)
        assert norm_err <= tol and diff <= (2 * tol) ** 0.5, (i, norm_err, diff)


def test_generator_noise_gradients_f32():
    check_generator_noise_grads(2e-3)


def test_generator_noise_gradients_bf16x3(bf16x3_mode):
    check_generator_noise_grads(5e-3)


def test_fir_activation_noise_gradient_on_the_device():
    """The route of an up-sampling StyledConv at the sizes the FIR tile kernel takes (the 32 x 32 generator never reaches it)."""
    pc.check_fir_act_noise_grad(DEV, 2e-5)


# ---- noise_regularize / noise_normalize_ ---------------------------------------------------------------------------------------------------
def make_maps(shapes, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for b, s in shapes:
        n = torch.randn(b, 1, s, s, generator=gen)
        if kind == 'smooth':          # strongly correlated, level means far from zero
            ramp = torch.linspace(0, 2 * np.pi, s)
            n = torch.sin(ramp)[None, None, :, None] * torch.cos(0.5 * ramp)[None, None, None, :] + 0.75 + 0.1 * n
        out.append(n)
    return out


def generator_list(size, batch):
    return [(batch, 4)] + [(batch, 2 ** i) for i in range(3, int(np.log2(size)) + 1) for _ in range(2)]


def reg_expected(maps, cot):
    leaves = [m.double().requires_grad_(True) for m in maps]
    loss = noise_ops.noise_regularize_reference(leaves)
    return loss.detach(), torch.autograd.grad(loss * cot, leaves)


def reg_on_device(maps, cot):
    leaves = [m.to(DEV).requires_grad_(True) for m in maps]
    loss = projection.noise_regularize(leaves)
    (loss * cot).backward()
    return loss.detach(), [m.grad for m in leaves]


def check_reg(maps, cot=-2.5e4, runs=3):
    want_loss, want_grads = reg_expected(maps, cot)
    loss, grads = reg_on_device(maps, cot)
    assert loss.dim() == 0
    e = rel_err(loss, want_loss)
    errs = [rel_err(g, w) for g, w in zip(grads, want_grads)]
    print('noise_regularize %s: loss %.3e, gradients max %.3e' % ([tuple(m.shape) for m in maps][:3], e, max(errs)))
    assert e <= 2e-5 and max(errs) <= 2e-5, (e, errs)
    for _ in range(runs - 1):
        l2, g2 = reg_on_device(maps, cot)
        assert torch.equal(bits(l2), bits(loss)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(g2, grads))
    return loss, grads


SINGLE = [(b, s) for s in (4, 8, 16, 32, 128, 256) for b in (1, 2, 3)]


@pytest.mark.parametrize('kind', ['white', 'smooth'])
@pytest.mark.parametrize('b,s', SINGLE, ids=['%dx%d' % p for p in SINGLE])
def test_noise_regularize_single_maps(b, s, kind):
    check_reg(make_maps([(b, s)], kind, 100 * s + b))


@pytest.mark.parametrize('kind', ['white', 'smooth'])
@pytest.mark.parametrize('size', [32, 256])
def test_noise_regularize_generator_lists(size, kind):
    check_reg(make_maps(generator_list(size, 2), kind, size))


@pytest.mark.parametrize('kind', ['white', 'smooth'])
def test_noise_regularize_full_eight_levels(kind):
    check_reg(make_maps([(1, 1024)], kind, 1024), runs=2)


@pytest.mark.parametrize('kind', ['white', 'smooth'])
def test_noise_regularize_against_the_fixture(kind):
    r = group(GOLD, 'reg/' + kind)
    maps = [r['x%d' % i].float().to(DEV).requires_grad_(True) for i in range(int(r['count']))]
    loss = projection.noise_regularize(maps)
    loss.backward()
    assert rel_err(loss, r['loss']) <= 2e-5
    for i, m in enumerate(maps):
        assert rel_err(m.grad, r['g%d' % i]) <= 2e-5, i


def test_noise_regularize_launch_count_does_not_depend_on_the_list():
    counts = []
    for size in (32, 256):
        maps = [m.to(DEV).requires_grad_(True) for m in make_maps(generator_list(size, 2), 'white', size)]
        with guarded_alloc.guarded(noise_ops, poison='nan') as guard:
            projection.noise_regularize(maps).backward()
            projection.noise_normalize_(maps)
            assert not guard.check()
        counts.append(list(guard.entries))
    assert counts[0] == counts[1] == [noise_ops.REG_FWD, noise_ops.REG_BWD, noise_ops.NORMALIZE]


@pytest.mark.parametrize('kind', ['white', 'smooth'])
def test_noise_regularize_on_guarded_buffers_with_hostile_inputs(kind):
    shapes = [(2, 4), (1, 8), (3, 16), (2, 32), (1, 256)]
    maps = make_maps(shapes, kind, 77)
    plain_loss, plain_grads = check_reg(maps, runs=1)
    for poison, fill, shift in (('nan', 'nan', 0), ('big', 'big', 4)):
        placed = [m.to(DEV) for m in maps]
        hostile = [guarded_alloc.hostile(p, fill, shift).requires_grad_(True) for p in placed]
        with guarded_alloc.guarded(noise_ops, poison=poison) as guard:          # the loss, the workspace and every gradient are guarded
            loss = projection.noise_regularize(hostile)
            (loss * -2.5e4).backward()
            violations = guard.check()
        assert not violations, violations
        assert guard.entries == [noise_ops.REG_FWD, noise_ops.REG_BWD] and len(guard.allocations) == 2 + len(maps)
        assert torch.equal(bits(loss), bits(plain_loss)), (poison, fill)
        for h, p, g in zip(hostile, placed, plain_grads):
            assert torch.equal(bits(h.grad), bits(g))
            rec = h.detach()
            rec._hostile = h._hostile
            assert guarded_alloc.hostile_changes(rec, p) is None


def norm_expected(maps):
    out = [m.double().clone() for m in maps]
    noise_ops.noise_normalize_reference_(out)
    return out


@pytest.mark.parametrize('kind', ['white', 'smooth'])
def test_noise_normalize_shapes(kind):
    for shapes in [[p] for p in SINGLE] + [generator_list(32, 2), generator_list(256, 2), [(1, 1024)]]:
        maps = make_maps(shapes, kind, 5 + len(shapes) + shapes[0][1])
        want = norm_expected(maps)
        dev = [m.to(DEV) for m in maps]
        assert projection.noise_normalize_(dev) is None
        errs = [rel_err(d, w) for d, w in zip(dev, want)]
        assert max(errs) <= 2e-5, (shapes[:2], errs)
        again = [m.to(DEV) for m in maps]
        projection.noise_normalize_(again)
        assert all(torch.equal(bits(a), bits(d)) for a, d in zip(again, dev))


def test_noise_normalize_keeps_its_accuracy_far_from_zero():
    """mean 1000, std 1: a one-pass variance (sum of squares minus squared sum) has lost every digit here."""
    gen = torch.Generator().manual_seed(12)
    maps = [torch.randn(2, 1, 128, 128, generator=gen) + 1000.0, torch.randn(1, 1, 8, 8, generator=gen) + 1000.0]
    want = norm_expected(maps)
    dev = [m.to(DEV) for m in maps]
    projection.noise_normalize_(dev)
    for d, w in zip(dev, want):
        err = float((d.double().cpu() - w).abs().max())
        print('normalised output, mean 1000: max abs err %.3e' % err)
        assert err <= 1e-3


def test_noise_normalize_on_guarded_buffers_with_hostile_inputs():
    maps = make_maps([(2, 4), (3, 16), (1, 128)], 'smooth', 9)
    plain = [m.to(DEV) for m in maps]
    projection.noise_normalize_(plain)
    for poison, fill, shift in (('nan', 'nan', 0), ('big', 'big', 4)):
        hostile = [guarded_alloc.hostile(m.to(DEV), fill, shift) for m in maps]
        with guarded_alloc.guarded(noise_ops, poison=poison) as guard:
            projection.noise_normalize_(hostile)
            violations = guard.check()
        assert not violations, violations
        assert guard.entries == [noise_ops.NORMALIZE] and len(guard.allocations) == 1
        for h, p in zip(hostile, plain):
            assert torch.equal(bits(h), bits(p))
            assert guarded_alloc.hostile_changes(h, p) is None          # nothing but the map's own elements was written


def test_noise_ops_refusals():
    with pytest.raises(ValueError, match=r'shape \(2, 1, 12, 12\)'):
        projection.noise_regularize([torch.zeros(2, 1, 12, 12, device=DEV)])
    with pytest.raises(ValueError, match=r'shape \(1, 1, 2048, 2048\)'):
        projection.noise_regularize([torch.zeros(1, 1, 8, 8, device=DEV), torch.zeros(1, 1, 2048, 2048, device=DEV)])
    with pytest.raises(ValueError, match='different devices'):
        projection.noise_regularize([torch.zeros(1, 1, 8, 8, device=DEV), torch.zeros(1, 1, 8, 8)])
    lib = _lib.load()
    import ctypes
    sizes, batches = (ctypes.c_int32 * 2)(8, 12), (ctypes.c_int32 * 2)(1, 1)
    assert lib.gc_noise_reg_workspace(sizes, batches, 2) == 0 and b'power of two' in lib.gc_last_error()
    x = torch.full((1, 1, 8, 8), 3.0, device=DEV)
    ptrs, loss = (ctypes.c_void_p * 1)(x.data_ptr()), torch.full((1,), 5.0, device=DEV)
    sizes, batches = (ctypes.c_int32 * 1)(8), (ctypes.c_int32 * 1)(1)
    hip, dev = _backend.get(), torch.device(DEV)
    with pytest.raises(RuntimeError, match='gc_noise_reg_fwd_f32 failed.*workspace'):
        hip._launch(dev, noise_ops.REG_FWD, ptrs, sizes, batches, 1, _lib.ptr(loss), _lib.ptr(x), 4, _lib.stream_of(x))
    with pytest.raises(RuntimeError, match='gc_noise_normalize_f32 failed.*null'):
        hip._launch(dev, noise_ops.NORMALIZE, None, (ctypes.c_int64 * 1)(64), 1, _lib.ptr(x), 1024, _lib.stream_of(x))
    torch.cuda.synchronize()
    assert float(loss) == 5.0 and bool((x == 3.0).all())


# ---- make_image and project ----------------------------------------------------------------------------------------------------------------
def test_make_image_bytes_on_the_device():
    x, want = torch.from_numpy(GOLD['make_image/x']), GOLD['make_image/bytes']
    dev = x.to(DEV)
    got = projection.make_image(dev)
    assert got.dtype == np.uint8 and np.array_equal(got, want)          # every quantisation edge is among these values
    assert torch.equal(dev.cpu(), x), 'make_image must leave its argument untouched'


def test_project_on_the_32_generator_bf16x3(bf16x3_mode):
    out = pc.run_projection(DEV, steps=24)
    pc.check_projection(out, 24)
