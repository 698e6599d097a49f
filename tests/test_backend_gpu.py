"""HipBackend's one launch path (HipBackend._launch): what the kernel timer records, which entry a failure names and what the device
guard does.  Needs an MI355X: ``-m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MODES = ['f32', 'bf16x3', 'bf16']


@pytest.fixture(scope='module', autouse=True)
def _native_loaded():
    from gan_control_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()


def _hip():
    from gan_control_amd.models.op import _backend
    assert _backend.get().name == 'hip'
    return _backend.get()


def _records(fn, mode='f32'):
    """[(kernel name, work)] that a KernelTimer(only=None) on the HIP backend tallies while fn(hip) runs in arithmetic `mode`."""
    from gan_control_amd.utils.profiling import KernelTimer
    hip = _hip()
    timer = KernelTimer(only=None)
    prev = hip.conv_mode, hip.timer
    hip.conv_mode, hip.timer = mode, timer
    try:
        fn(hip)
        torch.cuda.synchronize()
    finally:
        hip.conv_mode, hip.timer = prev
    return [(name, work) for name, _, _, work in timer.records]


def _rand(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).to(DEV)


# upfirdn2d: planes [1, 2, ., .]; bytes = 4 * (numel_in + numel_out).  (kernel, taps, up, down, pad, input h x w, output h x w, bytes)
FIR_CASES = [
    ('fir44_tile_kernel', 4, 1, 1, 0, (19, 67), (16, 64), 4.0 * (2 * 19 * 67 + 2 * 16 * 64)),           # 18376
    ('fir44_small_kernel', 4, 1, 1, 0, (11, 11), (8, 8), 4.0 * (2 * 11 * 11 + 2 * 8 * 8)),               # 1480
    ('fir44_down2_kernel', 4, 1, 2, 0, (18, 66), (8, 32), 4.0 * (2 * 18 * 66 + 2 * 8 * 32)),             # 11552
    ('fir44_up2_kernel', 4, 2, 1, 2, (4, 16), (8, 32), 4.0 * (2 * 4 * 16 + 2 * 8 * 32)),                 # 2560
    ('upfirdn2d_generic_kernel', 3, 1, 1, 0, (10, 10), (8, 8), 4.0 * (2 * 10 * 10 + 2 * 8 * 8)),         # 1312
]


@pytest.mark.parametrize('case', FIR_CASES, ids=[c[0] for c in FIR_CASES])
def test_timer_records_fir(case):
    name, k, up, down, pad, (h, w), (oh, ow), work = case
    x, taps = _rand(1, 2, h, w), _rand(k, k)
    assert _records(lambda hip: hip.upfirdn2d(x, taps, up, down, pad, pad, oh, ow, True)) == [(name, work)]


def test_timer_records_fused_fir_and_bias_act():
    """upfirdn2d_act / upfirdn2d_mask at the smallest output of the tile kernel (16 x 64), upfirdn2d_actbwd at the smallest plane the entry takes
    (the same: gc_upfirdn2d_actbwd_tiles counts tiles of any plane, the entry wants the tile kernel's 16 x 64), bias_act on [2, 3, 5]."""
    x, taps = _rand(1, 2, 19, 67), _rand(4, 4)
    bias, ref = _rand(2), _rand(1, 2, 16, 64)
    n_in, n_out = 2 * 19 * 67, 2 * 16 * 64
    assert _records(lambda hip: hip.upfirdn2d_act(x, taps, 0, 0, 16, 64, True, bias, None, None, 0.2, 1.4)) == [('fir44_tile_kernel', 4.0 * (n_in + n_out))]
    assert _records(lambda hip: hip.upfirdn2d_mask(x, taps, 0, 0, 16, 64, True, ref, 0.2, 1.4)) == [('fir44_tile_kernel', 4.0 * (n_in + 2 * n_out))]
    y_ref = _rand(1, 2, 19, 67)
    assert _records(lambda hip: hip.upfirdn2d_actbwd(x, y_ref, None, taps, 0, 0, 16, 64, False, 0.2, 1.4)) == [('fir44_tile_kernel', 4.0 * (2 * n_in + n_out))]
    v, b3 = _rand(2, 3, 5), _rand(3)
    assert _records(lambda hip: hip.bias_act(v, b3, None, None, 0.2, 1.4)) == [('bias_act_kernel', 4.0 * (2 * 30 + 3))]
    noise, nw = _rand(2, 1, 5), _rand(1)
    assert _records(lambda hip: hip.bias_act(v, b3, noise, nw, 0.2, 1.4)) == [('bias_act_kernel', 4.0 * (2 * 30 + 3 + 10))]


@pytest.mark.parametrize('mode', MODES)
def test_timer_records_conv(mode):
    """conv2d / conv2d_wgrad on [2, 8, 8, 8] -> 8 channels, 3 x 3: 2 * B * OC * IC * kh * kw * H_out * W_out = 2 * 2 * 8 * 8 * 9 * 64 flops.
    That shape has no per-sample weight gradient (fewer than 32 channels), so conv2d_wgrad_samples runs the smallest SAMPLE_WGRAD_CASES entry
    (tests/test_ops_gpu.py) that has one: 5 x 64 -> 64 @ 6 x 6 in the bf16 arithmetics, the thin 1 x 1 2 x 128 -> 3 @ 128 x 128 in fp32."""
    from gan_control_amd.models.op._backend import ConvGeom
    from gan_control_amd.utils.profiling import conv_variant
    geom = ConvGeom(3, 3, 1, 1, 1, 1, 8, 8)
    x, w_t, dy = _rand(2, 8, 8, 8), _rand(3, 3, 8, 8), _rand(2, 8, 8, 8) * 0.5
    flops = 2.0 * 2 * 8 * 8 * 9 * 64
    assert flops == 147456.0
    assert _records(lambda hip: hip.conv2d(x, w_t, None, None, geom), mode) == [(conv_variant(geom, 8, 2, 8, mode, in_hw=(8, 8)), flops)]
    assert _records(lambda hip: hip.conv2d_wgrad(x, dy, None, None, geom), mode) == [('wgrad_mfma_kernel(+reduce)', flops)]
    if mode == 'f32':
        b, k_in, n_out, hw, k, pad, flops = 2, 128, 3, 128, 1, 0, 2.0 * 2 * 128 * 3 * 128 * 128          # 25165824
    else:
        b, k_in, n_out, hw, k, pad, flops = 5, 64, 64, 6, 3, 1, 2.0 * 5 * 64 * 64 * 9 * 36               # 13271040
    sgeom = ConvGeom(k, k, 1, 1, pad, pad, hw, hw)
    sx, sdy = _rand(b, k_in, hw, hw), _rand(b, n_out, hw, hw) * 0.5

    def samples(hip):
        assert hip.conv2d_wgrad_samples_bytes(x, dy, geom) == 0
        hip.conv2d_wgrad_samples(sx, sdy, None, None, sgeom)
    assert _records(samples, mode) == [('wgrad_mfma_kernel(+reduce)', flops)]


def test_timer_records_pw_act_wgrad():
    """gc_pw_act_wgrad_f32 takes any positive extents: one sample, 1 -> 1 channel, one pixel: 2 * b * k * n * h * w = 2 flops."""
    x, dy, y = _rand(1, 1, 1, 1), _rand(1, 1, 1, 1) * 0.5, _rand(1, 1, 1, 1) - 0.1
    assert _records(lambda hip: hip.pw_act_wgrad(x, dy, y, 0.2, 1.4)) == [('wgrad_mfma_kernel(+reduce)', 2.0)]


def _fir_noise_without_strength(hip):
    # gc_upfirdn2d_pitched_f32, first statement (upfirdn2d.hip): noise and noise_w must both be set or both be null
    hip.upfirdn2d_act(_rand(1, 2, 19, 67), _rand(4, 4), 0, 0, 16, 64, True, None, _rand(1, 1, 16, 64), None, 1.0, 1.0, activate=False)


def _conv_noise_without_strength(hip):
    # validate_epilogue (conv_common.h), called by gc_conv2d_fused_bf16x3_packed_f32 before it looks at the shape: the same rule for the epilogue
    from gan_control_amd.models.op._backend import ConvGeom
    hip.conv2d(_rand(2, 8, 8, 8), _rand(3, 3, 8, 8), None, None, ConvGeom(3, 3, 1, 1, 1, 1, 8, 8), epilogue=(None, _rand(2, 1, 8, 8), None, 0.2, 1.4, True))


def _wgrad_5x5(hip, samples=False):
    # validate (conv_common.h), the first call of both weight-gradient entries: 1 x 1 and 3 x 3 taps only.  32 -> 32 channels, so that
    # the per-sample form's scratch query (which does not look at the taps) answers > 0 and the call gets as far as the entry
    from gan_control_amd.models.op._backend import ConvGeom
    geom = ConvGeom(5, 5, 1, 1, 1, 1, 6, 6)
    x, dy = _rand(2, 32, 8, 8), _rand(2, 32, 6, 6)
    if samples:
        assert hip.conv2d_wgrad_samples_bytes(x, dy, geom) > 0
        hip.conv2d_wgrad_samples(x, dy, None, None, geom)
    else:
        hip.conv2d_wgrad(x, dy, None, None, geom)


@pytest.mark.parametrize('entry,call', [
    ('gc_upfirdn2d_pitched_f32', _fir_noise_without_strength),
    ('gc_conv2d_fused_bf16x3_packed_f32', _conv_noise_without_strength),
    ('gc_conv2d_wgrad_bf16x3_f32', _wgrad_5x5),
    ('gc_conv2d_wgrad_samples_bf16x3_f32', lambda hip: _wgrad_5x5(hip, samples=True)),
], ids=lambda v: v if isinstance(v, str) else '')
def test_failure_names_the_entry_called(entry, call, bf16x3_mode):
    """A call the entry's own host-side argument check refuses before any launch is reported under the symbol that was called."""
    with pytest.raises(RuntimeError) as err:
        call(_hip())
    assert str(err.value).startswith(entry + ' failed'), str(err.value)


def _direct(x):
    """The library called directly, with x's device current: (global_avgpool(x), plane_reduce(x, x, 0.5))."""
    from gan_control_amd import _lib
    lib = _lib.load()
    b, c = x.shape[0], x.shape[1]
    with torch.cuda.device(x.device):
        avg = torch.empty((b, c, 1, 1), dtype=x.dtype, device=x.device)
        _lib.check(lib.gc_global_avgpool_f32(_lib.ptr(x), _lib.ptr(avg), b * c, x.numel() // (b * c), _lib.stream_of(x)), 'gc_global_avgpool_f32')
        red = torch.empty((b, c), dtype=x.dtype, device=x.device)
        _lib.check(lib.gc_plane_reduce_f32(_lib.ptr(x), _lib.ptr(x), _lib.ptr(red), b * c, x.numel() // (b * c), 0.5, _lib.stream_of(x)), 'gc_plane_reduce_f32')
        torch.cuda.synchronize()
    return avg, red


def test_guard_is_a_no_op_on_the_current_device():
    hip = _hip()
    x = _rand(2, 3, 9, 13)
    assert x.device.index == torch.cuda.current_device()
    avg, red = _direct(x)
    assert torch.equal(hip.global_avgpool(x), avg) and torch.equal(hip.plane_reduce(x, x, 0.5), red)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs a second GPU')
def test_guard_launches_on_the_tensors_device():
    hip = _hip()
    x = _rand(2, 3, 9, 13).to('cuda:1')
    with torch.cuda.device(0):
        avg, red = hip.global_avgpool(x), hip.plane_reduce(x, x, 0.5)
        torch.cuda.synchronize(1)
    assert avg.device == x.device and red.device == x.device
    ref_avg, ref_red = _direct(x)
    assert torch.equal(avg, ref_avg) and torch.equal(red, ref_red)
