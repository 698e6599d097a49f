"""Group interpolation without a GPU: the torch formulas of models/op/interp.py against a literal restatement of the reference's per-frame
lines (evaluation/inference_class.py:153-169), the weights, slerp, and Inference.interpolate_by_group / generate_matrix_by_group on a 32 x 32
model directory (CPU tensors, emulated backend): frame counts, files, GIFs, repeatability, and which slices of z move in which film."""
import json
import os

import numpy as np
import pytest
import torch

import inference_checks as ic
from conftest import GOLDEN

from gan_control_amd.inference import Inference
from gan_control_amd.models.gan_model import NoiseInjection
from gan_control_amd.models.op import interp

PLACES = {k: tuple(v['place_in_latent']) for k, v in json.load(open(os.path.join(GOLDEN, 'configs.json')))['ffhq']['training_config']['sub_groups_dict'].items()}


def slerp_formula(val, low, high):
    low_norm = low / torch.norm(low, dim=1, keepdim=True)
    high_norm = high / torch.norm(high, dim=1, keepdim=True)
    omega = torch.acos((low_norm * high_norm).sum(1))
    so = torch.sin(omega)
    return (torch.sin((1.0 - val) * omega) / so).unsqueeze(1) * low + (torch.sin(val * omega) / so).unsqueeze(1) * high


def restated(latent_1, z1, z2, group_chunk, pics, interpolation):
    """Lines 153-169 of the reference, frame by frame -> ([P, B, L] freeze group, [P, B, L] freeze everything else)."""
    z1_latent_start, z1_latent_end, z1_latent_group = z1[:, :group_chunk[0]], z1[:, group_chunk[1]:], z1[:, group_chunk[0]:group_chunk[1]]
    frozen, moving = [], []
    for _, p in zip(range(pics), np.linspace(0, 1, pics)):
        if interpolation == 'linear':
            start = (1 - p) * z1_latent_start + p * z2[:, :group_chunk[0]]
            end = (1 - p) * z1_latent_end + p * z2[:, group_chunk[1]:]
            group = (1 - p) * z1_latent_group + p * z2[:, group_chunk[0]:group_chunk[1]]
        elif interpolation == 'slerp':
            start = slerp_formula(p, z1_latent_start, z2[:, :group_chunk[0]])
            end = slerp_formula(p, z1_latent_end, z2[:, group_chunk[1]:])
            group = slerp_formula(p, z1_latent_group, z2[:, group_chunk[0]:group_chunk[1]])
        else:
            start = np.sqrt(1 - p) * z1_latent_start + np.sqrt(p) * z2[:, :group_chunk[0]]
            end = np.sqrt(1 - p) * z1_latent_end + np.sqrt(p) * z2[:, group_chunk[1]:]
            group = np.sqrt(1 - p) * z1_latent_group + np.sqrt(p) * z2[:, group_chunk[0]:group_chunk[1]]
        frozen.append(torch.cat([start, latent_1[:, group_chunk[0]:group_chunk[1]], end], dim=1))
        moving.append(torch.cat([latent_1[:, :group_chunk[0]], group, latent_1[:, group_chunk[1]:]], dim=1))
    return torch.stack(frozen), torch.stack(moving)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('pics', [1, 10])
@pytest.mark.parametrize('group', ['id', 'other', 'age'])
@pytest.mark.parametrize('interpolation', ['linear', 'slerp', 'sqrt'])
def test_reference_formula_is_the_reference_lines_bit_for_bit(interpolation, group, pics):
    assert (PLACES['id'], PLACES['other'], PLACES['age']) == ((0, 128), (448, 512), (320, 384))
    lo, hi = PLACES[group]
    gen = torch.Generator().manual_seed(7)
    latent_1 = torch.randn(1, 512, generator=gen).expand(3, -1)
    z1, z2 = torch.randn(3, 512, generator=gen), torch.randn(3, 512, generator=gen)
    wa, wb = interp.interpolation_weights(pics, interpolation)
    for z_from in (latent_1, z1):          # the first segment starts from the expanded row itself
        want = restated(latent_1, z_from, z2, (lo, hi), pics, interpolation)
        for fn in (interp.interpolate_latents_reference, interp.interpolate_latents):          # CPU tensors: the same formula
            got = fn(latent_1, z_from, z2, lo, hi, wa, wb, interpolation)
            assert got.shape == (2, pics, 3, 512) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
            assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))


def test_interpolation_weights():
    p = np.linspace(0, 1, 10)
    for mode, a, b in (('linear', 1 - p, p), ('slerp', 1 - p, p), ('sqrt', np.sqrt(1 - p), np.sqrt(p)), ('anything', np.sqrt(1 - p), np.sqrt(p))):
        wa, wb = interp.interpolation_weights(10, mode)
        assert wa.dtype == np.float32 and wb.dtype == np.float32 and wa.shape == wb.shape == (10,)
        assert np.array_equal(wa, a.astype(np.float32)) and np.array_equal(wb, b.astype(np.float32))
        assert (wa[0], wb[0], wa[-1], wb[-1]) == (1, 0, 0, 1)
    for mode in ('linear', 'slerp', 'sqrt'):
        wa, wb = interp.interpolation_weights(1, mode)          # linspace(0, 1, 1) is [0]
        assert wa.tolist() == [1.0] and wb.tolist() == [0.0]
    # rounded last: the float32 weight times x is what torch gives for the float64 scalar times x
    x = torch.randn(64, generator=torch.Generator().manual_seed(1))
    wa, _ = interp.interpolation_weights(10, 'linear')
    for k in range(10):
        assert torch.equal((1 - p[k]) * x, float(wa[k]) * x)


def test_slerp_is_the_formula_and_stays_on_the_sphere():
    gen = torch.Generator().manual_seed(2)
    low, high = torch.randn(4, 64, generator=gen), torch.randn(4, 64, generator=gen)
    for val in (0.0, 0.25, 1 / 3, 1.0):
        assert torch.equal(Inference.slerp(val, low, high), slerp_formula(val, low, high))
    assert torch.allclose(Inference.slerp(0.0, low, high), low, atol=1e-6) and torch.allclose(Inference.slerp(1.0, low, high), high, atol=1e-6)
    a, b = low.double() / low.double().norm(dim=1, keepdim=True), high.double() / high.double().norm(dim=1, keepdim=True)
    mid = Inference.slerp(0.5, a, b)
    assert torch.allclose(mid.norm(dim=1), torch.ones(4, dtype=torch.float64), atol=1e-12)          # unit inputs: the arc, not the chord


def test_blend_noise_reference_path():
    gen = torch.Generator().manual_seed(3)
    a = [torch.randn(2, 1, s, s, generator=gen) for s in (4, 8, 8)]
    b = [torch.randn(2, 1, s, s, generator=gen) for s in (4, 8, 8)]
    p = np.linspace(0, 1, 10)[3]
    wa, wb = interp.interpolation_weights(10, 'linear')
    want = [(1 - p) * x + p * y for x, y in zip(a, b)]
    got = interp.blend_noise(a, b, wa[3], wb[3])
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    out = [torch.empty_like(x) for x in a]
    assert interp.blend_noise(a, b, wa[3], wb[3], out=out) is not None and all(torch.equal(o, w) for o, w in zip(out, want))
    same = interp.blend_noise(a, a, wa[3], wb[3])
    assert all(torch.equal(g, (1 - p) * x + p * x) for g, x in zip(same, a))
    with pytest.raises(ValueError, match='one length'):
        interp.blend_noise(a, b[:2], 0.5, 0.5)
    with pytest.raises(ValueError, match='out must be'):
        interp.blend_noise(a, b, 0.5, 0.5, out=out[:2])


def noisy(inf):
    """The noise strengths are zero as constructed: give them values, so that the injected noise reaches the images."""
    with torch.no_grad():
        for k, m in enumerate(m for m in inf.model.modules() if isinstance(m, NoiseInjection)):
            m.weight.fill_(0.05 * (k + 1))
    return inf


@pytest.fixture
def inf32(tmp_path, emu_backend):
    ic.write_model_dir(str(tmp_path / 'model'), ic.ffhq_config(32))
    return noisy(Inference(str(tmp_path / 'model'), device='cpu'))


def _film(inf, seed, **kw):
    return inf.interpolate_by_group('age', None, batch=2, num_of_intermediate_latents=2, pics_per_interpolation=3, interpolation='linear',
                                    generator=torch.Generator().manual_seed(seed), return_list=True, **kw)


def test_interpolate_by_group_files_and_gifs(inf32, tmp_path):
    from PIL import Image
    save = str(tmp_path / 'films' / 'age_walk')
    os.makedirs(save)
    frozen, moving = inf32.interpolate_by_group('age', save, batch=2, num_of_intermediate_latents=2, pics_per_interpolation=3, interpolation='linear',
                                                generator=torch.Generator().manual_seed(5))
    assert len(frozen) == 6 and len(moving) == 6 and all(isinstance(im, Image.Image) for im in frozen + moving)
    assert frozen[0].size == (2 * 34 + 2, 36)          # make_grid of two 32 x 32 images in one row, padding 2
    assert sorted(os.listdir(save)) == ['freeze_group', 'freeze_group_age_walk.gif', 'freeze_not_group_age_walk.gif', 'freeze_not_same_group']
    for folder in ('freeze_group', 'freeze_not_same_group'):
        assert sorted(os.listdir(os.path.join(save, folder))) == ['%06d.jpg' % i for i in range(6)]
    for name in ('freeze_group_age_walk.gif', 'freeze_not_group_age_walk.gif'):
        with Image.open(os.path.join(save, name)) as gif:
            assert gif.format == 'GIF' and gif.n_frames == 6 and gif.info['loop'] == 0
            assert gif.size[0] <= 1024 and gif.size[1] <= 256 and (gif.size[0] == 1024 or gif.size[1] == 256)
            assert abs(gif.size[0] / gif.size[1] - 70 / 36) < 0.01          # the aspect ratio of the frames
            for k in range(6):
                gif.seek(k)
                assert gif.info['duration'] == 500
    # an index goes into the GIF's name, and frame 0 of both films is one image
    inf32.interpolate_by_group('age', save, batch=2, num_of_intermediate_latents=1, pics_per_interpolation=2, interpolation='linear', idx=7,
                               generator=torch.Generator().manual_seed(5))
    assert os.path.exists(os.path.join(save, 'freeze_group_age_walk0007.gif')) and os.path.exists(os.path.join(save, 'freeze_not_group_age_walk0007.gif'))
    assert frozen[0].tobytes() == moving[0].tobytes()


def test_interpolate_by_group_is_repeatable_and_moves_the_right_slices(inf32, monkeypatch):
    lo, hi = PLACES['age']
    zs, calls = [], []
    real = Inference.interpolation_latents

    def recording(self, group, latent_1, latent_from, latent_to, *a, **k):
        z = real(self, group, latent_1, latent_from, latent_to, *a, **k)
        zs.append((latent_1, z))
        return z

    monkeypatch.setattr(Inference, 'interpolation_latents', recording)
    hook = inf32.model.register_forward_pre_hook(lambda m, args, kwargs: calls.append((args[0][0], kwargs)), with_kwargs=True)
    try:
        frozen, moving = _film(inf32, 11)
    finally:
        hook.remove()
    segs = list(zs)          # (the films below record too)
    assert frozen.shape == (6, 2, 3, 32, 32) and moving.shape == (6, 2, 3, 32, 32) and frozen.dtype == torch.float32 and not frozen.is_cuda
    again = _film(inf32, 11)
    assert torch.equal(frozen, again[0]) and torch.equal(moving, again[1])
    other = _film(inf32, 12)
    assert not torch.equal(frozen, other[0])
    # one interpolation_latents call per segment; two generator calls per frame, on w, in the order frozen, moving
    assert len(segs) == 2 and len(calls) == 12 and all(kw.get('input_is_latent') is True and kw.get('noise') is not None for _, kw in calls)
    for seg, (latent_1, z) in enumerate(segs):
        assert z.shape == (2, 3, 2, 512) and latent_1.stride() == (0, 1)
        w = inf32.style(z.reshape(-1, 512)).reshape(2, 3, 2, 512)
        for f in range(3):
            # film 0: the group's slice of z is latent_1's; film 1: everything else is
            assert torch.equal(z[0, f][:, lo:hi], latent_1[:, lo:hi])
            assert torch.equal(z[1, f][:, :lo], latent_1[:, :lo]) and torch.equal(z[1, f][:, hi:], latent_1[:, hi:])
            assert not torch.equal(z[0, f][:, :lo], latent_1[:, :lo]) or (seg == 0 and f == 0)
            assert not torch.equal(z[1, f][:, lo:hi], latent_1[:, lo:hi]) or (seg == 0 and f == 0)
            for film in (0, 1):
                assert torch.equal(calls[6 * seg + 2 * f + film][0], w[film, f])
    # the second segment starts where the first ended
    assert torch.equal(segs[0][1][:, 2], segs[1][1][:, 0])
    # frame 0 of both films is the same image: both are latent_1 under the undisturbed noise blend
    assert torch.equal(segs[0][1][0, 0], segs[0][1][1, 0]) and torch.equal(frozen[0], moving[0])
    # per-segment noise: another film, as repeatable
    a, b = _film(inf32, 11, same_noise=False), _film(inf32, 11, same_noise=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], frozen)
    assert torch.equal(a[0][0], frozen[0])          # (frame 0 has weight 0 on the second noise)


def test_generate_matrix_by_group(inf32, tmp_path):
    with pytest.raises(ValueError, match='not in valid group names'):
        inf32.generate_matrix_by_group('orientations')
    with pytest.raises(ValueError, match='not in valid group names'):
        inf32.interpolate_by_group('nose', None, return_list=True)
    image = inf32.generate_matrix_by_group('orientation', save_path=str(tmp_path / 'matrix'), generator=torch.Generator().manual_seed(1))
    assert image.size == (6 * 34 + 2, 6 * 34 + 2) and os.path.exists(str(tmp_path / 'matrix.jpg'))
    again = inf32.generate_matrix_by_group('orientation', generator=torch.Generator().manual_seed(1))
    assert image.tobytes() == again.tobytes()
    small = inf32.generate_matrix_by_group('orientation', downsample=2, generator=torch.Generator().manual_seed(1))
    assert small.size == (103, 103)
