"""Image projection without a GPU: the generator's noise-map gradients over the emulated backend, the CPU paths of the helpers against the
reference's own results (tests/golden/projection.npz, written by tools/make_projection_golden.py) and the projection loop."""
import json

import numpy as np
import pytest
import torch

import projection_checks as pc
from conftest import group, rel_err

from gan_control_amd import projection
from gan_control_amd.evaluation import image_grid
from gan_control_amd.models.op import noise_grad
from gan_control_amd.projection import noise_ops

GOLD = pc.GOLD


def test_generator_noise_gradients_match_the_reference(emu_backend):
    """rel_err <= 1e-4, the bar oracle/make_golden.py holds oracle and reference to.  Before the noise-map gradient existed every one of these
    gradients was None.  (The issue asks for conv_transpose False as well: the reference's ModulatedConv2d raises ValueError for it, as
    this package's does, so there is no such generator to differentiate; the fixture records the refusal.)"""
    r = group(GOLD, 'gen')
    img, grads, zgrad = pc.generator_noise_grads('cpu')
    assert rel_err(img, r['img']) <= 1e-4
    assert len(grads) == int(r['count']) == 7 and zgrad is not None
    for i, g in enumerate(grads):
        assert g is not None, 'noise map %d has no gradient' % i
        assert g.shape == r['g%d' % i].shape
        err = rel_err(g, r['g%d' % i])
        print('noise map %d %s: rel err %.3e' % (i, tuple(g.shape), err))
        assert err <= 1e-4, (i, err)


def test_conv_transpose_false_is_refused_as_in_the_reference():
    from gan_control_amd.models.gan_model import Generator
    assert int(GOLD['gen/conv_transpose_false_raises']) == 1
    with pytest.raises(ValueError, match='conv_transpose'):
        Generator(32, 512, 8, channel_multiplier=2, conv_transpose=False)


def test_backward_without_noise_gradients_makes_the_calls_it_made_before(monkeypatch):
    """The recorded sequences come from the commit before the noise-map gradient; nothing of noise_grad runs either."""
    def never(*a, **kw):
        raise AssertionError('noise_grad ran although no noise map wants a gradient')
    monkeypatch.setattr(noise_grad, 'masked', never)
    monkeypatch.setattr(noise_grad, 'pixel_sums', never)
    with open(pc.CALLS_JSON) as f:
        want = json.load(f)
    assert pc.backward_call_sequence(False) == want['frozen_parameters']
    assert pc.backward_call_sequence(False, train_params=True) == want['trained_parameters']


def test_backward_with_noise_gradients_differs_only_in_the_activation_pass():
    with open(pc.CALLS_JSON) as f:
        want = json.load(f)['frozen_parameters']
    got = pc.backward_call_sequence(True)
    assert got == want          # under emulation g_pre is bias_act_bwd either way; the pixel sums are ATen


def test_fir_activation_noise_gradient(emu_backend):
    pc.check_fir_act_noise_grad('cpu', 2e-5)


def test_noise_gradient_is_a_first_derivative_only(emu_backend):
    from gan_control_amd.models.op.modulated_conv import modulated_conv2d_act
    gen = torch.Generator().manual_seed(2)
    x, w = torch.randn(1, 4, 8, 8, generator=gen), torch.randn(1, 4, 4, 3, 3, generator=gen)
    s, bias, noise_w = torch.randn(1, 4, generator=gen), torch.zeros(4), torch.tensor([0.5])
    noise = torch.randn(1, 1, 8, 8, generator=gen).requires_grad_(True)
    out = modulated_conv2d_act(x, w, s, bias, noise, noise_w)
    g, = torch.autograd.grad(out.sum(), noise, create_graph=True)
    assert g.shape == noise.shape
    with pytest.raises(RuntimeError, match='cannot be differentiated again'):
        g.sum().backward()


@pytest.mark.parametrize('kind', ['white', 'smooth'])
def test_noise_regularize_and_normalize_cpu_paths_match_the_reference(kind):
    r = group(GOLD, 'reg/' + kind)
    maps = [r['x%d' % i].clone().requires_grad_(True) for i in range(int(r['count']))]
    assert all(m.dtype == torch.float64 for m in maps)
    loss = projection.noise_regularize(maps)
    assert rel_err(loss, r['loss']) <= 1e-12
    for i, g in enumerate(torch.autograd.grad(loss, maps)):
        assert rel_err(g, r['g%d' % i]) <= 1e-12, i
    normed = [m.detach().clone() for m in maps]
    assert projection.noise_normalize_(normed) is None
    for i, n in enumerate(normed):
        assert rel_err(n, r['n%d' % i]) <= 1e-12, i


def test_noise_lists_are_checked():
    with pytest.raises(ValueError, match='non-empty list'):
        projection.noise_regularize([])
    with pytest.raises(ValueError, match='non-empty list'):
        projection.noise_normalize_([])
    # what the device path refuses, named by shape (the check itself needs no device)
    for bad in ([torch.zeros(2, 1, 12, 12)], [torch.zeros(2, 1, 8, 16)], [torch.zeros(2, 2, 8, 8)], [torch.zeros(1, 1, 2048, 2048)], [torch.zeros(8, 8)]):
        with pytest.raises(ValueError, match=r'shape \(%s\)' % ', '.join(map(str, bad[0].shape))):
            noise_ops._check_device_maps(bad, 'noise_regularize', True)
    with pytest.raises(ValueError, match='at most 32'):
        noise_ops._check_device_maps([torch.zeros(1, 1, 4, 4)] * 33, 'noise_regularize', True)
    with pytest.raises(ValueError, match='float32'):
        noise_ops._check_device_maps([torch.zeros(1, 1, 4, 4, dtype=torch.float64)], 'noise_regularize', True)
    with pytest.raises(ValueError, match='two elements'):
        noise_ops._check_device_maps([torch.zeros(1)], 'noise_normalize_', False)


def test_get_lr_and_latent_noise_match_the_reference():
    r = group(GOLD, 'lr')
    got = torch.tensor([projection.get_lr(float(t), 0.1) for t in r['t']], dtype=torch.float64)
    assert rel_err(got, r['value']) <= 1e-12
    got = torch.tensor([projection.get_lr(float(t), 0.05, 0.5, 0.1) for t in r['t']], dtype=torch.float64)
    assert rel_err(got, r['value_ramps']) <= 1e-12
    r = group(GOLD, 'latent_noise')
    torch.manual_seed(int(r['seed']))
    assert rel_err(projection.latent_noise(r['latent'], float(r['strength'])), r['out']) <= 1e-12
    a = projection.latent_noise(r['latent'], 0.5, generator=torch.Generator().manual_seed(1))
    b = projection.latent_noise(r['latent'], 0.5, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a, b) and not torch.equal(a, r['latent'])


def test_make_image_bytes_and_the_two_clamps():
    x, want = torch.from_numpy(GOLD['make_image/x']), GOLD['make_image/bytes']
    before = x.clone()
    got = projection.make_image(x)
    assert got.dtype == np.uint8 and got.shape == (2, 16, 16, 3) and np.array_equal(got, want)
    assert torch.equal(x, before), 'make_image must leave its argument untouched'
    assert np.array_equal(projection.make_image(x[:1]), want[:1])
    # (clamp(x, -1, 1) + 1) / 2 and clamp(0.5 * x + 0.5, 0, 1) are the same float32 function: on every float next to a byte boundary
    # (the edge fixture of the image output path), on both ends of the clamp and beyond them
    with np.load(pc.GOLDEN + '/image_output.npz') as z:
        edges = torch.from_numpy(z['edges/x'])
    assert edges.numel() == 510
    values = torch.cat([edges, torch.tensor([-1.0, 1.0, -1.5, 1.5, 0.0, -0.0, float('inf'), float('-inf')]),
                        torch.nextafter(torch.tensor([-1.0, 1.0]), torch.tensor([0.0, 0.0])), torch.nextafter(torch.tensor([-1.0, 1.0]), torch.tensor([-2.0, 2.0]))])
    a = values.clamp(min=-1, max=1).add(1).div(2)
    b = values.mul(0.5).add(0.5).clamp(min=0., max=1.)
    assert torch.equal(a, b)
    assert torch.equal(a.mul(255).to(torch.uint8), image_grid.quantize_reference(values))


def test_merge_group_latents_and_avg_latent():
    class Groups:
        def get_group_w_latent(self, latent, group):
            return latent[:, :, 4:8]

        def insert_group_w_latent(self, latent, value, group):
            latent[:, :, 4:8] = value

    latent = torch.arange(2 * 3 * 12, dtype=torch.float32).reshape(2, 3, 12)
    want = latent.clone()
    want[:, :, 4:8] = latent[:, :, 4:8].mean(1, keepdim=True)
    projection.merge_group_latents(Groups(), 'id', latent)
    assert torch.equal(latent, want)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.style = torch.nn.Linear(512, 512)

    torch.manual_seed(4)
    m = Model()
    torch.manual_seed(5)
    mean, std = projection.get_avg_latent(m, 64, 'cpu')
    torch.manual_seed(5)
    w = m.style(torch.randn(64, 512)).detach()
    assert mean.shape == (512,) and std.shape == () and np.allclose(mean, w.mean(0).numpy(), atol=1e-6)
    assert np.isclose(float(std), float(((w - w.mean(0)).pow(2).sum() / 64) ** 0.5), rtol=1e-6)


def test_load_source_images(tmp_path):
    from PIL import Image
    gen = np.random.default_rng(0)
    paths = []
    for i, (w, h) in enumerate([(40, 24), (16, 16), (20, 50)]):
        path = tmp_path / ('img%d.png' % i)
        Image.fromarray(gen.integers(0, 256, (h, w, 3), dtype=np.uint8), 'RGB').save(path)
        paths.append(str(path))
    out = projection.load_source_images(paths, res=16)
    assert out.shape == (3, 3, 16, 16) and out.dtype == torch.float32 and float(out.abs().max()) <= 1.0
    same = np.array(Image.open(paths[1]).convert('RGB'))
    assert torch.equal(out[1], torch.from_numpy(same).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5))
    wide = Image.open(paths[0]).convert('RGB').resize((26, 16), Image.BILINEAR).crop((5, 0, 21, 16))
    assert torch.equal(out[0], torch.from_numpy(np.array(wide)).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5))


def test_project_needs_a_loss(emu_backend):
    with pytest.raises(ValueError, match='nothing to optimise'):
        projection.project(object(), torch.zeros(1, 3, 32, 32))


def test_project_on_the_32_generator(emu_backend):
    """MSE only, 24 steps: measured final / first MSE ratio on the CPU path: see profiles/projection.md."""
    out = pc.run_projection('cpu', steps=24)
    pc.check_projection(out, 24)
