"""The Inference / Controller API on the GPU: the two fused w-space calls of gen_batch_by_controls, the module path when a gradient is wanted,
and the untouched launches of the existing callers.  Size 32, batch 3, the seven groups of the ffhq configuration."""
import pytest
import torch

import inference_checks as ic

from gan_control_amd.inference import Controller
from gan_control_amd.models.gan_model import EqualLinear
from gan_control_amd.models.op import _backend
from gan_control_amd.models.op import fc_stack as fcs

pytestmark = pytest.mark.gpu
BATCH = 3


@pytest.fixture(scope='module')
def ctl(tmp_path_factory):
    root = tmp_path_factory.mktemp('controller')
    ic.write_controller_dir(root)
    return Controller(str(root))


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


def _controls(batch):
    gen = torch.Generator().manual_seed(3)
    q = torch.zeros(batch, 8)
    q[torch.arange(batch), torch.arange(batch) % 8] = 1
    return {'orientation': torch.randn(batch, 3, generator=gen) * 30, 'age': torch.rand(batch, 1, generator=gen) * 60 + 10,
            'gamma': torch.randn(batch, 27, generator=gen), 'expression': q}


def _w_space_modules(ctl):
    nets = [ctl.model.style] + [c for c in ctl.fc_controls.values() if c is not None]
    return [m for net in nets for m in net.modules() if isinstance(m, EqualLinear)]


def test_gen_batch_by_controls_is_two_fused_calls(ctl, launches):
    assert ctl.device.type == 'cuda'
    z = torch.randn(BATCH, 512, generator=torch.Generator().manual_seed(1))
    controls = _controls(BATCH)
    fired = []
    hooks = [m.register_forward_hook(lambda m, i, o: fired.append(m)) for m in _w_space_modules(ctl)]
    try:
        img, latent, latent_w = ctl.gen_batch_by_controls(latent=z, normalize=False, **controls)
    finally:
        for h in hooks:
            h.remove()
    assert launches.count(fcs.ENTRY) == 2 and launches[:2] == [fcs.ENTRY, fcs.ENTRY] and not fired
    assert latent_w.shape == (BATCH, 512) and latent_w.is_cuda and torch.equal(latent.cpu(), z)
    # the module path on the same inputs, and both against the float64 composition
    with torch.no_grad():
        w_mod = ctl.model.style(z.cuda())
        for key, value in controls.items():
            name = 'expression_q' if key == 'expression' else key
            ctl.insert_group_w_latent(w_mod, ctl.fc_controls[name](value.cuda()), key)
    want = ic.oracle_latent_w(ctl, z, controls)
    scale = float(want.abs().max())
    e_k = float((latent_w.double().cpu() - want).abs().max()) / scale
    e_m = float((w_mod.double().cpu() - want).abs().max()) / scale
    print('gen_batch_by_controls latent_w: kernel %.3e  module path %.3e' % (e_k, e_m))
    assert e_k <= 4 * e_m, (e_k, e_m)
    # the image: the generator on the returned w with the concatenated noise list, bit for bit
    with torch.no_grad():
        ref, _ = ctl.model([latent_w], input_is_latent=True, noise=ctl.expend_noise(ctl.noise, BATCH))
    assert torch.equal(img, ref)
    del launches[:]
    img01, _, lw = ctl.gen_batch_by_controls(latent=z, **controls)
    assert launches.count(fcs.ENTRY) == 2 and torch.equal(lw, latent_w)
    assert img01.device.type == 'cpu' and torch.equal(img01, ref.mul(0.5).add(0.5).clamp(min=0., max=1.).cpu())


def test_gen_batch_is_one_fused_call(ctl, launches):
    z = torch.randn(BATCH, 512, generator=torch.Generator().manual_seed(2))
    mean = torch.randn(512, generator=torch.Generator().manual_seed(4))
    ctl.mean_w_latent, ctl.mean_w_latents = mean, {k: mean[lo:hi] for k, (lo, hi) in ctl.batch_utils.place_in_latent_dict.items()}
    try:
        img, lat, latents = ctl.gen_batch(latent=z, normalize=False, truncation=0.7)
        assert launches.count(fcs.ENTRY) == 1
        with torch.no_grad():
            w = ctl.style(z.cuda())
            ref, _ = ctl.model([lat], input_is_latent=True, noise=ctl.expend_noise(ctl.noise, BATCH))
        assert torch.equal(lat, 0.7 * (w - mean.cuda()) + mean.cuda()) and torch.equal(latents[:, 0], lat) and torch.equal(img, ref)
    finally:
        ctl.mean_w_latent = ctl.mean_w_latents = None


def test_an_expanded_control_takes_the_module_path(ctl, launches):
    """``age=one_value_on_the_gpu.expand(B, 1)`` has row stride 0 (and keeps it: it is on the device already), which the kernel cannot
    address: z -> w stays the fused call, the controllers run as modules, and the result is what the contiguous control gives there."""
    z = torch.randn(BATCH, 512, generator=torch.Generator().manual_seed(6))
    age = torch.tensor([[60.0]], device='cuda').expand(BATCH, 1)
    pose = torch.tensor([[30.0, -5.0, 0.0]], device='cuda').expand(BATCH, 3)
    assert age.stride() == (0, 1) and pose.stride() == (0, 1)
    _, _, latent_w = ctl.gen_batch_by_controls(latent=z, normalize=False, age=age, orientation=pose)
    assert launches.count(fcs.ENTRY) == 1 and launches[0] == fcs.ENTRY
    with torch.no_grad():
        want = ctl.style(z.cuda())
        ctl.insert_group_w_latent(want, ctl.fc_controls['age'](age.contiguous()), 'age')
        ctl.insert_group_w_latent(want, ctl.fc_controls['orientation'](pose.contiguous()), 'orientation')
    assert torch.equal(latent_w, want)


def test_a_wanted_gradient_takes_the_module_path(ctl, launches):
    z = torch.randn(2, 512, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    age = torch.tensor([[20.0], [60.0]])
    with torch.enable_grad():
        img, latent, latent_w = ctl.gen_batch_by_controls(latent=z, normalize=False, age=age)
        assert fcs.ENTRY not in launches and img.requires_grad and latent_w.requires_grad
        img.square().mean().backward()
    assert z.grad is not None and bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0
    assert not bool(z.grad[:, 320:384].abs().max() > 0)          # the age slice of z reaches nothing: its w slice was replaced
    for p in list(ctl.model.parameters()) + [p for c in ctl.fc_controls.values() if c is not None for p in c.parameters()]:
        p.grad = None
    # ... and without one the same call is fused again
    del launches[:]
    with torch.enable_grad():
        ctl.gen_batch_by_controls(latent=z.detach(), normalize=False, age=age)
    assert launches.count(fcs.ENTRY) == 2


def test_existing_callers_launch_what_they_launched(ctl, launches):
    z = torch.randn(BATCH, 512, device='cuda')
    with torch.no_grad():
        ctl.model.style(z)
        assert fcs.ENTRY not in launches and launches.count('gc_bias_act_f32') == 7 * 8 and len(launches) == 7 * 8
        del launches[:]
        ctl.fc_controls['gamma'](torch.randn(BATCH, 27, device='cuda'))
        assert launches == ['gc_bias_act_f32'] * ic.CTL_N_MLP
        del launches[:]
        ctl.model([z])
        assert fcs.ENTRY not in launches and launches
