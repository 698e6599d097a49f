"""Shared by test_projection.py and test_projection_gpu.py: the fixture, the 32 x 32 generator's noise-map gradients, the backend call recorder
and the projection scenario.

    python tests/projection_checks.py        writes tests/golden/projection_backward_calls.json: the backend calls of one backward pass of
                                             the 32 x 32 generator in which no noise map wants a gradient.  The committed file was recorded at
                                             the commit BEFORE the noise-map gradient was wired in; the test holds today's sequence to it.
"""
import json
import os

import torch

import op_checks as oc
from conftest import GOLDEN, EmulatedBackend, group, load_golden, rel_err

GOLD = load_golden('projection')
CALLS_JSON = os.path.join(GOLDEN, 'projection_backward_calls.json')


def gen_inputs(device):
    r = group(GOLD, 'gen')
    noises = oc.seeded_noise(32, 2, int(r['noise_seed']), device)
    return r, r['z'].to(device), noises, r['probe'].to(device)


def generator_noise_grads(device, noise_grads=True):
    """(image, [gradient of <image, probe> w.r.t. every noise map]) of the 32 x 32 generator with the fixture's inputs, parameters frozen."""
    r, z, noises, probe = gen_inputs(device)
    g, _ = oc.build_models(32, device)
    for p in g.parameters():
        p.requires_grad_(False)
    z = z.clone().requires_grad_(True)
    for n in noises:
        n.requires_grad_(noise_grads)
    img, _ = g([z], noise=noises)
    (img * probe).sum().backward()
    return img.detach(), [n.grad for n in noises], z.grad


class RecordingBackend:
    """An EmulatedBackend whose method calls are written down."""

    def __init__(self):
        self._inner, self.calls = EmulatedBackend(), []

    def __getattr__(self, name):
        value = getattr(self._inner, name)
        if not callable(value):
            return value

        def wrapped(*a, **kw):
            self.calls.append(name)
            return value(*a, **kw)
        return wrapped


def backward_call_sequence(noise_grads, train_params=False):
    """Names of the backend calls made by forward + backward of the 32 x 32 generator (the backward's alone: the forward's are cut off)."""
    from gan_control_amd.models.op import _backend
    rec = RecordingBackend()
    prev = _backend._install_for_tests(rec)
    try:
        r, z, noises, probe = gen_inputs('cpu')
        g, _ = oc.build_models(32, 'cpu')
        for p in g.parameters():
            p.requires_grad_(train_params)
        z = z.clone().requires_grad_(True)
        for n in noises:
            n.requires_grad_(noise_grads)
        img, _ = g([z], noise=noises)
        cut = len(rec.calls)
        (img * probe).sum().backward()
        return rec.calls[cut:]
    finally:
        _backend._install_for_tests(prev)


def fir_act_reference(x, taps, pad, bias, noise, noise_w, slope, gain):
    be = EmulatedBackend()
    p0, p1 = pad
    oh, ow = x.shape[2] + p0 + p1 - taps.shape[0] + 1, x.shape[3] + p0 + p1 - taps.shape[1] + 1
    y = be.upfirdn2d(x, taps.to(x.dtype), 1, 1, p0, p0, oh, ow, True)
    return torch.nn.functional.leaky_relu(y + noise_w * noise + bias.reshape(1, -1, 1, 1), slope) * gain


def check_fir_act_noise_grad(device, tol):
    """upfirdn2d_bias_act (the Blur + noise + activation of an up-sampling StyledConv, planes the tile kernel takes) w.r.t. its noise map,
    against float64 autograd of the unfused formula; with frozen and with trained bias / noise strength (the two routes of the backward)."""
    from gan_control_amd.models.op.upfirdn2d import upfirdn2d_bias_act
    gen = torch.Generator().manual_seed(8)
    x, noise = torch.randn(2, 5, 65, 65, generator=gen), torch.randn(2, 1, 64, 64, generator=gen)
    bias, noise_w, probe = torch.randn(5, generator=gen) * 0.1, torch.tensor([0.3]), torch.randn(2, 5, 64, 64, generator=gen)
    k = torch.tensor([1., 3., 3., 1.])
    taps = (k[None, :] * k[:, None]) / k.sum() ** 2 * 4
    leaves64 = [t.double().requires_grad_(True) for t in (x, noise, bias, noise_w)]
    want = torch.autograd.grad((fir_act_reference(leaves64[0], taps, (1, 1), *leaves64[2:3], leaves64[1], leaves64[3], 0.2, 2 ** 0.5) * probe.double()).sum(), leaves64)
    for train in (False, True):
        xs, ns, bs, ws = [t.clone().to(device).requires_grad_(flag) for t, flag in ((x, True), (noise, True), (bias, train), (noise_w, train))]
        out = upfirdn2d_bias_act(xs, taps.to(device), (1, 1), bs, ns, ws, 0.2, 2 ** 0.5)
        (out * probe.to(device)).sum().backward()
        assert ns.grad is not None and rel_err(ns.grad, want[1]) <= tol, (train, rel_err(ns.grad, want[1]))
        assert rel_err(xs.grad, want[0]) <= tol
        if train:
            assert rel_err(bs.grad, want[2]) <= tol and rel_err(ws.grad, want[3]) <= tol


def run_projection(device, steps=24):
    """MSE-only projection of a target rendered by the same generator from another latent.  -> dict of what the tests assert on."""
    from gan_control_amd import projection
    g, _ = oc.build_models(32, device)
    g.eval()
    flags = [p.requires_grad for p in g.parameters()]
    gen = torch.Generator().manual_seed(99)
    with torch.no_grad():
        w = g.style(torch.randn(2, 512, generator=gen).to(device))
        target, _ = g([w], input_is_latent=True, noise=[n.to(device) for n in oc.seeded_noise(32, 2, 5, 'cpu')])
    seen = {'stats': [], 'first': None}

    def on_step(i, info):
        if i == 0:
            seen['first'] = (info['latent'].detach().clone(), [n.detach().clone() for n in info['noises']],
                             info['latent'].grad is not None, [n.grad is not None for n in info['noises']])
        seen['stats'].append(torch.stack([torch.stack([n.detach().double().mean(), n.detach().double().std()]) for n in info['noises']]))

    latent, noises, image, history = projection.project(g, target, steps=steps, lr=0.1, mse_weight=1.0, n_mean_latent=256,
                                                         generator=torch.Generator().manual_seed(3), on_step=on_step)
    return {'latent': latent, 'noises': noises, 'image': image, 'history': history, 'seen': seen, 'target': target,
            'flags_before': flags, 'flags_after': [p.requires_grad for p in g.parameters()], 'generator': g}


def check_projection(out, steps):
    seen, history = out['seen'], out['history']
    assert len(history) == steps and len(seen['stats']) == steps
    first_latent, first_noises, latent_has_grad, noises_have_grad = seen['first']
    assert latent_has_grad and all(noises_have_grad), 'the latent and every noise map receive a gradient'
    # step 0 runs at learning rate get_lr(0) = 0: the maps have moved by the end, and so has the latent
    assert float((out['latent'] - first_latent).abs().max()) > 1e-3
    stats = torch.stack(seen['stats']).cpu()          # [steps, maps, 2]
    assert float(stats[:, :, 0].abs().max()) <= 1e-5 and float((stats[:, :, 1] - 1).abs().max()) <= 1e-5, stats
    moved = [float((a - b).abs().max()) > 1e-3 for a, b in zip(out['noises'], first_noises)]
    assert all(moved), moved
    final_mse = float((out['image'] - out['target']).pow(2).mean())
    print('projection: first mse %.6g, final mse %.6g, ratio %.4f' % (history[0]['mse'], final_mse, final_mse / history[0]['mse']))
    assert final_mse < history[0]['mse']
    assert out['flags_after'] == out['flags_before'] and any(out['flags_before'])
    return final_mse / history[0]['mse']


if __name__ == '__main__':
    calls = backward_call_sequence(False)
    calls_train = backward_call_sequence(False, train_params=True)
    with open(CALLS_JSON, 'w') as f:
        json.dump({'frozen_parameters': calls, 'trained_parameters': calls_train}, f, indent=0)
    print('wrote %s: %d and %d calls' % (CALLS_JSON, len(calls), len(calls_train)))
