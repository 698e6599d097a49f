"""Write tests/golden/projection.npz from the reference's own projection helpers and generator (build machine only; reads the reference, commits
none of its text).

* ``noise_regularize``, ``noise_normalize_``, ``get_lr``, ``latent_noise`` and ``make_image`` are taken out of the reference's
  projection/projection.py BY NAME (the module's own imports -- streamlit, torchvision, sklearn -- are not installed) and run on the CPU, in
  float64 wherever the function is a float function (``make_image`` is a float32 -> byte function and runs on float32);
* the real reference ``Generator`` at 32 x 32 (procedural weights of oracle.networks.procedural_fill_, B = 2, float64) is differentiated with
  respect to its noise maps, a seeded probe as cotangent.  The reference raises ValueError for ``conv_transpose=False``
  (models/gan_model.py:232-233): that fact is recorded instead of a second set of gradients.

    python tools/make_projection_golden.py [path to the reference's src directory]
"""
import ast
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REF_SRC = sys.argv[1] if len(sys.argv) > 1 else '/root/reference/src'
sys.path.insert(0, REF_SRC)

from oracle.make_golden import seeded_noise          # noqa: E402  (also puts the reference's models on the path)
from oracle.networks import procedural_fill_          # noqa: E402
import gan_control.models.gan_model as ref_gm          # noqa: E402

MARGIN = 2e-6          # see main(): the smallest |pre-activation| / layer rms the generator fixture accepts
NAMES = ('noise_regularize', 'noise_normalize_', 'get_lr', 'latent_noise', 'make_image')


def reference_functions():
    path = os.path.join(REF_SRC, 'gan_control', 'projection', 'projection.py')
    tree = ast.parse(open(path).read(), path)
    keep = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in NAMES]
    assert sorted(n.name for n in keep) == sorted(NAMES)
    space = {'torch': torch, 'math': math}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, 'exec'), space)
    return {name: space[name] for name in NAMES}


def noise_lists(gen):
    """White noise, and a strongly correlated field (smooth + offset: level means far from zero), float64."""
    shapes = [(2, 4), (2, 8), (1, 8), (2, 16), (3, 16), (2, 32), (1, 32)]
    white = [torch.randn(b, 1, s, s, generator=gen, dtype=torch.float64) for b, s in shapes]
    smooth = []
    for b, s in shapes:
        ramp = torch.linspace(0, 2 * math.pi, s, dtype=torch.float64)
        field = torch.sin(ramp)[None, None, :, None] * torch.cos(0.5 * ramp)[None, None, None, :] + 0.75
        smooth.append(field + 0.1 * torch.randn(b, 1, s, s, generator=gen, dtype=torch.float64))
    return {'white': white, 'smooth': smooth}


def main():
    fn = reference_functions()
    gen = torch.Generator().manual_seed(20240611)
    out = {}
    for kind, maps in noise_lists(gen).items():
        leaves = [m.clone().requires_grad_(True) for m in maps]
        loss = fn['noise_regularize'](leaves)
        grads = torch.autograd.grad(loss, leaves)
        normed = [m.clone() for m in maps]
        fn['noise_normalize_'](normed)
        out['reg/%s/count' % kind] = len(maps)
        out['reg/%s/loss' % kind] = loss.detach()
        for i, (m, g, z) in enumerate(zip(maps, grads, normed)):
            out['reg/%s/x%d' % (kind, i)] = m
            out['reg/%s/g%d' % (kind, i)] = g
            out['reg/%s/n%d' % (kind, i)] = z
    ts = torch.linspace(0, 1, 41, dtype=torch.float64)
    out['lr/t'] = ts
    out['lr/value'] = torch.tensor([fn['get_lr'](float(t), 0.1) for t in ts], dtype=torch.float64)
    out['lr/value_ramps'] = torch.tensor([fn['get_lr'](float(t), 0.05, 0.5, 0.1) for t in ts], dtype=torch.float64)
    latent = torch.randn(2, 512, generator=gen, dtype=torch.float64)
    torch.manual_seed(1234)
    out['latent_noise/latent'], out['latent_noise/seed'], out['latent_noise/strength'] = latent, 1234, 0.37
    out['latent_noise/out'] = fn['latent_noise'](latent, 0.37)
    # make_image: every float next to a byte boundary (the fixture of the image output path) and a spread of ordinary values
    with np.load(os.path.join(REPO, 'tests', 'golden', 'image_output.npz')) as z:
        edges = torch.from_numpy(z['edges/x'])
    spread = torch.rand(2 * 3 * 16 * 16 - edges.numel(), generator=gen) * 2.6 - 1.3
    x = torch.cat([edges, spread]).reshape(2, 3, 16, 16)
    out['make_image/x'] = x
    out['make_image/bytes'] = fn['make_image'](x.clone())
    # the reference generator's noise-map gradients
    try:
        ref_gm.Generator(32, 512, 8, channel_multiplier=2, conv_transpose=False)
        out['gen/conv_transpose_false_raises'] = 0
    except ValueError:
        out['gen/conv_transpose_false_raises'] = 1
    g = ref_gm.Generator(32, 512, 8, channel_multiplier=2, conv_transpose=True)
    g.load_state_dict(procedural_fill_(g.state_dict()))
    g = g.double()
    # The gradient is discontinuous where a pre-activation of a leaky-ReLU crosses zero: an evaluation in float32, whatever its summation order,
    # may land on the other side of a pre-activation that float64 puts within rounding distance of zero, and one such flip moves one pixel of a
    # noise-map gradient by ~1 % of the map's largest value.  Of the ~2.8 M pre-activations of this generator two or so lie within 1e-6 of zero
    # (relative to their layer's rms) for a typical draw.  The inputs are therefore drawn again (seed, seed + 1, ...) until the REFERENCE's own
    # float64 evaluation has none within MARGIN: a condition on the reference alone, several times the rounding error a float32 forward pass
    # accumulates (~2e-7 per convolution, ~1e-6 at the image).
    pre = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: pre.append((inp[0] + mod.bias.view(1, -1, 1, 1)).detach()))
             for m in g.modules() if isinstance(m, ref_gm.StyledConv) for m in [m.activate]]
    for seed in range(777, 777 + 2000):
        del pre[:]
        z = torch.randn(2, 512, generator=torch.Generator().manual_seed(seed))
        noises = [n.double().requires_grad_(True) for n in seeded_noise(32, 2, seed)]
        img, _ = g([z.double()], noise=noises)
        assert len(pre) == 7
        margin = min(float(v.abs().min() / v.pow(2).mean().sqrt()) for v in pre)
        if margin > MARGIN:
            break
    else:
        raise SystemExit('no draw with a margin above %g' % MARGIN)
    for h in hooks:
        h.remove()
    print('generator inputs: seed %d, smallest |pre-activation| / layer rms %.3e' % (seed, margin))
    probe = torch.randn(img.shape, generator=gen)
    grads = torch.autograd.grad(img, noises, probe.double())
    out.update({'gen/z': z, 'gen/noise_seed': seed, 'gen/margin': margin, 'gen/probe': probe, 'gen/img': img.detach(), 'gen/count': len(noises)})
    for i, gr in enumerate(grads):
        out['gen/g%d' % i] = gr
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(REPO, 'tests', 'golden', 'projection.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s: %d entries, %d bytes' % (path, len(arrays), os.path.getsize(path)))


if __name__ == '__main__':
    main()
