"""Shared pieces of the ArcFace predictor tests (tests/test_arcface*.py) and of tools/make_arcface_golden.py.

* ``fill_weights``: procedural, CRC32(key)-seeded parameters that keep the activations O(1) through all 24 units (He-scaled convolutions,
  BatchNorm gamma in [0.5, 1], running_var in [0.5, 2], small running means, PReLU alpha ~0.25, 1/sqrt(fan-in) SE and head weights);
  the fixture generator and the tests make the same weights from the key list alone.
* ``restated``: the network restated in plain PyTorch (F.conv2d / F.batch_norm / F.prelu ...) from the architecture, over a state dict;
  differentiable in the input.  It is held against the fixture, and is the predictor of the G-step comparison on the GPU.
* the fixture's cases, input draws and probe vectors.
"""
import math
import zlib

import torch
import torch.nn.functional as F

CASES = {             # name: (batch, image size, centre crop)
    'c1024': (2, 1024, 480),
    'c256': (4, 256, 120),
    'c64': (2, 64, 60),
}
SHAPES = ((64, 56), (128, 28), (256, 14), (512, 7))
FFHQ_EMBEDDING = {'enabled': True, 'center_crop': 480, 'model_path': 'pretrained_models/model_ir_se50.pth', 'num_layers': 50, 'drop_ratio': 0.6,
                  'mode': 'ir_se', 'lower_thres': [0.154, 0.161, 0.202, 0.166], 'upper_thres': [0.186, 0.185, 0.231, 0.129], 'last_lower_thres': 0.5,
                  'last_upper_thres': 1.8, 'intermediate_layers_weights': [0, 0, 0, 0], 'last_layer_weight': 0.25, 'same_group_name': 'id',
                  'focus_on_list': ['not_same_as_last_layer'] * 4 + ['same_as_last_layer']}


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) & 0x7FFFFFFF)


def fill_weights(state_dict):
    """In place; returns state_dict.  Keys ending in running_mean / running_var / num_batches_tracked / weight / bias, by module kind."""
    bn_prefixes = {k[:-len('running_var')] for k in state_dict if k.endswith('running_var')}
    for key in sorted(state_dict):
        t = state_dict[key]
        if key.endswith('num_batches_tracked'):
            continue
        g = _gen('arcface/' + key)
        prefix = key.rsplit('.', 1)[0] + '.'
        shape = t.shape
        if prefix in bn_prefixes:
            if key.endswith('.weight'):
                v = 0.5 + 0.5 * torch.rand(shape, generator=g, dtype=torch.float64)
            elif key.endswith('running_var'):
                v = 0.5 + 1.5 * torch.rand(shape, generator=g, dtype=torch.float64)
            else:                                   # bias, running_mean
                v = 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
        elif len(shape) == 1 and key.endswith('.weight'):        # PReLU
            v = 0.2 + 0.1 * torch.rand(shape, generator=g, dtype=torch.float64)
        elif len(shape) == 1:                                   # Linear bias
            v = 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
        else:
            fan_in = int(math.prod(shape[1:]))
            gain = 1.0 if ('.fc' in key or len(shape) == 2) else 2.0       # SE and head: 1/sqrt(fan-in); convolutions: He
            v = torch.randn(shape, generator=g, dtype=torch.float64) * math.sqrt(gain / fan_in)
        with torch.no_grad():
            t.copy_(v.to(t.dtype))
    return state_dict


def make_state_dict(keys_shapes, dtype=torch.float32):
    sd = {}
    for k, shape in keys_shapes:
        sd[k] = torch.zeros(tuple(int(s) for s in shape), dtype=torch.int64 if k.endswith('num_batches_tracked') else dtype)
    return fill_weights(sd)


def case_input(name, dtype=torch.float32):
    b, size, _ = CASES[name]
    return (torch.rand(b, 3, size, size, generator=_gen('arcface/input/' + name), dtype=torch.float64) * 2 - 1).to(dtype)


def probes(name, dtype=torch.float32):
    """The V of the scalar sum_levels <feature, V_level> whose input gradient the fixture records (each level scaled to unit total weight)."""
    b = CASES[name][0]
    out = []
    for i, (c, hw) in enumerate(SHAPES):
        v = torch.randn(b, c, hw, hw, generator=_gen('arcface/probe/%s/%d' % (name, i)), dtype=torch.float64)
        out.append((v / math.sqrt(c * hw * hw)).to(dtype))
    out.append(torch.randn(b, 512, generator=_gen('arcface/probe/%s/emb' % name), dtype=torch.float64).to(dtype))
    return out


def probe_scalar(feats, vs):
    return sum((f * v).sum() for f, v in zip(feats, vs))


def hinge_loss(feats):
    """The ffhq embedding_loss hinge on a B = 4 batch: rows 0-1 the 'same' block, rows 2-3 the 'not same' one."""
    from gan_control_amd.losses import LossModelClass
    lm = LossModelClass(FFHQ_EMBEDDING, 'embedding_loss', mini_batch_size=4, no_model=True)
    return lm.calc_mini_batch_loss([f[:2] for f in feats], [f[2:] for f in feats])


# -- the plain-PyTorch restatement --------------------------------------------------------------------------------------------------
def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + 'running_mean'], sd[p + 'running_var'], sd[p + 'weight'], sd[p + 'bias'], False, 0.0, 1e-5)


def _unit(sd, p, x, stride, se):
    if (p + 'shortcut_layer.0.weight') in sd:
        sc = _bn(sd, p + 'shortcut_layer.1.', F.conv2d(x, sd[p + 'shortcut_layer.0.weight'], stride=stride))
    else:
        sc = x[:, :, ::stride, ::stride]
    r = _bn(sd, p + 'res_layer.0.', x)
    r = F.conv2d(r, sd[p + 'res_layer.1.weight'], padding=1)
    r = F.prelu(r, sd[p + 'res_layer.2.weight'])
    r = F.conv2d(r, sd[p + 'res_layer.3.weight'], stride=stride, padding=1)
    r = _bn(sd, p + 'res_layer.4.', r)
    if se:
        m = r.mean((2, 3), keepdim=True)
        s = torch.sigmoid(F.conv2d(F.relu(F.conv2d(m, sd[p + 'res_layer.5.fc1.weight'])), sd[p + 'res_layer.5.fc2.weight']))
        r = r * s
    return r + sc


def unit_strides(num_layers=50):
    units = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}[num_layers]
    out = []
    for n in units:
        out += [2] + [1] * (n - 1)
    return out


def restated(sd, x, center_crop=None, num_layers=50, se=True):
    """[layer1, layer2, layer3, layer4, l2_norm(embedding)] of ArcFaceSkeleton on x [B, 3, H, W] (state dict on x's device / dtype)."""
    if x.shape[-1] != 112:
        if center_crop is not None:
            h, w = x.shape[2], x.shape[3]
            t, l = (h - center_crop) // 2, (w - center_crop) // 2
            x = x[:, :, t:t + center_crop, l:l + center_crop]
        x = F.interpolate(x, size=(112, 112), mode='bilinear', align_corners=True)
    x = F.prelu(_bn(sd, 'input_layer.1.', F.conv2d(x, sd['input_layer.0.weight'], padding=1)), sd['input_layer.2.weight'])
    levels = []
    for i, s in enumerate(unit_strides(num_layers)):
        x = _unit(sd, 'body.%d.' % i, x, s, se)
        if i + 1 in (3, 7, 21):
            levels.append(x)
    levels.append(x)
    e = _bn(sd, 'output_layer.0.', x).flatten(1)
    e = F.linear(e, sd['output_layer.3.weight'], sd['output_layer.3.bias'])
    e = F.batch_norm(e, sd['output_layer.4.running_mean'], sd['output_layer.4.running_var'], sd['output_layer.4.weight'], sd['output_layer.4.bias'],
                     False, 0.0, 1e-5)
    return levels + [e / torch.norm(e, 2, 1, True)]


class RestatedSkeleton(torch.nn.Module):
    """``restated`` as a predictor module (the plain-PyTorch baseline of the G-step comparison and of tools/arcface_bench.py).  With
    ``dtype=torch.float64`` the network runs in float64 and hands fp32 features back (an exact reference for an fp32 caller)."""

    def __init__(self, sd, center_crop, dtype=torch.float32):
        super().__init__()
        self.dtype = dtype
        self.sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        self.center_crop = center_crop

    def to(self, device):
        self.sd = {k: v.to(device) for k, v in self.sd.items()}
        return self

    def forward(self, x):
        return [f.to(x.dtype) for f in restated(self.sd, x.to(self.dtype), self.center_crop)]


# -- the fixture's record of one run -----------------------------------------------------------------------------------------------
def level_summary(f):
    """(per-channel means [B, C], strided sample) of a [B, C, h, w] level."""
    return f.mean((2, 3)), f[:, ::7, ::3, ::3]


def grad_summary(g):
    """(per-channel sums [B, 3], norm, strided sample) of an input gradient."""
    step = max(1, g.shape[2] // 24)
    return g.sum((2, 3)), g.norm(), g[:, :, ::step, ::step]


# -- the product against the fixture ------------------------------------------------------------------------------------------------
def load_fixture():
    from conftest import load_golden
    return load_golden('arcface')


def fixture_state_dict(gold):
    keys = [str(k) for k in gold['keys']]
    shapes = [tuple(int(s) for s in row if s > 0) for row in gold['key_shapes']]
    return make_state_dict(list(zip(keys, shapes)))


def run_product(gold, name, device, hinge=False):
    """-> (errors {what: relative error}, the skeleton) of the ArcFaceSkeleton on ``device`` against the fixture's case ``name``."""
    from conftest import rel_err
    from gan_control_amd.losses import ArcFaceSkeleton
    b, size, crop = CASES[name]
    skel = ArcFaceSkeleton(dict(FFHQ_EMBEDDING, center_crop=crop), state_dict=fixture_state_dict(gold)).to(device)
    x = case_input(name)
    assert torch.equal(x.reshape(-1)[:64], torch.from_numpy(gold[name + '/x_check']).float())
    x = x.to(device).requires_grad_(True)
    feats = skel(x)
    err = {}
    for i, f in enumerate(feats[:4]):
        mean, sample = level_summary(f.detach())
        err['level%d_mean' % i] = rel_err(mean, torch.from_numpy(gold['%s/level%d_mean' % (name, i)]))
        err['level%d_sample' % i] = rel_err(sample, torch.from_numpy(gold['%s/level%d_sample' % (name, i)]))
    err['embedding'] = rel_err(feats[4], torch.from_numpy(gold[name + '/embedding']))
    g, = torch.autograd.grad(probe_scalar(feats, [v.to(device) for v in probes(name)]), x, retain_graph=hinge)
    sums, norm, sample = grad_summary(g)
    err['grad_sums'] = rel_err(sums, torch.from_numpy(gold[name + '/grad_sums']))
    err['grad_norm'] = rel_err(norm, torch.from_numpy(gold[name + '/grad_norm']))
    err['grad_sample'] = rel_err(sample, torch.from_numpy(gold[name + '/grad_sample']))
    if hinge:
        loss = hinge_loss(feats)
        err['hinge'] = rel_err(loss, torch.from_numpy(gold[name + '/hinge']))
        g, = torch.autograd.grad(loss, x)
        sums, norm, sample = grad_summary(g)
        err['hinge_grad_sums'] = rel_err(sums, torch.from_numpy(gold[name + '/hinge_grad_sums']))
        err['hinge_grad_norm'] = rel_err(norm, torch.from_numpy(gold[name + '/hinge_grad_norm']))
        err['hinge_grad_sample'] = rel_err(sample, torch.from_numpy(gold[name + '/hinge_grad_sample']))
    return err, skel


# fp32 against the float64 fixture: the outputs agree to ~1e-5; the input gradient's per-pixel values move by up to ~1.4e-2 of their maximum
# and its per-channel sums by ~5e-3 (measured with the fp32 plain-PyTorch restatement itself: PReLU / ReLU slope choices of
# pre-activations within rounding of zero), its norm by ~1.5e-5.  The bounds are about twice that.
TOLERANCE = {'f32': {'out': 1e-4, 'grad': 3e-2, 'norm': 1e-4},
             'bf16x3': {'out': 1e-3, 'grad': 3e-2, 'norm': 1e-3}}


def kind(key):
    if key.endswith('grad_norm'):
        return 'norm'
    return 'grad' if 'grad' in key else 'out'


def over_tolerance(err, mode='f32'):
    return {k: v for k, v in err.items() if v > TOLERANCE[mode][kind(k)]}
