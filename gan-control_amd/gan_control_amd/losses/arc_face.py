"""The identity predictor of the embedding loss (ArcFace IR / IR-SE ResNet) on the HIP kernels: forward and input gradient.

The controllable step's ``embedding_loss`` (configs/ffhq.json: IR-SE50, ``center_crop`` 480) runs this frozen network on every
generator step and back-propagates through it into G.  Architecture (the published ArcFace "insightface" backbone):

    input_layer   conv3x3(3 -> 64) -> BatchNorm2d -> PReLU                                   at 112 x 112
    body          units of  x -> BN -> conv3x3 -> PReLU -> conv3x3(stride s) -> BN [-> SE]  +  shortcut(x)
                  shortcut = MaxPool2d(1, s) when the depth is unchanged, else conv1x1(stride s) -> BN;
                  SE = sigmoid(fc2(relu(fc1(mean_hw)))) * r  with a 16 x channel reduction
    output_layer  BatchNorm2d -> Dropout -> Flatten -> Linear(512 * 7 * 7 -> 512) -> BatchNorm1d,  then l2_norm

``ArcFaceSkeleton.forward`` returns the outputs of ``body[:3]``, ``body[3:7]``, ``body[7:21]``, ``body[21:]`` and the normalised embedding
(the reference's ``arc_face_skeleton.py`` level split, kept for every depth).

Execution (inference only: BatchNorm on its running statistics, Dropout the identity, every parameter frozen):
  * crop + resize: gc_crop_resize_ac_f32 (align_corners=True bilinear; its adjoint writes the full-size input gradient);
  * every convolution: the generalised convolution kernels (gc_conv2d_fused_*, the path of conv2d_gradfix._GConv) with the BatchNorm
    that follows folded into the weights and the epilogue bias, once per load (kernel-layout and adjoint weights are frozen tensors
    registered with the weight cache, so the split-bf16 packs are made once); no weight gradient is ever computed;
  * the BatchNorm in front of a unit's first convolution (zero padding follows it: it does not fold) and the PReLUs: gc_affine_prelu_f32;
  * squeeze-excitation: gc_plane_reduce_f32 -> gc_se_mlp_f32 -> gc_se_apply_f32 (the shortcut added in the same pass, the MaxPool(1, 2)
    subsample read with a stride);
  * the head: BN2d -> Linear -> BN1d folded (in float64) into one [512, 25088] weight and bias, a torch.addmm (hipBLASLt, like the mapping
    network's GEMMs); l2_norm is ATen (no eps, as the reference).
Each unit is one autograd Function whose backward returns the input gradient only (once-differentiable).
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ..models.op import _backend
from ..models.op._backend import ConvGeom

LEVEL_ENDS = (3, 7, 21)          # body[:3], body[3:7], body[7:21], body[21:]
UNITS = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}
DEPTHS = (64, 128, 256, 512)
SE_REDUCTION = 16
INPUT_SIZE = 112


class _Subsample(nn.Module):
    """MaxPool2d(1, stride): x[:, :, ::stride, ::stride] (no parameters)."""

    def __init__(self, stride):
        super().__init__()
        self.stride = stride


class SEModule(nn.Module):
    def __init__(self, channels, reduction=SE_REDUCTION):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, channels // reduction, 1, bias=False)
        self.fc2 = nn.Conv2d(channels // reduction, channels, 1, bias=False)


class BottleneckIR(nn.Module):
    """One residual unit (``ir``; with ``se`` the ``ir_se`` unit).  The submodules only hold the parameters under the reference's names."""

    def __init__(self, in_channel, depth, stride, se):
        super().__init__()
        if in_channel == depth:
            self.shortcut_layer = _Subsample(stride)
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(in_channel, depth, 1, stride, bias=False), nn.BatchNorm2d(depth))
        layers = [nn.BatchNorm2d(in_channel), nn.Conv2d(in_channel, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                  nn.Conv2d(depth, depth, 3, stride, 1, bias=False), nn.BatchNorm2d(depth)]
        if se:
            layers.append(SEModule(depth))
        self.res_layer = nn.Sequential(*layers)
        self.in_channel, self.depth, self.stride, self.se = in_channel, depth, stride, se


def _unit_specs(num_layers):
    specs, prev = [], 64
    for depth, n in zip(DEPTHS, UNITS[num_layers]):
        specs.append((prev, depth, 2))
        specs += [(depth, depth, 1)] * (n - 1)
        prev = depth
    return specs


class Backbone(nn.Module):
    """ArcFace IR / IR-SE backbone with the reference's ``Backbone`` state-dict keys and shapes (``model_ir_se50.pth`` loads strictly).
    ``forward`` returns the l2-normalised embedding [B, 512] of a [B, 3, 112, 112] input."""

    def __init__(self, num_layers, drop_ratio, mode='ir'):
        super().__init__()
        if num_layers not in UNITS:
            raise ValueError('num_layers should be 50, 100 or 152, got %r' % (num_layers,))
        if mode not in ('ir', 'ir_se'):
            raise ValueError("mode should be 'ir' or 'ir_se', got %r" % (mode,))
        self.num_layers, self.mode = num_layers, mode
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(512), nn.Dropout(drop_ratio), nn.Flatten(), nn.Linear(512 * 7 * 7, 512), nn.BatchNorm1d(512))
        self.body = nn.Sequential(*[BottleneckIR(i, d, s, mode == 'ir_se') for i, d, s in _unit_specs(num_layers)])
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        self._plan = None

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('ArcFace predictor: inference only (BatchNorm running statistics, frozen parameters); keep it in eval()')
        return super().train(False)

    # -- folded forms, rebuilt when a parameter / buffer is replaced or written ----------------------------------------------------
    def _state_key(self):
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def plan(self):
        dev = self.input_layer[0].weight.device
        key = (dev, self._state_key())
        if self._plan is None or self._plan[0] != key:
            self._plan = (key, _build_plan(self))
        return self._plan[1]

    def levels(self, x):
        """[B, 3, 112, 112] -> [layer1, layer2, layer3, layer4, embedding before l2_norm]."""
        if self.training:
            raise NotImplementedError('ArcFace predictor: inference only; call .eval()')
        plan = self.plan()
        x = _backend.call(_Stem, x, plan['stem'])
        out = []
        for i, unit in enumerate(plan['units']):
            x = _backend.call(_Unit, x, unit)
            if i + 1 in LEVEL_ENDS:
                out.append(x)
        out.append(x)
        w, b = plan['head']
        out.append(torch.addmm(b, x.reshape(x.shape[0], -1), w.t()))
        return out

    def forward(self, x):
        return l2_norm(self.levels(_check_input(x, INPUT_SIZE))[-1])


def l2_norm(x, axis=1):
    """x / ||x||_2 along ``axis`` (no eps, as the reference; ATen)."""
    return x / torch.norm(x, 2, axis, True)


def _bn_affine(bn):
    """BatchNorm (eval) -> float64 (scale, shift)."""
    scale = bn.weight.detach().double() * torch.rsqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


def _conv_weights(w, scale=None):
    """[N, K, kh, kw] (times the per-output-channel scale) -> (w_t [kh, kw, K, N], adjoint [kh, kw, N, K] with mirrored taps), frozen and
    registered with the weight cache (the split-bf16 packs of both are derived once)."""
    from ..models.op import weight_cache
    w = w.detach().double()
    if scale is not None:
        w = w * scale.reshape(-1, 1, 1, 1)
    w_t = w.permute(2, 3, 1, 0)
    adj = w_t.flip(0, 1).transpose(2, 3)
    out = []
    for t in (w_t, adj):
        p = nn.Parameter(t.float().contiguous(), requires_grad=False)
        weight_cache.register(p)
        out.append(p)
    return out


def _f32(t):
    return t.float().contiguous()


def _build_plan(net):
    conv, bn, prelu = net.input_layer
    s, t = _bn_affine(bn)
    w, w_adj = _conv_weights(conv.weight, s)
    stem = {'w': w, 'w_adj': w_adj, 'bias': _f32(t), 'alpha': _f32(prelu.weight.detach())}
    units = []
    for u in net.body:
        r = u.res_layer
        s_in, t_in = _bn_affine(r[0])
        w1, w1_adj = _conv_weights(r[1].weight)
        s2, t2 = _bn_affine(r[4])
        w2, w2_adj = _conv_weights(r[3].weight, s2)
        unit = {'stride': u.stride, 'bn_scale': _f32(s_in), 'bn_shift': _f32(t_in), 'w1': w1, 'w1_adj': w1_adj, 'alpha': _f32(r[2].weight.detach()),
                'w2': w2, 'w2_adj': w2_adj, 'b2': _f32(t2), 'sc': None, 'se': None}
        if isinstance(u.shortcut_layer, nn.Sequential):
            ss, ts = _bn_affine(u.shortcut_layer[1])
            wsc, wsc_adj = _conv_weights(u.shortcut_layer[0].weight, ss)
            unit['sc'] = (wsc, wsc_adj, _f32(ts))
        if u.se:
            se = r[5]
            unit['se'] = (_f32(se.fc1.weight.detach().flatten(1)), _f32(se.fc2.weight.detach().flatten(1)))
        units.append(unit)
    # BN2d -> flatten -> Linear -> BN1d:  emb = s1 * (W (x * s2 + t2) + b) + t1  =  W' x + b'   (float64, then fp32)
    bn2, _, _, lin, bn1 = net.output_layer
    s2, t2 = _bn_affine(bn2)
    s1, t1 = _bn_affine(bn1)
    hw = lin.in_features // s2.numel()
    s2e, t2e = s2.repeat_interleave(hw), t2.repeat_interleave(hw)
    wl = lin.weight.detach().double()
    w_head = s1[:, None] * wl * s2e[None, :]
    b_head = s1 * (wl @ t2e + lin.bias.detach().double()) + t1
    return {'stem': stem, 'units': units, 'head': (_f32(w_head), _f32(b_head))}


def _geom(k, stride, pad, in_hw):
    oh, ow = (in_hw[0] + 2 * pad - k) // stride + 1, (in_hw[1] + 2 * pad - k) // stride + 1
    return ConvGeom(k, k, 1, stride, pad, pad, oh, ow)


def _adjoint(g, in_hw):
    """Geometry of d/dx of a (down = stride) convolution: up = stride, mirrored pad, the input's extent (even outputs of stride-2 layers)."""
    return ConvGeom(g.kh, g.kw, g.down, g.up, g.kh - 1 - g.pad_y, g.kw - 1 - g.pad_x, in_hw[0], in_hw[1])


def _bias_ep(bias, residual=None):
    return (bias, None, None, 0.0, 1.0, False, residual)


class _CropResize(Function):
    """x [B, C, H, W] -> bilinear (align_corners=True) resize of the crop [top:top + ch, left:left + cw] to out x out."""

    @staticmethod
    def forward(ctx, x, top, left, ch, cw, out):
        ctx.cfg = (top, left, ch, cw, out, (x.shape[2], x.shape[3]))
        return _backend.get().crop_resize_ac(x, top, left, ch, cw, out, out)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        top, left, ch, cw, out, in_hw = ctx.cfg
        return _backend.get().crop_resize_ac(g, top, left, ch, cw, out, out, adjoint=True, in_hw=in_hw), None, None, None, None, None


class _Stem(Function):
    """input_layer: prelu(conv3x3(x, W * s) + t, alpha)."""

    @staticmethod
    def forward(ctx, x, p):
        be = _backend.get()
        geom = _geom(3, 1, 1, x.shape[2:])
        c0 = be.conv2d(x.contiguous(), p['w'], None, None, geom, epilogue=_bias_ep(p['bias']))
        ctx.p, ctx.geom, ctx.in_hw = p, geom, (x.shape[2], x.shape[3])
        ctx.save_for_backward(c0)
        return be.affine_prelu(c0, None, None, p['alpha'])

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        c0, = ctx.saved_tensors
        be, p = _backend.get(), ctx.p
        with _backend.pitched_outputs(False):
            gc0 = be.affine_prelu_bwd(g, c0, None, None, p['alpha'])
            return be.conv2d(gc0, p['w_adj'], None, None, _adjoint(ctx.geom, ctx.in_hw)), None


class _Unit(Function):
    """One residual unit (see the module docstring); backward = the input gradient through both branches, the shortcut's gradient added
    inside the first BatchNorm's backward pass."""

    @staticmethod
    def forward(ctx, x, u):
        be = _backend.get()
        x = x.contiguous()
        s = u['stride']
        in_hw = (x.shape[2], x.shape[3])
        g1 = _geom(3, 1, 1, in_hw)
        g2 = _geom(3, s, 1, in_hw)
        a = be.affine_prelu(x, u['bn_scale'], u['bn_shift'], None)
        c1 = be.conv2d(a, u['w1'], None, None, g1)
        del a
        p1 = be.affine_prelu(c1, None, None, u['alpha'])
        gsc = None
        if u['sc'] is not None:
            gsc = _geom(1, s, 0, in_hw)
            sc = be.conv2d(x, u['sc'][0], None, None, gsc, epilogue=_bias_ep(u['sc'][2]))
        else:
            sc = None
        ctx.u, ctx.geoms, ctx.in_hw = u, (g1, g2, gsc), in_hw
        if u['se'] is not None:
            r = be.conv2d(p1, u['w2'], None, None, g2, epilogue=_bias_ep(u['b2']))
            del p1
            fc1, fc2 = u['se']
            hw = r.shape[2] * r.shape[3]
            m = be.plane_reduce(r, None, 1.0 / hw)
            z, sg = be.se_mlp(m, fc1, fc2)
            out = be.se_apply(r, sg, sc, 1) if sc is not None else be.se_apply(r, sg, x, s)
            ctx.save_for_backward(c1, r, z, sg)
            return out
        residual = sc if sc is not None else x[:, :, ::s, ::s].contiguous()
        out = be.conv2d(p1, u['w2'], None, None, g2, epilogue=_bias_ep(u['b2'], residual))
        ctx.save_for_backward(c1)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        be, u = _backend.get(), ctx.u
        g1, g2, gsc = ctx.geoms
        g = g.contiguous()
        with _backend.pitched_outputs(False):
            if u['se'] is not None:
                c1, r, z, sg = ctx.saved_tensors
                fc1, fc2 = u['se']
                b, c, h, w = r.shape
                t = be.plane_reduce(g, r)
                gm = be.se_mlp_bwd(t, sg, z, fc1, fc2, 1.0 / (h * w))
                # g_r = g * s + g_mean / HW: one affine pass over B*C planes of a single sample
                gr = be.affine_prelu(g.reshape(1, b * c, h, w), sg.reshape(-1), gm.reshape(-1), None).reshape(b, c, h, w)
            else:
                c1, = ctx.saved_tensors
                gr = g
            gp = be.conv2d(gr, u['w2_adj'], None, None, _adjoint(g2, c1.shape[2:]))
            del gr
            gc1 = be.affine_prelu_bwd(gp, c1, None, None, u['alpha'])
            del gp
            ga = be.conv2d(gc1, u['w1_adj'], None, None, _adjoint(g1, ctx.in_hw))
            del gc1
            if u['sc'] is not None:
                g_sc, strided = be.conv2d(g, u['sc'][1], None, None, _adjoint(gsc, ctx.in_hw)), False
            else:
                g_sc, strided = g, u['stride'] != 1
            return be.affine_prelu_bwd(ga, None, u['bn_scale'], None, None, g_sc, strided), None


def _check_input(x, size=None):
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError('ArcFace predictor: [B, 3, H, W] images expected, got %s' % (tuple(x.shape),))
    if size is not None and (x.shape[2] != size or x.shape[3] != size):
        raise ValueError('ArcFace Backbone: %d x %d input expected, got %s' % (size, size, tuple(x.shape)))
    return x


class ArcFaceSkeleton(nn.Module):
    """The reference's ``ArcFaceSkeleton`` (losses/arc_face/arc_face_skeleton.py): ``config`` is the ``embedding_loss`` section (num_layers,
    drop_ratio, mode, model_path, center_crop).  ``state_dict``: the Backbone checkpoint (``model_ir_se50.pth``); without it the file at
    ``config['model_path']`` is loaded on the CPU.  Use it as ``LossModelClass(cfg, 'embedding_loss', skeleton_model=ArcFaceSkeleton(cfg))``."""

    def __init__(self, config, state_dict=None):
        super().__init__()
        self.config = config
        self.net = Backbone(config['num_layers'], config.get('drop_ratio', 0.0), mode=config['mode'])
        if state_dict is None:
            state_dict = torch.load(config['model_path'], map_location='cpu')
        self.net.load_state_dict(state_dict, strict=True)
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('ArcFaceSkeleton: inference only (BatchNorm running statistics, frozen parameters); keep it in eval()')
        return super().train(False)

    def forward(self, x):
        _check_input(x)
        if x.shape[-1] != INPUT_SIZE:
            h, w = x.shape[2], x.shape[3]
            crop = self.config.get('center_crop')
            if crop is not None:
                if crop > h or crop > w:
                    # AVOIDED REFERENCE QUIRK: center_crop_tensor's negative start index silently slices a wrong region there
                    raise ValueError('ArcFaceSkeleton: center_crop %d is larger than the %d x %d image' % (crop, h, w))
                top, left, ch, cw = (h - crop) // 2, (w - crop) // 2, crop, crop
            else:
                top, left, ch, cw = 0, 0, h, w
            x = _backend.call(_CropResize, x, top, left, ch, cw, INPUT_SIZE)
        elif x.shape[-2] != INPUT_SIZE:
            raise ValueError('ArcFaceSkeleton: a 112-wide input must be 112 x 112, got %s' % (tuple(x.shape),))
        levels = self.net.levels(x)
        return levels[:4] + [l2_norm(levels[4])]

    @staticmethod
    def normelize_to_model_input(batch):
        return batch


def embedding_loss_models(training_config, state_dicts, mini_batch_size=None, device='cuda'):
    """{'embedding_loss': LossModelClass} for a training config whose ``embedding_loss`` is enabled, else {}.  ``state_dicts`` maps the
    loss name to the Backbone checkpoint's state dict (nothing is read from ``model_path``)."""
    from .loss_model import LossModelClass
    cfg = training_config.get('embedding_loss')
    if not cfg or not cfg.get('enabled', False):
        return {}
    if 'embedding_loss' not in state_dicts:
        raise KeyError("embedding_loss_models: pass state_dicts={'embedding_loss': <model_ir_se50 state dict>}")
    net = ArcFaceSkeleton(cfg, state_dict=state_dicts['embedding_loss']).to(device)
    mb = mini_batch_size or training_config.get('mini_batch', 4)
    return {'embedding_loss': LossModelClass(cfg, 'embedding_loss', mini_batch_size=mb, skeleton_model=net)}
