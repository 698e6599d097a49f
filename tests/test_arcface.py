"""The ArcFace identity predictor (losses/arc_face.py) on the host: the plain-PyTorch restatement and the product (over an emulation of
the new C-ABI primitives written with ATen formulas) against tests/golden/arcface.npz, the reference's own IR-SE50 on procedural weights;
key set, refusals and the frozen-parameter contract."""
import pytest
import torch
import torch.nn.functional as F

import arcface_checks as ac
from conftest import EmulatedBackend, rel_err

GOLD = ac.load_fixture()


class ArcFaceEmulatedBackend(EmulatedBackend):
    """EmulatedBackend plus the predictor's primitives (include/gancontrol_hip.h: gc_crop_resize_ac_f32 ... gc_se_apply_f32)."""

    def crop_resize_ac(self, x, top, left, crop_h, crop_w, out_h, out_w, adjoint=False, in_hw=None):
        def fwd(img):
            return F.interpolate(img[:, :, top:top + crop_h, left:left + crop_w], size=(out_h, out_w), mode='bilinear', align_corners=True)
        if not adjoint:
            return fwd(x)
        probe = torch.zeros(x.shape[0], x.shape[1], *in_hw, dtype=x.dtype, requires_grad=True)
        with torch.enable_grad():
            g, = torch.autograd.grad(fwd(probe), probe, x.detach())
        return g

    @staticmethod
    def _c(t, x):
        return t.reshape([1, -1] + [1] * (x.ndim - 2))

    def affine_prelu(self, x, scale, shift, alpha):
        v = x if scale is None else x * self._c(scale, x)
        v = v if shift is None else v + self._c(shift, x)
        return v if alpha is None else torch.where(v > 0, v, v * self._c(alpha, x))

    def affine_prelu_bwd(self, g, x, scale, shift, alpha, g2=None, g2_strided=False):
        gx = g if scale is None else g * self._c(scale, g)
        if alpha is not None:
            pre = self.affine_prelu(x, scale, shift, None)
            gx = torch.where(pre > 0, gx, gx * self._c(alpha, g))
        if g2 is not None:
            gx = gx.clone()
            if g2_strided:
                gx[:, :, ::2, ::2] += g2
            else:
                gx = gx + g2
        return gx

    def plane_reduce(self, a, b=None, mul=1.0):
        return (a if b is None else a * b).flatten(2).sum(2) * mul

    def se_mlp(self, m, fc1, fc2):
        z = F.relu(m @ fc1.t())
        return z, torch.sigmoid(z @ fc2.t())

    def se_mlp_bwd(self, t, s, z, fc1, fc2, mul):
        gz = ((t * s * (1 - s)) @ fc2) * (z > 0)
        return (gz @ fc1) * mul

    def se_apply(self, r, s, shortcut=None, stride=1):
        out = r * s[:, :, None, None]
        return out if shortcut is None else out + shortcut[:, :, ::stride, ::stride]


@pytest.fixture
def arc_backend():
    from gan_control_amd.models.op import _backend
    prev = _backend._install_for_tests(ArcFaceEmulatedBackend())
    yield
    _backend._install_for_tests(prev)


@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_restatement_matches_fixture(name):
    sd = ac.fixture_state_dict(GOLD)
    x = ac.case_input(name).requires_grad_(True)
    feats = ac.restated(sd, x, ac.CASES[name][2])
    for i, f in enumerate(feats[:4]):
        mean, sample = ac.level_summary(f.detach())
        assert rel_err(mean, torch.from_numpy(GOLD['%s/level%d_mean' % (name, i)])) < 1e-4
        assert rel_err(sample, torch.from_numpy(GOLD['%s/level%d_sample' % (name, i)])) < 1e-4
    assert rel_err(feats[4], torch.from_numpy(GOLD[name + '/embedding'])) < 1e-4
    g, = torch.autograd.grad(ac.probe_scalar(feats, ac.probes(name)), x)
    sums, norm, sample = ac.grad_summary(g)
    assert not ac.over_tolerance({'grad_sums': rel_err(sums, torch.from_numpy(GOLD[name + '/grad_sums'])),
                                  'grad_norm': rel_err(norm, torch.from_numpy(GOLD[name + '/grad_norm'])),
                                  'grad_sample': rel_err(sample, torch.from_numpy(GOLD[name + '/grad_sample']))})


def test_fixture_weights_keep_activations_order_one():
    for name in ac.CASES:
        rms = GOLD[name + '/rms']
        assert (rms > 0.1).all() and (rms < 10).all(), (name, rms)


@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_product_matches_fixture_emulated(arc_backend, name):
    """Outputs and input gradient (fp32 host arithmetic against the float64 reference run)."""
    err, _ = ac.run_product(GOLD, name, 'cpu', hinge=(ac.CASES[name][0] == 4))
    bad = ac.over_tolerance(err)
    assert not bad, bad


def test_state_dict_keys_and_shapes_match_the_reference():
    from gan_control_amd.losses import Backbone
    net = Backbone(50, 0.6, mode='ir_se')
    sd = net.state_dict()
    keys = [str(k) for k in GOLD['keys']]
    assert sorted(sd) == keys and len(keys) == 397
    for k, row in zip(keys, GOLD['key_shapes']):
        assert tuple(sd[k].shape) == tuple(int(s) for s in row if s > 0), k
    assert sum(v.numel() for k, v in sd.items() if not k.endswith('num_batches_tracked')) == int(GOLD['n_values'][0])
    assert sum(v.numel() for v in sd.values()) == 43824118           # with the 54 BatchNorm counters


def test_load_round_trip(tmp_path):
    from gan_control_amd.losses import ArcFaceSkeleton
    sd = ac.fixture_state_dict(GOLD)
    path = tmp_path / 'model_ir_se50.pth'
    torch.save(sd, path)
    skel = ArcFaceSkeleton(dict(ac.FFHQ_EMBEDDING, model_path=str(path)))
    back = skel.net.state_dict()
    assert sorted(back) == sorted(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        ArcFaceSkeleton(ac.FFHQ_EMBEDDING, state_dict={k: v for k, v in sd.items() if 'body.23' not in k})


@pytest.mark.parametrize('layers,mode', [(100, 'ir'), (152, 'ir_se')])
def test_other_depths_build(layers, mode):
    from gan_control_amd.losses import Backbone
    net = Backbone(layers, 0.4, mode=mode)
    assert len(net.body) == {100: 49, 152: 50}[layers]
    assert any('res_layer.5.fc1' in k for k in net.state_dict()) == (mode == 'ir_se')


def test_refusals(arc_backend):
    from gan_control_amd.losses import ArcFaceSkeleton, Backbone
    skel = ArcFaceSkeleton(ac.FFHQ_EMBEDDING, state_dict=ac.fixture_state_dict(GOLD))
    with pytest.raises(NotImplementedError):
        skel.train()
    with pytest.raises(NotImplementedError):
        skel.net.train()
    skel.eval()
    with pytest.raises(ValueError, match='larger'):
        skel(torch.zeros(1, 3, 256, 256))                   # center_crop 480 > 256
    with pytest.raises(ValueError, match='3, H, W'):
        skel(torch.zeros(1, 1, 112, 112))
    with pytest.raises(ValueError):
        Backbone(34, 0.0, 'ir_se')
    with pytest.raises(ValueError):
        Backbone(50, 0.0, 'se')


def test_112_input_bypasses_crop_and_resize(arc_backend, monkeypatch):
    from gan_control_amd.losses import ArcFaceSkeleton
    from gan_control_amd.losses import arc_face
    skel = ArcFaceSkeleton(ac.FFHQ_EMBEDDING, state_dict=ac.fixture_state_dict(GOLD))

    def boom(*a, **k):
        raise AssertionError('crop / resize called on a 112 x 112 input')
    monkeypatch.setattr(arc_face._CropResize, 'forward', boom)
    x = torch.rand(1, 3, 112, 112, generator=torch.Generator().manual_seed(3)) * 2 - 1
    feats = skel(x)
    ref = ac.restated(ac.fixture_state_dict(GOLD), x, 480)
    assert all(rel_err(a, b) < 1e-4 for a, b in zip(feats, ref))
    assert rel_err(skel.net(x), ref[4]) < 1e-4


def test_parameters_never_get_grad(arc_backend, monkeypatch):
    from gan_control_amd.losses import ArcFaceSkeleton
    from gan_control_amd.models.op import _backend

    def no_wgrad(*a, **k):
        raise AssertionError('weight-gradient kernel called')
    monkeypatch.setattr(_backend.get(), 'conv2d_wgrad', no_wgrad)
    skel = ArcFaceSkeleton(dict(ac.FFHQ_EMBEDDING, center_crop=60), state_dict=ac.fixture_state_dict(GOLD))
    assert not any(p.requires_grad for p in skel.parameters())
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)) * 2 - 1).requires_grad_(True)
    sum(f.sum() for f in skel(x)).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert all(p.grad is None for p in skel.parameters())


def test_loss_model_still_needs_a_predictor():
    from gan_control_amd.losses import LossModelClass, embedding_loss_models
    with pytest.raises(RuntimeError, match='predictor'):
        LossModelClass(ac.FFHQ_EMBEDDING, 'embedding_loss')
    assert embedding_loss_models({'embedding_loss': dict(ac.FFHQ_EMBEDDING, enabled=False)}, {}) == {}
    with pytest.raises(KeyError):
        embedding_loss_models({'embedding_loss': ac.FFHQ_EMBEDDING}, {})


def test_embedding_loss_models_helper(arc_backend):
    from gan_control_amd.losses import ArcFaceSkeleton, LossModelClass, embedding_loss_models
    models = embedding_loss_models({'embedding_loss': dict(ac.FFHQ_EMBEDDING, center_crop=60), 'mini_batch': 4},
                                   {'embedding_loss': ac.fixture_state_dict(GOLD)}, device='cpu')
    lm = models['embedding_loss']
    assert isinstance(lm, LossModelClass) and isinstance(lm.skeleton_model, ArcFaceSkeleton)
    feats = lm.calc_features(ac.case_input('c64').repeat(2, 1, 1, 1))
    assert [tuple(f.shape) for f in feats] == [(4, 64, 56, 56), (4, 128, 28, 28), (4, 256, 14, 14), (4, 512, 7, 7), (4, 512)]
