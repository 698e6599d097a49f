"""The Inference / Controller API without a GPU: directory loading, the w-space composition in float64 against the oracle, splicing,
truncation, expression routing, directories written by the trainers, and the operator's module path (CPU tensors, emulated backend)."""
import pytest
import torch

import inference_checks as ic
from conftest import rel_err

from gan_control_amd import projection
from gan_control_amd.inference import Controller, Inference
from gan_control_amd.models.op import fc_stack as fcs
from gan_control_amd.models.op import _backend


@pytest.fixture
def no_launch(monkeypatch):
    """Any call of HipBackend._launch fails the test."""
    def boom(self, dev, entry, *a, **k):
        raise AssertionError('launched %s' % entry)
    monkeypatch.setattr(_backend.HipBackend, '_launch', boom)


@pytest.fixture
def f64_controller(tmp_path, emu_backend):
    ic.write_controller_dir(tmp_path)
    ctl = Controller(str(tmp_path), device='cpu')
    ctl.model.double()          # (the float32 values of the checkpoints, exactly)
    for net in ctl.fc_controls.values():
        if net is not None:
            net.double()
    ctl.reset_noise()
    return ctl


def _controls(batch, dtype=torch.float64, seed=3):
    gen = torch.Generator().manual_seed(seed)
    q = torch.zeros(batch, 8, dtype=dtype)
    q[torch.arange(batch), torch.arange(batch) % 8] = 1
    return {'orientation': torch.randn(batch, 3, generator=gen).to(dtype) * 30, 'age': torch.rand(batch, 1, generator=gen).to(dtype) * 60 + 10,
            'gamma': torch.randn(batch, 27, generator=gen).to(dtype), 'expression': q}


# ---- directory loading ---------------------------------------------------------------------------------------------------------------
def test_last_checkpoint_wins_and_g_ema_loads_strictly(tmp_path, emu_backend):
    cfg = ic.ffhq_config(32)
    last = ic.write_model_dir(str(tmp_path / 'm'), cfg, iters=(10, 200, 30))
    inf = Inference(str(tmp_path / 'm'), device='cpu')
    assert inf.ckpt_iter == '000200' and inf.config.model_config['size'] == 32 and inf.config.training_config['batch'] == 16
    want = last.state_dict()
    assert all(torch.equal(v, want[k]) for k, v in inf.model.state_dict().items())
    assert not inf.model.training and inf.batch_utils.sub_group_names[0] == 'id' and len(inf.noise) == 7
    # strict: a checkpoint with a missing key is refused
    sd = dict(want)
    sd.pop('style.age.1.bias')
    torch.save({'g_ema': sd}, tmp_path / 'm' / 'checkpoint' / '000300.pt')
    with pytest.raises(RuntimeError, match='style.age.1.bias'):
        Inference(str(tmp_path / 'm'), device='cpu')


def test_vanilla_has_no_batch_utils(tmp_path, emu_backend, no_launch):
    ic.write_model_dir(str(tmp_path), ic.ffhq_config(32, vanilla=True))
    inf = Inference(str(tmp_path), device='cpu')
    assert inf.batch_utils is None and isinstance(inf.model.style, torch.nn.Sequential)
    z = torch.randn(3, 512)
    assert torch.equal(inf.style(z), inf.model.style(z))
    with pytest.raises(ValueError, match='not in valid group names'):
        inf.check_valid_group('age')


def test_controller_directories(tmp_path, emu_backend):
    ic.write_controller_dir(tmp_path, names=('orientation', 'expression_q', 'age'))
    assert Controller.get_controller_dir(str(tmp_path), 'expression') is None          # expression_q_run is not the expression controller
    assert Controller.get_controller_dir(str(tmp_path), 'expression_q').endswith('expression_q_run')
    assert Controller.get_controller_dir(str(tmp_path), 'age').endswith('age_run')
    ctl = Controller(str(tmp_path), device='cpu')
    assert set(ctl.fc_controls) == set(ctl.batch_utils.sub_group_names) | {'expression_q'}
    assert ctl.fc_controls['hair'] is None and ctl.config_controls['hair'] is None and ctl.fc_controls['expression'] is None
    assert ctl.fc_controls['age'].in_dim == 1 and ctl.config_controls['age'].model_config['n_mlp'] == ic.CTL_N_MLP
    assert ctl.fc_controls['expression_q'].out_dim == 64 and not ctl.fc_controls['age'].training
    assert ctl.check_if_group_has_control('hair') is True
    with pytest.raises(ValueError, match='nose has no control'):
        ctl.check_if_group_has_control('nose')
    with pytest.raises(ValueError, match='hair'):
        ctl.gen_batch_by_controls(batch_size=2, hair=torch.zeros(2, 3))
    with pytest.raises(ValueError, match='expression'):
        ctl.gen_batch_by_controls(batch_size=2, expression=torch.zeros(2, 5))          # 5 columns: the (missing) expression controller
    with pytest.raises(ValueError, match='hair'):
        ctl.generate_group_w_latent('hair', torch.zeros(2, 3))


# ---- the w-space composition -----------------------------------------------------------------------------------------------------------
def test_gen_batch_by_controls_float64(f64_controller, no_launch):
    ctl, batch = f64_controller, 3
    z = torch.randn(batch, 512, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    controls = _controls(batch)
    img, latent, latent_w = ctl.gen_batch_by_controls(latent=z, normalize=False, **controls)
    assert torch.equal(latent, z) and latent.data_ptr() != z.data_ptr()
    want = ic.oracle_latent_w(ctl, z, controls)
    assert rel_err(latent_w, want) < 1e-12
    with torch.no_grad():
        ref, _ = ctl.model([latent_w], input_is_latent=True, noise=ctl.expend_noise(ctl.noise, batch))
    assert torch.equal(img, ref)          # the [1, 1, h, w] maps broadcast by StyledConv == the concatenated list, bit for bit
    # normalize=True: the CPU tensor in [0, 1]
    img01, _, _ = ctl.gen_batch_by_controls(latent=z, **controls)
    assert torch.equal(img01, ref.mul(0.5).add(0.5).clamp(min=0., max=1.)) and img01.device.type == 'cpu'
    # a given w: latent and latent_w are one tensor, the caller's is untouched
    w0 = want.clone()
    _, lat, lw = ctl.gen_batch_by_controls(latent=w0, input_is_latent=True, normalize=False, age=controls['age'])
    assert lat is lw and torch.equal(w0, want) and rel_err(lw[:, 320:384], ic.oracle_stack(ctl.fc_controls['age'], controls['age'])) < 1e-12
    assert torch.equal(lw[:, :320], want[:, :320]) and torch.equal(lw[:, 384:], want[:, 384:])
    # no controls: the plain w
    _, _, lw = ctl.gen_batch_by_controls(latent=z, normalize=False)
    assert torch.equal(lw, ctl.model.style(z))


def test_expression_with_8_columns_reaches_expression_q(f64_controller):
    ctl = f64_controller
    seen = []
    ctl.fc_controls['expression_q'].register_forward_hook(lambda m, i, o: seen.append('q'))
    ctl.fc_controls['expression'].register_forward_hook(lambda m, i, o: seen.append('e'))
    c = _controls(2)
    _, _, lw = ctl.gen_batch_by_controls(batch_size=2, normalize=False, expression=c['expression'])
    assert seen == ['q'] and rel_err(lw[:, 128:192], ic.oracle_stack(ctl.fc_controls['expression_q'], c['expression'])) < 1e-12
    _, _, lw = ctl.gen_batch_by_controls(batch_size=2, normalize=False, expression=torch.ones(2, 5, dtype=torch.float64))
    assert seen == ['q', 'e']


def test_insert_get_and_merge_group_latents(f64_controller):
    ctl = f64_controller
    for shape in ((4, 512), (4, 8, 512)):
        lat = torch.randn(*shape, dtype=torch.float64)
        keep = lat.clone()
        new = torch.randn(*shape[:-1], 64, dtype=torch.float64)
        out = ctl.insert_group_w_latent(lat, new, 'gamma')
        assert out is lat and torch.equal(ctl.get_group_w_latent(lat, 'gamma'), new)
        assert torch.equal(lat[..., :256], keep[..., :256]) and torch.equal(lat[..., 320:], keep[..., 320:])
        assert ctl.get_group_w_latent(lat, 'id').shape == shape[:-1] + (128,)
    with pytest.raises(ValueError, match='ndim'):
        ctl.insert_group_w_latent(torch.zeros(4, 8, 512), torch.zeros(4, 64), 'gamma')
    lat = torch.randn(2, 8, 512, dtype=torch.float64)
    keep = lat.clone()
    projection.merge_group_latents(ctl, 'age', lat)
    assert torch.equal(lat[:, :, 320:384], keep[:, :, 320:384].mean(dim=1, keepdim=True).expand(-1, 8, -1))
    assert torch.equal(lat[:, :, :320], keep[:, :, :320])
    mean, std = projection.get_avg_latent(ctl.model.float(), 16, 'cpu')
    assert mean.shape == (512,) and float(std) > 0


# ---- truncation ------------------------------------------------------------------------------------------------------------------------
def test_truncation_per_group(f64_controller, monkeypatch):
    ctl = f64_controller
    gen = torch.Generator().manual_seed(5)
    places = ctl.batch_utils.place_in_latent_dict
    z = torch.randn(3, 512, dtype=torch.float64, generator=gen)
    monkeypatch.setattr(ctl, 'calc_mean_w_latents', lambda *a, **k: pytest.fail('truncation=1 must not compute the means'))
    _, lat, latents = ctl.gen_batch(latent=z, normalize=False)
    w = ctl.model.style(z)
    assert lat is z or torch.equal(lat, z)
    assert latents.shape == (3, 8, 512) and torch.equal(latents[:, 0], w)
    mean = torch.randn(512, dtype=torch.float64, generator=gen)
    ctl.mean_w_latent, ctl.mean_w_latents = mean, {k: mean[lo:hi] for k, (lo, hi) in places.items()}
    z0 = z.clone()
    img, lat, latents = ctl.gen_batch(latent=z, normalize=False, truncation=0.6)
    assert torch.equal(z, z0)
    for k, (lo, hi) in places.items():
        assert torch.equal(lat[:, lo:hi], 0.6 * (w[:, lo:hi] - mean[lo:hi]) + mean[lo:hi]), k
    assert torch.equal(latents[:, 3], lat)
    # a given w latent: truncated on a clone
    w0 = w.clone()
    _, lat, _ = ctl.gen_batch(latent=w, input_is_latent=True, normalize=False, truncation=0.6)
    assert torch.equal(w, w0) and lat.data_ptr() != w.data_ptr() and torch.equal(lat, 0.6 * (w - mean) + mean)
    # group='random': the slice lo:hi is redrawn, nothing else, on a clone
    _, lat, _ = ctl.gen_batch(latent=w, input_is_latent=True, normalize=False, hair='random')
    assert torch.equal(w, w0) and torch.equal(lat[:, :384], w[:, :384]) and torch.equal(lat[:, 448:], w[:, 448:])
    assert not torch.equal(lat[:, 384:448], w[:, 384:448])
    with pytest.raises(ValueError, match='nose'):
        ctl.gen_batch(latent=w, input_is_latent=True, nose='random')


def test_calc_mean_w_latents(f64_controller):
    ctl = f64_controller
    ctl.model.float()
    torch.manual_seed(11)
    ctl.calc_mean_w_latents(2, 8)
    torch.manual_seed(11)
    want = torch.stack([ctl.model.style(torch.randn(8, 512)).mean(0) for _ in range(2)]).mean(0)
    assert torch.equal(ctl.mean_w_latent, want.detach())
    for k, (lo, hi) in ctl.batch_utils.place_in_latent_dict.items():
        assert torch.equal(ctl.mean_w_latents[k], want[lo:hi].detach())


# ---- directories the trainers write ----------------------------------------------------------------------------------------------------
def test_directories_written_by_the_trainers_load(tmp_path, emu_backend):
    from gan_control_amd.trainers.controller_trainer import ControllerTrainer, default_controller_config
    from gan_control_amd.trainers.utils import save_args
    cfg = ic.ffhq_config(32)
    gen = ic.write_model_dir(str(tmp_path / 'generator'), cfg)
    assert save_args(cfg, str(tmp_path / 'generator')) == str(tmp_path / 'generator' / 'args.json')
    ccfg = default_controller_config(in_dim=3, mid_dim=32, n_mlp=2)
    tr = ControllerTrainer(ccfg, cfg['training_config']['sub_groups_dict']['orientation']['place_in_latent'], device='cpu', seed=4)
    tr.controller_update((torch.randn(32, 3), torch.randn(32, 512)))
    save_args(ccfg, str(tmp_path / 'orientation_0'))
    assert tr.save_nets(7, str(tmp_path / 'orientation_0')) == str(tmp_path / 'orientation_0' / 'checkpoint' / '000007.pt')
    assert sorted(torch.load(tmp_path / 'orientation_0' / 'checkpoint' / '000007.pt')) == ['controller', 'fc_optim']
    ctl = Controller(str(tmp_path), device='cpu')
    got, want = ctl.fc_controls['orientation'].state_dict(), tr.fc_controller.state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want) and len(got) == len(want) == 4
    x = torch.randn(2, 3)
    with torch.no_grad():
        assert torch.equal(ctl.generate_group_w_latent('orientation', x), tr.fc_controller.eval()(x))
    assert all(torch.equal(v, gen.state_dict()[k]) for k, v in ctl.model.state_dict().items())


# ---- the operator's module path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('emulated', [False, True])
def test_operator_falls_back_to_the_modules(request, emulated, no_launch):
    """CPU tensors -- under the HIP backend object and under the emulated one -- take the module path: the same bits, nothing launched.
    (Under the HIP backend object EqualLinear itself refuses CPU tensors of any dtype -- the package has no CPU fallback -- so that leg
    shows that the modules WERE called: the call raises exactly what they raise, in float32 and in float64, and writes nothing.  The
    bit-for-bit comparison is the emulated leg's.)"""
    from gan_control_amd.models.controller_model import FcStack
    from gan_control_amd.models.gan_model import Generator
    if emulated:
        request.getfixturevalue('emu_backend')
    torch.manual_seed(0)
    stacks = [Generator.create_fc_stack(0.01, 3, w, mid_dim=32) for w in (16, 8, 24)]
    slices = [(0, 16), (16, 24), (24, 48)]
    ctl = FcStack(0.01, 2, 3, 32, 8)
    if not emulated:
        for dtype in (torch.float32, torch.float64):
            stacks = [s.to(dtype) for s in stacks]
            z, out = torch.randn(5, 48, dtype=dtype), torch.full((5, 48), 7.0, dtype=dtype)
            with pytest.raises(RuntimeError) as of_the_module:
                stacks[0](z[:, :16])
            with pytest.raises(RuntimeError) as of_the_operator:
                fcs.fc_stacks_forward(stacks, z, slices, out, slices)
            assert str(of_the_operator.value) == str(of_the_module.value) and 'no CPU fallback' in str(of_the_module.value)
            assert bool((out == 7).all())
        return
    z = torch.randn(5, 48)
    out = torch.full((5, 50), 7.0)
    got = fcs.fc_stacks_forward(stacks, z, slices, out, [(1, 17), (17, 25), (25, 49)])
    want = torch.cat([s(z[:, lo:hi]) for s, (lo, hi) in zip(stacks, slices)], dim=1)
    assert got is out and torch.equal(out[:, 1:49], want) and bool((out[:, 0] == 7).all()) and bool((out[:, 49] == 7).all())
    # one input tensor per stack, one shared output (the controllers' call); explicit pixel_norm flags
    w = want.clone()
    x = torch.randn(5, 3)
    fcs.fc_stacks_forward([ctl], [x], None, w, [(16, 24)])
    assert torch.equal(w[:, 16:24], ctl(x)) and torch.equal(w[:, :16], want[:, :16]) and torch.equal(w[:, 24:], want[:, 24:])
    o = torch.empty(5, 8)
    fcs.fc_stacks_forward([ctl], x, None, o, None, pixel_norm=[True])
    assert torch.equal(o, ctl(x * torch.rsqrt(x.pow(2).mean(dim=1, keepdim=True) + 1e-8)))
    with pytest.raises(ValueError, match='do not fit'):
        fcs.fc_stacks_forward([ctl], x, None, w, [(16, 25)])
    with pytest.raises(TypeError):
        fcs.fc_stacks_forward([torch.nn.Sequential(torch.nn.Linear(3, 3))], x, None, o, None)
    # gradients flow through the module path
    x.requires_grad_(True)
    o = torch.zeros(5, 8)
    fcs.fc_stacks_forward([ctl], x, None, o, None).sum().backward()
    assert x.grad is not None and ctl.fc_stack[0].weight.grad is not None


def test_rows_that_share_memory_take_the_module_path(emu_backend, no_launch):
    """An expanded tensor (row stride 0, shorter than its rows) is a legal input the kernel cannot address: the dispatch rule declines it,
    no stride is made up for it, and the module path gives what the modules give on the contiguous copy."""
    from gan_control_amd.models.controller_model import FcStack
    one = torch.randn(1, 3)
    wide = torch.randn(5, 8)
    assert not fcs._rows_apart(one.expand(5, 3)) and not fcs._rows_apart(torch.randn(3, 5).t()) and not fcs._rows_apart(wide[:, ::2])
    assert fcs._rows_apart(one) and fcs._rows_apart(one.expand(1, 3)) and fcs._rows_apart(wide) and fcs._rows_apart(wide[:, 2:5])
    assert fcs._rows_apart(torch.randn(5, 1)) and not fcs._rows_apart(torch.randn(1, 1).expand(5, 1))
    # the stride handed to the kernel is the tensor's own: rows of a slice are the parent's width apart, one row needs none
    assert fcs._row_stride(wide[:, 2:5], 3) == 8 and fcs._row_stride(wide, 8) == 8 and fcs._row_stride(one, 3) == 3
    # kernel_taken declines on the strides alone: a plan and a backend that would otherwise take the kernel for anything
    class Always:
        supported, max_bytes, device, params = True, 0, torch.device('cpu'), []
    class Hip:
        name = 'hip'
    class OnDevice:
        """What kernel_taken reads of a CUDA float32 tensor, with the geometry of a CPU one."""
        is_cuda, dtype, requires_grad = True, torch.float32, False

        def __init__(self, t):
            self.t, self.device, self.shape, self.stride = t, t.device, t.shape, t.stride

        def untyped_storage(self):
            return self.t.untyped_storage()
    prev = _backend._install_for_tests(Hip())
    try:
        out = OnDevice(torch.empty(5, 8))
        assert fcs.kernel_taken(Always, [OnDevice(torch.randn(5, 3))], [out], 5)
        assert fcs.kernel_taken(Always, [OnDevice(one.expand(1, 3))], [OnDevice(torch.empty(1, 8))], 1)
        assert not fcs.kernel_taken(Always, [OnDevice(one.expand(5, 3))], [out], 5)
        assert not fcs.kernel_taken(Always, [OnDevice(torch.randn(5, 3))], [OnDevice(torch.empty(1, 8).expand(5, 8))], 5)
        assert not fcs.kernel_taken(Always, [OnDevice(torch.randn(1, 64).expand(5, 64)[:, 8:11])], [out], 5)
    finally:
        _backend._install_for_tests(prev)
    torch.manual_seed(2)
    ctl = FcStack(0.01, 2, 3, 32, 8)
    with torch.no_grad():
        out = fcs.fc_stacks_forward([ctl], [one.expand(5, 3)], None, torch.zeros(5, 10), [(1, 9)])
        assert torch.equal(out[:, 1:9], ctl(one.expand(5, 3).contiguous())) and bool((out[:, [0, 9]] == 0).all())


def test_a_replaced_parameter_gets_a_new_plan():
    """The argument tables are cached per list of stacks; a layer whose Parameter object was replaced (assignment, load_state_dict with
    assign=True) or whose storage moved must not be served from the tables of the old weights."""
    from gan_control_amd.models.controller_model import FcStack
    ctl = FcStack(0.01, 2, 3, 32, 8)
    plan = fcs._plan_of([ctl], None)
    assert fcs._plan_of([ctl], None) is plan
    layer = ctl.fc_stack[1]
    old = layer.weight
    layer.weight = torch.nn.Parameter(torch.randn_like(old))
    new = fcs._plan_of([ctl], None)
    assert new is not plan and new.w[1] == layer.weight.data_ptr() != old.data_ptr()
    assert fcs._plan_of([ctl], None) is new
    ctl.load_state_dict({k: v.clone() for k, v in ctl.state_dict().items()}, assign=True)
    newer = fcs._plan_of([ctl], None)
    assert newer is not new and [newer.w[i] for i in range(2)] == [m.weight.data_ptr() for m in ctl.fc_stack]
    layer.bias.data = layer.bias.data.clone()          # the same Parameter object on new storage
    last = fcs._plan_of([ctl], None)
    assert last is not newer and last.bias[1] == layer.bias.data_ptr()


def test_make_resized_grid_image():
    """[0, 1] images -> the PIL grid (2 pixels of padding, as the reference's make_grid) and both resize forms.  The values go [0, 1] ->
    [-1, 1] -> uint8 by truncation (grid_image takes [-1, 1]); the detour moves a value by an ulp or two, so the test puts every value in
    the middle of its uint8 level, (k + 0.5) / 255, where the level is exact."""
    import numpy as np
    levels = torch.arange(5 * 3 * 8 * 8).reshape(5, 3, 8, 8) % 256
    grid = Inference.make_resized_grid_image((levels.float() + 0.5) / 255, nrow=4)
    assert grid.size == (4 * 10 + 2, 2 * 10 + 2) and grid.mode == 'RGB'
    pixels = np.asarray(grid)
    for i in range(5):
        top, left = 2 + 10 * (i // 4), 2 + 10 * (i % 4)
        assert np.array_equal(pixels[top:top + 8, left:left + 8], levels[i].permute(1, 2, 0).numpy().astype(np.uint8)), i
    assert not pixels[:2].any() and not pixels[12:, 12:].any()          # padding and the three empty cells
    assert Inference.make_resized_grid_image((levels.float() + 0.5) / 255, resize=11, nrow=4).size == (21, 11)          # int: the shorter side
    assert Inference.make_resized_grid_image((levels.float() + 0.5) / 255, resize=84, nrow=1).size == (84, int(84 * 52 / 12))
    assert Inference.make_resized_grid_image((levels.float() + 0.5) / 255, resize=(10, 30), nrow=4).size == (30, 10)          # (h, w)
