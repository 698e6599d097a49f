"""Controller training end to end without a GPU: the attribute frame, the device-resident frame, the trainer's loop with its evaluation, image
dumps and checkpoints, the directory inference.Controller loads, and the dispatch of the fused step on CPU tensors (emulated backend)."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

import inference_checks as ic
from conftest import rel_err

from gan_control_amd.datasets import DataFrameDataSet, DeviceFrame
from gan_control_amd.inference import Controller, Inference
from gan_control_amd.make_attributes_df import make_attributes_df
from gan_control_amd.models.op import _backend, fc_train
from gan_control_amd.trainers.controller_trainer import ControllerTrainer, default_controller_config


def _generator_config(size=32):
    cfg = ic.ffhq_config(size)
    cfg['training_config']['orientation_loss'] = {'same_group_name': 'orientation'}
    cfg['training_config']['age_loss'] = {'same_group_name': 'age'}
    cfg['training_config']['recon_3d_loss'] = {'gamma_loss': {'same_group_name': 'gamma'}}
    return cfg


def _frame(n=40, width=16):
    rng = np.random.default_rng(0)
    return pd.DataFrame({'latents_w': [rng.standard_normal(width).astype(np.float32) for _ in range(n)],
                         'age': rng.uniform(10, 80, n).astype(np.float32),
                         'orientation': [rng.standard_normal(3).astype(np.float32) for _ in range(n)],
                         'expression_q': rng.integers(0, 8, n)})


# ---- make_attributes_df -----------------------------------------------------------------------------------------------------------------
def test_make_attributes_df(tmp_path, emu_backend):
    ic.write_model_dir(str(tmp_path / 'g'), _generator_config())
    model = Inference(str(tmp_path / 'g'), device='cpu')
    predictors = {'age': lambda img: img.mean(dim=(1, 2, 3)) * 40 + 40,
                  'orientation': lambda img: img.mean(dim=(2, 3)) * 30}
    path = tmp_path / 'frames' / 'frame.pkl'
    frame = make_attributes_df(model, predictors, str(path), batch_size=4, number_of_samples=22, generator=torch.Generator().manual_seed(5))
    assert list(frame.columns) == ['latents', 'latents_w', 'age', 'orientation'] and len(frame) == 22 // 4 * 4
    assert frame.latents[0].shape == (512,) and frame.latents_w[3].shape == (512,) and frame.latents_w[3].dtype == np.float32
    assert frame.age.dtype == np.float32 and np.ndim(frame.age[2]) == 0 and frame.orientation[19].shape == (3,) and frame.orientation[19].dtype == np.float32
    # the w row is what the mapping network gives for the z row
    with torch.no_grad():
        w = model.model.style(torch.from_numpy(np.stack(frame.latents)))
    assert rel_err(torch.from_numpy(np.stack(frame.latents_w)), w) < 1e-5          # (fp32 GEMMs over 4 rows against 20 rows)
    # the pickle loads in both datasets
    ds, dev = DataFrameDataSet(str(path), 'orientation'), DeviceFrame(str(path), 'orientation', 'cpu')
    assert len(ds) == len(dev) == 18 and dev.controls.shape == (18, 3) and dev.latents_w.shape == (18, 512)
    a, lat = ds[7]
    assert torch.equal(a, dev[7][0]) and torch.equal(lat, dev[7][1])
    assert DeviceFrame(str(path), 'age', 'cpu', train=False).controls.shape == (2, 1)
    # the same seed: the same frame; no predictors and no path: latents alone
    again = make_attributes_df(model, predictors, None, batch_size=4, number_of_samples=22, generator=torch.Generator().manual_seed(5))
    for col in frame.columns:
        assert np.array_equal(np.stack(frame[col]), np.stack(again[col])), col
    other = make_attributes_df(model, predictors, None, batch_size=4, number_of_samples=8, generator=torch.Generator().manual_seed(6))
    assert not np.array_equal(np.stack(other.latents), np.stack(frame.latents)[:8])
    bare = make_attributes_df(model, {}, None, batch_size=3, number_of_samples=3)
    assert list(bare.columns) == ['latents', 'latents_w'] and len(bare) == 3
    with pytest.raises(ValueError, match='must return a tensor'):
        make_attributes_df(model, {'bad': lambda img: img.mean()}, None, batch_size=2, number_of_samples=2)


# ---- DeviceFrame ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('attribute', ['age', 'orientation', 'expression_q'])
@pytest.mark.parametrize('train', [True, False])
def test_device_frame_equals_dataframe_dataset(attribute, train):
    frame = _frame()
    ds, dev = DataFrameDataSet(frame, attribute, train=train), DeviceFrame(frame, attribute, 'cpu', train=train)
    assert len(ds) == len(dev) == (36 if train else 4)
    assert dev.controls.dtype == dev.latents_w.dtype == torch.float32 and dev.controls.is_contiguous() and dev.latents_w.is_contiguous()
    assert dev.controls.shape == (len(ds), {'age': 1, 'orientation': 3, 'expression_q': 8}[attribute]) and dev.latents_w.shape == (len(ds), 16)
    for i in range(len(ds)):
        a, w = ds[i]
        b, v = dev[i]
        assert a.shape == b.shape and torch.equal(a.float(), b) and torch.equal(w, v), (attribute, i)


def test_device_frame_epoch():
    frame = _frame(70)
    dev = DeviceFrame(frame, 'orientation', 'cpu')          # 63 rows
    batches = list(dev.epoch(8, shuffle=False))
    assert len(batches) == 7 and all(c.shape == (8, 3) and w.shape == (8, 16) for c, w in batches)
    assert torch.equal(torch.cat([c for c, _ in batches]), dev.controls[:56]) and torch.equal(torch.cat([w for _, w in batches]), dev.latents_w[:56])
    assert batches[1][0].data_ptr() == dev.controls[8:].data_ptr()          # views, not copies
    assert len(list(dev.epoch(8, shuffle=False, drop_last=False))) == 8
    # shuffled: 56 distinct rows of the frame, controls and latents still paired; the seed decides the order
    key = {tuple(w.tolist()): i for i, w in enumerate(dev.latents_w)}
    seen = []
    for c, w in dev.epoch(8, generator=torch.Generator().manual_seed(3)):
        for row_c, row_w in zip(c, w):
            i = key[tuple(row_w.tolist())]
            assert torch.equal(row_c, dev.controls[i])
            seen.append(i)
    assert len(seen) == 56 and len(set(seen)) == 56 and seen != sorted(seen)
    again = [key[tuple(r.tolist())] for _, w in dev.epoch(8, generator=torch.Generator().manual_seed(3)) for r in w]
    assert again == seen
    assert [key[tuple(r.tolist())] for _, w in dev.epoch(8, generator=torch.Generator().manual_seed(4)) for r in w] != seen


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
def _learnable_frame(n=64):
    """tests/test_controller.py::test_loader_feeds_the_step's relation, in the orientation slice [192, 256) of a 512-wide w."""
    frame = _frame(n, 512)
    mix = np.random.default_rng(1).standard_normal((3, 64)).astype(np.float32)
    rows = []
    for o, w in zip(frame.orientation, frame.latents_w):
        w = w.copy()
        w[192:256] = np.maximum(o @ mix, 0.0)
        rows.append(w)
    frame['latents_w'] = rows
    return frame


def _controller_config(batch=16):
    cfg = default_controller_config(3, 32, 3, batch=batch)
    cfg['model_config']['loss'] = 'orientation_loss'
    cfg['training_config'].update(lr=0.2, min_evaluate_interval=20, save_images_interval=40, save_nets_interval=30)
    return cfg


def test_default_config_keeps_its_fields_and_gains_the_intervals():
    tc = default_controller_config()['training_config']
    assert (tc['batch'], tc['reg_every'], tc['lr'], tc['rec_loss'], tc['losses'], tc['attribute_rec_w']) == (32, 4, 0.002, 'l1', ['latent_rec'], 1.0)
    assert (tc['min_evaluate_interval'], tc['save_images_interval'], tc['save_nets_interval'], tc['iter']) == (5000, 5000, 20000, 800000)


def test_from_generator_dir_picks_the_group_chunk(tmp_path, emu_backend):
    ic.write_model_dir(str(tmp_path / 'g'), _generator_config())
    for loss, group, chunk in (('orientation_loss', 'orientation', (192, 256)), ('age_loss', 'age', (320, 384)), ('gamma_loss', 'gamma', (256, 320))):
        cfg = _controller_config()
        cfg['model_config']['loss'] = loss
        tr = ControllerTrainer.from_generator_dir(cfg, str(tmp_path / 'g'), device='cpu')
        assert tr.working_group == group and tr.group_chunk == chunk == tuple(tr.batch_utils.place_in_latent_dict[group])
        assert tr.generator_dir == str(tmp_path / 'g') and tr.ckpt_iter == '000010' and tr.fc_controller.out_dim == 64
        assert not tr.generator.training and not any(p.requires_grad for p in tr.generator.parameters())


def test_train_writes_what_the_controller_api_loads(tmp_path, emu_backend):
    ic.write_model_dir(str(tmp_path / 'g'), _generator_config())
    tr = ControllerTrainer.from_generator_dir(_controller_config(), str(tmp_path / 'g'), device='cpu', seed=1)
    frame = _learnable_frame()
    save_dir = tmp_path / 'run' / 'orientation_test'
    log = tr.train(frame, 'orientation', str(save_dir), iters=81, log_interval=10, generator=torch.Generator().manual_seed(2))
    assert [i for i, _ in log] == list(range(0, 81, 10))
    assert np.mean([v for _, v in log[-3:]]) < 0.8 * np.mean([v for _, v in log[:3]]), log
    assert set(tr.evaluation_dict) >= {'eval_loss', 'eval_rec_loss', 'attribute_loss', 'loss'}
    assert tr.evaluation_dict['eval_loss'] == tr.evaluation_dict['eval_rec_loss'] > 0 and tr.evaluation_dict['attribute_loss'] == 0
    history = json.load(open(save_dir / 'graphs' / 'eval_loss.json'))
    assert [h['iter'] for h in history] == [0, 20, 40, 60, 80] and history[-1]['eval_loss'] == tr.eval_loss_list[-1] and len(tr.eval_loss_list) == 5
    assert history[-1]['eval_loss'] < history[0]['eval_loss']
    assert sorted(os.listdir(save_dir / 'images' / 'sample')) == ['000000.png', '000040.png', '000080.png']
    assert sorted(os.listdir(save_dir / 'checkpoint')) == ['000000.pt', '000030.pt', '000060.pt']
    from PIL import Image
    with Image.open(save_dir / 'images' / 'sample' / '000040.png') as im:
        assert im.size == (4 * 34 + 2, 8 * 34 + 2)          # 32 images of 32 x 32, four per row, make_grid's padding of 2
    # the evaluation is the mean loss over the eval rows
    ev = DeviceFrame(frame, 'orientation', 'cpu', train=False)
    with torch.no_grad():
        want = float((tr.fc_controller(ev.controls) - ev.latents_w[:, 192:256]).abs().mean())
    assert tr.evaluate(ev) == pytest.approx(want, rel=1e-6)
    # the layout inference.Controller expects: generator/ next to the group's directory
    tr.save_nets(81, str(save_dir))
    assert sorted(os.listdir(tmp_path / 'run')) == ['generator', 'orientation_test']
    assert sorted(os.listdir(tmp_path / 'run' / 'generator' / 'checkpoint')) == ['000010.pt']
    ctl = Controller(str(tmp_path / 'run'), device='cpu')
    assert ctl.fc_controls['orientation'] is not None and ctl.fc_controls['age'] is None
    assert ctl.config_controls['orientation'].training_config['save_nets_interval'] == 30
    controls = ev.controls[:3]
    images, _, latent_w = ctl.gen_batch_by_controls(batch_size=3, normalize=False, orientation=controls)
    with torch.no_grad():
        tr.fc_controller.eval()
        assert torch.equal(latent_w[:, 192:256], tr.fc_controller(controls))
    assert images.shape == (3, 3, 32, 32) and bool(torch.isfinite(images).all())


def test_controller_update_fused_on_cpu_is_controller_update(emu_backend, monkeypatch):
    def boom(self, dev, entry, *a, **k):
        raise AssertionError('launched %s' % entry)
    monkeypatch.setattr(_backend.HipBackend, '_launch', boom)
    frame = _learnable_frame()
    dev = DeviceFrame(frame, 'orientation', 'cpu')
    a = ControllerTrainer(_controller_config(), (192, 256), device='cpu', seed=4)
    b = ControllerTrainer(_controller_config(), (192, 256), device='cpu', seed=4)
    for batch in dev.epoch(16, shuffle=False):
        assert not fc_train.fused_step_taken(b.fc_controller, b.fc_optim, batch[0], batch[1], (192, 256), 'l1')
        want = a.controller_update(batch)
        got = b.controller_update_fused(batch)
        assert torch.is_tensor(got) and got.dim() == 0 and float(got) == want
    for p, q in zip(a.fc_controller.parameters(), b.fc_controller.parameters()):
        assert torch.equal(p, q)
    sa, sb = a.fc_optim.state_dict()['state'], b.fc_optim.state_dict()['state']
    assert all(torch.equal(sa[k][name], sb[k][name]) for k in sa for name in ('step', 'exp_avg', 'exp_avg_sq'))
    # fc_train.fused_step itself on CPU tensors: the module path, the same bits again
    c = ControllerTrainer(_controller_config(), (192, 256), device='cpu', seed=4)
    for batch in dev.epoch(16, shuffle=False):
        loss = fc_train.fused_step(c.fc_controller, c.fc_optim, batch[0], batch[1], (192, 256), 'l1')
    assert loss.dim() == 0 and not loss.requires_grad
    for p, q in zip(a.fc_controller.parameters(), c.fc_controller.parameters()):
        assert torch.equal(p, q)
