"""The fused controller step on the GPU (csrc/fc_train.hip through models/op/fc_train.py).

The forward is compared with gc_fc_stacks_fwd_f32 bit for bit; the loss kernel with its float64 formula; one step with a float64
``torch.optim.Adam`` step written here in plain torch, with the module path (``ControllerTrainer.controller_update`` in fp32 on the same
device from the same state) as the yardstick: per tensor, the fused step's error against float64 may be at most twice the module path's
(a different but fixed summation order).  Parameters are ~100 in size and a step moves them by ~2e-3, so the UPDATE (after - before) is
compared, not the parameter.  Every call runs on guard-banded, poisoned buffers (tests/guarded_alloc.py).  Measured pairs:
profiles/controller_training.md.
"""
import copy
import ctypes
import math

import numpy as np
import pandas as pd
import pytest
import torch
from torch import nn

import guarded_alloc
import inference_checks as ic
from conftest import load_golden, rel_err

from gan_control_amd import _lib
from gan_control_amd.models.gan_model import EqualLinear
from gan_control_amd.models.op import _backend
from gan_control_amd.models.op import fc_stack as fcs
from gan_control_amd.models.op import fc_train as fct
from gan_control_amd.trainers.controller_trainer import ControllerTrainer, default_controller_config

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = load_golden('controller')
GOLD_CHUNK = tuple(int(v) for v in GOLD['chunk'])

# name -> (batch, widths)
SHAPES = {
    'golden': (6, [3, 32, 32, 32, 24]),
    'odd': (5, [1, 100, 36]),                       # widths no multiple of 4 or of a slab of 8 columns, two layers
    'single': (1, [3, 16]),                         # one layer, batch 1
    'deep': (33, [27] + [256] * 7 + [40]),          # 8 layers, unaligned first weight, batch past a tile of 8
    'wide': (64, [3, 256, 512, 512]),               # k > 256, the widest rows, the largest batch
}
LATENT = 600          # width of the w rows the target slice is read from
LO = 37               # ... at an odd column offset


def make_stack(widths, seed):
    """EqualLinear draws randn / lr_mul itself (values ~100); the biases become non-zero."""
    torch.manual_seed(seed)
    layers = [EqualLinear(a, b, lr_mul=0.01, activation='fused_lrelu') for a, b in zip(widths[:-1], widths[1:])]
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in layers:
            m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 10)
    return nn.Sequential(*layers).to(DEV)


def make_data(name, seed=0):
    """(controls, latents_w): row slices of larger tensors, so that both are read in place at a row offset."""
    batch, widths = SHAPES[name]
    gen = torch.Generator().manual_seed(seed + batch)
    big_c = torch.randn(batch + 5, widths[0], generator=gen).to(DEV)
    big_w = torch.randn(batch + 5, LATENT, generator=gen).to(DEV)
    return big_c[2:2 + batch], big_w[3:3 + batch]


def chunk_of(name):
    return (LO, LO + SHAPES[name][1][-1])


def adam_for(stack, beta1=0.0, weight_decay=0.0):
    return torch.optim.Adam(stack.parameters(), lr=0.002 * 0.8, betas=(beta1, 0.99 ** 0.8), weight_decay=weight_decay)


def seed_state(opt, seed, step=3):
    """Non-trivial moments and a step count, as after a few steps: the same for every path that is compared."""
    gen = torch.Generator().manual_seed(seed)
    for p in opt.param_groups[0]['params']:
        opt.state[p] = {'step': torch.tensor(float(step)), 'exp_avg': (torch.randn(p.shape, generator=gen) * 1e-4).to(p.device),
                        'exp_avg_sq': (torch.rand(p.shape, generator=gen) * 1e-8).to(p.device)}


def snapshot(stack, opt):
    params = list(stack.parameters())
    return ([p.detach().clone() for p in params], [opt.state[p]['exp_avg'].clone() for p in params],
            [opt.state[p]['exp_avg_sq'].clone() for p in params])


def tables(layers):
    n = len(layers)
    vp = ctypes.c_void_p * n
    return (vp(*[m.weight.data_ptr() for m in layers]), vp(*[m.bias.data_ptr() for m in layers]),
            (ctypes.c_int32 * n)(*[m.weight.shape[0] for m in layers]), (ctypes.c_float * n)(*[m.scale for m in layers]),
            (ctypes.c_float * n)(*[m.lr_mul for m in layers]))


def launch(entry, *args):
    _backend.get()._launch(torch.device(DEV, torch.cuda.current_device()), entry, *args)


def f64_layers(stack, x):
    """Every layer's output by the documented formula in float64 on the upcast parameters (autograd-capable)."""
    h, outs = x, []
    for m in stack:
        t = m.scale * (h @ m.weight64.t()) + m.lr_mul * m.bias64
        h = torch.where(t > 0, t, 0.2 * t) * math.sqrt(2.0)
        outs.append(h)
    return outs


def f64_step(stack, opt, controls, latents_w, chunk, kind):
    """(loss, [exp_avg], [exp_avg_sq], [update]) of one torch.optim.Adam step (weight_decay 0, no amsgrad) in float64, from the state the
    optimiser holds now; nothing is modified."""
    group = opt.param_groups[0]
    for m in stack:
        m.weight64 = m.weight.detach().double().cpu().requires_grad_(True)
        m.bias64 = m.bias.detach().double().cpu().requires_grad_(True)
    pred = f64_layers(stack, controls.detach().double().cpu())[-1]
    d = pred - latents_w.detach().double().cpu()[:, chunk[0]:chunk[1]]
    loss = d.abs().mean() if kind == 'l1' else d.pow(2).mean()
    params64 = [t for m in stack for t in (m.weight64, m.bias64)]
    grads = torch.autograd.grad(loss, params64)
    beta1, beta2 = group['betas']
    ms, vs, ups = [], [], []
    for p, g in zip(stack.parameters(), grads):
        st = opt.state[p]
        t = float(st['step']) + 1
        m = beta1 * st['exp_avg'].double().cpu() + (1 - beta1) * g
        v = beta2 * st['exp_avg_sq'].double().cpu() + (1 - beta2) * g * g
        ups.append(-(group['lr'] / (1 - beta1 ** t)) * m / (v.sqrt() / math.sqrt(1 - beta2 ** t) + group['eps']))
        ms.append(m)
        vs.append(v)
    return float(loss.detach()), ms, vs, ups


def module_trainer(stack, opt, chunk, kind):
    """A ControllerTrainer whose network and optimiser are the given ones: its controller_update is the module path."""
    widths = [stack[0].weight.shape[1]] + [m.weight.shape[0] for m in stack]
    cfg = default_controller_config(widths[0], widths[1], 1, batch=1)
    cfg['training_config']['rec_loss'] = kind
    tr = ControllerTrainer(cfg, chunk, device=DEV, seed=0)
    tr.fc_controller, tr.fc_optim = stack, opt
    return tr


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SHAPES))
def test_forward_saves_every_layer_and_predicts_the_same_bits(name):
    batch, widths = SHAPES[name]
    stack = make_stack(widths, 3)
    x, _ = make_data(name)
    total = batch * sum(widths[1:])
    results = []
    for poison, fill, shift in (('nan', None, 0), ('big', 'nan', 4), ('nan', 'big', 0)):
        xin = x if fill is None else guarded_alloc.hostile(x, fill, shift)
        with torch.no_grad(), guarded_alloc.guarded(fct, poison=poison) as guard:
            acts = guard.empty(total, dtype=torch.float32, device=DEV)
            launch(fct.ENTRY_FWD, xin.data_ptr(), xin.stride(0) if batch > 1 else widths[0], widths[0], len(stack), *tables(stack), acts.data_ptr(),
                   batch, _lib.stream_of(acts))
            assert guard.check() == [] and guard.entries == [fct.ENTRY_FWD]
        results.append(acts)
    acts = results[0]
    assert bool(torch.isfinite(acts).all())          # every word of the workspace was written
    assert all(torch.equal(acts.view(torch.int32), r.view(torch.int32)) for r in results[1:])
    with torch.no_grad():
        want = fcs.fc_stacks_forward([stack], x, None, torch.empty(batch, widths[-1], device=DEV), None)
    pred = acts[total - batch * widths[-1]:].view(batch, widths[-1])
    assert torch.equal(pred, want)
    # every saved activation against the float64 formula, at the tolerance of tests/test_fc_stack_gpu.py: 4 x the module path's error
    for m in stack:
        m.weight64, m.bias64 = m.weight.detach().double().cpu(), m.bias.detach().double().cpu()
    ref = f64_layers(stack, x.double().cpu())
    at, h = 0, x
    with torch.no_grad():
        for l, m in enumerate(stack):
            h = m(h.contiguous())
            got = acts[at:at + batch * widths[l + 1]].view(batch, widths[l + 1])
            at += batch * widths[l + 1]
            e_k, e_m = rel_err(got, ref[l]), rel_err(h, ref[l])
            print('fc_train forward %-7s layer %d kernel %.3e  module path %.3e' % (name, l, e_k, e_m))
            assert e_k <= 4 * e_m, (l, e_k, e_m)


# ---- 2. loss and gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['l1', 'mse'])
@pytest.mark.parametrize('batch,n', [(6, 24), (1, 16), (5, 36), (64, 512)])
def test_loss_and_its_gradient(kind, batch, n):
    gen = torch.Generator().manual_seed(batch + n)
    pred = torch.randn(batch, n, generator=gen)
    wide = torch.randn(batch + 2, LATENT, generator=gen)
    pred[0, 0] = wide[1, LO]          # exact ties: sign(0) = 0
    pred[-1, -1] = wide[batch, LO + n - 1]
    pred, wide = pred.to(DEV), wide.to(DEV)
    target = wide[1:1 + batch]
    outs = []
    for poison, fill in (('nan', None), ('big', 'nan'), ('nan', 'big')):
        p, t = (pred, target) if fill is None else (guarded_alloc.hostile(pred, fill), guarded_alloc.hostile(target, fill, 4))
        with guarded_alloc.guarded(fct, poison=poison) as guard:
            dy = guard.empty(batch, n, dtype=torch.float32, device=DEV)
            loss = guard.empty((), dtype=torch.float32, device=DEV)
            launch(fct.ENTRY_LOSS, p.data_ptr(), t.data_ptr() + 4 * LO, LATENT, batch, n, fct.KINDS[kind], dy.data_ptr(), loss.data_ptr(),
                   _lib.stream_of(dy))
            assert guard.check() == []
        outs.append((dy, loss))
    dy, loss = outs[0]
    assert all(torch.equal(dy, d) and torch.equal(loss, s) for d, s in outs[1:])
    d64 = pred.double().cpu() - target.double().cpu()[:, LO:LO + n]
    count = batch * n
    if kind == 'l1':
        want_loss, want_dy = d64.abs().mean(), d64.sign() / count
        assert torch.equal(dy.cpu().sign().double(), d64.sign()) and float(dy[0, 0]) == 0.0 and float(dy[-1, -1]) == 0.0
    else:
        want_loss, want_dy = d64.pow(2).mean(), 2 * d64 / count
    assert rel_err(dy, want_dy) <= 1e-6
    with torch.no_grad():
        mod = (nn.functional.l1_loss if kind == 'l1' else nn.functional.mse_loss)(pred, target[:, LO:LO + n])
    e_k, e_m = abs(float(loss) - float(want_loss)) / float(want_loss), abs(float(mod) - float(want_loss)) / float(want_loss)
    print('fc_train loss %-3s [%d, %d] kernel %.3e  torch %.3e' % (kind, batch, n, e_k, e_m))
    # fp32 rounding of a mean: at most 32 + 6 + 16 additions on the path of any term, each half an ulp (6e-8): 1e-5, the relative bound the
    # forward tests use, holds with room
    assert e_k <= 1e-5


# ---- 3. one step against float64 Adam, the module path as the yardstick ----------------------------------------------------------------------
STEP_CASES = [(name, 'l1', 0.0) for name in SHAPES] + [('golden', 'mse', 0.0), ('odd', 'l1', 0.9), ('deep', 'mse', 0.9)]


@pytest.mark.parametrize('name,kind,beta1', STEP_CASES)
def test_one_step_against_float64_adam(name, kind, beta1):
    batch, widths = SHAPES[name]
    chunk = chunk_of(name)
    controls, latents_w = make_data(name)
    fused, module = make_stack(widths, 7), make_stack(widths, 7)
    opt_f, opt_m = adam_for(fused, beta1), adam_for(module, beta1)
    seed_state(opt_f, 11)
    seed_state(opt_m, 11)
    loss64, m64, v64, up64 = f64_step(fused, opt_f, controls, latents_w, chunk, kind)
    before = [p.detach().clone() for p in fused.parameters()]
    assert fct.fused_step_taken(fused, opt_f, controls, latents_w, chunk, kind)
    fct._plans.clear()
    with guarded_alloc.guarded(fct, poison='nan') as guard:
        loss_f = fct.fused_step(fused, opt_f, controls, latents_w, chunk, kind)
        assert guard.check() == [] and guard.entries == [fct.ENTRY_FWD, fct.ENTRY_LOSS, fct.ENTRY_BWD]
    fct._plans.clear()
    loss_m = module_trainer(module, opt_m, chunk, kind).controller_update((controls, latents_w))
    e_lf, e_lm = abs(float(loss_f) - loss64) / loss64, abs(loss_m - loss64) / loss64
    print('fc_train step %-7s %-3s beta1 %.1f loss: fused %.3e  module %.3e' % (name, kind, beta1, e_lf, e_lm))
    assert e_lf <= 1e-5          # the bound of test_loss_and_its_gradient; the fp32 forward in front of it adds ~1e-6 at most (profiles/inference.md)
    assert all(float(opt_f.state[p]['step']) == 4.0 for p in fused.parameters())
    names = [n for n, _ in fused.named_parameters()]
    worst = {}
    for i, (pf, pm) in enumerate(zip(fused.parameters(), module.parameters())):
        sf, sm = opt_f.state[pf], opt_m.state[pm]
        for what, got_f, got_m, want in (('exp_avg', sf['exp_avg'], sm['exp_avg'], m64[i]), ('exp_avg_sq', sf['exp_avg_sq'], sm['exp_avg_sq'], v64[i]),
                                         ('update', pf.detach() - before[i], pm.detach() - before[i], up64[i])):
            e_f, e_m = rel_err(got_f, want), rel_err(got_m, want)
            pair = worst.setdefault(what, [0.0, 0.0])
            pair[0], pair[1] = max(pair[0], e_f), max(pair[1], e_m)
            assert e_f <= 2 * e_m, (names[i], what, e_f, e_m)
    for what, (e_f, e_m) in worst.items():
        print('fc_train step %-7s %-3s beta1 %.1f %-10s: fused %.3e  module %.3e (largest over the tensors)' % (name, kind, beta1, what, e_f, e_m))


# ---- 4. three steps on the golden vectors, and a checkpoint that continues under torch.optim.Adam ---------------------------------------------
def golden_trainer():
    hyper = GOLD['hyper']
    cfg = default_controller_config(int(hyper[2]), int(hyper[3]), int(hyper[1]), batch=6)
    tr = ControllerTrainer(cfg, GOLD_CHUNK, device=DEV, seed=0)
    tr.fc_controller.load_state_dict({k.split('/', 1)[1]: torch.from_numpy(v).float() for k, v in GOLD.items() if k.startswith('init/')})
    return tr


def test_three_steps_match_the_golden_vectors_and_the_state_continues_under_torch_adam():
    tr = golden_trainer()
    batch = (torch.from_numpy(GOLD['controls']).float().to(DEV), torch.from_numpy(GOLD['w_latent']).float().to(DEV))
    assert fct.fused_step_taken(tr.fc_controller, tr.fc_optim, batch[0], batch[1], GOLD_CHUNK, tr.rec_loss)
    losses = [tr.controller_update_fused(batch) for _ in range(3)]
    assert all(torch.is_tensor(v) and v.dim() == 0 and v.is_cuda for v in losses)
    assert np.allclose([float(v) for v in losses], GOLD['losses'], rtol=1e-3)
    for k, v in tr.fc_controller.state_dict().items():
        assert rel_err(v, torch.from_numpy(GOLD['after3/' + k])) < 1e-3, k
    # the fourth step: torch.optim.Adam on a copy, from the fused optimiser's state_dict, against the fused step
    other = golden_trainer()
    other.fc_controller.load_state_dict(tr.fc_controller.state_dict())
    other.fc_optim.load_state_dict(copy.deepcopy(tr.fc_optim.state_dict()))
    loss_t = other.controller_update(batch)
    loss_f = float(tr.controller_update_fused(batch))
    assert abs(loss_t - loss_f) <= 1e-3 * abs(loss_f)
    for (k, a), b in zip(tr.fc_controller.state_dict().items(), other.fc_controller.state_dict().values()):
        assert rel_err(a, b) < 1e-3, k
    sa, sb = tr.fc_optim.state_dict()['state'], other.fc_optim.state_dict()['state']
    for key in sa:
        assert float(sa[key]['step']) == float(sb[key]['step']) == 4.0
        assert rel_err(sa[key]['exp_avg'], sb[key]['exp_avg']) < 1e-3 and rel_err(sa[key]['exp_avg_sq'], sb[key]['exp_avg_sq']) < 1e-3
    # ... and the other way round: the fused step continues from a state torch.optim.Adam wrote
    third = golden_trainer()
    third.controller_update(batch)
    assert fct.fused_step_taken(third.fc_controller, third.fc_optim, batch[0], batch[1], GOLD_CHUNK, third.rec_loss)
    loss2 = [float(third.controller_update_fused(batch)) for _ in range(2)]
    assert np.allclose(loss2, GOLD['losses'][1:], rtol=1e-3)
    for k, v in third.fc_controller.state_dict().items():
        assert rel_err(v, torch.from_numpy(GOLD['after3/' + k])) < 1e-3, k


# ---- 5. buffers and repeatability -------------------------------------------------------------------------------------------------------------
def words_outside(placed, backing_of):
    """How many words outside the logical elements of a placed (dense) tensor no longer hold the fill."""
    rec = backing_of
    first, count = rec.first // 4, placed.numel()
    return int((rec.backing[:first] != rec.word).sum()) + int((rec.backing[first + count:] != rec.word).sum())


@pytest.mark.parametrize('name', list(SHAPES))
def test_same_bits_guarded_buffers_and_hostile_inputs(name):
    batch, widths = SHAPES[name]
    chunk = chunk_of(name)
    controls, latents_w = make_data(name)
    results = []
    for poison, fill, shift in (('nan', None, 0), ('nan', None, 0), ('big', 'nan', 4), ('nan', 'big', 0)):
        stack = make_stack(widths, 9)
        opt = adam_for(stack)
        seed_state(opt, 13)
        # the regions the kernels write in place: W, bias, exp_avg, exp_avg_sq of every layer, each between canaries
        records = []
        for p in stack.parameters():
            state = opt.state[p]
            for holder, key in ((p, 'data'), (state, 'exp_avg'), (state, 'exp_avg_sq')):
                t = getattr(holder, key) if holder is p else holder[key]
                h = guarded_alloc.hostile(t, fill or 'nan')
                assert h.is_contiguous()
                records.append((h, h._hostile))
                if holder is p:
                    p.data = h
                else:
                    holder[key] = h
        c, w = (controls, latents_w) if fill is None else (guarded_alloc.hostile(controls, fill, shift), guarded_alloc.hostile(latents_w, fill, shift))
        fct._plans.clear()          # the workspaces of this run come from the guard
        with guarded_alloc.guarded(fct, poison=poison) as guard:
            loss = fct.fused_step(stack, opt, c, w, chunk, 'l1')
            assert guard.check() == [] and guard.entries == [fct.ENTRY_FWD, fct.ENTRY_LOSS, fct.ENTRY_BWD]
            assert [a.shape for a in guard.allocations] == [(batch * sum(widths[1:]),)] * 2 + [()]          # acts, grads, the loss
        plan = fct._plan_of(stack, opt)
        acts, grads = plan.work[batch]
        assert bool(torch.isfinite(acts).all()) and bool(torch.isfinite(grads).all())          # every word of both workspaces was written
        # no store outside the elements of any parameter or moment (slabs of 8 columns past k, chunks of 128 rows past n, the bias tail)
        for (h, rec), (pname, _) in zip(records, [(n, k) for n, _ in stack.named_parameters() for k in range(3)]):
            assert words_outside(h, rec) == 0, (pname, tuple(h.shape))
        assert all(p.data_ptr() == records[3 * i][0].data_ptr() for i, p in enumerate(stack.parameters()))          # updated where they were placed
        if fill is not None:
            assert guarded_alloc.hostile_changes(c, controls) is None and guarded_alloc.hostile_changes(w, latents_w) is None
        results.append([loss] + [t.detach().clone() for t in sum(snapshot(stack, opt), [])])
        fct._plans.clear()
    for other in results[1:]:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(results[0], other))
    # the step moved every tensor: the comparison above is not one of untouched buffers
    fresh = make_stack(widths, 9)
    assert all(not torch.equal(a, b) for a, b in zip(results[0][1:1 + 2 * (len(widths) - 1)], [p.detach() for p in fresh.parameters()]))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def _raw(widths, batch, x, ws, buf, null=False):
    """The forward and the backward entry with tables that point at the same buffers: the refusals come before any launch."""
    n = len(widths) - 1
    vp, i32, f32 = ctypes.c_void_p * n, ctypes.c_int32 * n, ctypes.c_float * n
    w = None if null else vp(*[buf.data_ptr()] * n)
    shared = (vp(*[buf.data_ptr()] * n), i32(*widths[1:]), f32(*[1.0] * n), f32(*[1.0] * n))
    stream = _lib.stream_of(x)
    yield lambda: launch(fct.ENTRY_FWD, x.data_ptr(), 1024, widths[0], n, w, *shared, ws.data_ptr(), batch, stream)
    yield lambda: launch(fct.ENTRY_BWD, x.data_ptr(), 1024, widths[0], n, w, *shared, *[vp(*[buf.data_ptr()] * n) for _ in range(4)], ws.data_ptr(),
                         ws.data_ptr(), batch, 1e-3, 0.0, 0.99, 1e-8, 1.0, 0.1, stream)


def test_unsupported_arguments_are_refused_before_any_launch():
    x = torch.full((4, 1024), 2.0, device=DEV)
    ws = torch.full((70 * 8 * 520,), 3.0, device=DEV)
    buf = torch.full((520 * 520,), 5.0, device=DEV)
    for widths, batch, word in (([16, 16], 0, 'batch 0'), ([16, 16], 65, 'batch 65'), ([513, 16], 4, 'input width 513'), ([16, 513], 4, 'output width 513'),
                                ([16] * 10, 4, '9 layers')):
        for call in _raw(widths, batch, x, ws, buf):
            with pytest.raises(_lib.UnsupportedError, match=word):
                call()
    for call in _raw([16, 16], 4, x, ws, buf, null=True):
        with pytest.raises(RuntimeError, match=r'code -1.*null table'):
            call()
    for batch, n, word in ((0, 16, 'batch 0'), (65, 16, 'batch 65'), (4, 513, 'width 513')):
        with pytest.raises(_lib.UnsupportedError, match=word):
            launch(fct.ENTRY_LOSS, buf.data_ptr(), x.data_ptr(), 1024, batch, n, 0, ws.data_ptr(), ws.data_ptr(), _lib.stream_of(x))
    with pytest.raises(RuntimeError, match='code -1'):
        launch(fct.ENTRY_LOSS, None, x.data_ptr(), 1024, 4, 16, 0, ws.data_ptr(), ws.data_ptr(), _lib.stream_of(x))
    torch.cuda.synchronize()
    assert bool((ws == 3.0).all()) and bool((buf == 5.0).all()) and bool((x == 2.0).all())


def test_dispatch_rule_and_the_module_path():
    batch, widths = SHAPES['golden']
    chunk = chunk_of('golden')
    controls, latents_w = make_data('golden')
    entries = (fct.ENTRY_FWD, fct.ENTRY_LOSS, fct.ENTRY_BWD)
    seen = []
    real = _backend.HipBackend._launch

    def counting(self, dev, entry, *a, **k):
        seen.append(entry)
        return real(self, dev, entry, *a, **k)

    _backend.HipBackend._launch = counting
    try:
        plain = make_stack(widths, 5)
        assert fct.fused_step_taken(plain, adam_for(plain), controls, latents_w, chunk, 'l1')
        assert fct.fused_step_taken(plain, adam_for(plain), controls, latents_w, chunk, nn.MSELoss())
        no_act = make_stack(widths, 5)
        no_act[1].activation = None
        cpu = make_stack(widths, 5).cpu()
        for stack, opt, c, w, why in ((plain, adam_for(plain, weight_decay=0.01), controls, latents_w, 'weight_decay'),
                                      (no_act, adam_for(no_act), controls, latents_w, 'a layer without activation'),
                                      (cpu, adam_for(cpu), controls.cpu(), latents_w.cpu(), 'CPU tensors'),
                                      (plain, adam_for(plain), controls.double(), latents_w, 'float64 controls'),
                                      (plain, adam_for(plain), controls[:1].expand(batch, 3), latents_w, 'rows that share memory')):
            assert not fct.fused_step_taken(stack, opt, c, w, chunk, 'l1'), why
            if why in ('weight_decay', 'a layer without activation'):
                before = [p.detach().clone() for p in stack.parameters()]
                del seen[:]
                loss = fct.fused_step(stack, opt, c, w, chunk, 'l1')
                assert not any(e in entries for e in seen) and loss.dim() == 0 and loss.is_cuda, why
                assert all(not torch.equal(a, b) for a, b in zip(before, stack.parameters())), why
        # options changed AFTER a plan was made are seen by the next call; a query creates no optimiser state
        later = make_stack(widths, 5)
        opt = adam_for(later)
        assert fct.fused_step_taken(later, opt, controls, latents_w, chunk, 'l1') and len(opt.state) == 0
        del seen[:]
        fct.fused_step(later, opt, controls, latents_w, chunk, 'l1')
        assert seen == list(entries) and len(opt.state) == 2 * (len(widths) - 1)
        for change, undo in ((lambda: opt.param_groups[0].update(weight_decay=0.01), lambda: opt.param_groups[0].update(weight_decay=0)),
                             (lambda: opt.param_groups[0].update(amsgrad=True), lambda: opt.param_groups[0].update(amsgrad=False)),
                             (lambda: later[0].bias.requires_grad_(False), lambda: later[0].bias.requires_grad_(True))):
            change()
            assert not fct.fused_step_taken(later, opt, controls, latents_w, chunk, 'l1')
            undo()
            assert fct.fused_step_taken(later, opt, controls, latents_w, chunk, 'l1')
        assert not fct.fused_step_taken(plain, torch.optim.SGD(plain.parameters(), lr=0.1), controls, latents_w, chunk, 'l1')
        assert not fct.fused_step_taken(plain, adam_for(plain), controls, latents_w, chunk, nn.SmoothL1Loss())
        assert not fct.fused_step_taken(plain, adam_for(plain), torch.cat([controls] * 11)[:65], torch.cat([latents_w] * 11)[:65], chunk, 'l1')
        # the trainer: attribute_rec in the losses is controller_update
        tr = module_trainer(plain, adam_for(plain), chunk, 'l1')
        tr.training_config['losses'] = ['latent_rec', 'attribute_rec']
        tr.calc_attribute_rec_controller_loss = lambda org, pred, ctl: pred.square().mean()
        del seen[:]
        loss = tr.controller_update_fused((controls, latents_w))
        assert not any(e in entries for e in seen) and loss.dim() == 0 and 'attribute_loss' in tr.evaluation_dict
        tr.training_config['losses'] = ['latent_rec']
        del seen[:]
        tr.controller_update_fused((controls, latents_w))
        assert seen == list(entries)
    finally:
        _backend.HipBackend._launch = real


# ---- 7. the trainer's loop on the device ------------------------------------------------------------------------------------------------------
def test_train_on_the_device_takes_n_layers_plus_two_launches_per_step(tmp_path):
    rng = np.random.default_rng(0)
    rows = 40
    orientation = [rng.standard_normal(3).astype(np.float32) for _ in range(rows)]
    mix = rng.standard_normal((3, 24)).astype(np.float32)
    latents = []
    for o in orientation:
        w = rng.standard_normal(96).astype(np.float32)
        w[GOLD_CHUNK[0]:GOLD_CHUNK[1]] = np.maximum(o @ mix, 0.0)
        latents.append(w)
    frame = pd.DataFrame({'latents_w': latents, 'orientation': orientation})
    tr = golden_trainer()
    tr.training_config.update(lr=0.2)
    tr.fc_optim.param_groups[0]['lr'] = 0.2 * 0.8
    n_layers = len(tr.fc_controller.fc_stack)
    launches = _lib.load().gc_fc_train_launches          # kernel launches the three entries issued so far, counted where they are issued
    before = launches()
    with guarded_alloc.guarded(fct, poison='nan') as guard:
        log = tr.train(frame, 'orientation', str(tmp_path / 'run' / 'orientation_gpu'), iters=20, log_interval=10,
                       generator=torch.Generator().manual_seed(1))
        assert guard.check() == []
    steps = [e for e in guard.entries if e in (fct.ENTRY_FWD, fct.ENTRY_LOSS, fct.ENTRY_BWD)]
    assert steps == [fct.ENTRY_FWD, fct.ENTRY_LOSS, fct.ENTRY_BWD] * 20
    assert launches() - before == 20 * (n_layers + 2)
    assert set(guard.entries) - set(steps) <= {fcs.ENTRY}          # evaluate at step 0: the inference kernel; nothing of the module path
    assert [i for i, _ in log] == [0, 10] and log[1][1] < log[0][1], log
    assert set(tr.evaluation_dict) >= {'eval_loss', 'eval_rec_loss', 'attribute_loss', 'loss'}
