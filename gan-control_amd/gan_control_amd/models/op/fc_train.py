"""One optimisation step of a controller in n_layers + 2 launches: the training side of models/op/fc_stack.py (csrc/fc_train.hip).

``fused_step`` is what ``ControllerTrainer.controller_update`` computes for the ``latent_rec`` objective -- the forward of an ``FcStack``, L1 or
MSE against the group's slice of the w latents, the backward pass and ``torch.optim.Adam`` -- as

    gc_fc_stack_fwd_save_f32   the forward of gc_fc_stacks_fwd_f32 (the same bits) that keeps every layer's output           1 launch
    gc_rec_loss_grad_f32       the mean loss into one device float and its gradient; the target is read in place            1 launch
    gc_fc_stack_bwd_adam_f32   per layer, last to first: db, dW, dX and Adam's update of the layer's parameters            n_layers launches

on CUDA float32 tensors under the HIP backend.  The kernels update the parameters and the very tensors ``optimizer.state[p]['exp_avg']`` /
``['exp_avg_sq']`` hold (created as ``torch.optim.Adam`` creates them where they are missing); the host advances ``state[p]['step']`` and computes
the two bias corrections in float64.  A ``state_dict()`` written after fused steps therefore loads into ``torch.optim.Adam`` and continues, and
the other way round.  Nothing synchronises: the loss comes back as a 0-dim device tensor.

Every other call -- CPU tensors, the emulated backend of the tests, a layer without activation or bias, a shape outside the kernels' limits
(1 .. 8 layers, widths 1 .. 512, batch 1 .. 64), an optimiser that is not a plain Adam with one param group, rows that share memory, anything
outside the measured rule below -- takes the module path: the autograd step ``controller_update`` takes, with the loss left on the device.
"""
import ctypes
import math
import weakref

import torch          # every workspace below is allocated through this name: tests swap it for a guard-banded allocator
from torch import nn

from ... import _lib
from . import _backend
from ._backend import HipBackend          # noqa: F401  (the launch path the guard-banded allocator of the tests wraps, as in fc_stack.py)
from .fc_stack import _rows_apart, _row_stride, _split, _params

ENTRY_FWD, ENTRY_LOSS, ENTRY_BWD = 'gc_fc_stack_fwd_save_f32', 'gc_rec_loss_grad_f32', 'gc_fc_stack_bwd_adam_f32'
MAX_LAYERS, MAX_WIDTH, MAX_BATCH = 8, 512, 64          # the kernels' limits (include/gancontrol_hip.h)
KINDS = {'l1': 0, 'mse': 1}                            # GC_REC_LOSS_L1 / GC_REC_LOSS_MSE

# The dispatch rule, from the table in profiles/controller_training.md (wall time per step, controller_update_fused against controller_update on
# the same device-resident batches): the fused step was measured for batch 8 / 32 / 64, in_dim 1 / 3 / 27 / 64, 4 and 8 layers, out 40 / 512,
# and it is not slower in any row.  FUSED_MAX_BATCH is the largest batch measured -- here also the kernels' own limit.
FUSED_MAX_BATCH = 64


class _Plan:
    """What one stack contributes to the argument tables -- the layers with the parameters and pointers they had when the plan was made, the
    optimiser and the moments its state held (all compared with what they are NOW on every call) -- and the workspaces, per batch size."""
    __slots__ = ('optimizer', 'layers', 'params', 'ptrs', 'moments', 'in_dim', 'out_dims', 'n_layers', 'supported', 'device',
                 'w', 'bias', 'out_dim', 'alpha', 'beta', 'w_m', 'w_v', 'b_m', 'b_v', 'work')


# stack -> its plan.  Held weakly: a plan refers to the stack's layers and to the optimiser, never to the stack, so it goes when the stack goes.
_plans = weakref.WeakKeyDictionary()


def kind_of(rec_loss):
    """'l1' / 'mse' of a name or of the trainer's nn.L1Loss / nn.MSELoss (mean reduction); None for anything else."""
    if isinstance(rec_loss, str):
        return rec_loss if rec_loss in KINDS else None
    if type(rec_loss) in (nn.L1Loss, nn.MSELoss) and rec_loss.reduction == 'mean':
        return 'l1' if type(rec_loss) is nn.L1Loss else 'mse'
    return None


def _plain_adam(optimizer, params):
    """A torch.optim.Adam with one param group over exactly these parameters."""
    if type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
        return False
    listed = optimizer.param_groups[0]['params']
    return len(listed) == len(params) and all(a is b for a, b in zip(listed, params))


def _options_ok(plan):
    """What a user may change between two steps: the options of the param group (the kernel implements weight_decay 0, no amsgrad, no
    maximize, float scalars) and a frozen parameter.  Checked on every call, like lr / betas / eps, which are read on every call."""
    g = plan.optimizer.param_groups[0]
    if g['weight_decay'] != 0 or g['amsgrad'] or g['maximize'] or g.get('capturable') or g.get('fused') or g.get('differentiable'):
        return False
    if torch.is_tensor(g['lr']) or any(torch.is_tensor(b) for b in g['betas']):
        return False
    return all(p.requires_grad for p in plan.params)


def _state_ok(optimizer, params):
    """The state the kernels update in place, where the optimiser has one: float32 moments next to their parameter, and a step count that is
    read without a synchronise.  A parameter without state is fine: the first fused step creates it."""
    for p in params:
        state = optimizer.state.get(p)
        if not state:
            continue
        step = state['step']
        if torch.is_tensor(step) and step.is_cuda:
            return False
        for t in (state['exp_avg'], state['exp_avg_sq']):
            if not (t.is_cuda and t.device == p.device and t.dtype == torch.float32 and t.shape == p.shape and t.is_contiguous()):
                return False
    return True


def _moments(optimizer, params):
    """exp_avg / exp_avg_sq of every parameter, created as torch.optim.Adam._init_group creates them where the state is empty."""
    out = []
    for p in params:
        state = optimizer.state[p]
        if len(state) == 0:
            state['step'] = torch.tensor(0.0, dtype=torch.float32)          # on the host, as Adam keeps it without capturable / fused
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        out += [state['exp_avg'], state['exp_avg_sq']]
    return out


def _current(plan):
    now = _params(plan.layers)
    return len(now) == len(plan.params) and all(t is u and t.data_ptr() == q for t, u, q in zip(now, plan.params, plan.ptrs))


def _plan_of(fc_stack, optimizer):
    p = _plans.get(fc_stack)
    if p is not None and p.optimizer is optimizer and _current(p):
        return p
    p = _plans[fc_stack] = _Plan()
    p.optimizer = optimizer
    p.work = {}
    try:
        norm, layers = _split(fc_stack)
    except TypeError:
        norm, layers = True, []
    p.layers = layers
    p.params = _params(layers)
    p.ptrs = [t.data_ptr() for t in p.params]
    p.moments = None
    p.supported = (not norm and 1 <= len(layers) <= MAX_LAYERS
                   and all(m.activation and m.bias is not None for m in layers)
                   and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == p.params[0].device for t in p.params)
                   and all(1 <= d <= MAX_WIDTH for m in layers for d in m.weight.shape)
                   and all(a.weight.shape[0] == b.weight.shape[1] for a, b in zip(layers[:-1], layers[1:]))
                   and _plain_adam(optimizer, p.params))
    if not p.supported:
        return p
    p.device = p.params[0].device
    p.in_dim = layers[0].weight.shape[1]
    p.out_dims = [m.weight.shape[0] for m in layers]
    n = p.n_layers = len(layers)
    vp = ctypes.c_void_p * n
    p.w = vp(*[m.weight.data_ptr() for m in layers])
    p.bias = vp(*[m.bias.data_ptr() for m in layers])
    p.out_dim = (ctypes.c_int32 * n)(*p.out_dims)
    p.alpha = (ctypes.c_float * n)(*[m.scale for m in layers])
    p.beta = (ctypes.c_float * n)(*[m.lr_mul for m in layers])
    return p


def _moment_tables(plan):
    """The pointer tables of the moments, made again whenever the optimiser holds other tensors than last time (load_state_dict)."""
    now = _moments(plan.optimizer, plan.params)
    if plan.moments is None or len(now) != len(plan.moments) or not all(a is b for a, b in zip(now, plan.moments)):
        plan.moments = now
        vp = ctypes.c_void_p * plan.n_layers
        plan.w_m, plan.w_v = vp(*[t.data_ptr() for t in now[0::4]]), vp(*[t.data_ptr() for t in now[1::4]])
        plan.b_m, plan.b_v = vp(*[t.data_ptr() for t in now[2::4]]), vp(*[t.data_ptr() for t in now[3::4]])


def _workspaces(plan, batch):
    """(acts, grads): every layer's output and its gradient, batch * sum(out_dim) floats each, kept for the next step of this batch size."""
    w = plan.work.get(batch)
    if w is None:
        if len(plan.work) > 4:
            plan.work.clear()
        count = batch * sum(plan.out_dims)
        w = plan.work[batch] = (torch.empty(count, dtype=torch.float32, device=plan.device),
                                torch.empty(count, dtype=torch.float32, device=plan.device))
    return w


def _taken(plan, controls, latents_w, chunk, kind):
    if not plan.supported or getattr(_backend.get(), 'name', None) != 'hip' or kind not in KINDS:
        return False
    if not _options_ok(plan) or not _state_ok(plan.optimizer, plan.params):
        return False
    if controls.dim() != 2 or latents_w.dim() != 2 or controls.shape[0] != latents_w.shape[0]:
        return False
    batch = controls.shape[0]
    if batch < 1 or batch > min(MAX_BATCH, FUSED_MAX_BATCH):
        return False
    lo, hi = chunk
    if controls.shape[1] != plan.in_dim or not (0 <= lo < hi <= latents_w.shape[1]) or hi - lo != plan.out_dims[-1]:
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.device == plan.device and _rows_apart(t) for t in (controls, latents_w)):
        return False
    return not (torch.is_grad_enabled() and (controls.requires_grad or latents_w.requires_grad))


def fused_step_taken(fc_stack, optimizer, controls, latents_w, chunk, kind):
    """The dispatch rule (module docstring): whether ``fused_step`` on these arguments is the n_layers + 2 kernel launches.  A query: the
    optimiser's state is read, never created."""
    return _taken(_plan_of(fc_stack, optimizer), controls, latents_w, chunk, kind_of(kind))


def fused_step(fc_stack, optimizer, controls, latents_w, chunk, kind):
    """One Adam step of ``fc_stack`` on mean |fc_stack(controls) - latents_w[:, lo:hi]| ('l1') or its square ('mse'); ``chunk`` = (lo, hi).
    -> the loss before the step, a 0-dim tensor on the parameters' device."""
    plan = _plan_of(fc_stack, optimizer)
    kind = kind_of(kind)
    if not _taken(plan, controls, latents_w, chunk, kind):
        return _module_step(fc_stack, optimizer, controls, latents_w, chunk, kind)
    _moment_tables(plan)
    batch, lo = controls.shape[0], chunk[0]
    acts, grads = _workspaces(plan, batch)
    loss = torch.empty((), dtype=torch.float32, device=plan.device)
    group = optimizer.param_groups[0]
    states = [optimizer.state[p] for p in plan.params]
    t = int(states[0]['step']) + 1
    beta1, beta2 = group['betas']
    bc1, bc2_sqrt = 1.0 - float(beta1) ** t, math.sqrt(1.0 - float(beta2) ** t)
    stream = _lib.stream_of(loss)
    launch = _backend.get()._launch
    x, x_stride = controls.data_ptr(), _row_stride(controls, plan.in_dim)
    last = 4 * batch * (sum(plan.out_dims) - plan.out_dims[-1])          # byte offset of the last layer's block of acts / grads
    launch(plan.device, ENTRY_FWD, x, x_stride, plan.in_dim, plan.n_layers, plan.w, plan.bias, plan.out_dim, plan.alpha, plan.beta,
           acts.data_ptr(), batch, stream)
    launch(plan.device, ENTRY_LOSS, acts.data_ptr() + last, latents_w.data_ptr() + 4 * lo, _row_stride(latents_w, plan.out_dims[-1]), batch,
           plan.out_dims[-1], KINDS[kind], grads.data_ptr() + last, loss.data_ptr(), stream)
    launch(plan.device, ENTRY_BWD, x, x_stride, plan.in_dim, plan.n_layers, plan.w, plan.bias, plan.out_dim, plan.alpha, plan.beta,
           plan.w_m, plan.w_v, plan.b_m, plan.b_v, acts.data_ptr(), grads.data_ptr(), batch, group['lr'], beta1, beta2, group['eps'], bc1, bc2_sqrt,
           stream)
    for state in states:
        state['step'] += 1
    return loss


def _module_step(fc_stack, optimizer, controls, latents_w, chunk, kind):
    """The step of ControllerTrainer.controller_update for ``latent_rec`` alone, without its three reads of the loss."""
    if kind not in KINDS:
        raise ValueError('fc_train.fused_step: kind is "l1" or "mse" (or nn.L1Loss / nn.MSELoss with mean reduction)')
    fc_stack.zero_grad()
    pred = fc_stack(controls.detach())
    target = latents_w[:, chunk[0]:chunk[1]]
    loss = nn.functional.l1_loss(pred, target) if kind == 'l1' else nn.functional.mse_loss(pred, target)
    loss.backward()
    optimizer.step()
    return loss.detach()
