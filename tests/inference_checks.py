"""Shared by test_inference.py (CPU) and test_inference_gpu.py: model / controller directories written the way a run leaves them, and the fp64
oracle composition of the w-space part of a call.  Nothing here reads the reference checkout."""
import copy
import json
import os

import torch

from conftest import GOLDEN
from oracle import controller as octl

# in_dim of the controllers the paper's face model ships: orientation / hair 3, age 1, illumination (gamma) 27, expression 64 -> here 5,
# quantised expression 8
CONTROLS = {'orientation': 3, 'age': 1, 'gamma': 27, 'expression': 5, 'expression_q': 8, 'hair': 3}
CTL_N_MLP, CTL_MID = 4, 512


def ffhq_config(size=32, vanilla=False):
    cfg = copy.deepcopy(json.load(open(os.path.join(GOLDEN, 'configs.json')))['ffhq'])
    cfg['model_config']['size'] = size
    if vanilla:
        cfg['model_config'].update(vanilla=True, split_fc=False)
    return {'model_config': cfg['model_config'], 'training_config': cfg['training_config']}


def randomize_(module, seed):
    """Parameters stay as their constructors draw them; the biases of the mapping stacks / the controller become non-zero (they are
    multiplied by lr_mul = 0.01)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith('bias') and (name.startswith('style.') or name.startswith('fc_stack.')):
                p.copy_(torch.randn(p.shape, generator=gen).to(p.dtype) * 10.0)
    return module


def write_model_dir(path, config, seed=0, iters=(10,), dtype=torch.float32):
    """args.json + checkpoint/<iter>.pt ('g_ema'); -> the Generator whose state the LAST checkpoint holds."""
    from gan_control_amd.models.gan_model import Generator
    from gan_control_amd.utils.mini_batch_utils import MiniBatchUtils
    mc, tc = config['model_config'], config['training_config']
    os.makedirs(os.path.join(path, 'checkpoint'), exist_ok=True)
    with open(os.path.join(path, 'args.json'), 'w') as f:
        json.dump(config, f)
    fc = None if mc['vanilla'] else MiniBatchUtils(tc['mini_batch'], tc['sub_groups_dict'], total_batch=tc['batch']).get_fc_config()
    model = None
    for k, it in enumerate(sorted(iters)):
        torch.manual_seed(seed + k)
        model = Generator(mc['size'], mc['latent_size'], mc['n_mlp'], channel_multiplier=mc['channel_multiplier'], out_channels=mc['img_channels'],
                          split_fc=mc['split_fc'], fc_config=fc, conv_transpose=mc['conv_transpose'], noise_mode=mc['g_noise_mode'])
        randomize_(model, seed + 100 + k)
        torch.save({'g_ema': model.to(dtype).state_dict()}, os.path.join(path, 'checkpoint', '%06d.pt' % it))
    return model


def write_controller(root, dirname, in_dim, out_dim, seed, dtype=torch.float32):
    from gan_control_amd.models.controller_model import FcStack
    path = os.path.join(root, dirname)
    os.makedirs(os.path.join(path, 'checkpoint'), exist_ok=True)
    cfg = {'model_config': {'lr_mlp': 0.01, 'n_mlp': CTL_N_MLP, 'in_dim': in_dim, 'mid_dim': CTL_MID}, 'training_config': {'batch': 32}}
    with open(os.path.join(path, 'args.json'), 'w') as f:
        json.dump(cfg, f)
    torch.manual_seed(seed)
    net = randomize_(FcStack(0.01, CTL_N_MLP, in_dim, CTL_MID, out_dim), seed + 1).to(dtype)
    torch.save({'controller': net.state_dict()}, os.path.join(path, 'checkpoint', '000500.pt'))
    return net


def write_controller_dir(root, size=32, names=('orientation', 'age', 'gamma', 'expression', 'expression_q'), dtype=torch.float32):
    """<root>/generator + one '<name>_run' directory per named controller; -> config."""
    config = ffhq_config(size)
    write_model_dir(os.path.join(root, 'generator'), config, dtype=dtype)
    places = {k: v['place_in_latent'] for k, v in config['training_config']['sub_groups_dict'].items()}
    for i, name in enumerate(names):
        lo, hi = places['expression' if name == 'expression_q' else name]
        write_controller(str(root), name + '_run', CONTROLS[name], hi - lo, 50 + i, dtype=dtype)
    return config


def stack_params(stack):
    """(pixel_norm, [weights], [biases], lr_mul) of a create_fc_stack Sequential or an FcStack, as float64 CPU tensors."""
    from gan_control_amd.models.gan_model import EqualLinear, PixelNorm
    mods = list(stack.fc_stack) if hasattr(stack, 'fc_stack') else list(stack)
    layers = [m for m in mods if isinstance(m, EqualLinear)]
    return (isinstance(mods[0], PixelNorm), [m.weight.detach().double().cpu() for m in layers], [m.bias.detach().double().cpu() for m in layers],
            layers[0].lr_mul)


def oracle_stack(stack, x):
    """The documented formula in float64: PixelNorm on the stack's own columns, then oracle.controller.fc_stack_forward."""
    norm, ws, bs, lr_mul = stack_params(stack)
    x = x.detach().double().cpu()
    if norm:
        x = x * torch.rsqrt(x.pow(2).mean(dim=1, keepdim=True) + 1e-8)
    return octl.fc_stack_forward(x, ws, bs, lr_mul)


def oracle_latent_w(ctl, z, controls):
    """w of the oracle mapping stacks with every driven group's slice replaced by the oracle controller output (float64, CPU)."""
    style = ctl.model.style
    w = torch.empty(z.shape[0], 512, dtype=torch.float64)
    for name in style.fc_config.in_order_group_names:
        lo, hi = style.fc_config.groups[name]['latent_place']
        w[:, lo:hi] = oracle_stack(getattr(style, name), z[:, lo:hi])
    for key, value in controls.items():
        name = 'expression_q' if key == 'expression' and value.shape[1] == 8 else key
        lo, hi = ctl.batch_utils.place_in_latent_dict[key]
        w[:, lo:hi] = oracle_stack(ctl.fc_controls[name], value)
    return w
