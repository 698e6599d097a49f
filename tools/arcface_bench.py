"""Cost of the ArcFace identity predictor of the embedding loss on one GPU (profiles/arcface_r07.md).

    python tools/arcface_bench.py [--batch 16] [--steps 10] [--warmup 3] [--gstep]

1. Predictor forward + input backward from a [B, 3, 1024, 1024] image (centre crop 480 -> 112), HIP path in f32 and bf16x3, and the
   plain-PyTorch restatement (tests/arcface_checks.restated: ATen / MIOpen, cudnn.benchmark on) as the baseline; ms per call and
   algorithmic TF/s (12.6 GFLOP per image forward, as much again for the input gradient).
2. --gstep: the FFHQ-config generator step at 1024^2 / mini-batch 16 with and without embedding_loss (HIP predictor, f32 and bf16x3).
Weights are the procedural ones of the test fixture (timing does not depend on them).  Prints one JSON line per measurement.
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, 'tests'), os.path.join(REPO, 'gan-control_amd'), REPO):
    sys.path.insert(0, p)

import arcface_checks as ac  # noqa: E402

GFLOP_FWD = 12.6


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def predictor_pass(net, x, vs):
    def run():
        xx = x.detach().requires_grad_(True)
        feats = net(xx)
        g, = torch.autograd.grad(feats[-1], xx, vs)
        return g
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--gstep', action='store_true')
    ap.add_argument('--skip-predictor', action='store_true')
    args = ap.parse_args()
    from gan_control_amd import _lib
    from gan_control_amd.losses import ArcFaceSkeleton
    from gan_control_amd.models.op import _backend
    _lib.load()
    dev = 'cuda'
    be = _backend.get()
    from gan_control_amd.losses import Backbone
    sd = ac.make_state_dict([(k, v.shape) for k, v in Backbone(50, 0.6, 'ir_se').state_dict().items()])
    b = args.batch
    x = (torch.rand(b, 3, 1024, 1024, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    vs = torch.randn(b, 512, generator=torch.Generator().manual_seed(1)).to(dev)
    flop = 2 * GFLOP_FWD * 1e9 * b
    if not args.skip_predictor:
        skel = ArcFaceSkeleton(dict(ac.FFHQ_EMBEDDING), state_dict=sd).to(dev)
        for mode in ('f32', 'bf16x3'):
            be.conv_mode = mode
            ms = timed(predictor_pass(skel, x, vs), args.steps, args.warmup)
            fwd = timed(lambda: skel(x), args.steps, args.warmup)
            print(json.dumps({'what': 'predictor_fwd_bwd', 'impl': 'hip', 'mode': mode, 'batch': b, 'ms': round(ms, 3), 'fwd_ms': round(fwd, 3),
                              'tflops': round(flop / ms / 1e9, 2)}), flush=True)
        be.conv_mode = 'f32'
        torch.backends.cudnn.benchmark = True
        ref = ac.RestatedSkeleton(sd, 480).to(dev)
        ms = timed(predictor_pass(ref, x, vs), args.steps, args.warmup)
        fwd = timed(lambda: ref(x), args.steps, args.warmup)
        print(json.dumps({'what': 'predictor_fwd_bwd', 'impl': 'aten_miopen', 'mode': 'f32', 'batch': b, 'ms': round(ms, 3), 'fwd_ms': round(fwd, 3),
                          'tflops': round(flop / ms / 1e9, 2)}), flush=True)
        del skel, ref
        torch.cuda.empty_cache()
    if args.gstep:
        import op_checks as oc
        from gan_control_amd.losses import LossModelClass
        from gan_control_amd.trainers.generator_trainer import GeneratorTrainer
        from gan_control_amd.trainers.utils import requires_grad
        conf = oc.load_configs()['ffhq']
        cfg = copy.deepcopy({'model_config': conf['model_config'], 'training_config': conf['training_config']})
        cfg['model_config']['size'] = 1024
        cfg['training_config']['batch'] = 16
        cfg['training_config']['mini_batch'] = 16
        cfg['training_config']['embedding_loss'] = dict(ac.FFHQ_EMBEDDING)
        noise = oc.seeded_noise(1024, 16, 7, dev)
        z = torch.randn(16, 512, generator=torch.Generator().manual_seed(9)).to(dev)
        for mode in ('f32', 'bf16x3'):
            be.conv_mode = mode
            for with_loss in (False, True):
                lm = {'embedding_loss': LossModelClass(cfg['training_config']['embedding_loss'], 'embedding_loss', mini_batch_size=16,
                                                       skeleton_model=ArcFaceSkeleton(ac.FFHQ_EMBEDDING, state_dict=sd).to(dev))} if with_loss else None
                tr = GeneratorTrainer(copy.deepcopy(cfg), device=dev, seed=0, fused_adam=False, loss_models=lm)
                requires_grad(tr.generator, True); requires_grad(tr.discriminator, False)
                ms = timed(lambda: tr.generator_step([[z]], noise=noise), max(2, args.steps // 2), args.warmup)
                print(json.dumps({'what': 'g_step_1024_mb16', 'mode': mode, 'embedding_loss': with_loss, 'ms': round(ms, 3)}), flush=True)
                del tr, lm
                torch.cuda.empty_cache()
        be.conv_mode = 'f32'


if __name__ == '__main__':
    main()
