"""Writes tests/golden/arcface.npz: the reference's own ArcFace IR-SE50 (Backbone / ArcFaceSkeleton of the gan-control sources) run on the
CPU in float64 with the procedural weights of tests/arcface_checks.fill_weights.

    python tools/make_arcface_golden.py /path/to/gan-control/src

Needs the reference sources (build machine only; no test reads them).  Records, per case of arcface_checks.CASES: the first 64 input values
(the tests redraw the input from its seed), per level the per-channel means and a strided sample, the full embedding, and the input
gradient of sum_levels <feature, V_level> (per-channel sums, norm, strided sample); for the B = 4 case also the gradient of the ffhq
embedding_loss hinge.  The per-level RMS is printed and stored (a check that the weights keep the activations O(1)).
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, 'tests'), os.path.join(REPO, 'gan-control_amd')):
    sys.path.insert(0, p)

import arcface_checks as ac  # noqa: E402


def main(ref_src):
    sys.path.insert(0, ref_src)
    from gan_control.losses.arc_face.arc_face_model import Backbone
    from gan_control.losses.arc_face.arc_face_skeleton import ArcFaceSkeleton
    net = Backbone(50, 0.6, mode='ir_se')
    keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = ac.make_state_dict(keys)
    out = {'keys': np.array(sorted(k for k, _ in keys))}
    shape_of = dict(keys)
    out['key_shapes'] = np.array([list(shape_of[k]) + [0] * (4 - len(shape_of[k])) for k in out['keys']], dtype=np.int64)
    out['n_values'] = np.array([sum(int(np.prod(s)) for k, s in keys if not k.endswith('num_batches_tracked'))])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'model.pth')
        torch.save(sd, path)
        cfg = dict(ac.FFHQ_EMBEDDING, model_path=path)
        torch.set_num_threads(16)
        for name, (b, size, crop) in ac.CASES.items():
            skel = ArcFaceSkeleton(dict(cfg, center_crop=crop)).double()
            x = ac.case_input(name, torch.float64).requires_grad_(True)
            feats = skel(x)
            restated = ac.restated({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.detach(), crop)
            err = max((a - r).abs().max().item() / r.abs().max().item() for a, r in zip(feats, restated))
            print('%s: restatement vs reference %.2e' % (name, err))
            assert err < 1e-9
            out[name + '/x_check'] = x.detach().reshape(-1)[:64].numpy()
            rms = []
            for i, f in enumerate(feats[:4]):
                mean, sample = ac.level_summary(f.detach())
                out['%s/level%d_mean' % (name, i)] = mean.numpy()
                out['%s/level%d_sample' % (name, i)] = sample.numpy().astype(np.float32)
                rms.append(f.detach().pow(2).mean().sqrt().item())
            out[name + '/embedding'] = feats[4].detach().numpy()
            out[name + '/rms'] = np.array(rms)
            print('  level RMS ' + ' '.join('%.3f' % r for r in rms))
            g, = torch.autograd.grad(ac.probe_scalar(feats, ac.probes(name, torch.float64)), x, retain_graph=True)
            sums, norm, sample = ac.grad_summary(g)
            out[name + '/grad_sums'], out[name + '/grad_norm'], out[name + '/grad_sample'] = sums.numpy(), norm.numpy(), sample.numpy()
            print('  probe gradient norm %.4e' % norm.item())
            if b == 4:
                loss = ac.hinge_loss(feats)
                g, = torch.autograd.grad(loss, x)
                sums, norm, sample = ac.grad_summary(g)
                out[name + '/hinge'] = loss.detach().numpy()
                out[name + '/hinge_grad_sums'], out[name + '/hinge_grad_norm'], out[name + '/hinge_grad_sample'] = sums.numpy(), norm.numpy(), sample.numpy()
                print('  hinge %.5f, gradient norm %.4e' % (loss.item(), norm.item()))
    dst = os.path.join(REPO, 'tests', 'golden', 'arcface.npz')
    np.savez_compressed(dst, **out)
    print('wrote %s (%d bytes)' % (dst, os.path.getsize(dst)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GAN_CONTROL_SRC', '.'))
