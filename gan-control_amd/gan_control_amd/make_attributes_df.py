"""The attribute frame of phase 2: samples of a trained generator with their latents and the attributes predictors read off the images.

Reference: src/gan_control/make_attributes_df.py.  ``make_attributes_df`` writes the pickled pandas DataFrame that
``datasets.DataFrameDataSet`` / ``datasets.DeviceFrame`` read and ``ControllerTrainer.train`` learns from: one row per sample with ``latents``
(the z), ``latents_w`` (the w row the generator ran on) and one column per predictor.  The predictors are the caller's, like ``skeleton_model=``
elsewhere: the only one in the tree is ArcFace (``'arcface_emb'``).  Results stay on the device while the batches run and become the frame once
at the end (the reference's per-row ``DataFrame.append`` no longer exists in pandas).

    python -m gan_control_amd.make_attributes_df --model_dir <dir> --save_path <frame.pkl> [--batch_size 40] [--number_of_samples 100000]
"""
import argparse
import os

import pandas as pd
import torch


@torch.no_grad()
def make_attributes_df(model, predictors, save_path=None, batch_size=40, number_of_samples=10000, generator=None):
    """model: an ``inference.Inference``; predictors: {column: callable(images [B, 3, h, w] in [-1, 1]) -> tensor [B, ...]}.
    ``number_of_samples // batch_size`` batches of ``model.gen_batch(batch_size, normalize=False)``.  -> the DataFrame with the columns
    ``latents``, ``latents_w`` (one 1-D array of the latent width per row) and one per predictor: a [B] result is stored as scalars, a
    [B, d, ...] result as arrays.  Pickled to ``save_path`` when one is given.  ``generator``: a ``torch.Generator`` that makes the call
    repeatable (latents and noise maps are drawn from it)."""
    predictors = dict(predictors or {})
    for name in predictors:
        if name in ('latents', 'latents_w'):
            raise ValueError('make_attributes_df: %r is a column of the frame itself' % name)
    columns = {name: [] for name in ['latents', 'latents_w', *predictors]}
    for _ in range(number_of_samples // batch_size):
        out, latent, latents = model.gen_batch(batch_size=batch_size, normalize=False, generator=generator)
        columns['latents'].append(latent)
        columns['latents_w'].append(latents[:, 0])          # the reference's latent_w_i[0][0]: every layer gets the same w row
        for name, predict in predictors.items():
            value = predict(out)
            if not torch.is_tensor(value) or value.dim() < 1 or value.shape[0] != batch_size:
                raise ValueError('make_attributes_df: predictor %r must return a tensor [%d, ...], got %s'
                                 % (name, batch_size, tuple(value.shape) if torch.is_tensor(value) else type(value)))
            columns[name].append(value.detach())
    frame = {}
    for name, parts in columns.items():
        if not parts:
            frame[name] = []
            continue
        values = torch.cat(parts, dim=0).cpu().numpy()          # one copy to the host per column
        frame[name] = values if values.ndim == 1 else list(values)
    attributes_df = pd.DataFrame(frame, columns=list(columns))
    if save_path is not None:
        os.makedirs(os.path.split(os.path.abspath(save_path))[0], exist_ok=True)
        attributes_df.to_pickle(save_path)
    return attributes_df


def arcface_predictor(loss_config, device):
    """'arcface_emb' of the reference's frame: the last feature of the ArcFace LossModelClass (``id_embedding_class.calc_features(out)[-1]``)."""
    from .losses import ArcFaceSkeleton, LossModelClass
    loss_class = LossModelClass(loss_config, 'embedding_loss', skeleton_model=ArcFaceSkeleton(loss_config).to(device).eval())
    return lambda images: loss_class.calc_features(images)[-1]


def main(argv=None):
    from .inference import Inference
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--model_dir', type=str, required=True, help='path to gan model dir')
    parser.add_argument('--batch_size', type=int, default=40)
    parser.add_argument('--number_of_samples', type=int, default=100000)
    parser.add_argument('--save_path', type=str, required=True, help='path of the pickled frame')
    args = parser.parse_args(argv)
    model = Inference(args.model_dir)
    predictors = {}
    embedding = model.config.training_config.get('embedding_loss')
    if isinstance(embedding, dict) and embedding.get('model_path') and os.path.exists(embedding['model_path']):
        predictors['arcface_emb'] = arcface_predictor(embedding, model.device)
    else:
        print('make_attributes_df: no embedding_loss.model_path on this machine: the frame holds latents only')
    frame = make_attributes_df(model, predictors, args.save_path, batch_size=args.batch_size, number_of_samples=args.number_of_samples)
    print('make_attributes_df: %d rows, columns %s -> %s' % (len(frame), list(frame.columns), args.save_path))


if __name__ == '__main__':
    main()
