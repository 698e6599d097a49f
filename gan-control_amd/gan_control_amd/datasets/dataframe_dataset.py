"""(attribute, w-latent) pairs for the controller.

Reference: datasets/dataframe_dataset.py:18-56 -- a pickled pandas DataFrame with a ``latents_w`` column and one column per
attribute; first 90 % train, last 10 % eval; ``age`` gets a trailing unit axis, ``expression_q`` becomes a one-hot of 8.
``make_attributes_df.py`` writes such a frame.  ``DeviceFrame`` is the same data as two tensors on the training device
(``ControllerTrainer.train`` reads it: 4 us per batch against 475 us for the loader, profiles/controller_training.md).
"""
import pandas as pd
import torch
from torch.utils import data


class DataFrameDataSet(data.Dataset):
    def __init__(self, dataframe_path, attribute=None, train=True):
        frame = dataframe_path if isinstance(dataframe_path, pd.DataFrame) else pd.read_pickle(dataframe_path)
        cut = int(len(frame.latents_w) * 0.9)
        frame = frame.iloc[:cut] if train else frame.iloc[cut:]
        self.train, self.attribute = train, attribute
        self.attributes_df = frame[['latents_w', attribute]] if attribute is not None else frame

    def __len__(self):
        return len(self.attributes_df.latents_w)

    def __getitem__(self, index):
        row = self.attributes_df.iloc[index]
        value = torch.tensor(row[self.attribute])
        if self.attribute == 'age':
            value = value.unsqueeze(0)
        elif self.attribute == 'expression_q':
            value = torch.nn.functional.one_hot(value, num_classes=8)
        return value, torch.tensor(row['latents_w'])


def get_dataframe_data_loader(dataframe_path, attribute, batch_size=32, shuffle=True, drop_last=True, workers=32, train=True):
    return data.DataLoader(DataFrameDataSet(dataframe_path, attribute=attribute, train=train), batch_size=batch_size,
                           shuffle=shuffle, drop_last=drop_last, num_workers=workers)


class DeviceFrame:
    """The same split and the same attribute shaping as ``DataFrameDataSet``, held as two contiguous tensors on ``device`` that are built once:
    ``controls`` [N, in_dim] and ``latents_w`` [N, W], float32.  ``epoch`` permutes both once and yields row slices: no launch per batch, no
    worker processes, no per-sample pandas ``iloc``."""

    def __init__(self, frame_or_path, attribute, device, train=True):
        import numpy as np
        frame = frame_or_path if isinstance(frame_or_path, pd.DataFrame) else pd.read_pickle(frame_or_path)
        cut = int(len(frame.latents_w) * 0.9)
        frame = frame.iloc[:cut] if train else frame.iloc[cut:]
        self.train, self.attribute, self.device = train, attribute, torch.device(device)
        values = torch.from_numpy(np.stack([np.asarray(v) for v in frame[attribute]])) if len(frame) else torch.zeros(0)
        if attribute == 'age':
            values = values.unsqueeze(1)
        elif attribute == 'expression_q':
            values = torch.nn.functional.one_hot(values.long(), num_classes=8)
        latents = torch.from_numpy(np.stack([np.asarray(v) for v in frame['latents_w']])) if len(frame) else torch.zeros(0, 0)
        if values.dim() != 2:
            raise ValueError('DeviceFrame: attribute %r gives controls of shape %s per batch; [N, in_dim] is what a controller takes'
                             % (attribute, tuple(values.shape)))
        self.controls = values.to(self.device, torch.float32).contiguous()
        self.latents_w = latents.to(self.device, torch.float32).contiguous()

    def __len__(self):
        return self.controls.shape[0]

    def __getitem__(self, index):
        """(control, w latent) of one row, the values ``DataFrameDataSet.__getitem__`` returns (as float32 on the device)."""
        return self.controls[index], self.latents_w[index]

    def epoch(self, batch_size, generator=None, shuffle=True, drop_last=True):
        """Yields (controls [B, in_dim], latents_w [B, W]) views over every row once: one ``randperm`` and two ``index_select`` per epoch,
        then contiguous row slices.  ``generator``: a ``torch.Generator`` (of the frame's device or of the CPU) that makes the order repeatable."""
        n = len(self)
        controls, latents = self.controls, self.latents_w
        if shuffle and n:
            on_device = generator is None or generator.device.type == self.device.type
            perm = torch.randperm(n, generator=generator, device=self.device if on_device else 'cpu').to(self.device)
            controls, latents = controls.index_select(0, perm), latents.index_select(0, perm)
        stop = n // batch_size * batch_size if drop_last else n
        for lo in range(0, stop, batch_size):
            yield controls[lo:lo + batch_size], latents[lo:lo + batch_size]
