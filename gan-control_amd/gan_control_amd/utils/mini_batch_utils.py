"""Mini-batch layout of the controllable generator step: which rows share which sub-latent.

Mirrors the reference's ``MiniBatchUtils`` (src/gan_control/utils/mini_batch_multi_split_utils.py:18-115): every attribute
group owns a slice of the latent vector (``place_in_latent``) and a block of rows of the mini-batch (``place_in_mini_batch``);
inside its block consecutive rows (2i, 2i + 1) are made to share the group's sub-latent, so the predictor of that attribute
must see "same" for exactly those pairs (losses/loss_model.py).

``RandomMiniBatchUtils`` (mini_batch_random_multi_split_utils.py:13-111, ``training_config.mini_batch_mode == 'random'``) re-draws every
group's rows before each mini-batch: a group then owns a LIST of row ranges, and the groups' ranges may overlap.
"""
import numpy as np
import torch

from .fc_config import FcConfig, fc_config_from_sub_groups


class MiniBatchUtils:
    def __init__(self, mini_batch, sub_groups_dict, total_batch=8, debug=False, latent_size=512):
        self.mini_batch, self.total_batch, self.sub_groups_dict, self.debug = mini_batch, total_batch, sub_groups_dict, debug
        self.place_in_mini_batch_dict = {n: g['place_in_mini_batch'] for n, g in sub_groups_dict.items()}
        self.place_in_latent_dict = {n: g['place_in_latent'] for n, g in sub_groups_dict.items()}
        self.sub_group_names = sorted(sub_groups_dict, key=lambda n: sub_groups_dict[n]['place_in_latent'][0])
        self.num_of_sub_groups = len(sub_groups_dict)
        self.num_of_mini_batchs = total_batch // mini_batch
        rows = sum(p[1] - p[0] for p in self.place_in_mini_batch_dict.values() if p is not None)
        if rows != mini_batch:
            raise ValueError('self.mini_batch %d != mini_batch_count %d' % (mini_batch, rows))
        width = sum(p[1] - p[0] for p in self.place_in_latent_dict.values())
        if width != latent_size:
            raise ValueError('%d != latent_count_size %d' % (latent_size, width))

    def get_ordered_group_names(self):
        return list(self.sub_group_names)

    def get_fc_config(self) -> FcConfig:
        return fc_config_from_sub_groups(self.sub_groups_dict, sum(p[1] - p[0] for p in self.place_in_latent_dict.values()))

    def get_sub_group(self, batch, sub_group_name='id'):
        lo, hi = self.place_in_mini_batch_dict[sub_group_name]
        return batch[lo:hi]

    def get_not_sub_group(self, batch, sub_group_name='id'):
        lo, hi = self.place_in_mini_batch_dict[sub_group_name]
        return batch[list(range(lo)) + list(range(hi, self.mini_batch))]

    def extract_same_not_same_from_list(self, feature_list, same_group_name):
        return ([self.get_sub_group(f, same_group_name) for f in feature_list],
                [self.get_not_sub_group(f, same_group_name) for f in feature_list])

    def same_not_same_rows(self, group):
        """(rows, n_same, n_not_same): the index form of extract_same_not_same_from_list -- ``rows`` lists the group's block and then every
        other row of the mini-batch, in the order get_sub_group / get_not_sub_group concatenate them, so that
        ``cat([get_sub_group(f), get_not_sub_group(f)]) == f[rows]`` for any per-row tensor f."""
        order = torch.arange(self.mini_batch)
        same, rest = self.get_sub_group(order, group).tolist(), self.get_not_sub_group(order, group).tolist()
        return same + rest, len(same), len(rest)

    def re_arrange_z(self, z_batch, batch_num=0):
        """In place: row 2i + 1 of every group's block takes row 2i's sub-latent of that group; further style codes (mixing)
        follow the first one outside the 'other' block (mini_batch_multi_split_utils.py:64-78)."""
        z0 = z_batch[0]
        for name in self.sub_group_names:
            rows = self.place_in_mini_batch_dict[name]
            if rows is None:
                continue
            lo, hi = self.place_in_latent_dict[name]
            z0[rows[0] + 1:rows[1]:2, lo:hi] = z0[rows[0]:rows[1] - 1:2, lo:hi].detach()
        other = self.place_in_mini_batch_dict.get('other') if 'other' in self.sub_group_names else None
        for i in range(1, len(z_batch)):
            if other is not None:
                z_batch[i][:other[0]] = z0[:other[0]]
                z_batch[i][other[1]:] = z0[other[1]:]
            else:
                z_batch[i] = z0
        return z_batch

    def re_arrange_inject_noise(self, noises, group_name='id'):
        rows = self.place_in_mini_batch_dict[group_name]
        for n in noises:
            n[rows[0] + 1:rows[1]:2] = n[rows[0]:rows[1] - 1:2].detach()
        return noises


class RandomMiniBatchUtils(MiniBatchUtils):
    """Every group with a ``count_in_mini_bach`` range [lo, hi] draws an even size in it and that many / 2 row pairs (2i, 2i + 1) of the
    mini-batch without replacement; adjacent pairs merge into one [start, end) range.  ``rng``: a ``numpy.random.RandomState`` / ``Generator``;
    None draws from the global ``np.random`` with the reference's two ``choice`` calls per group in its order, so a seed gives its places."""

    def __init__(self, mini_batch, sub_groups_dict, total_batch=8, debug=False, latent_size=512, rng=None):
        super().__init__(mini_batch, sub_groups_dict, total_batch=total_batch, debug=debug, latent_size=latent_size)
        self.rng = rng
        self.checks()
        self.count_in_mini_bach_dict = {n: g['count_in_mini_bach'] for n, g in sub_groups_dict.items()}
        self.randomize_places_in_batch()

    def checks(self):
        if self.mini_batch != self.total_batch:
            raise ValueError('RandomMiniBatchUtils has mini_batch %d vs. total_batch %d' % (self.mini_batch, self.total_batch))

    def randomize_places_in_batch(self):
        rng = np.random if self.rng is None else self.rng
        for name in self.sub_group_names:
            count = self.count_in_mini_bach_dict[name]
            if count is None:
                continue
            group_size = rng.choice(np.arange(count[0], count[1] + 2, 2), 1)
            places = None
            if group_size > 0:
                starts = sorted(rng.choice(np.arange(0, self.mini_batch, 2), int(group_size[0]) // 2, replace=False).tolist())
                places = []
                for start in starts:
                    if places and places[-1][1] == start:
                        places[-1][1] += 2
                    else:
                        places.append([start, start + 2])
            self.place_in_mini_batch_dict[name] = places

    def get_sub_group(self, batch, sub_group_name='id'):
        return torch.cat([batch[lo:hi] for lo, hi in self.place_in_mini_batch_dict[sub_group_name]], dim=0)

    def get_not_sub_group(self, batch, sub_group_name='id'):
        """The rows between the group's ranges.  REPRODUCED REFERENCE QUIRK (mini_batch_random_multi_split_utils.py:41): the tail after the
        last range is dropped when that range ends at row ``len(ranges) - 1`` -- a comparison of a row with a count that never holds for
        ranges of whole pairs, so the tail (possibly empty) is always there."""
        places = self.place_in_mini_batch_dict[sub_group_name]
        pieces, last = [], 0
        for lo, hi in places:
            if last != lo:
                pieces.append(batch[last:lo])
            last = hi
        if last != len(places) - 1:
            pieces.append(batch[last:])
        return torch.cat(pieces, dim=0)

    def re_arrange_z(self, z_batch, batch_num=0):
        for name in self.sub_group_names:
            places = self.place_in_mini_batch_dict[name]
            if places is None:
                continue
            lo, hi = self.place_in_latent_dict[name]
            for start, end in places:
                z_batch[0][start + 1:end:2, lo:hi] = z_batch[0][start:end - 1:2, lo:hi].detach()
        if len(z_batch) > 1:
            raise ValueError('len(z_batch) = %d > 1, RandomMiniBatchUtils is not suppurting mixing right now, need to implement' % len(z_batch))
        return z_batch

    def re_arrange_inject_noise(self, noises, group_name='id'):
        for start, end in self.place_in_mini_batch_dict[group_name]:
            for n in noises:
                n[start + 1:end:2] = n[start:end - 1:2].detach()
        return noises
