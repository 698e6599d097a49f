"""Per-group latent PCA (reference: projection/projection.py::get_pca_groups).

``get_pca_groups`` samples the mapping network, runs a PCA on every attribute group's slice of w and keeps the leading components that carry
``variance_percent`` of the variance: the subspace a projected latent stays in (``project(..., pca=)``), and per-group edit directions that
need no predictor (``Inference.generate_matrix_by_pca``).

The reference copies the 10 000 x 512 latents to the host and runs a float32 scikit-learn PCA per group.  Here the covariances are ONE
``group_moments`` call on the device (models/op/group_pca.py: float64 sums), only the covariances (at most 2 MiB) travel to the host, and the
eigenproblem of each group is ``numpy.linalg.eigh`` in float64.  What the result holds and how it is chosen -- scikit-learn's
``explained_variance_`` (divisor N - 1), its ``svd_flip`` signs (the largest-magnitude entry of every component positive, the first one on a
tie), the reference's selection rule ``idx = argmax(cumsum(ev) / sum(ev) > variance_percent)``, ``idx + 1`` kept -- is in ``GroupPCA.fit``.

Deviations from the reference ("Per-group latent PCA"): ``latent_mean`` is validated and otherwise unused -- PCA re-centres on the
sample mean, so the value never reached the reference's result either; ``.cuda()`` is ``device``.
"""
import numpy as np
import torch
from torch import nn

from ..models.op import fc_stack as fc_op
from ..models.op import group_pca as gp


class GroupPCA:
    """The result of a fit: ``places`` {group: (lo, hi)}; ``mean`` float32 [D] on the device (the group means, zeros elsewhere);
    ``components`` {group: float32 [r_g, D_g]} on the device; ``explained_variance`` {group: float64 numpy [D_g]}, descending; ``n_samples``;
    ``variance_percent``."""

    def __init__(self, places, mean, components, explained_variance, n_samples, variance_percent):
        self.places = dict(places)
        self.mean = mean
        self.components = components
        self.explained_variance = explained_variance
        self.n_samples = int(n_samples)
        self.variance_percent = float(variance_percent)

    @staticmethod
    def select(explained_variance, variance_percent):
        """How many leading components the reference keeps: idx + 1, idx = argmax(cumsum(ev) / sum(ev) > variance_percent)."""
        ev = np.asarray(explained_variance, dtype=np.float64)
        return int(np.argmax(np.cumsum(ev) / np.sum(ev) > variance_percent)) + 1

    @staticmethod
    def eig(cov):
        """(eigenvalues descending, clipped at 0; eigenvectors as rows with svd_flip's signs) of a float64 symmetric matrix."""
        ev, vec = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
        ev = np.clip(ev[::-1], 0.0, None)
        comps = np.ascontiguousarray(vec[:, ::-1].T)
        lead = np.argmax(np.abs(comps), axis=1)          # the first largest-magnitude entry of every row
        signs = np.sign(comps[np.arange(comps.shape[0]), lead])
        signs[signs == 0] = 1.0
        return ev, comps * signs[:, None]

    @classmethod
    def fit(cls, latent_w, places, variance_percent=0.5, skip=()):
        """Fit on the rows of ``latent_w`` [N, D]: one ``group_moments`` call, the covariances to the host in one copy, ``eigh`` per group.
        ``skip``: group names left out.  A group whose variance sums to 0 raises ValueError naming it."""
        places = {k: (int(v[0]), int(v[1])) for k, v in places.items() if k not in set(skip)}
        if not places:
            raise ValueError('GroupPCA.fit: no groups to fit')
        if not torch.is_tensor(latent_w) or latent_w.dim() != 2:
            raise ValueError('GroupPCA.fit: [N, D] latents expected, got %s' % (tuple(latent_w.shape) if torch.is_tensor(latent_w) else type(latent_w).__name__,))
        with torch.no_grad():
            mean64, cov64 = gp.group_moments_packed(latent_w.detach(), places)
            cov_host = cov64.cpu().numpy()
            means, _ = gp.unpack(mean64, cov64, places)
            dev = latent_w.device
            mean = torch.zeros(latent_w.shape[1], dtype=torch.float32, device=dev)
            _, offsets, _, _ = gp._offsets(places)
            components, variances = {}, {}
            for k, (lo, hi) in places.items():
                d = hi - lo
                ev, comps = cls.eig(cov_host[offsets[k]:offsets[k] + d * d].reshape(d, d))
                if not ev.sum() > 0:
                    raise ValueError('GroupPCA.fit: group %r has no variance over %d samples' % (k, latent_w.shape[0]))
                keep = cls.select(ev, variance_percent)
                mean[lo:hi] = means[k].to(torch.float32)
                components[k] = torch.from_numpy(comps[:keep].astype(np.float32)).to(dev)
                variances[k] = ev
        return cls(places, mean, components, variances, latent_w.shape[0], variance_percent)

    def weights(self):
        """{group: components}: the reference's return value."""
        return dict(self.components)

    def project_(self, latent):
        """``latent`` [B, D] or [B, n_latent, D] onto m + span(components) per group, in place (models/op/group_pca.py); returns it."""
        return gp.group_project_(latent, self.mean, self.components, self.places)


def _group_place(controller, group, width):
    """(lo, hi) of a group through the object's own ``get_group_w_latent`` (applied to a row of column indices)."""
    cols = controller.get_group_w_latent(torch.arange(width).view(1, width), group).reshape(-1)
    lo, hi = int(cols[0]), int(cols[-1]) + 1
    if cols.numel() != hi - lo or not torch.equal(cols, torch.arange(lo, hi)):
        raise ValueError('get_pca_groups: group %r is not one run of columns' % (group,))
    return lo, hi


def _places_of(controller, width):
    if hasattr(controller, 'fc_controls'):
        return {g: _group_place(controller, g, width) for g in controller.fc_controls.keys() if g != 'expression_q'}
    return dict(controller._places())


def _sample_w(controller, model, n, device, generator):
    """[n, D] latents w of n normal draws on ``device``: ``controller.style`` in row chunks inside fc_stacks_forward's measured batch limits,
    written into one buffer; ``model.style`` where the object has no ``style``."""
    z_dim = getattr(model, 'style_dim', 512)
    z = torch.randn(n, z_dim, device=generator.device if generator is not None else device, generator=generator).to(device)
    if not hasattr(controller, 'style'):
        return model.style(z)
    w = torch.empty(n, model.style_dim, dtype=z.dtype, device=device)
    chunk = min(fc_op.KERNEL_MAX_BATCH, fc_op.KERNEL_WIDE_MAX_BATCH)
    for a in range(0, n, chunk):
        controller.style(z[a:a + chunk], out=w[a:a + chunk])
    return w


def get_pca_groups(controller, latent_mean, n_mean_latent, device, *, variance_percent=0.5, generator=None, return_pca=False):
    """{group: float32 [r_g, D_g] on ``device``}: the reference's get_pca_groups (module docstring).  Groups: ``controller.fc_controls`` keys
    without ``'expression_q'``; an ``Inference`` without controllers: every group of ``_places()``.  ``generator``: a torch.Generator the
    draws come from.  ``return_pca=True``: the ``GroupPCA`` itself."""
    model = controller.model.module if isinstance(controller.model, nn.DataParallel) else controller.model
    with torch.no_grad():
        w = _sample_w(controller, model, int(n_mean_latent), torch.device(device), generator)
        width = w.shape[1]
        lm = latent_mean if torch.is_tensor(latent_mean) else torch.as_tensor(np.asarray(latent_mean))
        if lm.numel() != width or not bool(torch.isfinite(lm).all()):
            raise ValueError('get_pca_groups: latent_mean must hold %d finite values, got shape %s' % (width, tuple(lm.shape)))
        pca = GroupPCA.fit(w, _places_of(controller, width), variance_percent)
    return pca if return_pca else pca.weights()


def model_places(model):
    """{group: (lo, hi)} of a Generator: its fc_config groups when the mapping network is split, else one group over the whole row."""
    from ..models.gan_model import MultiFcStack
    if isinstance(model.style, MultiFcStack):
        cfg = model.style.fc_config
        return {n: tuple(int(v) for v in cfg.groups[n]['latent_place']) for n in cfg.in_order_group_names}
    return {None: (0, model.style_dim)}
