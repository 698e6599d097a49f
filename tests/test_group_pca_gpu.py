"""gc_group_moments_f32 and gc_group_project_f32 on the GPU (csrc/group_pca.hip through models/op/group_pca.py), and get_pca_groups /
project(pca=) end to end.

Every call runs on guard-banded, poisoned outputs and workspaces (tests/guarded_alloc.py, both poisons) and on hostile() copies of every input
(NaN -- or 1e30 -- between strided rows and around the buffers) at shift 0 (16-byte loads where the group allows them) and shift 4 (4-byte
loads): the results of the two must be the same bits.

Moments.  Oracle: the two-pass formula in numpy.longdouble on the upcast inputs (float64 where long double is no wider).  Derived elementwise
bound, u = 2^-53:
    |cov - ref| <= 2 (N + 8) u sqrt(sum_r x_ri^2 * sum_r x_rj^2) / (N - 1),      |mean - ref| <= 2 (N + 8) u sum_r |x_ri| / N.
Products of widened floats are exact; a sum of N terms in any order is within (N - 1) u of sum |terms|, which Cauchy-Schwarz bounds by
sqrt(sum x_i^2 sum x_j^2) -- the same holds for S1 S1^T / N; the subtraction and the division add a few u; the factor 2 covers the oracle's own
rounding.
Projection.  Oracle: the float64 formula on the upcast inputs.  Derived bound, u = 2^-24:
    |y - y64| <= (D_g + r_g + 4) u (|m| + |P|^T (|P| |x - m|)):
d = x - m adds one u of |x - m|; each c_k is a sum of D_g products (D_g u of |P| |d|); y = sum_k P_kj c_k is r_g more terms; m + y one u.
"""
import numpy as np
import pytest
import torch

import guarded_alloc
import op_checks as oc

from gan_control_amd import _lib
from gan_control_amd.models.op import _backend
from gan_control_amd.models.op import group_pca as gp
from gan_control_amd.projection import pca as pca_mod

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U64, U32 = 2.0 ** -53, 2.0 ** -24
S = gp.ROW_SPLIT
LD = np.longdouble if np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant else np.float64
FFHQ = [(0, 128)] + [(128 + 64 * i, 64) for i in range(6)]
SIXTEEN = [(0, 1), (1, 2), (3, 31), (34, 32), (66, 33), (99, 64), (163, 65), (228, 1), (229, 2), (231, 31), (263, 32), (296, 33), (330, 5),
           (335, 7), (342, 3), (346, 4)]

# (N, [(lo, width)], row width D, stride kind, NaN in the columns of no group)
MOMENT_CASES = [
    (2, [(0, 1), (1, 2)], 3, 'd', False),
    (3, [(1, 31), (33, 32)], 68, 'd', False),
    (31, [(0, 33), (36, 64)], 100, '2d', False),
    (32, [(3, 65)], 70, 'd+1', False),
    (33, [(0, 128), (129, 2)], 132, 'd', True),
    (257, [(5, 192)], 200, 'd', False),
    (S - 1, [(4, 64), (68, 33)], 104, 'd', False),
    (S, [(0, 512)], 512, 'd', False),
    (S + 1, [(1, 512)], 516, 'd+1', False),
    (S + 1, [(8, 65), (80, 31)], 112, '2d', True),
    (2 * S + 1, [(0, 192), (192, 192), (384, 128)], 512, 'd', False),
    (2 * S + 1, FFHQ, 512, 'd+1', False),
    (33, SIXTEEN, 352, 'd', False),
    (2 * S + 1, [(2, 1), (7, 2), (12, 33)], 48, '2d', False),
    (gp.MAX_SPLITS * S + 27, [(1, 33), (36, 31)], 68, 'd', False),          # past MAX_SPLITS splits of S rows: longer splits
]


def strided(rows, d, kind, gen, nan_cols=None):
    width = {'d': d, 'd+1': d + 1, '2d': 2 * d}[kind]
    base = torch.randn(rows, width, generator=gen) * 1.5 + 0.5
    if nan_cols is not None:
        base[:, nan_cols] = float('nan')
    base = base.to(DEV)
    return base.view(2 * rows, d)[::2] if kind == '2d' else base[:, :d]


def places_of(groups):
    return {'g%d' % i: (lo, lo + w) for i, (lo, w) in enumerate(groups)}


def moments_oracle(w, places):
    x = w.cpu().numpy().astype(LD)
    n = x.shape[0]
    out = {}
    for k, (lo, hi) in places.items():
        g = x[:, lo:hi]
        m = g.mean(0)
        c = g - m
        cov = np.einsum('ri,rj->ij', c, c) / LD(n - 1)
        sq = (g * g).sum(0)
        bound = 2 * (n + 8) * U64 * np.sqrt(np.outer(sq, sq).astype(np.float64)) / (n - 1)
        mb = 2 * (n + 8) * U64 * np.abs(g).sum(0).astype(np.float64) / n
        out[k] = (m, cov, mb, bound)
    return out


def run_moments(w, places, poison='nan', fill='nan', shift=0):
    hw = guarded_alloc.hostile(w, fill, shift)
    with torch.no_grad(), guarded_alloc.guarded(gp, poison=poison) as guard:
        mean, cov = gp.group_moments_packed(hw, places)
        assert guard.check() == []
    assert guarded_alloc.hostile_changes(hw, w) is None
    return mean, cov, guard.entries


def bits(t):
    return t.view(torch.int64) if t.element_size() == 8 else t.view(torch.int32)


@pytest.mark.parametrize('n,groups,d,kind,nan', MOMENT_CASES)
def test_moments_against_the_long_double_formula(n, groups, d, kind, nan):
    gen = torch.Generator().manual_seed(n * 7 + d)
    places = places_of(groups)
    outside = None
    if nan:
        inside = np.zeros(d, bool)
        for lo, hi in places.values():
            inside[lo:hi] = True
        outside = torch.from_numpy(np.nonzero(~inside)[0])
    w = strided(n, d, kind, gen, outside)
    assert gp.kernel_taken(w, places)
    mean, cov, entries = run_moments(w, places)
    assert entries == [gp.MOMENTS_ENTRY]
    means, covs = gp.unpack(mean, cov, places)
    ref = moments_oracle(w, places)
    for k in places:
        m, c = means[k].cpu().numpy(), covs[k].cpu().numpy()
        rm, rc, mb, cb = ref[k]
        em, ec = np.abs(m - rm.astype(np.float64)), np.abs(c - rc.astype(np.float64))
        print('moments N=%-4d %s [%d, %d) stride %-3s  cov error / bound %.3e  mean error / bound %.3e'
              % (n, k, *places[k], kind, float((ec / cb).max()), float((em / mb).max())))
        assert np.all(ec <= cb) and np.all(em <= mb)
        assert torch.equal(bits(covs[k]), bits(covs[k].T.contiguous()))
    m2, c2, _ = run_moments(w, places)
    assert torch.equal(bits(mean), bits(m2)) and torch.equal(bits(cov), bits(c2))
    m3, c3, e3 = run_moments(w, places, poison='big', fill='big', shift=4)
    assert e3 == [gp.MOMENTS_ENTRY] and torch.equal(bits(mean), bits(m3)) and torch.equal(bits(cov), bits(c3))


def orthonormal(r, d, gen):
    q, _ = torch.linalg.qr(torch.randn(d, r, generator=gen, dtype=torch.float64))
    return q.T.contiguous().float()


def project_case(rows, groups, d, kind, gen, shape=None):
    x = strided(rows, d, kind, gen)
    if shape is not None:
        x = x.view(*shape)
    mean = (torch.randn(d, generator=gen) * 0.7).to(DEV)
    comps = {'g%d' % i: orthonormal(r, w, gen).to(DEV) for i, (lo, w, r) in enumerate(groups)}
    places = {'g%d' % i: (lo, lo + w) for i, (lo, w, r) in enumerate(groups)}
    return x, mean, comps, places


def project64(x, mean, comps, places):
    y = x.double().clone()
    for k, (lo, hi) in places.items():
        m, p = mean[lo:hi].double(), comps[k].double()
        y[..., lo:hi] = m + ((y[..., lo:hi] - m) @ p.T) @ p
    return y


def project_bound(x, mean, comps, places):
    out = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    for k, (lo, hi) in places.items():
        m, p = mean[lo:hi].double(), comps[k].double()
        out[..., lo:hi] = (hi - lo + p.shape[0] + 4) * U32 * (m.abs() + ((x[..., lo:hi].double() - m).abs() @ p.abs().T) @ p.abs())
    return out


def run_project(x, mean, comps, places, poison='nan', fill='nan', shift=0):
    hx = guarded_alloc.hostile(x, fill, shift)
    hm = guarded_alloc.hostile(mean, fill, shift)
    hc = {k: guarded_alloc.hostile(v, fill, shift) for k, v in comps.items()}
    with torch.no_grad(), guarded_alloc.guarded(gp, poison=poison) as guard:
        assert gp.kernel_taken(hx, hm, hc, places)
        assert gp.group_project_(hx, hm, hc, places) is hx
        assert guard.check() == []
    y = hx.clone()
    assert guarded_alloc.hostile_changes(hx, y) is None          # nothing outside x's logical elements was written
    assert guarded_alloc.hostile_changes(hm, mean) is None and all(guarded_alloc.hostile_changes(hc[k], comps[k]) is None for k in comps)
    return y, guard.entries


# (rows, [(lo, D_g, r_g)], D, stride kind, shape)
PROJECT_CASES = [
    (1, [(0, 1, 1)], 1, 'd', None),
    (2, [(1, 33, 7)], 36, 'd+1', None),
    (7, [(4, 64, 64)], 70, '2d', None),
    (54, [(3, 128, 19)], 140, 'd', (3, 18, 140)),
    (7, [(0, 512, 100)], 512, 'd', None),
    (2, [(0, 512, 100)], 513, '2d', None),
    (54, [(lo, w, r) for (lo, w), r in zip(FFHQ, (19, 7, 5, 9, 3, 12, 6))], 512, 'd', (3, 18, 512)),
    (18, [(lo, w, r) for (lo, w), r in zip(FFHQ, (19, 7, 5, 9, 3, 12, 6))], 512, 'd+1', None),
]


@pytest.mark.parametrize('rows,groups,d,kind,shape', PROJECT_CASES)
def test_projection_against_the_float64_formula(rows, groups, d, kind, shape):
    gen = torch.Generator().manual_seed(rows * 13 + d)
    x, mean, comps, places = project_case(rows, groups, d, kind, gen, shape)
    y, entries = run_project(x, mean, comps, places)
    assert entries == [gp.PROJECT_ENTRY]
    ref = project64(x, mean, comps, places)
    bound = project_bound(x, mean, comps, places)
    err = (y.double() - ref).abs()
    inside = bound > 0
    print('project rows=%-3d D=%-3d stride %-3s groups %s  error / bound %.3e' % (rows, d, kind, [g[1:] for g in groups], float((err[inside] / bound[inside]).max())))
    assert bool((err <= bound).all())
    assert torch.equal(bits(y[..., ~inside.reshape(-1, d)[0]]), bits(x[..., ~inside.reshape(-1, d)[0]]))          # other columns keep their bits
    y2, _ = run_project(x, mean, comps, places)
    assert torch.equal(bits(y), bits(y2))
    y3, e3 = run_project(x, mean, comps, places, poison='big', fill='big', shift=4)
    assert e3 == [gp.PROJECT_ENTRY] and torch.equal(bits(y), bits(y3))


def test_dispatch_and_in_place_views():
    gen = torch.Generator().manual_seed(4)
    w = (torch.randn(80, 96, generator=gen) + 0.2).to(DEV)
    places = {'a': (3, 40), 'b': (40, 96)}
    assert gp.kernel_taken(w, places) and gp.kernel_taken(w[::2], places) and gp.kernel_taken(w[:, :60], {'a': (0, 60)})
    assert not gp.kernel_taken(w.double(), places) and not gp.kernel_taken(w.cpu(), places)
    assert not gp.kernel_taken(torch.zeros(8, 600, device=DEV), {'a': (0, 513)})
    assert not gp.kernel_taken(torch.zeros(8, 40, device=DEV), {i: (i, i + 1) for i in range(17)})
    assert not gp.kernel_taken(w[:, ::2], {'a': (0, 10)}) and not gp.kernel_taken(w[:1], places)
    with guarded_alloc.guarded(gp) as guard:
        mean, cov = gp.group_moments(w[::2], places)
        big_mean, big_cov = gp.group_moments(torch.zeros(8, 600, device=DEV), {'a': (0, 513)})
    assert guard.entries == [gp.MOMENTS_ENTRY] and big_cov['a'].shape == (513, 513)
    ref_mean, ref_cov = gp.group_moments(w[::2].cpu(), places)
    for k in places:
        assert float((cov[k].cpu() - ref_cov[k]).abs().max()) <= 1e-12 and float((mean[k].cpu() - ref_mean[k]).abs().max()) <= 1e-13
    comps = {'a': orthonormal(5, 37, gen).to(DEV), 'b': orthonormal(9, 56, gen).to(DEV)}
    m = torch.zeros(96, device=DEV)
    x = torch.randn(4, 18, 96, generator=gen).to(DEV)
    assert gp.kernel_taken(x, m, comps, places) and gp.kernel_taken(x[:, 3], m, comps, places)
    assert not gp.kernel_taken(x.double(), m.double(), {k: v.double() for k, v in comps.items()}, places)
    assert not gp.kernel_taken(x.transpose(0, 1), m, comps, places)          # no single row stride
    assert not gp.kernel_taken(x, m, comps, {'a': (3, 40), 'b': (39, 95)})          # overlapping groups
    want = gp.project_reference_(x.clone(), m, comps, places)
    xt = x.transpose(0, 1)          # not one row stride: the formula, in place
    with guarded_alloc.guarded(gp) as guard:
        gp.group_project_(xt, m, comps, places)
    assert guard.entries == [] and float((x - want).abs().max()) <= 1e-5


def _raw_moments(w, stride, n, lo, hi, groups, mean, cov, ws=None, nbytes=0):
    los, his = (ctypes_i32(lo), ctypes_i32(hi))
    _backend.get()._launch(w.device, gp.MOMENTS_ENTRY, _lib.ptr(w), stride, n, los, his, groups, _lib.ptr(mean), _lib.ptr(cov), _lib.ptr(ws), nbytes,
                           _lib.stream_of(w))


def ctypes_i32(v):
    import ctypes
    return (ctypes.c_int32 * max(1, len(v)))(*v)


def test_bad_arguments_are_refused_before_any_launch():
    w = torch.ones(10, 64, device=DEV)
    mean = torch.full((64,), 3.0, dtype=torch.float64, device=DEV)
    cov = torch.full((64 * 64,), 3.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    nb = ws.numel() * 8
    for word, args in (('null pointer', (w, 64, 10, [0], [64], 1, None, cov, ws, nb)), ('at least 2', (w, 64, 1, [0], [64], 1, mean, cov, ws, nb)),
                       ('at least 1', (w, 64, 10, [0], [64], 0, mean, cov, ws, nb)), ('at most 16', (w, 64, 10, list(range(17)), list(range(1, 18)), 17, mean, cov, ws, nb)),
                       ('outside rows', (w, 64, 10, [0], [65], 1, mean, cov, ws, nb)), ('outside rows', (w, 64, 10, [5], [5], 1, mean, cov, ws, nb)),
                       ('at most 512', (w, 600, 10, [0], [513], 1, mean, cov, ws, nb)), ('workspace too small', (w, 64, 10, [0], [64], 1, mean, cov, ws, 64))):
        with pytest.raises(RuntimeError, match=word):
            _raw_moments(*args)
    torch.cuda.synchronize()
    assert bool((mean == 3.0).all()) and bool((cov == 3.0).all())
    import ctypes
    x = torch.ones(4, 64, device=DEV)
    p = torch.ones(2, 32, device=DEV)
    ptrs = (ctypes.c_void_p * 2)(p.data_ptr(), p.data_ptr())
    for word, ranks, lo, hi in (('components of a', [0, 2], [0, 32], [32, 64]), ('components of a', [2, 33], [0, 32], [32, 64]), ('overlap', [2, 2], [0, 31], [32, 63])):
        with pytest.raises(RuntimeError, match=word):
            _backend.get()._launch(x.device, gp.PROJECT_ENTRY, _lib.ptr(x), 64, 4, _lib.ptr(mean), ptrs, ctypes_i32(ranks), ctypes_i32(lo), ctypes_i32(hi), 2,
                                   _lib.stream_of(x))
    torch.cuda.synchronize()
    assert bool((x == 1.0).all())


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def model_dirs(tmp_path_factory):
    import inference_checks as ic
    root = tmp_path_factory.mktemp('pca_models')
    out = {}
    for name, vanilla in (('split', False), ('vanilla', True)):
        cfg = ic.ffhq_config(32, vanilla=vanilla)
        cfg['model_config']['n_mlp'] = 2
        ic.write_model_dir(str(root / name), cfg, seed=3)
        out[name] = str(root / name)
    return out


class Transfers:
    """CUDA -> host copies made through Tensor.cpu / .to / .tolist / .item while installed: their shapes."""

    def __init__(self, monkeypatch):
        self.shapes = []
        for name in ('cpu', 'to', 'tolist', 'item'):
            real = getattr(torch.Tensor, name)

            def wrapped(t, *a, _real=real, _name=name, **k):
                out = _real(t, *a, **k)
                if t.is_cuda and (_name in ('tolist', 'item') or (torch.is_tensor(out) and not out.is_cuda)):
                    self.shapes.append(tuple(t.shape))
                return out
            monkeypatch.setattr(torch.Tensor, name, wrapped)


@pytest.mark.parametrize('kind', ['split', 'vanilla'])
def test_get_pca_groups_end_to_end(kind, model_dirs, monkeypatch):
    from gan_control_amd.inference import Inference
    inf = Inference(model_dirs[kind], device=DEV)
    seen = []
    real_fit = pca_mod.GroupPCA.fit.__func__

    def fit(cls, latent_w, places, *a, **k):
        seen.append((latent_w.detach().clone(), dict(places)))
        return real_fit(cls, latent_w, places, *a, **k)

    monkeypatch.setattr(pca_mod.GroupPCA, 'fit', classmethod(fit))
    n = 700
    with guarded_alloc.guarded(gp) as guard:
        moves = Transfers(monkeypatch)
        got = pca_mod.get_pca_groups(inf, torch.zeros(512), n, DEV, generator=torch.Generator().manual_seed(9), return_pca=True)
        monkeypatch.undo()
        assert guard.check() == []
    assert guard.entries.count(gp.MOMENTS_ENTRY) == 1 and gp.PROJECT_ENTRY not in guard.entries
    w, places = seen[0]
    assert w.shape == (n, 512) and w.is_cuda and places == inf._places()
    total = sum((hi - lo) ** 2 for lo, hi in places.values())
    assert moves.shapes == [(total,)], moves.shapes          # the covariances, once; never w
    oracle = pca_mod.GroupPCA.fit(w.cpu(), places)
    ref = moments_oracle(w, places)
    for k, (lo, hi) in places.items():
        ev_o = oracle.explained_variance[k]
        keep = oracle.components[k].shape[0]
        fro = float(np.linalg.norm(ref[k][3]))
        gaps = [float(np.min(np.abs(np.delete(ev_o, j) - ev_o[j]))) for j in range(keep)]
        print('get_pca_groups %s %s: kept %d, min relative gap %.3e, eigenvalue error %.3e (bound %.3e)'
              % (kind, k, keep, min(g / ev_o[j] for j, g in enumerate(gaps)), float(np.abs(got.explained_variance[k] - ev_o).max()), fro))
        assert all(g >= 1e-3 * ev_o[j] for j, g in enumerate(gaps)), 'degenerate draw'
        assert got.components[k].shape == (keep, hi - lo)
        assert np.all(np.abs(got.explained_variance[k] - ev_o) <= fro)
        for j in range(keep):
            err = float(np.linalg.norm(got.components[k][j].double().cpu().numpy() - oracle.components[k][j].double().numpy()))
            assert err <= 4 * fro / gaps[j] + np.sqrt(hi - lo) * U32, (k, j, err)


def test_project_with_pca_on_the_device(monkeypatch):
    g, _ = oc.build_models(32, DEV, fc_groups=[('id', (0, 128)), ('pose', (128, 192)), ('age', (192, 256)), ('rest', (256, 512))])
    g.eval()
    with torch.no_grad():
        target, _ = g([torch.randn(1, 512, generator=torch.Generator().manual_seed(8)).to(DEV)])
    from gan_control_amd import projection
    seen = []
    real_fit = pca_mod.GroupPCA.fit.__func__

    def fit(cls, latent_w, places, *a, **k):
        out = real_fit(cls, latent_w, places, *a, **k)
        seen.append((dict(places), out))
        return out

    monkeypatch.setattr(pca_mod.GroupPCA, 'fit', classmethod(fit))
    with guarded_alloc.guarded(gp) as guard:
        latent, _, _, history = projection.project(g, target, steps=2, lr=0.1, mse_weight=1.0, n_mean_latent=600, pca=0.5,
                                                   generator=torch.Generator().manual_seed(3))
        assert guard.check() == []
    monkeypatch.undo()
    assert guard.entries.count(gp.PROJECT_ENTRY) == 2 and guard.entries.count(gp.MOMENTS_ENTRY) == 1 and len(history) == 2
    assert latent.is_cuda and bool(torch.isfinite(latent).all())
    # the fit project() made itself: the model's groups, the given share, and it keeps the returned latent in place
    assert len(seen) == 1
    places, inner = seen[0]
    assert places == pca_mod.model_places(g) == inner.places and inner.variance_percent == 0.5 and inner.n_samples == 600
    again = latent.clone()
    inner.project_(again)
    bound = project_bound(latent, inner.mean, inner.components, inner.places)
    print('project(pca=0.5): |project_(x) - x| / bound %.3e' % float(((again - latent).double().abs() / bound.clamp_min(1e-300)).max()))
    assert bool(((again - latent).double().abs() <= bound).all())
