"""gc_pairwise_f32 on the GPU (csrc/pairwise.hip through models/op/pairwise.py).

Every case runs on fp32 inputs against the formula restated here in float64 on the upcast inputs,

    ABS: D64[i, j] = sum_k |S[i, k] - Q[j, k]| / K          SQ: D64[i, j] = sum_k (S[i, k] - Q[j, k])^2

with the DERIVED elementwise bound |D - D64| <= (K + 4) * 2^-24 * D64: every term is non-negative, so any summation order of K float32 terms is
within (K - 1) u of the exact sum relative to the sum; the subtraction, the square (or the absolute value: exact) and the final division add
at most one u each.  The bound is loose at large K, so the small-K cases are the ones that catch a dropped or doubled element.  Every call runs
on guard-banded, poisoned outputs and workspaces and on inputs with hostile surroundings (tests/guarded_alloc.py): NaN sits past each row's
K-th element, between strided rows and around the buffers, so an over-read reaches the result.  Measured errors: profiles/separability.md.

Shapes: m, n in {1, 2, 7, 63, 64, 65, 130} on each side (the 64-wide tile), 129 / 257 (the 128-wide tile), n in {15, 16, 17} (the 16 columns of
a finish workgroup); K in {1, 3, 4, 5, 31, 32, 33} (the 32-column chunk, the 16-byte path), 127, 480 / 481 / 512 (a split along K needs 16 chunks:
K > 480), 1029, 25088 .. 25092 (128-wide tiles on both load paths, with and without a ragged last chunk) and one 20 x 20 x 200704 long-row case;
row strides K, K + 1 and 2 K (features[::2] read in place).
"""
import numpy as np
import pytest
import torch

import guarded_alloc

from gan_control_amd import _lib
from gan_control_amd.models.op import _backend
from gan_control_amd.models.op import pairwise as pw

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24

# (m, n, K, row stride)
CASES = [(1, 1, 1, 'k'), (2, 7, 3, 'k'), (7, 2, 4, 'k+1'), (63, 65, 5, '2k'), (64, 63, 31, 'k'), (65, 64, 32, 'k'), (130, 1, 33, 'k+1'),
         (1, 130, 127, '2k'), (7, 16, 480, 'k'), (17, 7, 481, 'k+1'), (3, 15, 4, 'k'), (3, 17, 4, '2k'), (64, 130, 512, 'k'), (130, 65, 512, '2k'),
         (63, 2, 1029, 'k'), (2, 63, 1029, '2k'), (65, 130, 25088, 'k'), (130, 130, 25088, 'k'), (130, 130, 25088, 'k+1'), (129, 257, 25092, 'k'),
         (130, 129, 25091, 'k'), (7, 15, 25088, '2k'), (20, 20, 200704, 'k')]


def strided(rows, k, stride, gen, integer=False):
    """[rows, k] values as a view with the row stride of the case (the bytes between rows are replaced by hostile())."""
    width = {'k': k, 'k+1': k + 1, '2k': 2 * k}[stride]
    base = torch.randint(-8, 9, (rows, width), generator=gen).float() if integer else torch.randn(rows, width, generator=gen)
    base = base.to(DEV)
    if stride == '2k':
        return base.view(2 * rows, k)[::2]
    return base[:, :k]


def formula64(s, q, mode):
    """The float64 restatement, a few signature rows at a time."""
    s64, q64 = s.double(), q.double()
    k = s.shape[1]
    step = max(1, (1 << 24) // (q.shape[0] * k))
    rows = []
    for i in range(0, s.shape[0], step):
        d = s64[i:i + step, None, :] - q64[None, :, :]
        rows.append(d.abs().sum(-1) / k if mode == 'abs' else (d * d).sum(-1))
    return torch.cat(rows, 0)


def pids_of(m, n):
    """Repeated pids on both sides; every query has a signature of another pid."""
    s = np.arange(m) % 5
    q = (np.arange(n) * 3) % 5 + (1 if m == 1 else 0)
    return s, q


def run(s, q, mode, pids=None, poison='nan', fill='nan', shift=0):
    """One pairwise_distances call on guarded outputs and hostile copies of the inputs -> (result, entries)."""
    hs, hq = guarded_alloc.hostile(s, fill, shift), guarded_alloc.hostile(q, fill, shift)
    with torch.no_grad(), guarded_alloc.guarded(pw, poison=poison) as guard:
        out = pw.pairwise_distances(hs, hq, mode) if pids is None else pw.pairwise_distances(hs, hq, mode, *pids)
        assert guard.check() == []
    assert guarded_alloc.hostile_changes(hs, s) is None and guarded_alloc.hostile_changes(hq, q) is None
    return out, guard.entries


def check_minima(d, best, best_idx, s_pid, q_pid):
    """best / best_idx are min and FIRST argmin of the returned matrix over the rows with another pid, exactly."""
    dn, bn, idx = d.cpu().numpy(), best.cpu().numpy(), best_idx.cpu().numpy()
    for j in range(dn.shape[1]):
        rows = np.nonzero(s_pid != q_pid[j])[0]
        col = dn[rows, j]
        assert bn[j] == col.min() and idx[j] == rows[np.argmin(col)], (j, bn[j], col.min(), idx[j], rows[np.argmin(col)])


@pytest.mark.parametrize('mode', ['abs', 'sq'])
@pytest.mark.parametrize('m,n,k,stride', CASES)
def test_kernel_against_the_float64_formula(m, n, k, stride, mode):
    gen = torch.Generator().manual_seed(1000 * m + 10 * n + k % 997)
    s, q = strided(m, k, stride, gen), strided(n, k, stride, gen)
    pids = pids_of(m, n)
    (d, best, best_idx), entries = run(s, q, mode, pids)
    assert entries == [pw.ENTRY] and d.shape == (m, n) and d.is_contiguous()
    ref = formula64(s, q, mode)
    err = float(((d.double() - ref).abs() / ref.clamp_min(1e-300)).max())
    print('pairwise %-3s m=%-3d n=%-3d K=%-6d stride %-3s  max relative error %.3e  (bound %.3e)' % (mode, m, n, k, stride, err, (k + 4) * U))
    assert bool(((d.double() - ref).abs() <= (k + 4) * U * ref).all()), err
    check_minima(d, best, best_idx, *pids)
    # the same bytes again, without the pids too, and on the other poison / fill at another alignment (the 4-byte load path where the first
    # run took 16-byte loads: both stage the same images, so the sums are the same sums)
    (d2, best2, idx2), _ = run(s, q, mode, pids)
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32)) and torch.equal(best.view(torch.int32), best2.view(torch.int32)) and torch.equal(best_idx, idx2)
    d3, entries = run(s, q, mode)
    assert entries == [pw.ENTRY] and torch.equal(d.view(torch.int32), d3.view(torch.int32))
    (d4, best4, idx4), _ = run(s, q, mode, pids, poison='big', fill='big', shift=4)
    assert torch.equal(d.view(torch.int32), d4.view(torch.int32)) and torch.equal(best, best4) and torch.equal(best_idx, idx4)


@pytest.mark.parametrize('mode', ['abs', 'sq'])
@pytest.mark.parametrize('k', [33, 1029])
def test_one_element_a_million_times_the_rest(k, mode):
    gen = torch.Generator().manual_seed(k)
    s, q = strided(9, k, 'k', gen), strided(66, k, 'k+1', gen)
    s[3, k - 1] = 1e6
    d, _ = run(s, q, mode)
    ref = formula64(s, q, mode)
    assert bool(((d.double() - ref).abs() <= (k + 4) * U * ref).all())
    assert float(d[3].min()) > 100 * float(d[2].max())


@pytest.mark.parametrize('mode,m,n,k,stride', [('sq', 65, 66, 127, 'k'), ('sq', 7, 130, 1029, 'k+1'), ('sq', 130, 130, 25088, 'k'), ('abs', 64, 65, 512, '2k'),
                                               ('abs', 7, 3, 4, 'k'), ('abs', 3, 70, 1, 'k'), ('abs', 9, 9, 32, 'k+1'), ('abs', 20, 21, 1024, 'k')])
def test_integer_inputs_equal_the_torch_path_bit_for_bit(mode, m, n, k, stride):
    """Sums of small integers are exact in any order (below 2^24) and a division by a power of two is exact: SQ at any K, ABS at K = 2^p."""
    gen = torch.Generator().manual_seed(k + m)
    s, q = strided(m, k, stride, gen, integer=True), strided(n, k, stride, gen, integer=True)
    pids = pids_of(m, n)
    (d, best, best_idx), entries = run(s, q, mode, pids)
    assert entries == [pw.ENTRY]
    with torch.no_grad():
        want = pw.chunked_distances(s, q, pw._mode_fn(mode))
    assert torch.equal(d.view(torch.int32), want.view(torch.int32))
    check_minima(d, best, best_idx, *pids)          # (integer distances tie often: the FIRST row of a tie is the one reported)
    tb, ti = pw.masked_minima(want, *pw.pid_codes(*pids, m, n))
    assert torch.equal(best, tb) and torch.equal(best_idx, ti)


def test_feature_maps_and_even_odd_views_are_read_in_place():
    gen = torch.Generator().manual_seed(5)
    f = torch.randn(14, 3, 5, 7, generator=gen).to(DEV)
    (d, best, best_idx), entries = run(f[::2], f[1::2], 'abs', (np.arange(7), np.arange(7)))
    assert entries == [pw.ENTRY]
    ref = formula64(f[::2].reshape(7, -1), f[1::2].reshape(7, -1), 'abs')
    assert bool(((d.double() - ref).abs() <= (105 + 4) * U * ref).all())
    check_minima(d, best, best_idx, np.arange(7), np.arange(7))


def _raw(s, s_stride, q, q_stride, m, n, k, mode, d, sp=None, qp=None, best=None, idx=None, ws=None, ws_bytes=0):
    _backend.get()._launch(q.device, pw.ENTRY, _lib.ptr(s), s_stride, _lib.ptr(q), q_stride, m, n, k, mode, _lib.ptr(d), _lib.ptr(sp), _lib.ptr(qp),
                           _lib.ptr(best), _lib.ptr(idx), _lib.ptr(ws), ws_bytes, _lib.stream_of(q))


def test_bad_arguments_are_refused_before_any_launch():
    x = torch.zeros(20, 200704, device=DEV)
    d = torch.full((20, 20), 3.0, device=DEV)
    pid = torch.zeros(20, dtype=torch.int32, device=DEV)
    best, idx = torch.zeros(20, device=DEV), torch.zeros(20, dtype=torch.int32, device=DEV)
    for word, call in (('null pointer', lambda: _raw(None, 8, x, 8, 4, 4, 8, 0, d)), ('null pointer', lambda: _raw(x, 8, x, 8, 4, 4, 8, 0, None)),
                       ('at least 1', lambda: _raw(x, 8, x, 8, 0, 4, 8, 0, d)), ('at least 1', lambda: _raw(x, 8, x, 8, 4, 4, 0, 1, d)),
                       ('shorter than the rows', lambda: _raw(x, 7, x, 8, 4, 4, 8, 0, d)), ('unknown mode 2', lambda: _raw(x, 8, x, 8, 4, 4, 8, 2, d)),
                       ('go together', lambda: _raw(x, 8, x, 8, 4, 4, 8, 0, d, sp=pid, best=best, idx=idx)),
                       ('best / best_idx', lambda: _raw(x, 8, x, 8, 4, 4, 8, 0, d, sp=pid, qp=pid)),
                       ('workspace too small', lambda: _raw(x, 200704, x, 200704, 20, 20, 200704, 0, d)),
                       ('workspace too small', lambda: _raw(x, 200704, x, 200704, 20, 20, 200704, 0, d, ws=x, ws_bytes=1024))):
        with pytest.raises(RuntimeError, match=word):
            call()
    torch.cuda.synchronize()
    assert bool((d == 3.0).all())
    lib = _lib.load()
    assert lib.gc_pairwise_workspace(20, 20, 200704) > 0 and lib.gc_pairwise_workspace(20, 20, 64) == 0 and lib.gc_pairwise_workspace(0, 20, 64) == 0
    _raw(x, 8, x, 8, 4, 4, 8, 0, d)          # the same call within the rules runs: equal rows are at distance zero
    torch.cuda.synchronize()
    assert bool((d.view(-1)[:16] == 0).all()) and bool((d.view(-1)[16:] == 3.0).all())


def test_query_without_a_not_same_signature_raises_before_any_launch():
    s, q = torch.randn(3, 8, device=DEV), torch.randn(4, 8, device=DEV)
    with guarded_alloc.guarded(pw) as guard:
        with pytest.raises(ValueError, match='query 2'):
            pw.pairwise_distances(s, q, 'sq', np.array([7, 7, 7]), np.array([1, 2, 7, 3]))
    assert guard.entries == [] and guard.allocations == []


def entries_of(fn):
    with guarded_alloc.guarded(pw) as guard:
        out = fn()
        assert guard.check() == []
    return out, guard.entries


def test_operator_dispatch():
    """Which inputs launch the entry (module docstring of models/op/pairwise.py) -- and that nothing else started to."""
    gen = torch.Generator().manual_seed(3)
    s, q = torch.randn(6, 24, generator=gen).to(DEV), torch.randn(5, 24, generator=gen).to(DEV)
    with torch.no_grad():
        want, e = entries_of(lambda: pw.pairwise_distances(s, q, 'abs'))
        assert e == [pw.ENTRY]
        for a, b in ((s.view(6, 2, 3, 4), q.view(5, 2, 3, 4)), (s.repeat_interleave(2, 0)[::2], q), (torch.cat([s, s], 1)[:, :24], q)):
            got, e = entries_of(lambda: pw.pairwise_distances(a, b, 'abs'))
            assert e == [pw.ENTRY] and torch.equal(got, want)
        chunked = pw.chunked_distances(s, q, pw._mode_fn('abs'))
        for a, b, kw in ((s.double(), q.double(), {}), (s.cpu(), q.cpu(), {}), (torch.cat([s, s], 1)[:, ::2], torch.cat([q, q], 1)[:, ::2], {}),
                         (s[:1].expand(6, 24), q, {}), (s.view(6, 4, 6).transpose(1, 2), q.view(5, 4, 6).transpose(1, 2), {}),
                         (s, q, {'criterion': pw._mode_fn('abs')})):
            got, e = entries_of(lambda: pw.pairwise_distances(a, b, 'abs', **kw))
            assert pw.ENTRY not in e and got.shape == (6, 5)
        got, e = entries_of(lambda: pw.pairwise_distances(s, q, 'abs', criterion=pw._mode_fn('abs')))
        assert torch.equal(got, chunked) and float((got - want).abs().max()) <= 2 * 28 * U * float(want.max())
        sg = s.clone().requires_grad_(True)
        _, e = entries_of(lambda: pw.pairwise_distances(sg, q, 'sq'))          # grad mode is off: nothing is wanted
        assert e == [pw.ENTRY]
    sg = s.clone().requires_grad_(True)
    got, e = entries_of(lambda: pw.pairwise_distances(sg, q, 'sq'))
    assert pw.ENTRY not in e and got.requires_grad
    got.sum().backward()
    assert sg.grad is not None and bool(torch.isfinite(sg.grad).all())
    with pytest.raises(ValueError, match='matrix'):
        pw.pairwise_distances(s.view(6, 2, 3, 4), q.view(5, 2, 3, 4), None, criterion=lambda a, b: (a.unsqueeze(1) - b.unsqueeze(0)).pow(2).sum(-1))


def test_existing_callers_launch_what_they_launched():
    """The mini-batch loss and a training iteration do not reach the new entry; LossModelClass.calc_distances does."""
    from gan_control_amd.losses import LossModelClass, L1Expend
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    cfg = {'lower_thres': [0.1], 'upper_thres': [0.2], 'last_lower_thres': 0.5, 'last_upper_thres': 1.8, 'intermediate_layers_weights': [1.0],
           'last_layer_weight': 0.25, 'focus_on_list': ['not_same_as_last_layer', 'same_as_last_layer']}
    lm = LossModelClass(cfg, 'embedding_loss', mini_batch_size=4, no_model=True)
    gen = torch.Generator().manual_seed(2)
    feats = [torch.randn(4, 3, 5, 5, generator=gen).to(DEV), torch.randn(4, 16, generator=gen).to(DEV)]
    _, e = entries_of(lambda: lm.calc_mini_batch_loss([f[:2] for f in feats], [f[2:] for f in feats]))
    assert pw.ENTRY not in e
    d, e = entries_of(lambda: lm.calc_distances(feats[0], feats[0], L1Expend()))
    assert e == [pw.ENTRY] and d.shape == (4, 4)
    tr = GeneratorTrainer(default_config(32, 4), device=DEV, seed=0, fused_adam=False)
    _, e = entries_of(lambda: tr.train(iters=1))
    assert len(e) > 50 and pw.ENTRY not in e
