"""gc_feature_moments_accumulate_f32 / _finish_f64 / _merge_f64 on the GPU (csrc/feature_stats.hip through models/op/feature_moments.py),
FeatureStats on the device and evaluate_fid(streaming=True, method='eigh') end to end.

Every kernel call runs on guard-banded, poisoned buffers (tests/guarded_alloc.py, both poisons; the accumulator comes from the module's
own ``zeros``) and on hostile() copies of the features (NaN -- or 1e30 -- between strided rows and around the buffer) at shift 0 (16-byte
loads) and shift 4 (4-byte loads): the results of the two must be the same bits, so the edge tiles and the K tail read nothing outside the
rows.

Shapes: the output tile is T = 64, one MFMA consumes K = 4 rows (whole K steps past the last row are skipped) and 32 rows are staged per
chunk; F sits on both sides of 16 (one MFMA block), T and 2 T, n on both sides of 4 and, at 67, past two chunks; F = 2048 is the workload's
width, n = 1031 walks 33 chunks.

Derived elementwise bound (include/gancontrol_stats.h), u = 2^-53, gamma_n = n u / (1 - n u), P_ij = sum_k |x_ki x_kj|, A_i = sum_k |x_ki|.
Products of widened floats are exact, and a sum of n terms in ANY order is within gamma_n of the sum of their magnitudes, so
    |s2 - exact| <= gamma_n P,      |s1 - exact| <= gamma_n A
for the kernel and for the float64 formula ``xd.T @ xd`` / ``xd.sum(0)`` alike: the tolerance is the sum of the two, 2 gamma_n P and
2 gamma_n A.  Finish adds four roundings: |cov - exact| <= (2 gamma_n + 8 u)(P + A_i A_j / n) / (n - 1), |mean - exact| <= (gamma_n + u) A / n.
The two-pass reference (np.mean, np.cov): its mean is within (gamma_n + u) A_i / n; the centred values satisfy sum_k |c_ki c_kj| <= P + 3 A_i A_j / n,
their sum of products adds gamma_n of that, the centring, the division and the mean's own error (at most (gamma_n + u) A_i / n times
sum_k |c_kj| <= 2 A_j, twice) fit in (gamma_n + 4 u)(P + 7 A_i A_j / n) / (n - 1).  The cov tolerance is the sum of the kernel's and the reference's.
"""
import pickle

import numpy as np
import pytest
import torch

import guarded_alloc
import stream_order as so
from feature_stats_checks import bounds, fid_tolerance

from gan_control_amd import _lib
from gan_control_amd.fid_utils import fid as fid_module
from gan_control_amd.fid_utils.feature_stats import FeatureStats
from gan_control_amd.models.op import _backend
from gan_control_amd.models.op import feature_moments as fm

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = fm.TILE
WIDTHS = [1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3]
ROWS = [1, 3, 4, 5, 67]
# (68, 132: F % 4 == 0 with a ragged last tile -- 16-byte loads whose column clamp works at a non-zero tile column)
CASES = [(f, n) for f in WIDTHS for n in ROWS] + [(2048, 40), (130, 1031), (68, 5), (132, 67)]


def features(n, f, seed, kind='d'):
    """[n, f] float32 on the device: dense ('d'), every second row of a [2 n, f] buffer ('2d') or the first f columns of rows f + 5 apart ('p')."""
    gen = torch.Generator().manual_seed(seed)
    width = {'d': f, '2d': 2 * f, 'p': f + 5}[kind]
    base = (torch.randn(n, width, generator=gen) * 1.5 + 0.5).to(DEV)
    return base.view(2 * n, f)[::2] if kind == '2d' else base[:, :f]


def bits(t):
    return t.contiguous().view(torch.int64)


def upper(s2):
    return torch.triu(s2)


def run(chunks, poison='nan', fill='nan', shift=0):
    """Append every chunk to a fresh accumulator and finish it (n >= 2) under the guards.  -> (s1, s2, mean | None, cov | None, entries)."""
    n = sum(c.shape[0] for c in chunks)
    hostile = [guarded_alloc.hostile(c, fill, shift) for c in chunks]
    with torch.no_grad(), guarded_alloc.guarded(fm, poison=poison) as guard:
        s1, s2 = fm.new_accumulator(chunks[0].shape[1], DEV)
        for h in hostile:
            assert fm.kernel_taken(s1, s2, h)
            fm.accumulate_(s1, s2, h)
        mean, cov = fm.finish(s1, s2, n) if n >= 2 else (None, None)
        assert guard.check() == []
    for h, c in zip(hostile, chunks):
        assert guarded_alloc.hostile_changes(h, c) is None
    return s1, s2, mean, cov, guard.entries


def check_against_formulas(x, s1, s2, mean, cov, tag):
    x64 = x.cpu().numpy().astype(np.float64)
    n = x64.shape[0]
    t1, t2, tm, tc = bounds(x64)
    e1 = np.abs(s1.cpu().numpy() - x64.sum(0))
    e2 = np.triu(np.abs(s2.cpu().numpy() - x64.T @ x64))
    line = '%s n=%-4d F=%-4d  s1 error / bound %.3e  s2 error / bound %.3e' % (tag, n, x64.shape[1], float((e1 / t1).max()), float((e2 / t2).max()))
    ok = bool(np.all(e1 <= t1) and np.all(e2 <= t2))
    if mean is not None:
        em = np.abs(mean.cpu().numpy() - x64.mean(0))
        ec = np.abs(cov.cpu().numpy() - np.cov(x64, rowvar=False).reshape(x64.shape[1], x64.shape[1]))
        line += '  mean error / bound %.3e  cov error / bound %.3e' % (float((em / tm).max()), float((ec / tc).max()))
        ok = ok and bool(np.all(em <= tm) and np.all(ec <= tc))          # the whole matrix: the lower triangle is filled
        assert torch.equal(bits(cov), bits(cov.T))          # exactly symmetric
    print(line)
    assert ok, line


@pytest.mark.parametrize('f,n', CASES)
def test_moments_against_the_float64_formulas(f, n):
    x = features(n, f, 31 * f + n)
    s1, s2, mean, cov, entries = run([x])
    assert entries == [fm.ACCUMULATE_ENTRY] + ([fm.FINISH_ENTRY] if n >= 2 else [])
    check_against_formulas(x, s1, s2, mean, cov, 'moments')
    again = run([x])          # the same calls: the same bits
    other = run([x], poison='big', fill='big', shift=4)          # other poison, other surroundings, 4-byte loads: the same bits
    for got in (again, other):
        assert torch.equal(bits(s1), bits(got[0])) and torch.equal(bits(upper(s2)), bits(upper(got[1])))
        if n >= 2:
            assert torch.equal(bits(mean), bits(got[2])) and torch.equal(bits(cov), bits(got[3]))


@pytest.mark.parametrize('f,n,kind', [(T + 1, 67, '2d'), (T + 1, 67, 'p'), (130, 20, '2d'), (17, 5, 'p'), (2048, 20, '2d'), (132, 67, '2d'), (68, 5, '2d')])
def test_strided_rows_are_read_in_place(f, n, kind):
    x = features(n, f, 5 * f + n, kind)
    assert not x.is_contiguous() and fm.kernel_taken(*fm.new_accumulator(f, DEV), x)
    dense = run([x.contiguous()])
    for shift in (0, 4):
        got = run([x], shift=shift)
        assert got[4] == dense[4]
        assert torch.equal(bits(got[0]), bits(dense[0])) and torch.equal(bits(upper(got[1])), bits(upper(dense[1])))
        assert torch.equal(bits(got[2]), bits(dense[2])) and torch.equal(bits(got[3]), bits(dense[3]))


@pytest.mark.parametrize('f,n,step', [(T + 1, 67, 1), (T + 1, 67, 3), (2 * T + 3, 67, 20), (2048, 40, 20)])
def test_chunked_appends_keep_the_accumulator(f, n, step):
    """Append, then append again: the accumulator equals the formula on the concatenation, within the bound of n rows."""
    x = features(n, f, 7 * f + step)
    chunks = list(x.split(step))
    s1, s2, mean, cov, entries = run(chunks)
    assert entries == [fm.ACCUMULATE_ENTRY] * len(chunks) + [fm.FINISH_ENTRY]
    check_against_formulas(x, s1, s2, mean, cov, 'chunks of %d' % step)
    again = run(chunks, poison='big', fill='big', shift=4)
    assert torch.equal(bits(s1), bits(again[0])) and torch.equal(bits(cov), bits(again[3]))


@pytest.mark.parametrize('f,n', [(1, 5), (T - 1, 67), (2 * T + 3, 67), (2048, 40)])
def test_merge_of_two_halves(f, n):
    x = features(n, f, 11 * f + n)
    a, b = x[:n // 2], x[n // 2:]
    sa, sb = run([a]), run([b])
    s1a, s2a, s1b, s2b = sa[0].clone(), sa[1].clone(), sb[0], sb[1]
    below = torch.tril(torch.ones(f, f, dtype=torch.bool, device=DEV), -1)
    s2a[below] = 7.0          # what is below the diagonal is not part of the accumulator: merge keeps its bits, finish never reads it
    s2b = torch.where(below, torch.full_like(s2b, float('nan')), s2b)
    with torch.no_grad(), guarded_alloc.guarded(fm) as guard:
        assert fm.kernel_taken(s1a, s2a, other=(s1b, s2b))
        fm.merge_(s1a, s2a, s1b, s2b)
        mean, cov = fm.finish(s1a, s2a, n)
        assert guard.check() == []
    assert guard.entries == [fm.MERGE_ENTRY, fm.FINISH_ENTRY]
    assert bool((s2a[below] == 7.0).all())
    check_against_formulas(x, s1a, s2a, mean, cov, 'merge')
    # ... and through FeatureStats
    st = FeatureStats.from_features(a).merge_(FeatureStats.from_features(b))
    assert st.n == n and torch.equal(bits(st.cov()), bits(cov)) and torch.equal(bits(st.mean()), bits(mean))


def test_dispatch_and_limits():
    s1, s2 = fm.new_accumulator(24, DEV)
    x = features(6, 24, 1)
    assert fm.kernel_taken(s1, s2, x) and fm.kernel_taken(s1, s2) and fm.kernel_taken(s1, s2, other=(s1.clone(), s2.clone()))
    assert not fm.kernel_taken(s1, s2, x.double()) and not fm.kernel_taken(s1, s2, x.cpu()) and not fm.kernel_taken(s1.cpu(), s2.cpu(), x.cpu())
    assert not fm.kernel_taken(s1, s2, torch.cat([x, x], 1)[:, ::2]) and not fm.kernel_taken(s1.float(), s2.float(), x)
    big = fm.new_accumulator(fm.MAX_FEATURES + 1, DEV)
    assert not fm.kernel_taken(*big)
    with guarded_alloc.guarded(fm) as guard:
        fm.accumulate_(s1, s2, x[:0])          # b = 0: nothing
        fm.accumulate_(s1, s2, x.double())          # another dtype: the formula
    assert guard.entries == []
    assert float((s1.cpu() - x.double().sum(0).cpu()).abs().max()) <= 1e-12
    with pytest.raises(ValueError, match='at least 2'):
        fm.finish(s1, s2, 1)
    # the entries refuse what they do not build, before any launch
    launch = _backend.get()._launch
    m, c = torch.full((24,), 3.0, dtype=torch.float64, device=DEV), torch.full((24, 24), 3.0, dtype=torch.float64, device=DEV)
    keep1, keep2 = s1.clone(), s2.clone()
    st = _lib.stream_of(x)
    for word, entry, args in (('null pointer', fm.ACCUMULATE_ENTRY, (None, 24, 6, 24, _lib.ptr(s1), _lib.ptr(s2), st)),
                              ('at least 1', fm.ACCUMULATE_ENTRY, (_lib.ptr(x), 24, 0, 24, _lib.ptr(s1), _lib.ptr(s2), st)),
                              ('at least 1', fm.ACCUMULATE_ENTRY, (_lib.ptr(x), 24, 6, 0, _lib.ptr(s1), _lib.ptr(s2), st)),
                              ('elements apart', fm.ACCUMULATE_ENTRY, (_lib.ptr(x), 23, 6, 24, _lib.ptr(s1), _lib.ptr(s2), st)),
                              ('at most 4096', fm.ACCUMULATE_ENTRY, (_lib.ptr(x), 4097, 1, 4097, _lib.ptr(s1), _lib.ptr(s2), st)),
                              ('at least 2', fm.FINISH_ENTRY, (_lib.ptr(s1), _lib.ptr(s2), 1, 24, _lib.ptr(m), _lib.ptr(c), st)),
                              ('at most 4096', fm.FINISH_ENTRY, (_lib.ptr(s1), _lib.ptr(s2), 9, 4097, _lib.ptr(m), _lib.ptr(c), st)),
                              ('null pointer', fm.MERGE_ENTRY, (_lib.ptr(s1), _lib.ptr(s2), None, _lib.ptr(s2), 24, st))):
        with pytest.raises(RuntimeError, match=word):
            launch(x.device, entry, *args)
    with pytest.raises(_lib.UnsupportedError):
        launch(x.device, fm.ACCUMULATE_ENTRY, _lib.ptr(x), 4097, 1, 4097, _lib.ptr(s1), _lib.ptr(s2), st)
    torch.cuda.synchronize()
    assert torch.equal(s1, keep1) and torch.equal(s2, keep2) and bool((m == 3.0).all()) and bool((c == 3.0).all())


# ---- side stream behind late inputs -------------------------------------------------------------------------------------------------

def _late(name, entry, tensors, call):
    held = so.snapshot(tensors)
    plain = so.clone_outs(call())
    torch.cuda.synchronize()
    late = so.late_run(held, call, [fm])
    print('%s: entries %s, %s, issued in %.3f ms' % (name, late.entries, 'CONCLUSIVE' if late.conclusive else 'inconclusive', late.issue_ms))
    assert late.entries == [entry]
    assert late.conclusive, '%s: the inputs were restored before the call returned on the host: the run proves nothing' % name
    diff = so.difference(plain, late.outs)
    assert diff is None, '%s behind late inputs on a side stream: %s -- a launch did not go to the current stream' % (name, diff)


def test_every_entry_on_a_side_stream_behind_late_inputs():
    assert _backend.get().name == 'hip'
    so.calibrate()
    so.side_stream()
    f, n = 2 * T + 3, 67
    x = features(n, f, 3)
    first = features(21, f, 4)
    with torch.no_grad():
        s1, s2 = fm.new_accumulator(f, DEV)
        fm.accumulate_(s1, s2, first)          # the accumulator is an input of every call: it holds rows already
        o1, o2 = fm.new_accumulator(f, DEV)
        fm.accumulate_(o1, o2, x)
        torch.cuda.synchronize()
        _late('accumulate_', fm.ACCUMULATE_ENTRY, {'x': x, 's1': s1, 's2': s2}, lambda: list(fm.accumulate_(s1, s2, x)))
        _late('finish', fm.FINISH_ENTRY, {'s1': s1, 's2': s2}, lambda: list(fm.finish(s1, s2, n + 21)))
        _late('merge_', fm.MERGE_ENTRY, {'s1': s1, 's2': s2, 'o1': o1, 'o2': o2}, lambda: list(fm.merge_(s1, s2, o1, o2)))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def test_streaming_eigh_fid_end_to_end(tmp_path):
    """evaluate_fid(streaming=True, method='eigh') on the generator / feature-net pair of tests/test_fid.py against the default call on the same
    seed: the same draws, the same images and features; five accumulate launches and one finish; no feature batch reaches the host.  Tolerance:
    against the eigen form on the host statistics of the same features, what the moment bound propagates to (feature_stats_checks.fid_tolerance);
    against the default call, that plus what sqrtm itself is good for -- 1e-6 of the traces, the tolerance tests/test_fid.py gives the
    reference form for a distance that is 0."""
    from gan_control_amd.models.gan_model import Generator
    torch.manual_seed(3)
    g = Generator(32, 512, 2, channel_multiplier=2, conv_transpose=True, fc_config=None).cuda().eval()
    pool = torch.nn.AdaptiveAvgPool2d(4)
    net = lambda img: (pool(img),)
    gen = torch.Generator().manual_seed(6)
    real = (torch.randn(150, 48, generator=gen) * 0.2).double().numpy()
    rm, rc = fid_module.feature_statistics(real)
    path = str(tmp_path / 'real.pkl')
    with open(path, 'wb') as fh:
        pickle.dump({'mean': rm, 'cov': rc}, fh)
    torch.manual_seed(1)
    want = fid_module.evaluate_fid(g, net, 20, 100, DEV, path)
    state = torch.cuda.get_rng_state()
    torch.manual_seed(1)
    feats = fid_module.sample_features(g, net, 20, 100, DEV)
    moved = []
    real_to = torch.Tensor.to

    def to(t, *a, **k):
        out = real_to(t, *a, **k)
        if t.is_cuda and not out.is_cuda:
            moved.append(tuple(t.shape))
        return out

    torch.manual_seed(1)
    with guarded_alloc.guarded(fm) as guard:
        torch.Tensor.to = to
        try:
            got = fid_module.evaluate_fid(g, net, 20, 100, DEV, path, streaming=True, method='eigh')
        finally:
            torch.Tensor.to = real_to
        assert guard.check() == []
    assert torch.equal(torch.cuda.get_rng_state(), state)          # the same draws were consumed
    mine = (fm.ACCUMULATE_ENTRY, fm.FINISH_ENTRY, fm.MERGE_ENTRY)          # (the generator's own launches are recorded too)
    assert [e for e in guard.entries if e in mine] == [fm.ACCUMULATE_ENTRY] * 5 + [fm.FINISH_ENTRY]
    assert (20, 48) not in moved and (100, 48) not in moved, moved
    mean, cov = fid_module.feature_statistics(feats.numpy())
    scale = float(np.trace(cov) + np.trace(rc))
    same_stats = fid_module.frechet_distance_eigh(mean, cov, rm, rc)
    _, _, tm, tc = bounds(feats.numpy().astype(np.float64))
    tol = fid_tolerance(tm, tc, cov, rc, mean - rm)
    print('streaming + eigh %.12g, default %.12g, eigh on host statistics %.12g, traces %.6g, propagated moment bound %.3e'
          % (got, want, same_stats, scale, tol))
    assert np.isfinite(got) and abs(got - same_stats) <= tol and abs(got - want) <= 1e-6 * scale + tol
