"""gc_knn_radius_f32, gc_manifold_hits_f32 and gc_poly_mmd_f32 on the GPU (csrc/manifold.hip through models/op/manifold.py).

Every case runs on fp32 inputs against the formulas restated in float64 on the upcast inputs (tests/quality_refs.py), u = 2^-24:

* radii: |radius2 - ref| <= (F + 4) u ref.  DERIVED: every term of a squared distance is non-negative, so any order of F float32 terms is
  within (F - 1) u of the exact sum relative to it, the subtraction and the square add one u each, and an order statistic of values that are
  each perturbed by a relative e moves by at most e;
* hits: with e = 3 (F + 4) u (radius and distance each carry (F + 4) u) a decision is undecided when any(D64 <= r64 (1 - e)) differs from
  any(D64 <= r64 (1 + e)); every other decision equals the float64 one exactly, from the one-pass call and from the probe-only call, and at
  most 2 % of a case's decisions may be undecided (the float64 reference alone: at most 0.8 % on these inputs, tests/test_quality_metrics.py
  prints them);
* KID sums: within 3 (F + 3) u relative -- the products are non-negative, so the dot product is within (F + 1) u, the division adds to it and the cube
  triples the total; everything behind the dot product is float64.  The KID value is then within 3 (F + 3) u (A + B) of its float64 value A - B;
* integer inputs: distances are exact and tie often, so radii and hits equal the torch path bit for bit (<= against <, the ties of the
  k-smallest merge), and the KID sums equal numpy's float64 exactly.

Every call runs on guard-banded, poisoned outputs and workspaces and on inputs with hostile surroundings (tests/guarded_alloc.py): NaN behind
each row's F-th element, between strided rows and around the buffers; a second run on the other poison at a 4-byte shift (the 4-byte load
path) must give identical bits and intact guards.
"""
import os
import pickle

import numpy as np
import pytest
import torch

import guarded_alloc
import quality_refs as qr
from quality_refs import U

from gan_control_amd import _lib
from gan_control_amd.models.op import _backend
from gan_control_amd.models.op import manifold as mf

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ENTRIES = (mf.KNN_ENTRY, mf.HITS_ENTRY, mf.MMD_ENTRY)


def strided(values, stride):
    """The [rows, F] array on the GPU as a view with the row stride of the case (hostile() replaces the bytes between the rows)."""
    t = torch.from_numpy(np.ascontiguousarray(values)).to(DEV)
    rows, f = t.shape
    width = {'k': f, 'k+1': f + 1, '2k': 2 * f}[stride]
    base = torch.zeros(rows, width, device=DEV)
    base[:, :f] = t
    return base.view(2 * rows, f)[::2] if stride == '2k' else base[:, :f]


def run(fn, inputs, poison='nan', fill='nan', shift=0):
    """fn(*hostile copies of the inputs) on guarded allocations -> (result, entries)."""
    hostile = [guarded_alloc.hostile(t, fill, shift) for t in inputs]
    with torch.no_grad(), guarded_alloc.guarded(mf, poison=poison) as guard:
        out = fn(*hostile)
        assert guard.check() == []
    for h, t in zip(hostile, inputs):
        assert guarded_alloc.hostile_changes(h, t) is None
    return out, guard.entries


def both_runs(fn, inputs):
    """The call on NaN poison, and again on the other poison at a 4-byte shift: the same bits.  -> (result, entries)"""
    out, entries = run(fn, inputs)
    again, _ = run(fn, inputs, poison='big', fill='big', shift=4)
    outs, agains = (out, again) if isinstance(out, tuple) else ((out,), (again,))
    for a, b in zip(outs, agains):
        assert (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)))
    return out, entries


def check_radii(got, ref, f):
    got = got.double().cpu()
    err = float(((got - ref).abs() / ref.clamp_min(1e-300)).max())
    print('  radii: max relative error %.3e (bound %.3e)' % (err, (f + 4) * U))
    assert bool(((got - ref).abs() <= (f + 4) * U * ref).all()), err


def check_hits(got, ref, undecided, name):
    share = float(undecided.double().mean())
    print('  %s: undecided share %.4f, float64 mean %.3f' % (name, share, float(ref.double().mean())))
    assert share <= 0.02, (name, share)
    assert bool((got.cpu() == ref)[~undecided].all()), name


@pytest.mark.parametrize('n_r,n_f,f,kth,stride', qr.DISTANCE_CASES + qr.STRIP_HITS_CASES + [qr.BIG_TILE_HITS_CASE])
def test_radii_and_hits_against_float64(n_r, n_f, f, kth, stride):
    case = qr.distance_case(n_r, n_f, f, kth)
    real, fake = strided(case['real'], stride), strided(case['fake'], stride)
    print('n_r=%d n_f=%d F=%d kth=%d stride %s' % (n_r, n_f, f, kth, stride))
    rr, e = both_runs(lambda a: mf.knn_radii(a, kth), [real])
    assert e == [mf.KNN_ENTRY] and rr.shape == (n_r,) and rr.dtype == torch.float32
    check_radii(rr, case['real_r2'], f)
    fr, e = both_runs(lambda a: mf.knn_radii(a, kth), [fake])
    assert e == [mf.KNN_ENTRY]
    check_radii(fr, case['fake_r2'], f)
    (p_hit, r_hit), e = both_runs(mf.manifold_hits, [real, rr, fake, fr])
    assert e == [mf.HITS_ENTRY] and p_hit.dtype == r_hit.dtype == torch.bool and p_hit.shape == (n_f,) and r_hit.shape == (n_r,)
    check_hits(p_hit, case['probe_hit'], case['probe_undecided'], 'probe_hit')
    check_hits(r_hit, case['ref_hit'], case['ref_undecided'], 'ref_hit')
    (only, none), e = both_runs(mf.manifold_hits, [real, rr, fake])
    assert e == [mf.HITS_ENTRY] and none is None and torch.equal(only, p_hit)          # the probe-only call: the same decisions


@pytest.mark.parametrize('n,f,kth,stride', qr.STRIP_KNN_CASES)
def test_radii_over_more_tiles_than_a_strip_holds(n, f, kth, stride):
    values = qr.feature_set(1, n, 1.0, 0.0, f)
    a = strided(values, stride)
    rr, e = both_runs(lambda t: mf.knn_radii(t, kth), [a])
    assert e == [mf.KNN_ENTRY]
    ref = torch.cat([(a.double()[i:i + 512, None, :] - a.double()[None, :, :]).pow(2).sum(-1).sort(dim=1).values[:, kth] for i in range(0, n, 512)])
    check_radii(rr, ref.cpu(), f)


@pytest.mark.parametrize('n_r,n_f,f,kth,stride', [(65, 66, 127, 3, 'k'), (7, 130, 1029, 1, 'k+1'), (130, 129, 32, 7, '2k'), (300, 257, 5, 3, 'k'),
                                                  (4, 2113, 4, 3, 'k'), (2113, 9, 3, 7, 'k+1'), (2113, 2177, 4, 3, 'k'), (2177, 2113, 3, 1, '2k'),
                                                  (4161, 4225, 4, 7, 'k')])
def test_integer_inputs_equal_the_torch_path_bit_for_bit(n_r, n_f, f, kth, stride):
    gen = torch.Generator().manual_seed(n_r + f)
    real = strided(torch.randint(-8, 9, (n_r, f), generator=gen).float().numpy(), stride)
    fake = strided(torch.randint(-8, 9, (n_f, f), generator=gen).float().numpy(), stride)
    rr, e1 = both_runs(lambda a: mf.knn_radii(a, kth), [real])
    fr, e2 = both_runs(lambda a: mf.knn_radii(a, kth), [fake])
    (p_hit, r_hit), e3 = both_runs(mf.manifold_hits, [real, rr, fake, fr])
    (only, _), _ = both_runs(mf.manifold_hits, [real, rr, fake])
    assert e1 + e2 + e3 == [mf.KNN_ENTRY, mf.KNN_ENTRY, mf.HITS_ENTRY]
    with torch.no_grad():
        want_rr, want_fr = mf.knn_radii_torch(real, kth), mf.knn_radii_torch(fake, kth)
        want_p, want_r = mf.manifold_hits_torch(real, want_rr, fake, want_fr)
    assert torch.equal(rr.view(torch.int32), want_rr.view(torch.int32)) and torch.equal(fr.view(torch.int32), want_fr.view(torch.int32))
    assert torch.equal(p_hit, want_p) and torch.equal(r_hit, want_r) and torch.equal(only, want_p)
    d = (real.double()[:, None, :] - fake.double()[None, :, :]).pow(2).sum(-1)
    print('n_r=%d n_f=%d F=%d kth=%d: %d probe and %d ref hits, %d distances equal to the radius of their row'
          % (n_r, n_f, f, kth, int(want_p.sum()), int(want_r.sum()), int((d == want_rr.double()[:, None]).sum())))


def test_a_tie_is_a_hit():
    ref_v = np.array([[0, 0], [3, 0], [50, 50], [50, 54], [52, 46]], np.float32)
    probe_v = np.array([[0, 3], [0, 3.5], [54, 50], [20, 20], [50, 52]], np.float32)
    sq = lambda a, b: ((a[:, None].astype(np.float64) - b[None]) ** 2).sum(-1)          # (exact: small integers and halves)
    r64, p64, d = np.sort(sq(ref_v, ref_v), 1)[:, 1], np.sort(sq(probe_v, probe_v), 1)[:, 1], sq(ref_v, probe_v)
    assert d[0, 0] == r64[0] and not (d[:, 0] < r64).any()          # probe 0 lies ON the sphere of ref 0 and inside no ball
    assert d[4, 2] == p64[2] and not (d[4] < p64).any()             # ref 4 lies ON the sphere of probe 2 and inside no ball
    ref, probe = torch.from_numpy(ref_v).to(DEV), torch.from_numpy(probe_v).to(DEV)
    r2, _ = both_runs(lambda a: mf.knn_radii(a, 1), [ref])
    p2, _ = both_runs(lambda a: mf.knn_radii(a, 1), [probe])
    assert r2.tolist() == r64.tolist() and p2.tolist() == p64.tolist()
    (p_hit, r_hit), e = both_runs(mf.manifold_hits, [ref, r2, probe, p2])
    assert e == [mf.HITS_ENTRY] and p_hit[0] and r_hit[4]
    assert p_hit.tolist() == (d <= r64[:, None]).any(0).tolist() and r_hit.tolist() == (d <= p64[None, :]).any(1).tolist()


@pytest.mark.parametrize('m,subsets,f,stride', qr.MMD_CASES)
def test_kid_sums_against_float64(m, subsets, f, stride):
    case = qr.mmd_case(m, subsets, f)
    x, y = strided(case['x'], stride), strided(case['y'], stride)
    sums, e = both_runs(lambda a, b: mf.poly_mmd_sums(a, b, case['idx_x'], case['idx_y']), [x, y])
    assert e == [mf.MMD_ENTRY] and sums.dtype == torch.float64 and sums.shape == (subsets, 3)
    got, ref = sums.cpu().numpy(), case['sums']
    err = float((np.abs(got - ref) / ref).max())
    print('m=%d subsets=%d F=%d stride %s: max relative error of the sums %.3e (bound %.3e)' % (m, subsets, f, stride, err, 3 * (f + 3) * U))
    assert (np.abs(got - ref) <= 3 * (f + 3) * U * ref).all(), err
    from gan_control_amd.fid_utils.kid import kid_from_sums
    a, b = qr.kid_parts64(ref, m)
    assert abs(kid_from_sums(got, m) - (a - b)) <= 3 * (f + 3) * U * (a + b)


@pytest.mark.parametrize('m,subsets,f,stride', [(70, 3, 8, 'k'), (130, 2, 64, 'k+1'), (5, 1, 2, '2k')])
def test_kid_sums_of_integer_rows_are_exact(m, subsets, f, stride):
    """Mixed signs, F a power of two: dot / F + 1 has at most log2(F) fraction bits, its cube and every sum of cubes are exact in float64."""
    rs = np.random.RandomState(m)
    xv, yv = rs.randint(-8, 9, (m + 3, f)).astype(np.float32), rs.randint(-8, 9, (m + 4, f)).astype(np.float32)
    idx_x = np.stack([rs.choice(m + 3, m, replace=False) for _ in range(subsets)])
    idx_y = np.stack([rs.choice(m + 4, m, replace=False) for _ in range(subsets)])
    sums, e = both_runs(lambda a, b: mf.poly_mmd_sums(a, b, idx_x, idx_y), [strided(xv, stride), strided(yv, stride)])
    assert e == [mf.MMD_ENTRY]
    assert np.array_equal(sums.cpu().numpy(), qr.mmd_sums64(xv, yv, idx_x, idx_y))


def _launch(entry, *args):
    _backend.get()._launch(torch.device(DEV, torch.cuda.current_device()), entry, *args)


def test_bad_arguments_are_refused_before_any_launch():
    a = torch.zeros(40, 8, device=DEV)
    r2 = torch.ones(40, device=DEV)
    out_f = torch.full((40,), 3.0, device=DEV)
    out_b = torch.full((80,), 3, dtype=torch.uint8, device=DEV)
    out_d = torch.full((6,), 3.0, dtype=torch.float64, device=DEV)
    idx = torch.zeros(8, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p, st, big = _lib.ptr, _lib.stream_of(a), 1 << 16
    knn = lambda *args: _launch(mf.KNN_ENTRY, *args)
    hits = lambda *args: _launch(mf.HITS_ENTRY, *args)
    mmd = lambda *args: _launch(mf.MMD_ENTRY, *args)
    for word, call in (
            ('null pointer', lambda: knn(None, 8, 40, 8, 3, p(out_f), p(ws), big, st)),
            ('null pointer', lambda: knn(p(a), 8, 40, 8, 3, None, p(ws), big, st)),
            ('at least 1', lambda: knn(p(a), 8, 0, 8, 3, p(out_f), p(ws), big, st)),
            ('at least 1', lambda: knn(p(a), 8, 40, 0, 3, p(out_f), p(ws), big, st)),
            ('kth 0 is outside', lambda: knn(p(a), 8, 40, 8, 0, p(out_f), p(ws), big, st)),
            ('kth 8 is outside', lambda: knn(p(a), 8, 40, 8, 8, p(out_f), p(ws), big, st)),
            ('no neighbour number 3', lambda: knn(p(a), 8, 3, 8, 3, p(out_f), p(ws), big, st)),
            ('shorter than the rows', lambda: knn(p(a), 7, 40, 8, 3, p(out_f), p(ws), big, st)),
            ('workspace too small', lambda: knn(p(a), 8, 40, 8, 3, p(out_f), None, 0, st)),
            ('workspace too small', lambda: knn(p(a), 8, 40, 8, 3, p(out_f), p(ws), 40 * 4 * 4 - 1, st)),
            ('null pointer', lambda: hits(None, 8, p(r2), 40, p(a), 8, p(r2), 40, 8, p(out_b), p(out_b) + 40, p(ws), big, st)),
            ('null pointer', lambda: hits(p(a), 8, None, 40, p(a), 8, p(r2), 40, 8, p(out_b), p(out_b) + 40, p(ws), big, st)),
            ('null pointer', lambda: hits(p(a), 8, p(r2), 40, p(a), 8, p(r2), 40, 8, None, p(out_b) + 40, p(ws), big, st)),
            ('at least 1', lambda: hits(p(a), 8, p(r2), 0, p(a), 8, p(r2), 40, 8, p(out_b), p(out_b) + 40, p(ws), big, st)),
            ('at least 1', lambda: hits(p(a), 8, p(r2), 40, p(a), 8, p(r2), 40, 0, p(out_b), p(out_b) + 40, p(ws), big, st)),
            ('shorter than the rows', lambda: hits(p(a), 8, p(r2), 40, p(a), 7, p(r2), 40, 8, p(out_b), p(out_b) + 40, p(ws), big, st)),
            ('go together', lambda: hits(p(a), 8, p(r2), 40, p(a), 8, p(r2), 40, 8, p(out_b), None, p(ws), big, st)),
            ('go together', lambda: hits(p(a), 8, p(r2), 40, p(a), 8, None, 40, 8, p(out_b), p(out_b) + 40, p(ws), big, st)),
            ('workspace too small', lambda: hits(p(a), 8, p(r2), 40, p(a), 8, p(r2), 40, 8, p(out_b), p(out_b) + 40, p(ws), 79, st)),
            ('null pointer', lambda: mmd(p(a), 8, 40, p(a), 8, 40, 8, None, p(idx), 2, 4, p(out_d), p(ws), big, st)),
            ('null pointer', lambda: mmd(p(a), 8, 40, p(a), 8, 40, 8, p(idx), p(idx), 2, 4, None, p(ws), big, st)),
            ('at least 1', lambda: mmd(p(a), 8, 40, p(a), 8, 40, 8, p(idx), p(idx), 0, 4, p(out_d), p(ws), big, st)),
            ('at least 1', lambda: mmd(p(a), 8, 40, p(a), 8, 0, 8, p(idx), p(idx), 2, 4, p(out_d), p(ws), big, st)),
            ('shorter than the rows', lambda: mmd(p(a), 7, 40, p(a), 8, 40, 8, p(idx), p(idx), 2, 4, p(out_d), p(ws), big, st)),
            ('workspace too small', lambda: mmd(p(a), 8, 40, p(a), 8, 40, 8, p(idx), p(idx), 2, 4, p(out_d), p(ws), 47, st))):
        with pytest.raises(RuntimeError, match=word):
            call()
    torch.cuda.synchronize()
    assert bool((out_f == 3.0).all()) and bool((out_b == 3).all()) and bool((out_d == 3.0).all()) and bool((ws == 0).all())
    # the same calls within the rules run: equal rows are at distance zero, inside any radius; kappa(0, 0) = 1
    knn(p(a), 8, 40, 8, 3, p(out_f), p(ws), big, st)
    hits(p(a), 8, p(r2), 40, p(a), 8, p(r2), 40, 8, p(out_b), p(out_b) + 40, p(ws), big, st)
    mmd(p(a), 8, 40, p(a), 8, 40, 8, p(idx), p(idx), 2, 4, p(out_d), p(ws), big, st)
    torch.cuda.synchronize()
    assert bool((out_f == 0.0).all()) and bool((out_b == 1).all()) and out_d.tolist() == [12.0, 12.0, 16.0] * 2
    with guarded_alloc.guarded(mf) as guard:
        with pytest.raises(ValueError, match='kth'):
            mf.knn_radii(a[:3], 3)
        with pytest.raises(ValueError, match='outside'):
            mf.poly_mmd_sums(a, a, np.array([[0, 40]]), np.array([[0, 1]]))
    assert guard.entries == [] and guard.allocations == []


def test_workspaces_are_linear_in_the_rows():
    lib = _lib.load()
    n, f = 50000, 2048
    sizes = [lib.gc_knn_radius_workspace(n, f, 3), lib.gc_manifold_hits_workspace(n, n, f), lib.gc_poly_mmd_workspace(100, n, f)]
    print('workspaces at 50000 x 50000 x 2048:', sizes)
    assert all(0 < s < 256 << 20 for s in sizes)
    assert sizes[0] <= 32 * n * 4 * 4 and sizes[1] <= 32 * 2 * n + 16
    assert lib.gc_knn_radius_workspace(n, f, 8) == 0 and lib.gc_knn_radius_workspace(0, f, 3) == 0 and lib.gc_manifold_hits_workspace(n, 0, f) == 0
    assert lib.gc_poly_mmd_workspace(100, 1000, f) == 100 * 3 * 8 * 8 * 8


def entries_of(fn):
    with guarded_alloc.guarded(mf) as guard:
        out = fn()
        assert guard.check() == []
    return out, guard.entries


def test_operator_dispatch():
    """Which inputs launch which entry (module docstring of models/op/manifold.py) -- and which launch none."""
    real, fake = (torch.from_numpy(a).to(DEV) for a in qr.real_fake(40, 30, 24))
    idx = np.stack([np.arange(20), np.arange(20)[::-1]])
    with torch.no_grad():
        r2, e = entries_of(lambda: mf.knn_radii(real))
        assert e == [mf.KNN_ENTRY]
        f2, _ = entries_of(lambda: mf.knn_radii(fake))
        (want_p, want_r), e = entries_of(lambda: mf.manifold_hits(real, r2, fake, f2))
        assert e == [mf.HITS_ENTRY]
        want_s, e = entries_of(lambda: mf.poly_mmd_sums(fake, real, idx, idx))
        assert e == [mf.MMD_ENTRY]
        for a in (real.repeat_interleave(2, 0)[::2], torch.cat([real, real], 1)[:, :24]):          # rows 2 F and F + 24 apart, read in place
            got, e = entries_of(lambda: mf.knn_radii(a))
            assert e == [mf.KNN_ENTRY] and torch.equal(got, r2)
            got, e = entries_of(lambda: mf.manifold_hits(a, r2, fake, f2))
            assert e == [mf.HITS_ENTRY] and torch.equal(got[0], want_p) and torch.equal(got[1], want_r)
            got, e = entries_of(lambda: mf.poly_mmd_sums(fake, a, torch.from_numpy(idx).to(DEV), idx))
            assert e == [mf.MMD_ENTRY] and torch.equal(got, want_s)
        for a, b in ((real.double(), fake.double()), (real.cpu(), fake.cpu()), (torch.cat([real, real], 1)[:, ::2], torch.cat([fake, fake], 1)[:, ::2]),
                     (real[:1].expand(40, 24), fake)):
            ra, e1 = entries_of(lambda: mf.knn_radii(a))
            rb = mf.knn_radii(b)          # (the last pair's b is within the rule; one tensor outside it keeps the whole call off the kernels)
            _, e3 = entries_of(lambda: mf.manifold_hits(a, ra, b, rb))
            _, e4 = entries_of(lambda: mf.poly_mmd_sums(b, a, idx, idx))
            assert not set(e1 + e3 + e4) & set(ENTRIES)
        got, e = entries_of(lambda: mf.knn_radii(real, 8))          # kth beyond the kernel's limit: the torch path
        assert e == [] and got.shape == (40,)
        rg = real.clone().requires_grad_(True)
        _, e = entries_of(lambda: mf.knn_radii(rg))          # grad mode is off: nothing is wanted
        assert e == [mf.KNN_ENTRY]
    rg = real.clone().requires_grad_(True)
    got, e = entries_of(lambda: mf.knn_radii(rg))
    assert e == [] and got.requires_grad


def test_metrics_stay_on_the_device_and_existing_callers_launch_what_they_launched(tmp_path):
    from gan_control_amd.evaluation.tracker import Tracker
    from gan_control_amd.fid_utils import real_stats
    from gan_control_amd.fid_utils.kid import kid
    from gan_control_amd.fid_utils.precision_recall import precision_recall
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    gen = torch.Generator().manual_seed(4)
    real, fake = torch.randint(-4, 5, (90, 16), generator=gen).float(), torch.randint(-3, 6, (70, 16), generator=gen).float()
    with torch.no_grad():
        got, e = entries_of(lambda: precision_recall(real.to(DEV), fake.to(DEV)))
        assert e == [mf.KNN_ENTRY, mf.KNN_ENTRY, mf.HITS_ENTRY] and got == precision_recall(real, fake)          # integer rows: exact on both paths
        got, e = entries_of(lambda: kid(real.to(DEV), fake.to(DEV), num_subsets=3, max_subset_size=50))
        assert e == [mf.MMD_ENTRY] and got == kid(real, fake, num_subsets=3, max_subset_size=50)
    tr = GeneratorTrainer(default_config(32, 4), device=DEV, seed=0, fused_adam=False)
    _, e = entries_of(lambda: tr.train(iters=1))
    assert len(e) > 50 and not set(e) & set(ENTRIES)
    pool = torch.nn.AdaptiveAvgPool2d(2)
    net = lambda img: (pool(img),)
    path = str(tmp_path / 'real.pkl')
    real_stats.save_real_features(path, torch.randn(64, 12, generator=gen) * 0.3)
    cfg = {'enabled': True, 'fid_interval': 1, 'num_of_samples': 40, 'inception_stat_path': path}
    plain = Tracker(torch.zeros(4, 512), None, net, 'normal', fid_config=cfg)
    _, e = entries_of(lambda: plain.fid_evaluation(1, tr.g_ema, graph_save_path=str(tmp_path / 'plain')))
    assert e and not set(e) & set(ENTRIES) and sorted(os.listdir(str(tmp_path / 'plain'))) == ['fid.json']
    full = Tracker(torch.zeros(4, 512), None, net, 'normal', fid_config=dict(cfg, kid=True, precision_recall=True))
    _, e = entries_of(lambda: full.fid_evaluation(1, tr.g_ema, graph_save_path=str(tmp_path / 'full')))
    assert [x for x in e if x in ENTRIES] == [mf.MMD_ENTRY, mf.KNN_ENTRY, mf.KNN_ENTRY, mf.HITS_ENTRY]
    assert sorted(full.evaluation_dict) == ['fid', 'kid', 'precision', 'recall'] and sorted(os.listdir(str(tmp_path / 'full'))) == ['fid.json', 'quality.json']
    with open(path, 'rb') as f:
        assert pickle.load(f)['features'].shape == (64, 12)
