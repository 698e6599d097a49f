"""gc_pair_hinge_fwd_f32 / gc_pair_hinge_bwd_f32 on the GPU (csrc/pair_hinge.hip through models/op/pair_hinge.py).

Every case runs on fp32 inputs against the formulas restated here in float64 on the upcast inputs (formula64): for the pairs i > j of the
pair order, with v = the rows' validity flags,

    ABS: D64 = v_i v_j sum_k |F_i,k - F_j,k| / K      SQ: D64 = sum_k (F_i,k - F_j,k)^2      MSQ: D64 = scale sum_k (F_i,k - F_j,k)^2 / K
    loss64 = weight (mean_S max(D64 - lower, 0) + mean_R max(upper - D64, 0)),   C64 = dloss64 / dD64
    dF64[i, k] = g sum_{j != i} C64[max(i, j), min(i, j)] v_i v_j phi'(F_i,k - F_j,k),   phi' = sign / K, 2 d, 2 scale d / K

The bounds (u = 2^-24; all of them first-order in u, each with two u of slack for the higher-order terms):

* D: |D - D64| <= (K + 4) u D64 elementwise -- the derived bound of tests/test_pairwise_gpu.py: every term is non-negative, so any summation
  order of K float32 terms is within (K - 1) u of the exact sum relative to the sum; the subtraction, the square (the absolute value is
  exact), the division and the scale add at most one u each.
* C: the hinge is a step in D.  Integer-valued cases (inputs in [-8, 8]: every fp32 sum is exact) put the thresholds at (a + 0.5) / K (ABS),
  a + 0.5 (SQ), (a + 0.5) scale / K (MSQ): off the grid of attainable values.  Gaussian cases put each threshold at the midpoint of two
  adjacent sorted float64 distances and assert FIRST, on the float64 values alone, that the gap exceeds 16 x the distance bound (rows are
  scaled by 2^(i/4), or 2^i for K > 4096, so that a gap that wide exists among a few hundred to two thousand distances).  The active sets then
  are the float64 ones: |C - C64| <= 2 u |C64| on EVERY element (one division; zeros are exact zeros), none excluded.
* loss: the bound of D applied to the hinge sums -- a term max(t, 0) carries D's error plus one u of t; P <= n (n - 1) / 2 non-negative terms
  add (P - 1) u of the sum, the division, the addition and the weight one u each:
  |loss - loss64| <= weight (mean_S e + mean_R e) + (P + 4) u loss64 with e = (K + 4) u D64 + u max(t64, 0) over the active elements.
* dF: an element is a sum of m <= n - 1 terms coef_j phi_j.  coef = ((C g) m) v_i v_j with m = 1 / K, 2 or (2 scale) / K: C, m and the two
  products carry one u each (4 u; the flags are exact); phi is one subtraction (one u; its sign is exact); the product is exact (ABS: +-coef)
  or fused into the sum (SQ, MSQ); a sum of m terms in any order adds at most (m - 1) u of sum_j |term_j|.  So
  |dF - dF64| <= (n + 4) u A with A = |g| sum_j |C64 v_i v_j phi'64|; asserted with (n + 6) u.

Every call runs on guard-banded, poisoned outputs and workspaces and on inputs with hostile surroundings (tests/guarded_alloc.py), once with
NaN poison / NaN fill at the allocator's alignment and once with 1e30 / 1e30 and a 4-byte shift (the 4-byte load path where the first run took
16-byte loads); both runs must give the same bits, and no guard word may change.  Measured errors: profiles/attribute_losses.md.

Shapes: (n_same, n_not_same) in {(2, 2), (2, 14), (12, 4), (3, 5), (4, 3), (2, 62)} (odd counts: the 2 (n // 2) edges; n = 64: the row
limit; n = 65 is refused) x K in {1, 2, 3, 27, 64, 80, 101, 198, 512}, modes, focus values, layouts and input kinds cycling over the grid so
that every value meets every path; the one-launch limit n K <= 8192 from both sides (n = 16: K = 512, 513, 514; n = 64: 128, 129, 130; n = 7:
1170, 1171, 1172; n = 4: 2048, 2049, 2050); K = 25089 and one 16-row K = 200704 case; rows dense, K + 1 apart, features[::2] and the seven
column slices of a [16, 257] buffer; row_valid with zero / one / all rows invalid; row_index picking 6 rows of 16.
"""
import json
import os

import pytest
import torch

import guarded_alloc

from gan_control_amd.losses import LossModelClass
from gan_control_amd.losses.loss_model import RECON_SLICES
from gan_control_amd.models.op import pair_hinge as ph

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
FOCUS = ['same_as_last_layer', 'not_same_as_last_layer']
MODES = ['abs', 'sq', 'msq']
LAYOUTS = ['k', 'k+1', '::2']
SCALE = {'abs': 1.0, 'sq': 1.0, 'msq': 1e5}


def make_rows(n_rows, k, layout, gen, integer, scaled=True):
    """[n_rows, k] values as a view with the row layout of the case."""
    width, rows = {'k': (k, n_rows), 'k+1': (k + 1, n_rows), '::2': (k, 2 * n_rows)}[layout]
    if integer:
        base = torch.randint(-8, 9, (rows, width), generator=gen).float()
    else:
        base = torch.randn(rows, width, generator=gen)
        if scaled:
            step = 2 if layout == '::2' else 1
            power = torch.arange(rows).div(step, rounding_mode='floor').double() * (1.0 if k > 4096 else 0.25)
            base = base * (2.0 ** power).float()[:, None]
    base = base.to(DEV)
    return base[::2] if layout == '::2' else base[:, :k]


def formula64(f, v, n_same, n_not_same, mode, scale, focus, lower, upper, weight, g):
    """The float64 restatement on rows already in pair order -> D64, C64, loss64, dF64, A (the sum of the absolute terms of dF64)."""
    f64 = f.double()
    n, k = f64.shape
    v64 = torch.ones(n, dtype=torch.float64, device=f.device) if v is None else (v != 0).double()
    d = torch.zeros(n, n, dtype=torch.float64, device=f.device)
    for i in range(n):
        diff = f64[i][None, :] - f64
        d[i] = diff.abs().sum(-1) / k * v64[i] * v64 if mode == 'abs' else (diff * diff).sum(-1) * (scale / k if mode == 'msq' else 1.0)
    valid, same, not_same = LossModelClass.pair_masks(n_same, n_not_same, device=f.device)
    s_mask = same if focus == 'same_as_last_layer' else not_same
    r_mask = ~s_mask & valid
    t = torch.where(s_mask, d - lower, upper - d)
    active = (t >= 0) & valid
    w_same = torch.tensor(weight / float(s_mask.sum()), dtype=torch.float64, device=f.device)
    w_rest = torch.tensor(-weight / float(r_mask.sum()), dtype=torch.float64, device=f.device)
    c = torch.where(s_mask, w_same, w_rest) * active
    hinge = t.clamp_min(0) * valid
    loss = weight * (hinge[s_mask].mean() + hinge[r_mask].mean())
    d = d * valid
    csym = c + c.t()
    df, a = torch.zeros_like(f64), torch.zeros_like(f64)
    for i in range(n):
        diff = f64[i][None, :] - f64
        phi = diff.sign() / k if mode == 'abs' else diff * (2.0 if mode == 'sq' else 2.0 * scale / k)
        terms = (csym[i] * v64[i] * v64)[:, None] * phi * g
        df[i], a[i] = terms.sum(0), terms.abs().sum(0)
    return d, c, loss, df, a, (s_mask, r_mask, active, hinge)


def raw64(f, v, mode, scale):
    """The distances below the diagonal, sorted (what the thresholds are chosen from)."""
    n = f.shape[0]
    d = formula64(f, v, 2, n - 2, mode, scale, FOCUS[0], 0.0, 0.0, 1.0, 1.0)[0]
    return d[torch.tril(torch.ones(n, n, dtype=torch.bool, device=f.device), -1)].sort().values


def thresholds(f, v, mode, scale, k, integer):
    """(lower, upper) as float32-representable Python floats, by the rule of the module docstring."""
    vals = raw64(f, v, mode, scale)
    if integer:
        unit = {'abs': 1.0 / k, 'sq': 1.0, 'msq': scale / k}[mode]
        sums = (vals / unit).round()
        out = [float((sums[int(q * (len(sums) - 1))] + 0.5) * unit) for q in (0.3, 0.7)]
    else:
        out = []
        for lo, hi in ((0.1, 0.5), (0.5, 0.9)):
            part = vals[int(lo * len(vals)):max(int(hi * len(vals)), int(lo * len(vals)) + 2)]
            part = part[part > 0] if int((part > 0).sum()) >= 2 else part
            gaps = part[1:] - part[:-1]
            at = int(gaps.argmax())
            # the precondition, on the float64 values alone: the gap is wider than 16 x the distance bound at its upper end
            assert float(gaps[at]) > 16 * (k + 4) * U * float(part[at + 1]), ('no gap wide enough for a threshold', float(gaps[at]), float(part[at + 1]), k)
            out.append(float((part[at] + part[at + 1]) / 2))
    lower, upper = (float(torch.tensor(x, dtype=torch.float32)) for x in out)
    return lower, upper


def run(features, n_same, n_not_same, mode, lower, upper, focus, weight, rows, valid, scale, g, poison, fill, shift):
    """One forward and one backward call on guarded outputs and hostile copies of the inputs -> (loss, D, C, dF)."""
    hf = guarded_alloc.hostile(features, fill, shift)
    hv = None if valid is None else guarded_alloc.hostile(valid, fill, shift)
    hg = guarded_alloc.hostile(g, fill, shift)
    n = n_same + n_not_same
    with torch.no_grad(), guarded_alloc.guarded(ph, poison=poison) as guard:
        loss, d, c, v32 = ph.pair_hinge_forward(hf, n_same, n_not_same, mode, lower, upper, focus, weight, rows, hv, scale)
        assert guard.entries == [ph.FWD_ENTRY]
        df = ph.pair_hinge_backward(hf, c, hg, n, mode, rows, v32, scale)
        assert guard.entries == [ph.FWD_ENTRY, ph.BWD_ENTRY]
        assert guard.check() == []
        nbytes = ph._lib.load().gc_pair_hinge_workspace(n, features[0].numel())
        assert len(guard.allocations) == (5 if nbytes else 4) and (nbytes > 0) == (n * features[0].numel() > ph.ONE_LAUNCH_VALUES)
    assert guarded_alloc.hostile_changes(hf, features) is None and guarded_alloc.hostile_changes(hg, g) is None
    assert hv is None or guarded_alloc.hostile_changes(hv, valid) is None
    return loss, d, c, df


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def check_case(tag, features, n_same, n_not_same, mode, focus, integer, rows=None, valid=None, weight=0.75, g_value=1.0):
    """The whole contract of one case: both poisons, the same bits, and the four bounds against float64."""
    scale = SCALE[mode]
    n = n_same + n_not_same
    picked = features if rows is None else features[rows]
    k = picked[0].numel()
    v_picked = None if valid is None or mode != 'abs' else (valid if rows is None else valid[rows])
    lower, upper = thresholds(picked.reshape(n, k), v_picked, mode, scale, k, integer)
    g = torch.tensor([g_value], dtype=torch.float32, device=DEV)
    args = (features, n_same, n_not_same, mode, lower, upper, focus, weight, rows, valid, scale, g)
    out = run(*args, 'nan', 'nan', 0)
    assert same_bits(out, run(*args, 'big', 'big', 4)), tag
    loss, d, c, df = out
    d64, c64, loss64, df64, a64, (s_mask, r_mask, active, hinge) = formula64(picked.reshape(n, k), v_picked, n_same, n_not_same, mode, scale, focus, lower, upper,
                                                                             weight, float(g[0]))
    assert d.shape == (n, n) and c.shape == (n, n) and loss.dim() == 0 and df.shape == (features.shape[0], k)
    e_d = (d.double() - d64).abs()
    assert bool((e_d <= (k + 4) * U * d64).all()), (tag, 'D', float((e_d / d64.clamp_min(1e-300)).max()), (k + 4) * U)
    e_c = (c.double() - c64).abs()
    assert bool((e_c <= 2 * U * c64.abs()).all()), (tag, 'C', int((e_c > 2 * U * c64.abs()).sum()))
    assert bool((c[~active] == 0).all()) and int(active.sum()) > 0
    e = ((k + 4) * U * d64 + U * hinge) * active
    loss_bound = weight * float(e[s_mask].mean() + e[r_mask].mean()) + (n * (n - 1) // 2 + 4) * U * float(loss64)
    assert abs(float(loss) - float(loss64)) <= loss_bound, (tag, 'loss', float(loss), float(loss64), loss_bound)
    full64, full_a = torch.zeros_like(df, dtype=torch.float64), torch.zeros_like(df, dtype=torch.float64)
    index = torch.arange(n, device=DEV) if rows is None else torch.tensor(rows, device=DEV)
    full64[index], full_a[index] = df64, a64
    e_f = (df.double() - full64).abs()
    assert bool((e_f <= (n + 6) * U * full_a).all()), (tag, 'dF', float((e_f / full_a.clamp_min(1e-300)).max()), (n + 6) * U)
    if rows is not None:
        rest = [r for r in range(features.shape[0]) if r not in rows]
        assert bool((df[rest].view(torch.int32) == 0).all())
    if integer:          # every sum is exact: the distances are the float64 ones after the division and the scale, one rounding each
        assert bool(((d.double() - d64).abs() <= 2 * U * d64).all())
    ratios = (float((e_d / ((k + 4) * U * d64).clamp_min(1e-300)).max()), abs(float(loss) - float(loss64)) / max(loss_bound, 1e-300),
              float((e_f / ((n + 6) * U * full_a).clamp_min(1e-300)).max()))
    print('pair_hinge %-44s error / bound:  D %.3f   loss %.3f   dF %.3f   (active %d of %d pairs)' % ((tag,) + ratios + (int(active.sum()), n * (n - 1) // 2)))
    return out


PAIRS = [(2, 2), (2, 14), (12, 4), (3, 5), (4, 3), (2, 62)]
SMALL_K = [1, 2, 3, 27, 64, 80, 101, 198, 512]
GRID = [(ns, nn, k, MODES[(a + b) % 3], FOCUS[(a + b // 3) % 2], LAYOUTS[(a + 2 * b) % 3], (a + b) % 4 == 0)
        for a, (ns, nn) in enumerate(PAIRS) for b, k in enumerate(SMALL_K)]
# the one-launch limit n K <= 8192 from both sides, every mode on both sides of it; K = 25089 (a ragged last chunk, 4-byte loads)
LIMIT = [(4, 12, 512, 'abs', 0, 'k', False), (4, 12, 513, 'sq', 1, 'k', False), (4, 12, 514, 'msq', 0, 'k+1', True), (4, 12, 516, 'abs', 1, 'k', False),
         (2, 62, 128, 'sq', 0, 'k', False), (2, 62, 129, 'msq', 1, '::2', False), (2, 62, 130, 'abs', 0, 'k', True),
         (4, 3, 1170, 'msq', 1, 'k', False), (4, 3, 1171, 'abs', 0, 'k+1', False), (4, 3, 1172, 'sq', 1, 'k', True),
         (2, 2, 2048, 'abs', 1, '::2', False), (2, 2, 2049, 'sq', 0, 'k', False), (2, 2, 2050, 'msq', 1, 'k', False),
         (3, 5, 25089, 'abs', 0, 'k', False), (2, 14, 25089, 'sq', 1, 'k+1', True), (4, 3, 25089, 'msq', 0, '::2', False)]
LIMIT = [(ns, nn, k, m, FOCUS[f], lay, integer) for ns, nn, k, m, f, lay, integer in LIMIT]


@pytest.mark.parametrize('n_same,n_not_same,k,mode,focus,layout,integer', GRID + LIMIT)
def test_kernels_against_the_float64_formulas(n_same, n_not_same, k, mode, focus, layout, integer):
    n = n_same + n_not_same
    gen = torch.Generator().manual_seed(1000 * n_same + 10 * n_not_same + k % 997)
    features = make_rows(n, k, layout, gen, integer)
    tag = '%s %s n=%d+%d K=%d %s %s' % (mode, focus[:-14], n_same, n_not_same, k, layout, 'int' if integer else 'gauss')
    check_case(tag, features, n_same, n_not_same, mode, focus, integer)


def test_grid_meets_every_path():
    """The cycling of the grid leaves no mode / focus / layout / input kind out on either forward path."""
    for one_launch in (True, False):
        cases = [c for c in GRID + LIMIT if ((c[0] + c[1]) * c[2] <= ph.ONE_LAUNCH_VALUES) == one_launch]
        assert {c[3] for c in cases} == set(MODES) and {c[4] for c in cases} == set(FOCUS) and {c[5] for c in cases} == set(LAYOUTS)
        assert {c[6] for c in cases} == {True, False} and {(c[3], c[4]) for c in cases} == {(m, f) for m in MODES for f in FOCUS}


@pytest.mark.parametrize('mode,focus', [('abs', FOCUS[0]), ('sq', FOCUS[1])])
def test_long_rows_of_an_intermediate_level(mode, focus):
    """16 rows of K = 200704 ([n, 64, 56, 56] maps flattened), read as the 4-D tensor they are."""
    gen = torch.Generator().manual_seed(7)
    features = make_rows(16, 200704, 'k', gen, False).view(16, 64, 56, 56)
    check_case('%s %s n=4+12 K=200704 maps' % (mode, focus[:-14]), features, 4, 12, mode, focus, False)


@pytest.mark.parametrize('index', range(7))
def test_column_slices_of_the_3dmm_vector_are_read_in_place(index):
    """vec[:, lo:hi] of a [16, 257] buffer: rows 257 elements apart that start at any 4-byte alignment."""
    x, lo, hi = RECON_SLICES[index]
    gen = torch.Generator().manual_seed(index)
    vec = (torch.randint(-8, 9, (16, 257), generator=gen).float() if index % 2 else torch.randn(16, 257, generator=gen) * (2.0 ** (torch.arange(16.) / 4))[:, None]).to(DEV)
    out = check_case('abs slice %s [%d:%d]' % (x, lo, hi), vec[:, lo:hi], 2 * (index % 3) + 2, 14 - 2 * (index % 3), 'abs', FOCUS[index % 2], bool(index % 2))
    assert out[3].shape == (16, hi - lo)


@pytest.mark.parametrize('invalid', [(), (3,), tuple(range(8))])
@pytest.mark.parametrize('focus', FOCUS)
def test_row_valid_zeroes_the_pairs_of_invalid_rows(invalid, focus):
    """The hair criterion's flags: zero / one / all rows invalid.  An invalid row's pairs are at distance zero and carry no gradient."""
    gen = torch.Generator().manual_seed(len(invalid))
    colours = torch.rand(8, 3, generator=gen).to(DEV)
    valid = torch.ones(8, device=DEV)
    valid[list(invalid)] = 0
    if len(invalid) == 8:          # every distance is zero: thresholds off zero, by hand (no two distinct distances to sit between)
        g = torch.ones(1, device=DEV)
        loss, d, c, df = run(colours, 4, 4, 'abs', 0.25, 0.5, focus, 1.0, None, valid, 1.0, g, 'nan', 'nan', 0)
        assert bool((d == 0).all()) and bool((df == 0).all()) and float(loss) == 0.5
        assert same_bits((loss, d, c, df), run(colours, 4, 4, 'abs', 0.25, 0.5, focus, 1.0, None, valid, 1.0, g, 'big', 'big', 4))
        return
    loss, d, c, df = check_case('abs valid -%d %s' % (len(invalid), focus[:-14]), colours, 4, 4, 'abs', focus, False, valid=valid)
    for r in invalid:
        assert bool((d[r] == 0).all()) and bool((d[:, r] == 0).all()) and bool((df[r] == 0).all())
    # the flags are read as flags (any non-zero value is 1), and SQ / MSQ ignore them
    other = check_case('abs valid*7 -%d %s' % (len(invalid), focus[:-14]), colours, 4, 4, 'abs', focus, False, valid=valid * 7)
    assert same_bits((loss, d, c, df), other)


@pytest.mark.parametrize('mode,focus,k,integer', [('abs', FOCUS[0], 198, False), ('sq', FOCUS[1], 512, True), ('msq', FOCUS[0], 1500, False)])
def test_row_index_picks_six_rows_of_sixteen(mode, focus, k, integer):
    """A permutation of the batch's rows selects 6: the other 10 gradient rows are exactly zero, and the result is the one of the picked rows
    handed in as a batch of their own."""
    gen = torch.Generator().manual_seed(k)
    batch = make_rows(16, k, 'k+1', gen, integer)
    rows = [int(r) for r in torch.randperm(16, generator=gen)[:6]]
    valid = (torch.arange(16, device=DEV) != rows[4]).float() if mode == 'abs' else None
    loss, d, c, df = check_case('%s index K=%d' % (mode, k), batch, 2, 4, mode, focus, integer, rows=rows, valid=valid)
    alone = check_case('%s picked K=%d' % (mode, k), batch[rows].contiguous(), 2, 4, mode, focus, integer, valid=None if valid is None else valid[rows])
    assert same_bits((loss, d, c, df[rows]), alone)


def test_sixty_five_rows_are_refused_and_nothing_is_written():
    f = torch.randn(65, 8, device=DEV)
    assert not ph.kernel_taken(f, 2, 63, FOCUS[0]) and ph.kernel_taken(f[:64], 2, 62, FOCUS[0])
    with guarded_alloc.guarded(ph) as guard:
        with pytest.raises(ph._lib.UnsupportedError, match='at most 64 rows'):
            ph.pair_hinge_forward(f, 2, 63, 'abs', 0.1, 0.5, FOCUS[0])
        assert guard.check() == []
    assert guard.entries == [ph.FWD_ENTRY]
    # the operator itself routes such a call to the torch path
    with guarded_alloc.guarded(ph) as guard:
        loss = ph.pair_hinge_loss(f, 2, 63, 'abs', 0.1, 0.5, FOCUS[0])
    assert guard.entries == [] and bool(torch.isfinite(loss))


def test_determinism():
    """Two calls on the same inputs give identical bits in the loss, D, C and dF, on both forward paths."""
    gen = torch.Generator().manual_seed(3)
    for n_same, n_not_same, k, mode in ((4, 12, 512, 'abs'), (4, 12, 3000, 'sq'), (2, 62, 130, 'msq')):
        f = make_rows(n_same + n_not_same, k, 'k', gen, False)
        g = torch.full((1,), 0.5, device=DEV)
        lower, upper = thresholds(f, None, mode, SCALE[mode], k, False)
        runs = [run(f, n_same, n_not_same, mode, lower, upper, FOCUS[0], 1.0, None, None, SCALE[mode], g, 'nan', 'nan', 0) for _ in range(2)]
        assert same_bits(*runs)


@pytest.mark.parametrize('mode,shape', [('abs', (3, 66)), ('sq', (512,)), ('msq', (24, 24)), ('abs', (2, 40, 40))])
def test_autograd_wiring(mode, shape):
    """pair_hinge_loss(...).backward() against the torch path on the same device, and an upstream factor that reaches dF from the device."""
    gen = torch.Generator().manual_seed(len(shape))
    k = 1
    for s in shape:
        k *= s
    flat = make_rows(16, k, 'k', gen, False)
    lower, upper = thresholds(flat, None, mode, SCALE[mode], k, False)
    rows = [4, 5, 6, 7, 0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 15]
    leaf_a, leaf_b = flat.view(16, *shape).clone().requires_grad_(True), flat.view(16, *shape).clone().requires_grad_(True)
    with guarded_alloc.guarded(ph) as guard:
        loss = ph.pair_hinge_loss(leaf_a, 4, 12, mode, lower, upper, FOCUS[0], 0.75, rows, None, SCALE[mode])
        assert guard.entries == [ph.FWD_ENTRY] and loss.dim() == 0 and loss.requires_grad
        torch.cuda.synchronize()
        previous = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode('error')          # a host sync inside backward() raises
        try:
            (loss / 3).backward()
        finally:
            torch.cuda.set_sync_debug_mode(previous)
        assert guard.entries == [ph.FWD_ENTRY, ph.BWD_ENTRY] and guard.check() == []
    want = ph.torch_pair_hinge(leaf_b, 4, 12, mode, lower, upper, FOCUS[0], 0.75, rows, None, SCALE[mode])
    (want / 3).backward()
    third = float(torch.tensor(1.0) / 3)
    d64, c64, loss64, df64, a64, _ = formula64(flat[rows], None, 4, 12, mode, SCALE[mode], FOCUS[0], lower, upper, 0.75, third)
    full64, full_a = torch.zeros_like(df64), torch.zeros_like(df64)
    full64[rows], full_a[rows] = df64, a64
    assert leaf_a.grad.shape == leaf_a.shape
    assert bool(((leaf_a.grad.reshape(16, k).double() - full64).abs() <= (16 + 6) * U * full_a).all())
    # the torch path is within its own rounding of the same float64 values (K-term sums forward, n-term sums backward): the loss bound of the
    # module docstring with every element's error at its maximum, for each of the two
    loss_bound = 0.75 * 2 * ((k + 4) * U * float(d64.max()) + U * float(d64.max() + upper)) + (120 + 4) * U * float(loss64)
    assert abs(float(loss) - float(loss64)) <= loss_bound and abs(float(want) - float(loss64)) <= loss_bound
    assert bool(((leaf_a.grad - leaf_b.grad).reshape(16, k).double().abs() <= 2 * (16 + 6) * U * full_a).all())
    with pytest.raises(RuntimeError):          # first derivative only
        x = flat.clone().requires_grad_(True)
        gx, = torch.autograd.grad(ph.pair_hinge_loss(x, 4, 12, mode, lower, upper, FOCUS[0]), x, create_graph=True)
        gx.sum().backward()


def test_loss_model_fused_levels_launch_the_entries():
    """LossModelClass(fused=True): one forward call per level with a non-zero weight, the hair colours included; fused=False launches none."""
    gen = torch.Generator().manual_seed(5)
    cfg = {'lower_thres': [0.3, 0.2], 'upper_thres': [1.2, 0.9], 'last_lower_thres': 0.2, 'last_upper_thres': 1.3, 'intermediate_layers_weights': [0.5, 0.0],
           'last_layer_weight': 1.5, 'focus_on_list': ['not_same_as_last_layer', 'same_as_last_layer', 'same_as_last_layer']}
    hair = torch.rand(16, 4, 16, 16, generator=gen)
    hair[:, :3] = (hair[:, :3] * 2 - 1) * hair[:, 3:]
    hair[5, 3] = 0
    for name, last in (('embedding_loss', torch.randn(16, 512, generator=gen)), ('orientation_loss', torch.randn(16, 3, 66, generator=gen)),
                       ('hair_loss', hair), ('style_loss', torch.randn(16, 8, 8, generator=gen) * 3e-3), ('recon_gamma_loss', torch.randn(16, 257, generator=gen)[:, 227:254])):
        feats = [torch.randn(16, 4, 6, 6, generator=gen).to(DEV), torch.randn(16, 2, 3, 3, generator=gen).to(DEV), last.to(DEV)]
        rows = [8, 9, 0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15]
        got = {}
        for fused in (False, True):
            fs = [f.clone().requires_grad_(True) for f in feats]
            lm = LossModelClass(cfg, name, mini_batch_size=16, no_model=True, fused=fused)
            with guarded_alloc.guarded(ph) as guard:
                loss = lm.calc_mini_batch_loss_rows(fs, rows, 2, 14)
                grads = torch.autograd.grad(loss, [fs[0], fs[2]])
                assert guard.check() == []
            assert guard.entries == ([ph.FWD_ENTRY] * 2 + [ph.BWD_ENTRY] * 2 if fused else []), (name, fused, guard.entries)
            got[fused] = (loss, grads)
        assert abs(float(got[True][0]) - float(got[False][0])) <= 1e-5 * abs(float(got[False][0])), name
        for a, b in zip(got[True][1], got[False][1]):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), name


def test_controllable_generator_step_fused_against_unfused():
    """One 32 x 32 controllable generator step with fused_attribute_losses on against the same step with it off: the generator's gradients
    within what tests/golden/parity_measured.json records for the generator pass in fp32 arithmetic (global norm, per-parameter norms)."""
    from test_attribute_losses import controllable_trainer, generator_step
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'parity_measured.json')) as f:
        measured = json.load(f)['step_512_b16/f32']
    grads, stats = {}, {}
    for fused in (False, True):
        tr = controllable_trainer(DEV, fused_attribute_losses=fused)
        with guarded_alloc.guarded(ph) as guard:
            generator_step(tr, DEV)
            assert guard.check() == []
        # embedding_loss: two levels; recon_3d_loss: its gamma and ex slices
        assert [e for e in guard.entries if 'pair_hinge' in e] == ([ph.FWD_ENTRY] * 4 + [ph.BWD_ENTRY] * 4 if fused else [])
        grads[fused] = {n: p.grad.double() for n, p in tr.generator.named_parameters() if p.grad is not None}
        stats[fused] = {k: float(v) for k, v in tr.stats.items()}
    assert sorted(grads[True]) == sorted(grads[False]) and sorted(stats[True]) == sorted(stats[False])
    for key in ('g_embedding_loss', 'gamma_loss', 'ex_loss'):
        assert abs(stats[True][key] - stats[False][key]) <= 1e-5 * abs(stats[False][key]), key
    total = {f: float(torch.stack([g.pow(2).sum() for g in grads[f].values()]).sum().sqrt()) for f in grads}
    err_global = abs(total[True] - total[False]) / total[False]
    floor = 1e-3 * total[False]
    err_param = max(abs(float(grads[True][n].norm()) - float(g.norm())) / max(float(g.norm()), floor) for n, g in grads[False].items())
    err_elems = max(float((grads[True][n] - g).norm()) / max(float(g.norm()), floor) for n, g in grads[False].items())
    print('controllable step, fused against unfused: global %.3e (recorded %.3e)   per parameter %.3e (recorded %.3e)   elementwise %.3e'
          % (err_global, measured['iso/g:global'], err_param, measured['iso/g:param'], err_elems))
    assert err_global <= measured['iso/g:global'] and err_param <= measured['iso/g:param'] and err_elems <= measured['iso/g:elems']
