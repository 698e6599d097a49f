"""gc_weight_refresh_grouped_f32 on the GPU: every form against the single-purpose entry that made it before, the EMA against the two foreach
kernels, bit for bit; and the trainer with the fused refresh on against the same trainer with it off."""
import itertools

import pytest
import torch

import guarded_alloc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CASES = [(32, 32, 9), (72, 40, 9), (64, 33, 9), (32, 3, 1), (3, 32, 1), (8, 20, 1)]          # (N, K, taps)
FORMS = ('w_t', 'adj', 'adj2', 'pack_w', 'pack_adj', 'wsq')
TRAINER_DECAY = 0.5 ** (32 / 10000.0)
DECAYS = (TRAINER_DECAY, 0.999, 0.0)


def _hip():
    from gan_control_amd.models.op import _backend
    hip = _backend.get()
    assert hip.name == 'hip'
    return hip


def _foreach_ema(ema, src, decay):
    out = ema.clone()
    torch._foreach_mul_([out], decay)
    torch._foreach_add_([out], [src], alpha=1 - decay)
    return out


def _pack_formula(w):
    """hi / lo packs of w [taps, K, N] in the format of pack_weights_kernel, as int16 words: units [t][kg][n] of 8 bf16 along k, zeros beyond K."""
    taps, k, n = w.shape
    groups = (k + 7) // 8
    x = torch.zeros(taps, groups * 8, n, device=w.device)
    x[:, :k] = w
    x = x.view(taps, groups, 8, n).permute(0, 1, 3, 2).contiguous()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.cat([hi.reshape(-1), lo.reshape(-1)]).view(torch.int16)


def _pack_entry(hip, w4, k, n, ks):
    """The packs of w4 [ks, ks, k, n] from gc_conv2d_pack_weights_bf16x3, or None where the library runs such a convolution without packs."""
    from gan_control_amd import _lib
    desc = _lib.ConvDesc(4, k, n, 16, 16, 16, 16, ks, ks, 1, 1, ks // 2, ks // 2, 0, 0)
    nbytes = _lib.load().gc_conv2d_bf16x3_packed_bytes(desc)
    if nbytes == 0:
        return None
    assert nbytes == 2 * ks * ks * ((k + 7) // 8) * n * 16
    buf = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    hip._launch(torch.device(DEV), 'gc_conv2d_pack_weights_bf16x3', desc, w4.data_ptr(), buf.data_ptr(), nbytes, _lib.stream_of(w4))
    return buf.view(torch.int16)


def _references(hip, w, taps, flip, scale):
    """Every form of the parameter view w [N, K, ks, ks] from the entries the level-by-level refill uses."""
    n, k, ks = w.shape[0], w.shape[1], w.shape[2]
    prev, hip.conv_mode = hip.conv_mode, 'bf16x3'
    try:
        w_t = hip.weight_layout(w, taps, k, n, (1, taps, k * taps), (ks, ks, k, n), (k * n, n, 1), flip, scale)
        adj = hip.weight_layout(w_t, taps, k, n, (k * n, n, 1), (ks, ks, n, k), (n * k, 1, k), True, 1.0)
        adj2 = hip.weight_layout(adj, taps, n, k, (n * k, k, 1), (ks, ks, k, n), (k * n, 1, n), True, 1.0)
        ref = {'w_t': w_t, 'adj': adj, 'adj2': adj2, 'wsq': hip.weight_prep_batch('wsq', [(w,)])[0],
               'pack_w': _pack_formula(w_t.view(taps, k, n)), 'pack_adj': _pack_formula(adj.view(taps, n, k))}
        for name, t, kk, nn in (('pack_w', w_t, k, n), ('pack_adj', adj, n, k)):
            entry = _pack_entry(hip, t, kk, nn, ks)
            if entry is not None:
                assert torch.equal(entry, ref[name]), 'the pack formula of this test is not what the pack entry writes (%s)' % name
    finally:
        hip.conv_mode = prev
    return ref


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'N%d-K%d-T%d' % c)
def test_every_form_matches_its_single_purpose_entry(case, flip):
    """All 64 subsets of the outputs x with / without EMA x a parameter at storage offset 0 / at a non-zero offset ([1, N, K, k, k] viewed
    [N, K, k, k]): 256 items in ONE call, which also crosses the 16-weight-item table several times; the outputs are guard-banded, poisoned."""
    from gan_control_amd.models.op import weight_refresh
    hip = _hip()
    n, k, taps = case
    ks = 3 if taps == 9 else 1
    scale = 0.37
    gen = torch.Generator().manual_seed(n * 1000 + k * 10 + taps)
    dense = torch.randn(n, k, ks, ks, generator=gen).to(DEV)
    shifted = torch.randn(2, n, k, ks, ks, generator=gen).to(DEV)
    shifted[1].copy_(dense)
    param = shifted[1:2]                                   # [1, N, K, k, k] at storage offset N * K * k * k
    view = param.view(n, k, ks, ks)
    assert view.storage_offset() == dense.numel() and view.is_contiguous()
    ema0 = torch.randn(n, k, ks, ks, generator=gen).to(DEV)
    ref = _references(hip, dense, taps, flip, scale)
    ref_ema = {d: _foreach_ema(ema0, dense, d) for d in DECAYS}
    items, emas = [], []
    for i, (subset, with_ema, src) in enumerate(itertools.product(range(64), (False, True), (dense, view))):
        want = {f for j, f in enumerate(FORMS) if subset >> j & 1}
        decay = DECAYS[i % 3]
        ema = ema0.clone() if with_ema else None
        emas.append((ema, decay))
        items.append({'src': src, 'taps': taps, 'k': k, 'n': n, 'flip': flip, 'scale': scale,
                      'w_t': (ks, ks, k, n) if 'w_t' in want else None, 'adj': (ks, ks, n, k) if 'adj' in want else None, 'adj2': (ks, ks, k, n) if 'adj2' in want else None,
                      'pack_w': 2 * taps * ((k + 7) // 8) * n * 16 if 'pack_w' in want else 0,
                      'pack_adj': 2 * taps * ((n + 7) // 8) * k * 16 if 'pack_adj' in want else 0,
                      'wsq': 'wsq' in want, 'ema': (ema, decay, 1 - decay) if with_ema else None})
    before = weight_refresh.launches()
    with guarded_alloc.guarded(weight_refresh, 'nan') as guard:
        outs = weight_refresh.run(items)
        assert guard.check() == []
    assert guard.entries == [weight_refresh.ENTRY]
    assert weight_refresh.launches() - before == len(items) // 16
    assert torch.equal(shifted[1], dense) and torch.equal(view, dense), 'the source parameter changed'
    for it, out, (ema, decay) in zip(items, outs, emas):
        want = {f for f in FORMS if it[f]}
        assert set(out) == want
        for f in want:
            got = out[f].view(torch.int16) if f.startswith('pack') else out[f]
            assert got.shape == ref[f].shape and torch.equal(got, ref[f]), (f, sorted(want), it['src'] is view, ema is not None)
        if ema is not None:
            assert torch.equal(ema, ref_ema[decay]), ('ema', decay, sorted(want), it['src'] is view)


def test_flat_items_and_table_chunking():
    """EMA-only items of 1, 5, 1027 and 5000 elements, 16-byte aligned and one float off, with every decay; 100 of them in one call (more than
    the 76 a launch's table holds) next to weight items."""
    from gan_control_amd.models.op import weight_refresh
    _hip()
    gen = torch.Generator().manual_seed(5)
    flats, refs, srcs = [], [], []
    bystander = torch.randn(4096, generator=gen).to(DEV)
    keep = bystander.clone()
    for i in range(100):
        count = (1, 5, 1027, 5000)[i % 4]
        off = (i // 4) % 2
        src = torch.randn(count + 1, generator=gen).to(DEV)[off:off + count]
        ema = torch.randn(count + 3, generator=gen).to(DEV)
        decay = DECAYS[i % 3]
        dst = ema[off:off + count]
        refs.append((_foreach_ema(dst, src, decay), ema.clone()))
        flats.append((src, dst, decay, 1 - decay))
        srcs.append(src.clone())
    w = torch.randn(8, 20, 1, 1, generator=gen).to(DEV)
    item = {'src': w, 'taps': 1, 'k': 20, 'n': 8, 'flip': False, 'scale': 1.0, 'w_t': (1, 1, 20, 8), 'adj': None, 'adj2': None, 'pack_w': 0, 'pack_adj': 0,
            'wsq': False, 'ema': None}
    before = weight_refresh.launches()
    outs = weight_refresh.run([item], flats)
    assert weight_refresh.launches() - before == 2
    assert torch.equal(outs[0]['w_t'].view(20, 8), w.view(8, 20).t())
    for (src, dst, decay, _), (want, whole), src0 in zip(flats, refs, srcs):
        assert torch.equal(dst, want), (dst.numel(), decay)
        assert torch.equal(src, src0)
        ema = dst._base
        off = dst.storage_offset()
        assert torch.equal(ema[:off], whole[:off]) and torch.equal(ema[off + dst.numel():], whole[off + dst.numel():]), 'a store outside the item'
    assert torch.equal(bystander, keep)


def test_unsupported_items_are_refused_before_any_launch():
    from gan_control_amd import _lib
    from gan_control_amd.models.op import weight_refresh
    _hip()
    w = torch.randn(4, 4, 2, 2, device=DEV)
    before = weight_refresh.launches()
    with pytest.raises(_lib.UnsupportedError):
        weight_refresh.run([{'src': w, 'taps': 4, 'k': 4, 'n': 4, 'flip': False, 'scale': 1.0, 'w_t': (2, 2, 4, 4), 'adj': None, 'adj2': None, 'pack_w': 0,
                             'pack_adj': 0, 'wsq': False, 'ema': None}])
    table = (_lib.WRefreshItem * 1)()
    table[0].src, table[0].w_t, table[0].n, table[0].k, table[0].taps = w.data_ptr(), w.data_ptr(), 4, 4, 4
    assert _lib.load().gc_weight_refresh_grouped_f32(table, 1, None) == _lib.GC_ERR_UNSUPPORTED
    assert weight_refresh.launches() == before


def _train(mode, knob, counters=None):
    from gan_control_amd.models.op import _backend, weight_cache, weight_refresh
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    hip = _hip()
    prev_mode, hip.conv_mode = hip.conv_mode, mode
    prev_knob, weight_refresh.ENABLED = weight_refresh.ENABLED, knob
    real_run, real_prep = weight_refresh._Runner.run, _backend.HipBackend.weight_prep_batch

    def counted_run(items, flats=()):
        before = weight_refresh.launches()
        outs = real_run(items, flats)
        with_ema = bool(flats) or any(it.get('ema') is not None for it in items)
        counters['refresh'].append((with_ema, weight_refresh.launches() - before))
        return outs

    def counted_prep(self, kind, items):
        counters['prep'].append(kind)
        return real_prep(self, kind, items)

    if counters is not None:
        weight_refresh._Runner.run = staticmethod(counted_run)
        _backend.HipBackend.weight_prep_batch = counted_prep
    weight_cache.clear()
    try:
        tr = GeneratorTrainer(default_config(64, 4), device=DEV, seed=0)
        real = tr.synthetic_batch()
        for i in range(4):                   # iteration 0 fires R1 and the path-length pass
            tr.train_iteration(i, real)
        torch.cuda.synchronize()
        return {name: {k: v.detach().clone() for k, v in net.state_dict().items()}
                for name, net in (('generator', tr.generator), ('discriminator', tr.discriminator), ('g_ema', tr.g_ema))}
    finally:
        weight_refresh._Runner.run, _backend.HipBackend.weight_prep_batch = real_run, real_prep
        hip.conv_mode, weight_refresh.ENABLED = prev_mode, prev_knob
        weight_cache.clear()


@pytest.mark.parametrize('mode', ['f32', 'bf16x3', 'bf16'])
def test_trainer_is_bit_identical_with_the_fused_refresh(mode):
    on_counts, off_counts = {'refresh': [], 'prep': []}, {'refresh': [], 'prep': []}
    on = _train(mode, True, on_counts)
    off = _train(mode, False, off_counts)
    for net in on:
        for k in on[net]:
            assert torch.equal(on[net][k], off[net][k]), (net, k)
    # knob on: every refresh within its launch bound, both kinds seen, and the refill never fell back to the grouped re-layout
    assert any(e for e, _ in on_counts['refresh']) and any(not e for e, _ in on_counts['refresh'])
    for with_ema, n in on_counts['refresh']:
        assert 1 <= n <= (4 if with_ema else 2), on_counts['refresh']
    assert 'layout' not in on_counts['prep'], on_counts['prep']
    # knob off: the hook never ran and the grouped kernels did the refills
    assert not off_counts['refresh'] and 'layout' in off_counts['prep']
