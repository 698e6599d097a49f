"""The fused refresh of derived weight forms (op/weight_refresh.py behind weight_cache.refresh_runner), without a GPU: the translation of recipe
chains into items with a runner that computes the forms with torch, the ABI of the new entry, and that the emulated backend never sees the hook."""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import REPO


class FakeRunner:
    """The interface of op/weight_refresh.py's runner; every form from its definition in include/gancontrol_hip.h, with torch."""
    taps = (1, 9)

    def __init__(self):
        self.calls = []

    @staticmethod
    def pack_bytes(fields, taps, k, n):
        return 2 * taps * ((k + 7) // 8) * n * 16 if (fields[1], fields[2], fields[7] * fields[8]) == (k, n, taps) else 0

    @staticmethod
    def ema_ok(tensors):
        return all(t.dtype == torch.float32 and t.is_contiguous() for t in tensors)

    def run(self, items, flats=()):
        self.calls.append(([dict(it) for it in items], list(flats)))
        outs = []
        for it in items:
            n, k, taps = it['n'], it['k'], it['taps']
            w = it['src'].reshape(n, k, taps)
            w_t = w.permute(2, 1, 0) * it['scale']
            if it['flip']:
                w_t = w_t.flip(0)
            out = {}
            if it['w_t'] is not None:
                out['w_t'] = w_t.contiguous().view(it['w_t'])
            if it['adj'] is not None:
                out['adj'] = w_t.flip(0).transpose(1, 2).contiguous().view(it['adj'])
            if it['adj2'] is not None:
                out['adj2'] = w_t.contiguous().view(it['adj2'])
            for name in ('pack_w', 'pack_adj'):
                if it[name]:
                    out[name] = torch.zeros(it[name] // 4)
            if it['wsq']:
                out['wsq'] = it['src'].reshape(n, k, taps).pow(2).sum(2)
            if it['ema'] is not None:
                dst, decay, alpha = it['ema']
                dst.mul_(decay).add_(it['src'].reshape(dst.shape), alpha=alpha)
            outs.append(out)
        for src, dst, decay, alpha in flats:
            dst.mul_(decay).add_(src, alpha=alpha)
        return outs


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(11)
        self.a = torch.nn.Parameter(torch.randn(1, 6, 5, 3, 3, generator=gen))      # a modulated convolution's weight: viewed [6, 5, 3, 3]
        self.b = torch.nn.Parameter(torch.randn(4, 6, 1, 1, generator=gen))
        self.c = torch.nn.Parameter(torch.randn(3, 5, 5, 5, generator=gen))         # 25 taps: not expressible
        self.bias = torch.nn.Parameter(torch.randn(7, generator=gen))


def _forms(net):
    """Every form of the three weights through the front ends the model uses: {name: tensor}."""
    from gan_control_amd.models.op import _backend
    from gan_control_amd.models.op.modulated_conv import _WeightSq
    from gan_control_amd.models.op.weight_layout import kernel_layout, adjoint_layout
    out = {}
    with torch.no_grad():
        for name, w, scale, flip in (('a', net.a.view(6, 5, 3, 3), 0.5, True), ('b', net.b, 0.25, False), ('c', net.c, 2.0, False)):
            w_t = kernel_layout(w, scale, flip=flip)
            out[name + '.w_t'] = w_t
            out[name + '.adj'] = adjoint_layout(w_t)
            out[name + '.adj2'] = adjoint_layout(out[name + '.adj'])          # the weights of a double-backward convolution
        out['a.wsq'] = _backend.call(_WeightSq, net.a.view(6, 5, 3, 3))
    return out


@pytest.fixture
def fake(emu_backend, monkeypatch):
    from gan_control_amd.models.op import weight_cache
    weight_cache.unregister_all()
    runner = FakeRunner()
    monkeypatch.setattr(weight_cache, 'refresh_runner', lambda: runner)
    monkeypatch.setattr(weight_cache, 'ENABLED', True)
    monkeypatch.setattr(weight_cache, 'BATCHED', True)
    yield runner
    weight_cache.unregister_all()


def _pack_recipes(net, weight_cache):
    """What conv2d records for a split-bf16 convolution over w_t and over adj(w_t): ('pack', the fields of its descriptor)."""
    fields = lambda k, n, ks: (2, k, n, 8, 8, 8, 8, ks, ks, 1, 1, ks // 2, ks // 2, 0, 0)
    added = []
    for root, n, k, ks in ((net.a, 6, 5, 3), (net.b, 4, 6, 1)):
        recipes = weight_cache._recipes_of(root)
        for key in list(recipes):
            if len(key) == 3 and recipes[key][0] == 'layout':
                recipes[key + (('pack_bf16x3',),)] = ('pack', fields(k, n, ks))
                added.append((id(root), key + (('pack_bf16x3',),)))
            if len(key) == 4 and recipes[key][0] == 'layout':
                recipes[key + (('pack_bf16x3',),)] = ('pack', fields(n, k, ks))
                added.append((id(root), key + (('pack_bf16x3',),)))
    return added


def test_recipe_chains_become_items_and_every_form_is_remembered(fake, monkeypatch):
    from gan_control_amd.models.op import weight_cache
    net = Net()
    weight_cache.register(net)
    want = _forms(net)                       # discovers the recipes one form at a time: nothing is offered to the hook yet
    assert not fake.calls
    packs = _pack_recipes(net, weight_cache)
    assert len(packs) == 4
    monkeypatch.setattr(weight_cache, 'pack_wanted', lambda: True)
    weight_cache.invalidate(net.parameters())
    batched = weight_cache.stats['batched']
    got = _forms(net)                        # the first miss refills the group
    assert len(fake.calls) == 1
    items, flats = fake.calls[0]
    assert not flats and len(items) == 2     # one item per expressible chain: a and b
    by_n = {it['n']: it for it in items}
    assert by_n[6]['taps'] == 9 and by_n[6]['flip'] and by_n[6]['scale'] == 0.5 and by_n[6]['wsq'] and tuple(by_n[6]['src'].shape) == (6, 5, 3, 3)
    assert by_n[4]['taps'] == 1 and not by_n[4]['flip'] and not by_n[4]['wsq']
    for it in items:
        assert it['w_t'] is not None and it['adj'] is not None and it['adj2'] == it['w_t'] and it['ema'] is None
        assert it['pack_w'] == 2 * it['taps'] * ((it['k'] + 7) // 8) * it['n'] * 16
        assert it['pack_adj'] == 2 * it['taps'] * ((it['n'] + 7) // 8) * it['k'] * 16
    # 2 x (w_t, adj, adj2, two packs) + wsq from the hook, c's three layouts from the level-by-level code
    assert weight_cache.stats['batched'] - batched == 14
    for name in want:
        assert torch.equal(want[name], got[name]), name
    # every remembered key is present, and asking again is a hit
    for root in (net.a, net.b, net.c):
        bucket = weight_cache._roots[id(root)][2]
        assert set(weight_cache._recipes_of(root)) == set(bucket)
    hits, misses = weight_cache.stats['hit'], weight_cache.stats['miss']
    again = _forms(net)
    assert weight_cache.stats['miss'] == misses and weight_cache.stats['hit'] > hits and len(fake.calls) == 1
    for name in want:
        assert again[name].data_ptr() == got[name].data_ptr(), name


def test_inexpressible_recipes_stay_on_the_old_path(fake):
    """An in-major source (the conv_transpose2d parameter layout) and a 25-tap weight are left to the level-by-level refill, without an error."""
    from gan_control_amd.models.op import weight_cache
    from gan_control_amd.models.op.weight_layout import kernel_layout
    net = Net()
    weight_cache.register(net)
    with torch.no_grad():
        first = [kernel_layout(net.b, 1.0, in_major=True), kernel_layout(net.c, 1.0)]
        weight_cache.invalidate(net.parameters())
        batched = weight_cache.stats['batched']
        second = [kernel_layout(net.b, 1.0, in_major=True), kernel_layout(net.c, 1.0)]
    assert not fake.calls                    # no item at all: the runner is not called
    assert weight_cache.stats['batched'] - batched == 2
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_packs_are_not_rebuilt_in_exact_fp32(fake, monkeypatch):
    from gan_control_amd.models.op import weight_cache
    net = Net()
    weight_cache.register(net)
    _forms(net)
    _pack_recipes(net, weight_cache)
    monkeypatch.setattr(weight_cache, 'pack_wanted', lambda: False)
    weight_cache.invalidate(net.parameters())
    _forms(net)
    assert len(fake.calls) == 1 and all(not it['pack_w'] and not it['pack_adj'] for it in fake.calls[0][0])


def test_accumulate_runs_the_ema_and_the_refresh_in_one_call(fake):
    from gan_control_amd.models.op import weight_cache
    from gan_control_amd.trainers.utils import accumulate
    net, ema = Net(), Net()
    with torch.no_grad():
        for p in ema.parameters():
            p.mul_(0.5)
    weight_cache.register(net)
    weight_cache.register(ema)
    want = _forms(net)
    weight_cache.invalidate(net.parameters())
    ref = {k: v.detach().clone() for k, v in ema.named_parameters()}
    torch._foreach_mul_(list(ref.values()), 0.75)
    torch._foreach_add_(list(ref.values()), [p.detach() for p in net.parameters()], alpha=1 - 0.75)
    accumulate(ema, net, 0.75)
    assert len(fake.calls) == 1
    items, flats = fake.calls[0]
    assert len(items) == 2 and all(it['ema'] is not None and it['ema'][1:] == (0.75, 0.25) for it in items)
    assert len(flats) == 2                   # c (no item) and the bias
    for k, v in ema.named_parameters():
        assert torch.equal(v.detach(), ref[k]), k
    hits = weight_cache.stats['hit']
    got = _forms(net)                        # a's and b's forms were made by accumulate's call; c refills on the old path, alone
    assert len(fake.calls) == 1 and weight_cache.stats['hit'] > hits
    for name in want:
        assert torch.equal(want[name], got[name]), name


@pytest.mark.parametrize('off', ['ENABLED', 'BATCHED'])
def test_cache_switches_keep_the_hook_out(fake, monkeypatch, off):
    from gan_control_amd.models.op import weight_cache
    from gan_control_amd.trainers.utils import accumulate
    net, ema = Net(), Net()
    weight_cache.register(net)
    weight_cache.register(ema)
    _forms(net)
    monkeypatch.setattr(weight_cache, off, False)
    weight_cache.invalidate(net.parameters())
    batched = weight_cache.stats['batched']
    ref = [0.5 * e.detach() + (1 - 0.5) * p.detach() for e, p in zip(ema.parameters(), net.parameters())]
    accumulate(ema, net, 0.5)
    _forms(net)
    assert not fake.calls and weight_cache.stats['batched'] == batched
    assert all(torch.allclose(e.detach(), r) for e, r in zip(ema.parameters(), ref))


def test_unregistered_source_takes_the_foreach_ema(fake):
    from gan_control_amd.trainers.utils import accumulate
    net, ema = Net(), Net()
    accumulate(ema, net, 0.0)
    assert not fake.calls
    assert all(torch.equal(e.detach(), p.detach()) for e, p in zip(ema.parameters(), net.parameters()))


@pytest.mark.parametrize('knob', [True, False])
def test_the_knob_changes_nothing_on_the_emulated_backend(emu_backend, monkeypatch, knob):
    from gan_control_amd.models.op import weight_cache, weight_refresh
    from gan_control_amd.trainers.utils import accumulate
    monkeypatch.setattr(weight_refresh, 'ENABLED', knob)
    assert weight_cache.refresh_runner is not None and weight_cache.refresh_runner() is None
    weight_cache.unregister_all()
    net, ema = Net(), Net()
    weight_cache.register(net)
    weight_cache.register(ema)
    first = _forms(net)
    weight_cache.invalidate(net.parameters())
    accumulate(ema, net, 0.0)
    second = _forms(net)
    assert all(torch.equal(first[k], second[k]) for k in first)
    assert all(torch.equal(e.detach(), p.detach()) for e, p in zip(ema.parameters(), net.parameters()))
    weight_cache.unregister_all()


def test_item_struct_has_one_size_in_header_binding_and_library(tmp_path):
    from gan_control_amd import _lib
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include "gancontrol_hip.h"\nint main(void) { printf("%zu", sizeof(gc_wrefresh_item)); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.run(['gcc', '-I', os.path.join(REPO, 'include'), str(src), '-o', str(exe)], check=True)
    header = int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert header == ctypes.sizeof(_lib.WRefreshItem) == _lib.load().gc_weight_refresh_item_bytes()


def test_entry_rejects_bad_items_before_any_launch():
    from gan_control_amd import _lib
    lib = _lib.load()
    before = lib.gc_weight_refresh_launches()
    assert lib.gc_weight_refresh_grouped_f32(None, 0, None) == 0
    assert lib.gc_weight_refresh_grouped_f32(None, 1, None) == -1
    item = (_lib.WRefreshItem * 1)()
    item[0].src, item[0].n, item[0].k, item[0].taps = 64, 8, 8, 4
    assert lib.gc_weight_refresh_grouped_f32(item, 1, None) == _lib.GC_ERR_UNSUPPORTED and b'taps' in lib.gc_last_error()
    item[0].taps, item[0].k = 9, 0
    assert lib.gc_weight_refresh_grouped_f32(item, 1, None) == -1
    item[0].taps, item[0].k, item[0].count = 0, 8, 16          # flat item without an EMA destination
    assert lib.gc_weight_refresh_grouped_f32(item, 1, None) == -1
    item[0].src = None
    assert lib.gc_weight_refresh_grouped_f32(item, 1, None) == -1
    assert lib.gc_weight_refresh_launches() == before


def test_trainer_routes_every_refill_through_the_hook(emu_backend, monkeypatch):
    """Two iterations (R1 and the path-length pass fire in the first) of the trainer on the emulated backend with the torch runner as the hook against the same trainer without it: the same
    parameters and EMA, bit for bit; with the hook the grouped re-layout never runs, and accumulate's call carries the EMA."""
    import conftest
    from gan_control_amd.models.op import weight_cache
    from gan_control_amd.trainers.generator_trainer import GeneratorTrainer, default_config
    kinds = []
    real_prep = conftest.EmulatedBackend.weight_prep_batch
    monkeypatch.setattr(conftest.EmulatedBackend, 'weight_prep_batch', lambda self, kind, items: (kinds.append(kind), real_prep(self, kind, items))[1])
    monkeypatch.setattr(weight_cache, 'ENABLED', True)
    monkeypatch.setattr(weight_cache, 'BATCHED', True)
    out, runner = [], FakeRunner()
    for hook in (lambda: runner, lambda: None):
        weight_cache.unregister_all()
        monkeypatch.setattr(weight_cache, 'refresh_runner', hook)
        del kinds[:]
        tr = GeneratorTrainer(default_config(16, 4), device='cpu', seed=0, fused_adam=True)
        real = tr.synthetic_batch()
        for i in range(2):
            tr.train_iteration(i, real)
        out.append({name + '.' + k: v.clone() for name, net in (('g', tr.generator), ('d', tr.discriminator), ('ema', tr.g_ema))
                    for k, v in net.state_dict().items()})
        assert ('layout' in kinds) == (hook() is None), kinds
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
    with_ema = [c for c in runner.calls if c[1] or any(it['ema'] is not None for it in c[0])]
    assert len(with_ema) == 1 + 2 and len(runner.calls) > len(with_ema)          # the trainer's initial copy and one per iteration; D's refreshes carry none
    assert all(any(it['ema'] is not None for it in c[0]) for c in with_ema[1:])   # from the first iteration on the EMA rides on the weight items
    weight_cache.unregister_all()
