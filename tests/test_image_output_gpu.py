"""gc_image_f32_to_u8_grid on the GPU (csrc/image_output.hip through evaluation/image_grid.py), the device resize behind it and gen_matrix.

Every expectation is made on the host -- quantize_reference + make_grid_reference, or the torch / PIL fixture (tests/golden/image_output.npz) --
and BYTES are compared, with no tolerance anywhere.  Each case runs plainly, into an output pre-filled with a byte no expectation relies on, and
once on poisoned, guard-banded allocations (tests/guarded_alloc.py swaps the ``torch`` of image_grid and image_ops) with the input placed
between NaN or 1e30 words: the guards stay untouched, the input buffer unchanged, the bytes the same."""
import numpy as np
import pytest
import torch

import guarded_alloc
import op_checks as oc
from conftest import load_golden

from gan_control_amd import _lib
from gan_control_amd.datasets import image_ops
from gan_control_amd.evaluation import generation, image_grid
from gan_control_amd.models.op import _backend

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GOLD = load_golden('image_output')
GRID, RESAMPLE = 'gc_image_f32_to_u8_grid', 'gc_image_resample_u8'
PREFILL = 0xA5


def make_input(shape, seed):
    """Floats around [-1, 1] with values beyond both ends, exact ends, zeros, infinities and a NaN sprinkled in."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=gen) * 2.6 - 1.3
    flat = x.reshape(-1)
    special = torch.tensor([1.0, -1.0, 0.0, -0.0, float('inf'), float('-inf'), float('nan'), 1e-45, 2.0, -2.0])
    n = min(flat.numel(), special.numel())
    flat[torch.randperm(flat.numel(), generator=gen)[:n]] = special[:n]
    return x


def expected(x, nrow, padding, pad):
    u8 = image_grid.quantize_reference(x).numpy()
    if u8.shape[0] == 1:
        return np.ascontiguousarray(u8[0].transpose(1, 2, 0))
    return image_grid.make_grid_reference(u8, nrow, padding, pad)


def prefilled_out(shape, shift=0, pitch=0):
    """A uint8 [gh, gw, 3] device view, rows ``pitch`` bytes apart beyond their own, the first byte ``shift`` bytes past a 512-byte boundary,
    inside a buffer of PREFILL bytes.  -> (view, backing, offset of the view's first byte)."""
    gh, gw, _ = shape
    rs = 3 * gw + pitch
    backing = torch.full((gh * rs + 2048,), PREFILL, dtype=torch.uint8, device=DEV)
    first = (-backing.data_ptr()) % 512 + 512 + shift
    return torch.as_strided(backing, (gh, gw, 3), (rs, 3, 1), first), backing, first


def check_view(view, backing, first, want):
    """The view holds ``want`` and every other byte of the buffer is still PREFILL."""
    assert np.array_equal(view.cpu().numpy(), want)
    ref = torch.full_like(backing, PREFILL).cpu()
    torch.as_strided(ref, tuple(view.shape), tuple(view.stride()), first).copy_(torch.from_numpy(want))
    assert torch.equal(backing.cpu(), ref)


def run_everywhere(x, nrow, padding, pad, place=None):
    """to_u8_grid of x (host tensor) plainly into a pre-filled view, then guarded with hostile inputs; -> nothing, asserts."""
    want = expected(x, nrow, padding, pad)
    place = place or (lambda t: t.to(DEV))
    view, backing, first = prefilled_out(want.shape)
    got = image_grid.to_u8_grid(place(x), nrow=nrow, padding=padding, pad_value=pad, out=view)
    assert got is view
    check_view(view, backing, first, want)
    for fill, shift in (('nan', 0), ('big', 4)):
        src = place(x)
        h = guarded_alloc.hostile(src, fill, shift)
        with guarded_alloc.guarded(image_grid, poison='nan') as guard:
            got = image_grid.to_u8_grid(h, nrow=nrow, padding=padding, pad_value=pad)
            violations = guard.check()
        assert not violations, violations
        assert guard.entries == [GRID]
        assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), fill
        assert guarded_alloc.hostile_changes(h, src) is None


SHAPES = [((3, 3, 5, 13), 8),          # ragged groups: 13 pixels, rows of 39 bytes
          ((3, 3, 4, 16), 8),
          ((5, 3, 7, 36), 4),           # a ragged last row: three empty tiles of pad_value
          ((1, 3, 1, 1), 8),
          ((2, 3, 6, 9), 8)]            # xmaps = batch


@pytest.mark.parametrize('pad', [0, 0x5A])
@pytest.mark.parametrize('padding', [0, 2, 3])
@pytest.mark.parametrize('shape,nrow', SHAPES, ids=['x'.join(map(str, s)) for s, _ in SHAPES])
def test_grid_bytes_and_guard_bands(shape, nrow, padding, pad):
    run_everywhere(make_input(shape, sum(shape) + padding), nrow, padding, pad)


def test_more_than_one_block_and_more_rows_than_grid_slots():
    run_everywhere(make_input((2, 3, 3, 700), 1), 2, 2, 0x33)            # 4218 bytes per row: 352 lanes, two workgroups
    run_everywhere(make_input((2, 3, 33000, 2), 2), 1, 0, 0)            # 66000 rows: more than one launch dimension holds


def test_nrow_1_padding_0_is_a_dense_byte_batch():
    x = make_input((4, 3, 6, 10), 3)
    got = image_grid.to_u8_grid(x.to(DEV), nrow=1, padding=0)
    assert tuple(got.shape) == (24, 10, 3)
    assert torch.equal(got.cpu().reshape(4, 6, 10, 3), image_grid.quantize_reference(x).permute(0, 2, 3, 1))


def test_strided_slice_of_a_larger_batch():
    x = make_input((5, 3, 7, 12), 4)

    def place(t):          # samples 1 .. 3 of five, rows 3 floats apart beyond their own, read in place
        big = torch.full((5, 3, 7, 15), float('nan'), device=DEV)
        big[:, :, :, :12] = t.to(DEV)
        view = big[1:4, :, :, :12]
        assert not view.is_contiguous() and image_grid._dense_enough(view)
        return view

    want = expected(x[1:4], 2, 2, 7)
    view = place(x)
    with guarded_alloc.guarded(image_grid, poison='nan') as guard:
        got = image_grid.to_u8_grid(view, nrow=2, padding=2, pad_value=7)
        assert not guard.check() and guard.entries == [GRID]
    assert np.array_equal(got.cpu().numpy(), want)
    run_everywhere(x[1:4], 2, 2, 7, place=lambda t: place(torch.cat([x[:1], t, x[4:]])))


@pytest.mark.parametrize('shift', [1, 2, 3])
@pytest.mark.parametrize('pitch', [0, 5])
def test_output_at_every_byte_alignment(shift, pitch):
    x = make_input((5, 3, 7, 36), 5)
    want = expected(x, 4, 2, 0x5A)
    view, backing, first = prefilled_out(want.shape, shift, pitch)
    assert view.data_ptr() % 512 == shift
    image_grid.to_u8_grid(x.to(DEV), nrow=4, padding=2, pad_value=0x5A, out=view)
    check_view(view, backing, first, want)


def test_every_quantisation_edge():
    edges, want = torch.from_numpy(GOLD['edges/x']), torch.from_numpy(GOLD['edges/byte'])
    extra = torch.tensor([float('nan'), float('inf'), float('-inf')])
    values = torch.cat([edges, extra]).repeat(3)[:3 * 8 * 64]
    bytes_ = torch.cat([want, torch.tensor([0, 255, 0], dtype=torch.uint8)]).repeat(3)[:3 * 8 * 64]
    x = values.reshape(1, 3, 8, 64)
    got = image_grid.to_u8_grid(x.to(DEV), nrow=8)
    assert tuple(got.shape) == (8, 64, 3)
    assert torch.equal(got.cpu().permute(2, 0, 1).reshape(-1), bytes_)
    assert torch.equal(image_grid.quantize_reference(x).reshape(-1), bytes_)


def test_refusals_launch_nothing():
    hip, dev = _backend.get(), torch.device(DEV)
    x = torch.zeros((2, 3, 4, 5), device=DEV)
    y = torch.full((8, 16, 3), PREFILL, dtype=torch.uint8, device=DEV)
    args = dict(x=_lib.ptr(x), row=5, plane=20, sample=60, y=_lib.ptr(y), ys=48, gh=8, gw=16)
    for kw, text in (({'x': None}, 'null'), ({'gh': 9}, 'grid_h'), ({'row': 4}, 'short stride'), ({'ys': 47}, 'short stride')):
        a = dict(args, **kw)
        with pytest.raises(RuntimeError, match='gc_image_f32_to_u8_grid failed.*' + text):
            hip._launch(dev, GRID, a['x'], a['row'], a['plane'], a['sample'], a['y'], a['ys'], 2, 4, 5, 8, 2, 0, a['gh'], a['gw'], _lib.stream_of(x))
    torch.cuda.synchronize()
    assert bool((y == PREFILL).all())
    with pytest.raises(RuntimeError, match='3-channel'):
        image_grid.to_u8_grid(torch.zeros((2, 1, 4, 4), device=DEV))


@pytest.mark.parametrize('name', ['g6x16_d4', 'g2x28x42_d2', 'g36x32_d4'])
def test_grid_image_equals_pil_on_the_device(name):
    tiles, nrow, d = torch.from_numpy(GOLD[name + '/tiles']), int(GOLD[name + '/nrow']), int(GOLD[name + '/downsample'])
    x = ((tiles.float() + 0.5) / 255 * 2 - 1).to(DEV)
    assert np.array_equal(image_grid.to_u8_grid(x, nrow=nrow).cpu().numpy(), GOLD[name + '/grid'])
    plain = image_grid.grid_image(x, nrow, downsample=d)
    with guarded_alloc.guarded(image_grid, poison='nan') as g1, guarded_alloc.guarded(image_ops, poison='nan') as g2:
        guarded = image_grid.grid_image(x, nrow, downsample=d)
        violations = g1.check() + g2.check()
    assert not violations, violations
    assert g1.entries == [GRID, RESAMPLE, RESAMPLE]
    for img in (plain, guarded):
        assert img.size == tuple(reversed(GOLD[name + '/out'].shape[:2]))
        assert np.array_equal(np.asarray(img), GOLD[name + '/out'])


def check_gen_matrix():
    g, _ = oc.build_models(32, DEV)
    g.eval()
    latents, noises = generation.make_noise_id_pose_matrix(g, device='cpu', generator=torch.Generator().manual_seed(5))
    floats = generation.gen_matrix(g, latents=latents, injection_noises=noises, same_noise_per_id=True, return_list=True)
    assert floats.shape == (36, 3, 32, 32) and floats.device.type == 'cpu' and bool(torch.isfinite(floats).all())
    for d in (None, 2):
        img = generation.gen_matrix(g, latents=latents, injection_noises=noises, same_noise_per_id=True, downsample=d)
        assert np.array_equal(np.asarray(img), np.asarray(image_grid.grid_image(floats, nrow=6, downsample=d))), d


def test_gen_matrix_f32():
    check_gen_matrix()


def test_gen_matrix_bf16x3(bf16x3_mode):
    check_gen_matrix()
