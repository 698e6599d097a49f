"""The image output path on the host (evaluation/image_grid.py, evaluation/generation.py) and the argument checks of gc_image_f32_to_u8_grid.

The expectations are the torch / PIL fixture (tests/golden/image_output.npz, tools/make_image_output_golden.py), PIL itself, or geometry written
out here; bytes are compared with no tolerance.  Only the generator comparisons carry one (op_checks.TOL, what the network tests use)."""
import numpy as np
import pytest
import torch

import op_checks as oc
from conftest import load_golden, rel_err

from gan_control_amd.evaluation import generation, image_grid

GOLD = load_golden('image_output')
CASES = ['g6x16_d4', 'g2x28x42_d2', 'g4x18_d3', 'g36x32_d4']


def floats_of(tiles):
    """Floats in [-1, 1] that quantise to the given bytes: the middle of each byte's interval."""
    return (torch.as_tensor(tiles).float() + 0.5) / 255 * 2 - 1


def test_quantize_reference_on_every_edge():
    x, want = torch.from_numpy(GOLD['edges/x']), torch.from_numpy(GOLD['edges/byte'])
    assert x.numel() == 510 and want.tolist() == [v for k in range(1, 256) for v in (k - 1, k)]
    assert torch.equal(image_grid.quantize_reference(x), want)
    # the edge set keeps its teeth: the closed form is another function
    closed = (x * 127.5 + 127.5).clamp(0, 255).to(torch.uint8)
    assert int((closed != want).sum()) >= 1


def test_quantize_reference_special_values():
    x = torch.tensor([float('inf'), float('-inf'), float('nan'), 0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 3e38, -3e38, 1e-45, -1e-45])
    want = [255, 0, 0, 127, 127, 255, 0, 255, 0, 255, 0, 127, 127]
    assert image_grid.quantize_reference(x).tolist() == want
    assert image_grid.quantize_reference(floats_of(torch.arange(256))).tolist() == list(range(256))


@pytest.mark.parametrize('batch,nrow,padding', [(3, 8, 2), (5, 4, 2), (5, 4, 3), (5, 4, 0), (6, 3, 2), (2, 8, 3), (7, 1, 0), (1, 8, 2)])
def test_grid_geometry(batch, nrow, padding):
    h, w, pad = 3, 5, 0x5A
    rng = np.random.default_rng(batch * 10 + padding)
    tiles = rng.integers(0, 256, (batch, 3, h, w), dtype=np.uint8)
    tiles[tiles == pad] = 0          # so that a padding byte is told from an image byte
    grid = image_grid.make_grid_reference(tiles, nrow, padding, pad)
    xmaps = min(nrow, batch)
    ymaps = -(-batch // xmaps)
    assert grid.shape == (ymaps * (h + padding) + padding, xmaps * (w + padding) + padding, 3)
    assert image_grid.grid_geometry(batch, h, w, nrow, padding) == (xmaps, ymaps) + grid.shape[:2]
    covered = np.zeros(grid.shape[:2], bool)
    for k in range(batch):
        top, left = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        assert np.array_equal(grid[top:top + h, left:left + w], tiles[k].transpose(1, 2, 0)), k
        covered[top:top + h, left:left + w] = True
    assert int(covered.sum()) == batch * h * w and bool((grid[~covered] == pad).all())          # bands and the empty tiles of a ragged row
    # ... and through to_u8_grid from floats; one image comes back bare, as make_grid returns it
    got = image_grid.to_u8_grid(floats_of(tiles), nrow=nrow, padding=padding, pad_value=pad)
    want = tiles[0].transpose(1, 2, 0) if batch == 1 else grid
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)


def test_nrow_1_is_a_dense_byte_batch():
    x = torch.rand(4, 3, 6, 7, generator=torch.Generator().manual_seed(0)) * 2.4 - 1.2
    got = image_grid.to_u8_grid(x, nrow=1, padding=0)
    assert torch.equal(got.reshape(4, 6, 7, 3), image_grid.quantize_reference(x).permute(0, 2, 3, 1))


def test_to_u8_grid_refusals(emu_backend):
    with pytest.raises(RuntimeError, match='3-channel'):
        image_grid.to_u8_grid(torch.zeros(2, 1, 4, 4))
    with pytest.raises(RuntimeError, match='float tensor'):
        image_grid.to_u8_grid(torch.zeros(2, 3, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        image_grid.to_u8_grid(torch.zeros(2, 3, 4, 4), nrow=0)
    with pytest.raises(ValueError):
        image_grid.to_u8_grid(torch.zeros(2, 3, 4, 4), pad_value=256)
    # a CUDA tensor never detours over the host: on another backend than the HIP one it is an error (a meta tensor says is_cuda to no one,
    # so the check is made on a stand-in)

    class OnDevice(torch.Tensor):
        is_cuda = True

    with pytest.raises(RuntimeError, match='HIP backend only'):
        image_grid.to_u8_grid(torch.zeros(2, 3, 4, 4).as_subclass(OnDevice))


@pytest.mark.parametrize('name', CASES)
def test_grid_image_equals_pil(name):
    """CPU tensors: the grid, then PIL's resize under the reference's (width // d, height // d) -> (h, w) rule, non-square grids included."""
    from PIL import Image
    tiles, nrow, d = GOLD[name + '/tiles'], int(GOLD[name + '/nrow']), int(GOLD[name + '/downsample'])
    x = floats_of(tiles)
    assert np.array_equal(image_grid.to_u8_grid(x, nrow=nrow).numpy(), GOLD[name + '/grid'])
    img = image_grid.grid_image(x, nrow, downsample=d)
    gh, gw = GOLD[name + '/grid'].shape[:2]
    assert isinstance(img, Image.Image) and img.mode == 'RGB' and img.size == (gh // d, gw // d)          # PIL's size is (width, height)
    assert np.array_equal(np.asarray(img), GOLD[name + '/out'])
    pil = Image.fromarray(GOLD[name + '/grid'], 'RGB').resize((gh // d, gw // d), Image.BILINEAR)
    assert np.array_equal(np.asarray(img), np.asarray(pil))
    assert np.array_equal(np.asarray(image_grid.grid_image(x, nrow)), GOLD[name + '/grid'])


# ---- generation.py on the emulated backend ------------------------------------------------------------------------------------------------
SIZE = 32


@pytest.fixture
def generator_32(emu_backend):
    g, _ = oc.build_models(SIZE, 'cpu')
    return g.eval()


def test_matrix_latent_structure(generator_32):
    gen = torch.Generator().manual_seed(3)
    latents, noises = generation.make_noise_id_pose_matrix(generator_32, ids_in_row=4, pose_in_col=3, id_chunk=(100, 300), generator=gen)
    assert len(latents) == 12 and len(noises) == 4 and all(z.shape == (1, 512) for z in latents)
    assert [tuple(n.shape) for n in noises[0]] == [tuple(n.shape) for n in generator_32.make_noise()]
    z = torch.cat(latents).reshape(3, 4, 512)
    inside = z[:, :, 100:300]
    outside = torch.cat([z[:, :, :100], z[:, :, 300:]], 2)
    for row in range(3):
        for col in range(4):
            assert torch.equal(inside[row, col], inside[row, 0])            # a row shares the chunk ...
            assert torch.equal(outside[row, col], outside[0, col])          # ... a column shares the rest
    assert not torch.equal(inside[0, 0], inside[1, 0]) and not torch.equal(outside[0, 0], outside[0, 1])
    # sample s gives row s its chunk and column s its rest: the diagonal images are the samples themselves
    again, _ = generation.make_noise_id_pose_matrix(generator_32, ids_in_row=4, pose_in_col=3, id_chunk=(100, 300), generator=torch.Generator().manual_seed(3))
    assert all(torch.equal(a, b) for a, b in zip(latents, again))          # reproducible from the generator
    assert latents[0].device == next(generator_32.parameters()).device     # the model's device by default


@pytest.mark.parametrize('mode', ['same_noise_for_all', 'same_noise_per_id'])
def test_gen_matrix_equals_per_image_calls(generator_32, mode):
    """6 x 6 with given latents and noises: the row-batched calls against one generator call per image with the noise the reference's loop
    gives it (the running injection_num in the per-id mode: all 36 images run), and the returned image against grid_image of those floats."""
    g = generator_32
    gen = torch.Generator().manual_seed(5)
    latents, noises = generation.make_noise_id_pose_matrix(g, generator=gen)
    kw = {mode: True}
    floats = generation.gen_matrix(g, latents=latents, injection_noises=noises, return_list=True, **kw)
    assert floats.shape == (36, 3, SIZE, SIZE) and floats.device.type == 'cpu'
    with torch.no_grad():
        for pic in (0, 5, 6, 17, 35):
            noise = noises[pic // 6 if mode == 'same_noise_per_id' else 0]
            want, _ = g([latents[pic]], noise=noise)
            assert rel_err(floats[pic:pic + 1], want) <= oc.TOL, pic
    if mode == 'same_noise_per_id':
        assert not torch.equal(floats[0], floats[6])
    img = generation.gen_matrix(g, latents=latents, injection_noises=noises, **kw)
    assert img.size == (6 * (SIZE + 2) + 2,) * 2
    assert np.array_equal(np.asarray(img), np.asarray(image_grid.grid_image(floats, nrow=6)))
    small = generation.gen_matrix(g, latents=latents, injection_noises=noises, downsample=2, **kw)
    assert np.array_equal(np.asarray(small), np.asarray(image_grid.grid_image(floats, nrow=6, downsample=2)))


def test_gen_grid_and_random_matrix(generator_32):
    g = generator_32
    z = torch.randn(5, 512, generator=torch.Generator().manual_seed(1))
    noise = oc.seeded_noise(SIZE, 5, 2)
    img = generation.gen_grid(g, z, injection_noise=noise, nrow=4)
    with torch.no_grad():
        want, _ = g([z], noise=noise)
    assert img.size == (4 * (SIZE + 2) + 2, 2 * (SIZE + 2) + 2)
    assert np.array_equal(np.asarray(img), np.asarray(image_grid.grid_image(want, nrow=4)))
    # no latents, no noises: drawn from the generator argument, the model draws its own injection noise
    img = generation.gen_matrix(g, ids_in_row=3, pose_in_col=2, generator=torch.Generator().manual_seed(2))
    assert img.size == (3 * (SIZE + 2) + 2, 2 * (SIZE + 2) + 2)
    assert generation.IterableModel(g, batch_size=3).gen_random().shape == (3, 3, SIZE, SIZE)


# ---- the entry's argument checks: nothing is launched, so they run without a GPU ----------------------------------------------------------
def test_argument_validation_without_gpu():
    from gan_control_amd import _lib
    lib = _lib.load()
    # [2, 3, 4, 5], nrow 8, padding 2 -> a 8 x 16 grid
    good = dict(x=1, row=5, plane=20, sample=60, y=1, ystride=48, batch=2, h=4, w=5, nrow=8, padding=2, pad=0, gh=8, gw=16)

    def call(**kw):
        a = dict(good, **kw)
        return lib.gc_image_f32_to_u8_grid(a['x'], a['row'], a['plane'], a['sample'], a['y'], a['ystride'], a['batch'], a['h'], a['w'], a['nrow'],
                                           a['padding'], a['pad'], a['gh'], a['gw'], None)

    for kw, text in (({'x': None}, b'null'), ({'y': None}, b'null'), ({'gh': 9}, b'grid_h'), ({'gw': 15}, b'grid_h'), ({'nrow': 1}, b'grid_h'),
                     ({'row': 4}, b'short stride'), ({'plane': 19}, b'short stride'), ({'sample': 59}, b'short stride'),
                     ({'ystride': 47}, b'short stride'), ({'batch': 0}, b'batch 0'), ({'h': 0}, b'batch 2'), ({'padding': -1}, b'padding -1'),
                     ({'pad': 256}, b'pad_value 256')):
        assert call(**kw) == -1, kw
        assert text in lib.gc_last_error(), (kw, lib.gc_last_error())
