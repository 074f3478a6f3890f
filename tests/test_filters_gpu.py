"""gaussian-filter and median-filter on the device: every result equals
scipy, run on the host in the same test, by np.array_equal. Shapes that
depend on the kernels' geometry are built from the constants of
csrc/filter.hip."""
import os
import re

import numpy as np
import pytest
import scipy.ndimage
import torch
from click.testing import CliRunner

from chunkflow_amd import filters
from chunkflow_amd.chunk import Chunk
from chunkflow_amd.filters import gaussian_filter_2d, median_filter
from chunkflow_amd.plugin import Plugin

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.uint8, np.float32]
GAUSS_CASES = [((3, 5), (2, 2)), ((1, 1), 1), ((2, 40), (3, 0.5)),
               ((33, 70), (1.5, 0)), ((17, 9), (0, 2))]


def constant(name):
    with open(os.path.join(REPO, 'chunkflow_amd', 'csrc',
                           'filter.hip')) as f:
        m = re.search(rf'constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;', f.read())
    assert m, f'filter.hip: {name} not found'
    return int(m.group(1))


TILE_Y, TILE_X = constant('GAUSS_TILE_Y'), constant('GAUSS_TILE_X')
MAX_RADIUS = constant('GAUSS_MAX_RADIUS')
MEDIAN_BLOCK = constant('MEDIAN_BLOCK')


def image(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.standard_normal(shape) * 50).astype(np.float32)


def scipy_gaussian(arr, sigma):
    out = np.empty_like(arr)
    for lead in np.ndindex(*arr.shape[:-2]):
        out[lead] = scipy.ndimage.gaussian_filter(arr[lead], sigma=sigma)
    return out


def scipy_median(arr, size, mode):
    if arr.ndim == 3:
        return scipy.ndimage.median_filter(arr, size=size, mode=mode)
    return np.stack([scipy.ndimage.median_filter(c, size=size, mode=mode)
                     for c in arr])


def device_gaussian(arr, sigma, **kwargs):
    out = gaussian_filter_2d(torch.from_numpy(arr).cuda(), sigma, **kwargs)
    assert out.is_device and out.shape == arr.shape
    return out.numpy().array


def device_median(arr, size, mode='reflect'):
    out = median_filter(torch.from_numpy(arr).cuda(), size=size, mode=mode)
    assert out.is_device and out.shape == arr.shape
    return out.numpy().array


# --- gaussian ----------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape,sigma', GAUSS_CASES)
def test_gaussian_cases(shape, sigma, dtype):
    arr = image((3,) + shape, dtype)
    got = device_gaussian(arr, sigma)
    assert got.dtype == arr.dtype
    assert np.array_equal(got, scipy_gaussian(arr, sigma))


def test_gaussian_uint8_truncation():
    const = np.full((2, 12, 20), 255, dtype=np.uint8)
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    for arr in (const, ramp, ramp.reshape(1, 4, 64)):
        for sigma in (1, 2, (0.7, 3)):
            assert np.array_equal(device_gaussian(arr, sigma),
                                  scipy_gaussian(arr, sigma))


@pytest.mark.parametrize('dtype', DTYPES)
def test_gaussian_4d_per_channel(dtype):
    arr = image((2, 3, 9, 14), dtype, seed=1)
    chunk = Chunk(torch.from_numpy(arr).cuda(), voxel_offset=(1, 2, 3),
                  voxel_size=(40, 4, 4))
    out = gaussian_filter_2d(chunk, (1, 1.5))
    assert out.is_device
    assert tuple(out.voxel_offset) == (1, 2, 3)
    assert tuple(out.voxel_size) == (40, 4, 4)
    assert np.array_equal(out.numpy().array, scipy_gaussian(arr, (1, 1.5)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_gaussian_tile_edges(dtype):
    """one tile plus one voxel in y and in x: an interior tile edge and a
    ragged last tile on both axes; then two tiles plus a ragged one"""
    for shape in ((2, TILE_Y + 1, TILE_X + 1),
                  (1, 2 * TILE_Y + 3, 2 * TILE_X + 5)):
        arr = image(shape, dtype, seed=2)
        for sigma in ((1.5, 1), 3):
            assert np.array_equal(device_gaussian(arr, sigma),
                                  scipy_gaussian(arr, sigma))


@pytest.mark.parametrize('dtype', DTYPES)
def test_gaussian_non_contiguous(dtype):
    base = image((3, 40, 50), dtype, seed=3)
    t = torch.from_numpy(base).cuda()
    for view, ref in ((t[:, ::2, 1:], base[:, ::2, 1:]),
                      (t.transpose(1, 2), base.transpose(0, 2, 1))):
        assert not view.is_contiguous()
        out = gaussian_filter_2d(view, 1)
        assert np.array_equal(out.numpy().array,
                              scipy_gaussian(np.ascontiguousarray(ref), 1))
    assert np.array_equal(t.cpu().numpy(), base)
    # in place through a strided view
    view = t[:, ::2, 1:]
    gaussian_filter_2d(view, 1, inplace=True)
    assert np.array_equal(
        t.cpu().numpy()[:, ::2, 1:],
        scipy_gaussian(np.ascontiguousarray(base[:, ::2, 1:]), 1))
    assert np.array_equal(t.cpu().numpy()[:, 1::2], base[:, 1::2])


@pytest.mark.parametrize('dtype', DTYPES)
def test_gaussian_radius_cap(dtype):
    arr = image((2, TILE_Y + 8, TILE_X + 6), dtype, seed=4)
    at_cap = MAX_RADIUS / 4.0
    assert filters.gaussian_weights(at_cap)[0] == MAX_RADIUS
    assert np.array_equal(device_gaussian(arr, at_cap),
                          scipy_gaussian(arr, at_cap))
    # the cap against axes shorter than the radius
    small = image((2, 5, 3), dtype, seed=5)
    assert np.array_equal(device_gaussian(small, at_cap),
                          scipy_gaussian(small, at_cap))
    above = (MAX_RADIUS + 1) / 4.0
    assert filters.gaussian_weights(above)[0] == MAX_RADIUS + 1
    for sigma in (above, (above, 1), (1, above)):
        with pytest.raises(ValueError, match=f'cap of {MAX_RADIUS}'):
            gaussian_filter_2d(torch.from_numpy(arr).cuda(), sigma)


def test_gaussian_library_refuses_what_it_cannot_hold():
    """the C entry itself, behind the Python checks"""
    from chunkflow_amd.hip import CfxError
    from chunkflow_amd.ops import shared_hip_ops
    cfx = shared_hip_ops(0).cfx
    t = torch.zeros((1, 8, 8), dtype=torch.uint8, device='cuda')
    out = torch.full_like(t, 7)
    w = torch.ones(2 * MAX_RADIUS + 3, dtype=torch.float64, device='cuda')
    with pytest.raises(CfxError, match=str(MAX_RADIUS)):
        cfx.gaussian2d(t.data_ptr(), out.data_ptr(), False, 1, 8, 8,
                       w.data_ptr(), MAX_RADIUS + 1, None, 0)
    with pytest.raises(CfxError):
        cfx.gaussian2d(t.data_ptr(), t.data_ptr(), False, 1, 8, 8,
                       w.data_ptr(), 1, None, 0)
    with pytest.raises(CfxError):
        cfx.gaussian2d(t.data_ptr(), out.data_ptr(), False, 1, 8, 8,
                       None, 1, None, 0)
    assert (out == 7).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_gaussian_inplace(dtype):
    arr = image((3, 20, 30), dtype, seed=6)
    t = torch.from_numpy(arr).cuda()
    chunk = Chunk(t, voxel_offset=(5, 6, 7))
    ptr = t.data_ptr()
    out = gaussian_filter_2d(chunk, 2, inplace=True)
    assert out.array.data_ptr() == ptr and chunk.array.data_ptr() == ptr
    assert tuple(out.voxel_offset) == (5, 6, 7)
    assert np.array_equal(t.cpu().numpy(), scipy_gaussian(arr, 2))
    # not in place: a new array, the input untouched
    t2 = torch.from_numpy(arr).cuda()
    out = gaussian_filter_2d(t2, 2)
    assert out.array.data_ptr() != t2.data_ptr()
    assert np.array_equal(t2.cpu().numpy(), arr)
    # Chunk.gaussian_filter_2d is the in-place form
    chunk = Chunk(torch.from_numpy(arr).cuda())
    ptr = chunk.array.data_ptr()
    assert chunk.gaussian_filter_2d(2) is chunk
    assert chunk.array.data_ptr() == ptr
    assert np.array_equal(chunk.numpy().array, scipy_gaussian(arr, 2))


def test_gaussian_both_axes_skipped_is_a_copy():
    arr = image((2, 6, 7), np.float32, seed=7)
    assert np.array_equal(device_gaussian(arr, 0), arr)


# --- median ------------------------------------------------------------------
def median_data(shape, kind, seed=0):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == 'u8_ties':
        arr = rng.integers(0, 8, shape, dtype=np.uint8)
    elif kind == 'u8_full':
        arr = rng.integers(0, 256, shape, dtype=np.uint8)
        arr.flat[n // 3] = 0
        arr.flat[-1] = 255
    else:
        # negatives, repeated values and both infinities, no NaN
        arr = (rng.integers(-4, 5, shape) * 0.75).astype(np.float32)
        arr[rng.random(shape) < 0.3] *= np.float32(1e-3)
        arr.flat[n // 3] = np.inf
        arr.flat[-1] = -np.inf
        assert not np.isnan(arr).any()
    return arr


KINDS = ['u8_ties', 'u8_full', 'f32']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('mode', filters.MODES)
def test_median_modes(mode, kind):
    arr = median_data((7, 9, 11), kind)
    assert np.array_equal(device_median(arr, (3, 3, 3), mode),
                          scipy_median(arr, (3, 3, 3), mode))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape,size', [
    ((2, 3, 4), (3, 1, 1)), ((2, 3, 4), (1, 3, 1)), ((2, 3, 4), (1, 1, 3)),
    ((1, 1, 1), (3, 3, 3)), ((4, 6, 5), (5, 3, 1)), ((3, 4, 9), (1, 5, 5)),
    ((5, 5, 5), (5, 5, 5)), ((3, 4, 5), (1, 1, 1))])
def test_median_cases(shape, size, kind):
    arr = median_data(shape, kind, seed=1)
    assert np.array_equal(device_median(arr, size),
                          scipy_median(arr, size, 'reflect'))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('mode', filters.MODES)
def test_median_of_three_paths(mode, kind):
    """windows of three voxels: rows of whole 16-byte groups take the vector
    kernel along z and y (more than one workgroup of them here), every
    other row width and the x axis the one-voxel-per-lane kernel"""
    for shape in ((6, 40, 32), (3, 5, 37), (1, 2, 16)):
        arr = median_data(shape, kind, seed=2)
        for size in ((3, 1, 1), (1, 3, 1), (1, 1, 3)):
            assert np.array_equal(device_median(arr, size, mode),
                                  scipy_median(arr, size, mode)), (shape,
                                                                   size)


@pytest.mark.parametrize('kind', KINDS)
def test_median_more_than_one_workgroup(kind):
    """rows longer than a workgroup, so that workgroups change along x, y
    and z, with a ragged last one"""
    arr = median_data((3, 3, MEDIAN_BLOCK + 5), kind, seed=3)
    for size, mode in (((3, 3, 3), 'reflect'), ((1, 1, 3), 'mirror'),
                       ((3, 1, 5), 'wrap')):
        assert np.array_equal(device_median(arr, size, mode),
                              scipy_median(arr, size, mode))


@pytest.mark.parametrize('kind', KINDS)
def test_median_4d_per_channel(kind):
    arr = median_data((2, 4, 6, 16), kind, seed=4)
    chunk = Chunk(torch.from_numpy(arr).cuda(), voxel_offset=(1, 2, 3),
                  voxel_size=(8, 8, 8))
    for size in ((3, 1, 1), (3, 3, 3)):
        out = median_filter(chunk, size=size, mode='nearest')
        assert out.is_device and tuple(out.voxel_offset) == (1, 2, 3)
        assert tuple(out.voxel_size) == (8, 8, 8)
        assert np.array_equal(out.numpy().array,
                              scipy_median(arr, size, 'nearest'))
    assert np.array_equal(chunk.numpy().array, arr)


def test_median_non_contiguous_input():
    base = median_data((6, 8, 20), 'f32', seed=5)
    view = torch.from_numpy(base).cuda()[::2, :, 2:18]
    assert not view.is_contiguous()
    assert np.array_equal(
        median_filter(view, (3, 3, 1)).numpy().array,
        scipy_median(np.ascontiguousarray(base[::2, :, 2:18]), (3, 3, 1),
                     'reflect'))


def test_device_errors():
    t = torch.zeros((4, 4, 4), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='odd'):
        median_filter(t, (2, 1, 1))
    with pytest.raises(ValueError, match='125'):
        median_filter(t, (5, 5, 7))
    with pytest.raises(ValueError, match='mode'):
        median_filter(t, (3, 1, 1), mode='grid-wrap')
    with pytest.raises(TypeError):
        median_filter(t.to(torch.int32))
    with pytest.raises(TypeError):
        gaussian_filter_2d(t.to(torch.int32))
    with pytest.raises(ValueError, match='negative'):
        gaussian_filter_2d(t, -1)


def test_indices_past_2_to_the_31():
    """a uint8 volume of more than 2^31 voxels: the last slab of every
    kernel's result equals scipy on the slab it depends on"""
    d, h, w = 2 ** 31 // (1024 * 1024) + 2, 1024, 1024
    assert d * h * w > 2 ** 31
    t = torch.randint(0, 256, (d, h, w), dtype=torch.uint8, device='cuda')
    tail = t[-4:].cpu().numpy()
    out = gaussian_filter_2d(t, 1).array[-1:].cpu().numpy()
    assert np.array_equal(out, scipy_gaussian(tail[-1:], 1))
    for size in ((3, 1, 1), (1, 1, 3), (3, 3, 1)):
        out = median_filter(t, size).array[-2:].cpu().numpy()
        assert np.array_equal(out,
                              scipy_median(tail, size, 'reflect')[-2:]), size


# --- operator and plugins ----------------------------------------------------
def test_operator_on_the_device(tmp_path):
    from chunkflow_amd.flow import gaussian_filter as command, main
    arr = image((3, 12, 18), np.uint8, seed=8)
    task = {'chunk': Chunk(arr.copy(), voxel_offset=(2, 0, 0)),
            'log': {'timer': {}}}
    stage = command.callback(name='gaussian-filter',
                             input_chunk_name='chunk', sigma=2)
    out = list(stage(iter([None, task])))
    assert out[0] is None and out[1] is task
    assert 'gaussian-filter' in task['log']['timer']
    assert task['chunk'].is_device       # uploaded, and it stays there
    assert tuple(task['chunk'].voxel_offset) == (2, 0, 0)
    assert np.array_equal(task['chunk'].numpy().array,
                          scipy_gaussian(arr, 2))
    # and through the command line
    before, after = tmp_path / 'before.npy', tmp_path / 'after.npy'
    result = CliRunner().invoke(main, [
        'create-chunk', '--size', '3', '10', '12', '--dtype', 'uint8',
        'save-npy', '-f', str(before), 'gaussian-filter',
        'save-npy', '-f', str(after)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    assert np.array_equal(np.load(after),
                          scipy_gaussian(np.load(before), 1))


def test_plugins_on_the_device():
    arr = image((4, 10, 16), np.float32, seed=9)
    chunk = Chunk(torch.from_numpy(arr).cuda(), voxel_offset=(3, 2, 1))
    out = Plugin('gaussian_filter')([chunk], args='sigma=2')
    assert out.is_device and tuple(out.voxel_offset) == (3, 2, 1)
    host = Plugin('gaussian_filter')([Chunk(arr.copy())], args='sigma=2')
    assert np.array_equal(out.numpy().array, host.array)
    assert np.array_equal(host.array, scipy_gaussian(arr, 2))
    assert np.array_equal(chunk.numpy().array, arr)

    out = Plugin('median_filter')([chunk], args='size=(3,1,1)')
    assert isinstance(out, list) and out[0].is_device
    assert tuple(out[0].voxel_offset) == (3, 2, 1)
    host = Plugin('median_filter')([Chunk(arr.copy())], args='size=(3,1,1)')
    assert np.array_equal(out[0].numpy().array, host[0].array)
    assert np.array_equal(host[0].array,
                          scipy_median(arr, (3, 1, 1), 'reflect'))
    out = Plugin('median_filter')([chunk], args='size=(3,3,3);mode=mirror')
    assert np.array_equal(out[0].numpy().array,
                          scipy_median(arr, (3, 3, 3), 'mirror'))
