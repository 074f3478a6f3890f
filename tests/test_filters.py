"""gaussian-filter and median-filter without a GPU: the numpy restatement of
the kernel arithmetic against scipy, the host paths, the operator, the
plugins, the device-rule checkers and the C-ABI symbols. Every comparison
is np.array_equal."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.ndimage
import torch
from click.testing import CliRunner

from chunkflow_amd import filters
from chunkflow_amd.chunk import Chunk
from chunkflow_amd.filters import (check_gaussian_device,
                                   check_median_device, gaussian_filter_2d,
                                   gaussian_filter_2d_restated,
                                   median_filter, median_filter_restated)
from chunkflow_amd.flow import main
from chunkflow_amd.plugin import Plugin

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (section shape, (sigma_y, sigma_x)): a radius above the axis length, a
# single voxel, each axis skipped in turn
GAUSS_CASES = [((3, 5), (2, 2)), ((1, 1), 1), ((2, 40), (3, 0.5)),
               ((33, 70), (1.5, 0)), ((17, 9), (0, 2))]
MEDIAN_CASES = [((7, 9, 11), (3, 3, 3)), ((2, 3, 4), (3, 1, 1)),
                ((2, 3, 4), (1, 3, 1)), ((2, 3, 4), (1, 1, 3)),
                ((1, 1, 1), (3, 3, 3)), ((4, 6, 5), (5, 3, 1)),
                ((3, 4, 9), (1, 5, 5)), ((5, 5, 5), (5, 5, 5))]


def sections(shape, dtype, seed=0, count=2):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (count,) + shape, dtype=np.uint8)
    return (rng.standard_normal((count,) + shape) * 50).astype(np.float32)


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


# --- the restatement is scipy ------------------------------------------------
@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('shape,sigma', GAUSS_CASES)
def test_restated_gaussian_equals_scipy(shape, sigma, dtype):
    arr = sections(shape, dtype)
    got = gaussian_filter_2d_restated(arr, sigma)
    assert got.dtype == arr.dtype
    assert np.array_equal(got, scipy_gaussian(arr, sigma))


def test_restated_gaussian_uint8_truncates():
    const = np.full((1, 12, 20), 255, dtype=np.uint8)
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    for arr in (const, ramp, ramp.reshape(1, 4, 64)):
        for sigma in (1, 2, (0.7, 3)):
            want = scipy_gaussian(arr, sigma)
            assert np.array_equal(gaussian_filter_2d_restated(arr, sigma),
                                  want)
    # rounding instead of truncating would not pass: some ramp voxel's f64
    # sum has a fraction of one half or more
    w = filters.gaussian_weights(1)
    t = ramp[0].astype(np.float64)
    rows = filters.border_index(np.arange(16)[:, None]
                                + np.arange(-4, 5)[None, :], 16, 'reflect')
    frac = np.modf((t[rows] * w[1][None, :, None]).sum(axis=1))[0]
    assert (frac >= 0.5).any()


@pytest.mark.parametrize('mode', filters.MODES)
@pytest.mark.parametrize('shape,size', MEDIAN_CASES)
def test_restated_median_equals_scipy(shape, size, mode):
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 8, shape, dtype=np.uint8)
    f32 = rng.integers(-3, 4, shape).astype(np.float32) * 0.5
    f32.flat[0], f32.flat[-1] = np.inf, -np.inf
    for arr in (u8, f32):
        assert np.array_equal(median_filter_restated(arr, size, mode),
                              scipy.ndimage.median_filter(arr, size=size,
                                                          mode=mode))


# --- host paths --------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('lead', [(3,), (2, 3)])
def test_host_gaussian(lead, dtype):
    arr = sections((9, 14), dtype, seed=1, count=int(np.prod(lead)))
    arr = arr.reshape(lead + (9, 14))
    chunk = Chunk(arr.copy(), voxel_offset=(4, 5, 6), voxel_size=(40, 4, 4))
    want = scipy_gaussian(arr, (1.5, 1))
    out = gaussian_filter_2d(chunk, (1.5, 1))
    assert isinstance(out, Chunk) and out.array is not chunk.array
    assert np.array_equal(out.array, want)
    assert np.array_equal(chunk.array, arr)          # input untouched
    assert tuple(out.voxel_offset) == (4, 5, 6)
    assert tuple(out.voxel_size) == (40, 4, 4)
    same = gaussian_filter_2d(chunk, (1.5, 1), inplace=True)
    assert same.array is chunk.array
    assert np.array_equal(chunk.array, want)
    # the reference's method name, in place
    again = Chunk(arr.copy())
    assert again.gaussian_filter_2d((1.5, 1)) is again
    assert np.array_equal(again.array, want)


def test_host_gaussian_accepts_arrays_and_tensors():
    arr = sections((6, 7), np.float32, seed=2, count=3)
    want = scipy_gaussian(arr, 1)
    assert np.array_equal(gaussian_filter_2d(arr).array, want)
    t = torch.from_numpy(arr.copy())
    assert np.array_equal(gaussian_filter_2d(t).numpy().array, want)
    assert np.array_equal(t.numpy(), arr)
    gaussian_filter_2d(t, inplace=True)
    assert np.array_equal(t.numpy(), want)


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('lead', [(), (2,)])
def test_host_median(lead, dtype):
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 200, lead + (4, 6, 5)).astype(dtype)
    chunk = Chunk(arr.copy(), voxel_offset=(1, 2, 3), voxel_size=(8, 8, 8))
    for size, mode in (((3, 1, 1), 'reflect'), ((3, 3, 3), 'mirror')):
        out = median_filter(chunk, size=size, mode=mode)
        assert np.array_equal(out.array, scipy_median(arr, size, mode))
        assert out.array.dtype == arr.dtype
        assert tuple(out.voxel_offset) == (1, 2, 3)
        assert tuple(out.voxel_size) == (8, 8, 8)
    assert np.array_equal(chunk.array, arr)
    # defaults: the z-median
    assert np.array_equal(median_filter(arr).array,
                          scipy_median(arr, (3, 1, 1), 'reflect'))


# --- operator and plugins ----------------------------------------------------
def test_operator_through_cli(tmp_path):
    before, after = tmp_path / 'before.npy', tmp_path / 'after.npy'
    result = CliRunner().invoke(main, [
        'create-chunk', '--size', '3', '10', '12', '--dtype', 'uint8',
        'save-npy', '-f', str(before),
        'gaussian-filter', '--sigma', '2',
        'save-npy', '-f', str(after)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    src, got = np.load(before), np.load(after)
    assert got.dtype == np.uint8
    assert np.array_equal(got, scipy_gaussian(src, 2))
    assert not np.array_equal(got, src)


def test_operator_timer_and_none_task():
    from chunkflow_amd.flow import gaussian_filter as command
    arr = sections((8, 8), np.uint8, seed=7, count=2)
    task = {'img': Chunk(arr.copy()), 'log': {'timer': {}}}
    stage = command.callback(name='blur', input_chunk_name='img', sigma=1)
    out = list(stage(iter([None, task])))
    assert out[0] is None
    assert out[1] is task and 'blur' in task['log']['timer']
    assert np.array_equal(task['img'].numpy().array, scipy_gaussian(arr, 1))


def test_plugins():
    arr = sections((7, 9), np.float32, seed=8, count=4)
    chunk = Chunk(arr.copy(), voxel_offset=(3, 2, 1))
    out = Plugin('gaussian_filter')([chunk], args='sigma=2')
    assert isinstance(out, Chunk) and tuple(out.voxel_offset) == (3, 2, 1)
    assert np.array_equal(out.array, scipy_gaussian(arr, 2))
    assert np.array_equal(chunk.array, arr)
    Plugin('gaussian_filter')([chunk], args='sigma=2;inplace=True')
    assert np.array_equal(chunk.array, scipy_gaussian(arr, 2))

    chunk = Chunk(arr.copy(), voxel_offset=(3, 2, 1))
    out = Plugin('median_filter')([chunk])
    assert isinstance(out, list) and len(out) == 1
    assert np.array_equal(out[0].array,
                          scipy_median(arr, (3, 1, 1), 'reflect'))
    out = Plugin('median_filter')([chunk], args='size=(3,3,1);mode=wrap')
    assert tuple(out[0].voxel_offset) == (3, 2, 1)
    assert np.array_equal(out[0].array, scipy_median(arr, (3, 3, 1), 'wrap'))
    # a bare array comes back as a chunk
    out = Plugin('median_filter')([arr], args='size=(3,1,1)')
    assert np.array_equal(out[0].array,
                          scipy_median(arr, (3, 1, 1), 'reflect'))


def test_plugin_through_cli(tmp_path):
    before, after = tmp_path / 'before.npy', tmp_path / 'after.npy'
    result = CliRunner().invoke(main, [
        'create-chunk', '--size', '5', '6', '7', '--dtype', 'uint8',
        'save-npy', '-f', str(before),
        'plugin', '-f', 'median_filter', '-i', 'chunk', '-o', 'chunk',
        '--args', 'size=(3,1,1)',
        'save-npy', '-f', str(after)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    assert np.array_equal(
        np.load(after), scipy_median(np.load(before), (3, 1, 1), 'reflect'))


# --- the device rules, checked without a device -----------------------------
def test_device_rule_errors():
    with pytest.raises(ValueError, match='odd'):
        check_median_device(np.uint8, (2, 1, 1), 'reflect')
    with pytest.raises(ValueError, match='125'):
        check_median_device(np.uint8, (5, 5, 7), 'reflect')
    with pytest.raises(ValueError, match='mode'):
        check_median_device(np.uint8, (3, 1, 1), 'grid-wrap')
    with pytest.raises(ValueError, match='3 entries'):
        check_median_device(np.uint8, (3, 3), 'reflect')
    with pytest.raises(TypeError):
        check_median_device(np.int32, (3, 1, 1), 'reflect')
    with pytest.raises(TypeError):
        check_median_device(torch.int32, (3, 1, 1), 'reflect')
    with pytest.raises(TypeError):
        check_gaussian_device(np.int32, 1)
    with pytest.raises(ValueError, match='negative'):
        check_gaussian_device(np.uint8, -1)
    with pytest.raises(ValueError, match='sigma_y'):
        check_gaussian_device(np.uint8, (1, 2, 3))
    cap = filters.GAUSS_MAX_RADIUS
    assert check_gaussian_device(torch.float32, cap / 4.0)[0][0] == cap
    with pytest.raises(ValueError, match=f'cap of {cap}'):
        check_gaussian_device(np.float32, (cap + 1) / 4.0)
    assert check_median_device(torch.uint8, (5, 5, 5), 'wrap') == \
        ((5, 5, 5), 4)
    assert check_gaussian_device(np.uint8, (0, 1))[0] is None
    # the host path has the same argument rules
    with pytest.raises(ValueError):
        gaussian_filter_2d(np.zeros((2, 3, 4), np.uint8), -1)
    with pytest.raises(ValueError):
        median_filter(np.zeros((2, 3, 4), np.uint8), mode='bogus')
    with pytest.raises(ValueError):
        median_filter(np.zeros((5,), np.uint8))


def test_constants_match_the_kernel_source():
    with open(os.path.join(REPO, 'chunkflow_amd', 'csrc',
                           'filter.hip')) as f:
        text = f.read()

    def constant(name):
        return int(re.search(rf'constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;',
                             text).group(1))
    assert constant('GAUSS_MAX_RADIUS') == filters.GAUSS_MAX_RADIUS
    assert constant('MEDIAN_MAX_WINDOW') == filters.MEDIAN_MAX_WINDOW
    # the halo at the cap fits the 64 KiB of LDS a launch may ask for
    ty, tx = constant('GAUSS_TILE_Y'), constant('GAUSS_TILE_X')
    r = filters.GAUSS_MAX_RADIUS
    assert (2 * ty + 2 * r) * (tx + 2 * r) * 4 <= 65536
    # one lane's keys at the cap fit the median's LDS budget at wave width
    assert 64 * filters.MEDIAN_MAX_WINDOW * 4 <= constant('MEDIAN_LDS_BYTES')


def test_symbols():
    from chunkflow_amd.build import build
    from chunkflow_amd.hip import KERNEL_IDS, SIGNATURES, SYMBOLS
    lib = ctypes.CDLL(build())
    for sym in ('cfx_gaussian2d', 'cfx_median3d'):
        assert sym in SYMBOLS and sym in SIGNATURES
        assert hasattr(lib, sym)
    assert len(KERNEL_IDS) == 13
