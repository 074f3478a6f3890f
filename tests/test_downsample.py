"""downsample on the host: the numpy path is pinned byte-for-byte to the
reference's vendored numpy implementation through
tests/golden/downsample_cases.npz (tools/gen_downsample_golden.py)."""
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from chunkflow_amd.chunk import Chunk
from chunkflow_amd.downsample import (average_host, downsample,
                                      downsample_pyramid, mode_host)
from chunkflow_amd.flow import main
from chunkflow_amd.ops import TorchOps

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden',
                      'downsample_cases.npz')


@pytest.fixture(scope='module')
def cases():
    z = np.load(GOLDEN)
    names = sorted({k.rsplit('/', 1)[0] for k in z.files})
    return [(n, z[n + '/in'], tuple(int(f) for f in z[n + '/factor']),
             z[n + '/out']) for n in names]


def same_bytes(got, want):
    return (got.dtype == want.dtype and got.shape == want.shape
            and np.ascontiguousarray(got).tobytes() == want.tobytes())


def test_golden_covers_the_issue_cases(cases):
    names = [c[0] for c in cases]
    assert sum(n.startswith('avg_u8') for n in names) == 25
    assert sum(n.startswith('avg_f32') for n in names) == 25
    assert sum(n.startswith('mode_uint32') for n in names) == 51
    assert sum(n.startswith('mode_uint64') for n in names) == 51
    u32 = np.concatenate([c[1].ravel() for c in cases
                          if c[0].startswith('mode_uint32')])
    assert (u32 >= 2**31).any() and (u32 == 0).any()
    u64 = np.unique(np.concatenate([c[1].ravel() for c in cases
                                    if c[0].startswith('mode_uint64_a2')]))
    assert len(u64) == 2 and (u64[0] ^ u64[1]) & np.uint64(0xffffffff) == 0


def test_host_path_equals_every_golden_case(cases):
    bad = []
    for name, arr, factor, want in cases:
        chunk = Chunk(arr.copy())
        if arr.ndim == 4 and arr.dtype == np.uint8:
            # no chunk type: pins the channel loop below the dispatch
            got = average_host(chunk.array, factor)
        else:
            got = downsample(chunk, factor).array
        if not same_bytes(got, want):
            bad.append((name, arr.shape, factor))
        assert np.array_equal(chunk.array, arr), 'input was modified'
    assert not bad, bad


def test_uint8_average_truncates():
    arr = np.array([[[0, 255], [255, 255]]], dtype=np.uint8)  # 191.25
    assert downsample(Chunk(arr), (1, 2, 2)).array.tolist() == [[[191]]]
    arr = np.array([[[1, 2], [2, 2]]], dtype=np.uint8)  # 1.75
    assert downsample(Chunk(arr), (1, 2, 2)).array.tolist() == [[[1]]]


def test_mode2_odd_axis_front_mirror():
    arr = np.array([[[3, 2, 4]]], dtype=np.uint32).repeat(2, axis=1)
    # x: [3,2,4] -> [3,3,2,4] -> blocks (3,3) and (2,4)
    got = downsample(Chunk(arr), (1, 2, 2)).array
    assert got.tolist() == [[[3, 2]]]


def test_identity_factor_returns_input():
    arr = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    assert downsample(Chunk(arr), (1, 1, 1)).array is arr
    seg = arr.astype(np.uint32)
    assert downsample(Chunk(seg), (1, 1, 1)).array is seg


def test_voxel_offset_and_size():
    arr = np.zeros((4, 6, 8), dtype=np.uint8)
    out = downsample(Chunk(arr, voxel_offset=(5, 6, 7),
                           voxel_size=(40, 4, 4)), (1, 2, 2))
    assert tuple(out.voxel_offset) == (5, 3, 3)
    assert tuple(out.voxel_size) == (40, 8, 8)
    assert out.shape == (4, 3, 4)
    out = downsample(Chunk(arr, voxel_offset=(-3, 9, 2)), (2, 2, 2))
    assert tuple(out.voxel_offset) == (-2, 4, 1)
    assert out.voxel_size is None
    aff = np.zeros((3, 4, 6, 8), dtype=np.float32)
    out = downsample(Chunk(aff, voxel_offset=(2, 2, 2)), (2, 2, 2))
    assert out.shape == (3, 2, 3, 4)
    assert tuple(out.voxel_offset) == (1, 1, 1)


@pytest.mark.parametrize('shape,factor', [
    ((4, 8, 8), (1, 4, 4)), ((8, 8, 8), (4, 4, 4)), ((4, 4, 4), (1, 2, 1)),
    ((4, 4, 4), (2, 2, 4)), ((5, 5, 5), (1, 1, 2)),
])
def test_rejected_mode_factors(shape, factor):
    seg = np.zeros(shape, dtype=np.uint32)
    with pytest.raises(ValueError, match='downsample_pyramid'):
        downsample(Chunk(seg), factor)


def test_nonpositive_factor_rejected():
    for arr in (np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint32)):
        with pytest.raises(ValueError):
            downsample(Chunk(arr), (2, 0, 2))


@pytest.mark.parametrize('arr', [
    np.zeros((4, 4, 4), dtype=bool),
    np.zeros((4, 4, 4), dtype=np.float64),
    np.zeros((2, 4, 4, 4), dtype=np.uint8),
    np.zeros((2, 4, 4, 4), dtype=np.uint32),
], ids=['bool', 'float64', 'uint8-4d', 'uint32-4d'])
def test_unsupported_chunks_raise_type_error(arr):
    with pytest.raises(TypeError,
                       match='only support image or segmentation, but got'):
        downsample(Chunk(arr), (2, 2, 2))


def test_power_of_two_factor_on_odd_shape_strides():
    seg = np.arange(5 * 7 * 9, dtype=np.uint32).reshape(5, 7, 9)
    got = downsample(Chunk(seg), (4, 4, 4)).array
    assert np.array_equal(got, seg[::4, ::4, ::4])


def test_pyramid_equals_repeated_calls():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(9, 21, 37), dtype=np.uint8)
    seg = rng.integers(0, 4, size=(6, 21, 37)).astype(np.uint64)
    for arr, factor in ((img, (1, 2, 2)), (img, (2, 2, 2)),
                        (seg, (1, 2, 2))):
        chunk = Chunk(arr, voxel_offset=(8, 17, 33), voxel_size=(40, 4, 4))
        levels = downsample_pyramid(chunk, factor, 3)
        assert len(levels) == 3
        step = chunk
        for level in levels:
            step = downsample(step, factor)
            assert same_bytes(level.array, step.array)
            assert level.voxel_offset == step.voxel_offset
            assert level.voxel_size == step.voxel_size
        assert tuple(levels[2].voxel_size) == tuple(
            v * f ** 3 for v, f in zip((40, 4, 4), factor))


def test_cli_chain(tmp_path):
    full, half = tmp_path / 'full.npy', tmp_path / 'half.npy'
    runner = CliRunner()
    result = runner.invoke(main, [
        'create-chunk', '--size', '6', '10', '14', '--dtype', 'uint8',
        '--pattern', 'sin', 'save-npy', '-f', str(full),
        'downsample', '-f', '1', '2', '2', '-i', 'chunk', '-o', 'mip1',
        'save-npy', '-i', 'mip1', '-f', str(half)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    src, got = np.load(full), np.load(half)
    assert got.shape == (6, 5, 7) and got.dtype == np.uint8
    assert same_bytes(got, average_host(src, (1, 2, 2)))


def test_cli_default_factor(tmp_path):
    out = tmp_path / 'seg.npy'
    result = CliRunner().invoke(main, [
        'create-chunk', '--size', '8', '8', '8', '--dtype', 'uint32',
        'downsample', 'save-npy', '-f', str(out)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    got = np.load(out)
    assert got.shape == (4, 4, 4) and got.dtype == np.uint32


def test_torch_ops_equal_host_path(cases):
    ops = TorchOps()
    as_signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    for name, arr, factor, want in cases:
        if name.startswith('avg_'):
            got = ops.downsample_average(torch.from_numpy(arr.copy()), factor)
            assert same_bytes(got.numpy(), average_host(arr, factor)), name
        else:
            # device tensors carry uint32/uint64 labels as int32/int64
            signed = arr.view(as_signed[arr.dtype]).copy()
            got = ops.downsample_mode(torch.from_numpy(signed), factor)
            host = mode_host(arr, factor)
            assert same_bytes(got.numpy().view(arr.dtype), host), name
    with pytest.raises(TypeError):
        ops.downsample_mode(torch.zeros((2, 2, 2)), (2, 2, 2))
    with pytest.raises(TypeError):
        ops.downsample_average(torch.zeros((2, 2, 2), dtype=torch.int32),
                               (2, 2, 2))
