"""downsample on the device: the gfx950 kernels equal the golden cases and
the host path (itself pinned by the goldens in tests/test_downsample.py)
byte-for-byte."""
import os

import numpy as np
import pytest
import torch

from chunkflow_amd.chunk import Chunk
from chunkflow_amd.downsample import (average_host, downsample,
                                      downsample_pyramid, mode_host)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden',
                      'downsample_cases.npz')
SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}

ZY = (1, 2, 3, 5, 8)
# X: vector body, tail and unaligned row starts (uint8 with odd X)
XS = (1, 2, 15, 16, 17, 33, 70)
AVG_FACTORS = ((2, 2, 2), (1, 2, 2), (2, 1, 2), (2, 2, 1), (1, 1, 2),
               (1, 2, 1), (2, 1, 1), (3, 2, 2), (2, 3, 5), (1, 1, 3))


@pytest.fixture(scope='module')
def ops():
    from chunkflow_amd.ops import HipOps
    return HipOps(0)


def same_bytes(got, want):
    return (got.dtype == want.dtype and got.shape == want.shape
            and np.ascontiguousarray(got).tobytes() == want.tobytes())


def to_device(arr, misalign=False):
    """Upload; uint32/uint64 labels travel as int32/int64. With misalign the
    tensor starts one element into its buffer, so its rows are not 16-byte
    aligned whatever the shape."""
    if arr.dtype in SIGNED:
        arr = arr.view(SIGNED[arr.dtype])
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if not misalign:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def from_device(t, dtype):
    return t.cpu().numpy().view(dtype)


def fuzz_shapes(xs, big_xs, n=40, even=False):
    """n seeded (z,y,x) shapes: every X of xs and big_xs at least once."""
    rng = np.random.default_rng(7)
    zy = [v for v in ZY if not even or v % 2 == 0]
    pool = list(xs) + list(big_xs)
    shapes = []
    for i in range(n):
        x = pool[i % len(pool)]
        shapes.append((int(rng.choice(zy)), int(rng.choice(zy)), x))
    return shapes


def test_device_path_equals_every_golden_case(ops):
    z = np.load(GOLDEN)
    names = sorted({k.rsplit('/', 1)[0] for k in z.files})
    assert len(names) == 152
    bad = []
    for name in names:
        arr = z[name + '/in']
        factor = tuple(int(f) for f in z[name + '/factor'])
        if arr.ndim == 4 and arr.dtype == np.uint8:
            # no chunk type: pins the channel loop below the dispatch
            got = ops.downsample_average(to_device(arr), factor)
        else:
            got = downsample(Chunk(to_device(arr)), factor).array
        assert got.is_cuda
        if not same_bytes(from_device(got, arr.dtype),
                          z[name + '/out']):
            bad.append((name, arr.shape, factor))
    assert not bad, bad


@pytest.mark.parametrize('dtype,big_xs', [
    # 2*256*2+3: general kernel past one workgroup; 16-byte chunks * 259:
    # vector kernel past one workgroup
    (np.uint8, (1027, 16 * 259)),
    (np.float32, (1027, 4 * 259)),
], ids=['u8', 'f32'])
def test_average_fuzz_equals_host(ops, dtype, big_xs):
    rng = np.random.default_rng(11)
    bad = []
    for i, shape in enumerate(fuzz_shapes(XS, big_xs)):
        factor = AVG_FACTORS[i % len(AVG_FACTORS)]
        if dtype == np.uint8:
            arr = rng.integers(0, 256, size=shape, dtype=np.uint8)
        else:
            arr = (rng.standard_normal(shape) * 10.0 ** rng.integers(
                -3, 6, size=shape)).astype(np.float32)
        got = ops.downsample_average(to_device(arr, misalign=i % 5 == 4),
                                     factor)
        if not same_bytes(from_device(got, dtype), average_host(arr, factor)):
            bad.append((shape, factor))
    assert not bad, bad


@pytest.mark.parametrize('dtype,big_xs', [
    (np.uint32, (1027, 4 * 259)),
    (np.uint64, (1027, 2 * 259)),
], ids=['u32', 'u64'])
def test_mode2_fuzz_equals_host(ops, dtype, big_xs):
    rng = np.random.default_rng(13)
    factors = ((1, 2, 2), (2, 1, 2), (2, 2, 1))
    bad = []
    for i, shape in enumerate(fuzz_shapes(XS, big_xs, n=42)):
        factor = factors[i % 3]
        nlabels = (2, 3, 50)[(i // 3) % 3]
        arr = rng.integers(0, nlabels, size=shape).astype(dtype)
        if dtype == np.uint64:
            arr = (arr << np.uint64(32)) + np.uint64(9)  # high halves differ
        else:
            arr = arr * np.uint32(2**31 // 25)           # some >= 2**31
        got = ops.downsample_mode(to_device(arr, misalign=i % 5 == 4),
                                  factor)
        if not same_bytes(from_device(got, dtype), mode_host(arr, factor)):
            bad.append((shape, factor))
    assert not bad, bad


@pytest.mark.parametrize('dtype,xs,big_xs', [
    # uint32: X % 4 == 0 takes the vector kernel, X % 4 == 2 the general one
    (np.uint32, (2, 16, 70, 4, 6, 32), (4 * 259, 4 * 259 + 2)),
    # uint64: every even X is 16-byte aligned; misalignment runs the general
    (np.uint64, (2, 16, 70, 4, 6, 32), (2 * 259, 2 * 259 + 2)),
], ids=['u32', 'u64'])
def test_mode3_fuzz_equals_host(ops, dtype, xs, big_xs):
    rng = np.random.default_rng(17)
    bad = []
    for i, shape in enumerate(fuzz_shapes(xs, big_xs, even=True)):
        nlabels = (2, 3, 4, 50)[i % 4]
        arr = rng.integers(0, nlabels, size=shape).astype(dtype)
        if dtype == np.uint64:
            arr = (arr << np.uint64(32)) + np.uint64(9)
        else:
            arr = arr * np.uint32(2**31 // 25)
        got = ops.downsample_mode(to_device(arr, misalign=i % 3 == 2),
                                  (2, 2, 2))
        if not same_bytes(from_device(got, dtype),
                          mode_host(arr, (2, 2, 2))):
            bad.append(shape)
    assert not bad, bad


def test_affinity_map_goes_through_in_one_call(ops):
    rng = np.random.default_rng(19)
    for shape in ((3, 6, 10, 32), (3, 5, 7, 18)):
        aff = rng.random(shape, dtype=np.float32)
        for factor in ((2, 2, 2), (1, 2, 2)):
            got = downsample(Chunk(to_device(aff), voxel_offset=(4, 6, 8),
                                   voxel_size=(40, 4, 4)), factor)
            assert got.is_device and got.shape[0] == 3
            assert same_bytes(got.array.cpu().numpy(),
                              average_host(aff, factor))
            assert tuple(got.voxel_offset) == tuple(
                o // f for o, f in zip((4, 6, 8), factor))


def test_connected_component_labels_mode_pool(ops):
    from chunkflow_amd.connected import connected_component
    rng = np.random.default_rng(23)
    prob = torch.from_numpy(rng.random((12, 20, 32), dtype=np.float32))
    seg = connected_component(Chunk(prob.cuda()), threshold=0.55)
    assert seg.is_device and seg.array.dtype == torch.int32
    labels = seg.array.cpu().numpy().view(np.uint32)
    assert labels.max() > 3
    for factor in ((2, 2, 2), (1, 2, 2), (2, 2, 1)):
        got = downsample(seg, factor)
        assert got.array.dtype == torch.int32
        assert same_bytes(from_device(got.array, np.uint32),
                          mode_host(labels, factor))


def test_device_pyramid_equals_host_pyramid():
    rng = np.random.default_rng(29)
    img = rng.integers(0, 256, size=(9, 40, 70), dtype=np.uint8)
    seg = rng.integers(0, 3, size=(8, 40, 72)).astype(np.uint32)
    aff = rng.standard_normal((3, 8, 24, 40)).astype(np.float32)
    for arr, factor in ((img, (2, 2, 2)), (img, (1, 2, 2)),
                        (seg, (1, 2, 2)), (seg, (2, 2, 2)),
                        (aff, (2, 2, 2))):
        kw = dict(voxel_offset=(8, 16, 24), voxel_size=(40, 4, 4))
        host = downsample_pyramid(Chunk(arr, **kw), factor, 3)
        dev = downsample_pyramid(Chunk(to_device(arr), **kw), factor, 3)
        assert len(dev) == 3
        for h, d in zip(host, dev):
            assert d.is_device
            assert same_bytes(from_device(d.array, arr.dtype), h.array)
            assert d.voxel_offset == h.voxel_offset
            assert d.voxel_size == h.voxel_size


def test_cli_chain_on_a_device_chunk(tmp_path):
    """normalize-intensity leaves the chunk in HBM; downsample keeps it
    there."""
    from click.testing import CliRunner
    from chunkflow_amd.flow import main
    full, half = tmp_path / 'full.npy', tmp_path / 'half.npy'
    result = CliRunner().invoke(main, [
        'create-chunk', '--size', '6', '10', '48', '--dtype', 'uint8',
        'normalize-intensity', '-o', 'norm',
        'save-npy', '-i', 'norm', '-f', str(full),
        'downsample', '-f', '1', '2', '2', '-i', 'norm', '-o', 'mip1',
        'save-npy', '-i', 'mip1', '-f', str(half)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    src, got = np.load(full), np.load(half)
    assert src.dtype == np.float32 and got.shape == (6, 5, 24)
    assert same_bytes(got, average_host(src, (1, 2, 2)))


def test_device_rejections(ops):
    seg = torch.zeros((4, 8, 8), dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='downsample_pyramid'):
        ops.downsample_mode(seg, (1, 4, 4))
    with pytest.raises(TypeError):
        ops.downsample_mode(seg.to(torch.int16), (1, 2, 2))
    with pytest.raises(TypeError):
        downsample(Chunk(seg.to(torch.bool)), (2, 2, 2))
    assert ops.downsample_mode(seg, (1, 1, 1)) is seg
