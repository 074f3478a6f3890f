"""Segmentation cleanup on the device, byte for byte against the host path:
equal-value connected components (A), per-label counts and masks (B), the
error returns of the label-table entries (C) and the CLI chain with the
chunk resident in HBM (D). Everything is integer: no tolerance anywhere."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cc_cases import as_dtype  # noqa: E402  (the u8/u32/u64 label mappings)
from chunkflow_amd.chunk import Chunk
from chunkflow_amd.connected import connected_component, equal_value_label
from chunkflow_amd.segmentation import (mask_except, mask_except_host,
                                        mask_fragments, mask_fragments_host,
                                        mask_out_objects, unique_counts)

pytestmark = pytest.mark.gpu

SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


@pytest.fixture(scope='module')
def ops():
    from chunkflow_amd.ops import HipOps
    return HipOps(0)


def to_device(arr, misalign=False):
    """Upload; uint32/uint64 labels travel as int32/int64. With misalign the
    tensor starts one element into its buffer, so it is not 16-byte aligned
    whatever the shape."""
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


# --- A: equal-value connected components -----------------------------------
CC_SHAPES = ((1, 1, 1), (1, 1, 70), (2, 3, 1), (3, 5, 17), (5, 33, 70),
             (8, 16, 64))


def serpentine(shape):
    """Value 3 along one path through every plane (full even rows joined by
    a single voxel at alternating ends of the odd rows); the gaps hold 5."""
    vol = np.full(shape, 5, dtype=np.int64)
    vol[:, 0::2, :] = 3
    for y in range(1, shape[1], 2):
        vol[:, y, -1 if (y // 2) % 2 == 0 else 0] = 3
    return vol


def cc_volumes(shape):
    """name -> volume of small ints; 0 is background."""
    rng = np.random.default_rng(sum(shape) * 31 + shape[2])
    z, y, x = np.indices(shape)
    slab_axis = int(np.argmax(shape))
    vols = {f'random{k}': rng.integers(0, k + 1, size=shape)
            for k in (2, 3, 7)}
    vols['checkerboard'] = (z + y + x) % 2 + 1
    vols['slabs'] = np.where(
        np.indices(shape)[slab_axis] < (shape[slab_axis] + 1) // 2, 1, 2)
    vols['serpentine'] = serpentine(shape)
    vols['binary'] = rng.integers(0, 2, size=shape)
    return vols


_CC_REF = {}


def cc_reference(shape, name, vol, connectivity):
    """equal_value_label of the small-int volume, computed once: the
    partition by equal value is the same for every dtype mapping."""
    key = (shape, name, connectivity)
    if key not in _CC_REF:
        ref = equal_value_label(np.ascontiguousarray(vol), connectivity)
        ref.setflags(write=False)
        _CC_REF[key] = ref
    return _CC_REF[key]


@pytest.mark.parametrize('connectivity', [6, 18, 26])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint32, np.uint64],
                         ids=['u8', 'u32', 'u64'])
def test_equal_value_components_equal_host(ops, dtype, connectivity):
    bad = []
    for shape in CC_SHAPES:
        for name, vol in cc_volumes(shape).items():
            want = cc_reference(shape, name, vol, connectivity)
            seg = to_device(as_dtype(vol, dtype))
            labels = torch.empty(shape, dtype=torch.int32, device='cuda')
            scratch = torch.empty_like(labels)
            n = ops.cfx.connected_components_labels(
                seg.data_ptr(), seg.element_size(), shape, connectivity,
                labels.data_ptr(), scratch.data_ptr())
            got = from_device(labels, np.uint32)
            if got.tobytes() != want.astype(np.uint32).tobytes() \
                    or n != int(want.max()):
                bad.append((shape, name, n, int(want.max())))
            if name == 'binary':
                # the existing entry on the same foreground
                fg = to_device((vol != 0).astype(np.uint8))
                old = torch.empty_like(labels)
                n_old = ops.cfx.connected_components(
                    fg.data_ptr(), shape, connectivity, old.data_ptr(),
                    scratch.data_ptr())
                if n_old != n or not torch.equal(old, labels):
                    bad.append((shape, 'binary-vs-existing', n, n_old))
    assert not bad, bad


def test_equal_value_known_partitions(ops):
    """The structure the volumes were built for, stated directly."""
    shape = (8, 16, 64)
    vols = cc_volumes(shape)
    n_vox = 8 * 16 * 64

    def count(name, connectivity):
        chunk = Chunk(to_device(as_dtype(vols[name], np.uint64)))
        out = connected_component(chunk, connectivity=connectivity)
        return int(from_device(out.array, np.uint32).max())

    assert count('checkerboard', 6) == n_vox     # no merges at all
    assert count('checkerboard', 18) == 2        # one component per value
    assert count('checkerboard', 26) == 2
    for connectivity in (6, 18, 26):
        assert count('slabs', connectivity) == 2  # touching, never merged
    # the path is one component; each gap of 5s between its turns another
    serp = equal_value_label(vols['serpentine'], 6)
    assert count('serpentine', 6) == int(serp.max())
    assert len(np.unique(serp[vols['serpentine'] == 3])) == 1


def test_connected_component_multivalued_stays_on_device():
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 4, size=(6, 20, 33)).astype(np.uint32) * 1000
    chunk = Chunk(to_device(arr), voxel_offset=(1, 2, 3),
                  voxel_size=(40, 4, 4))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        out = connected_component(chunk, threshold=None, connectivity=26)
    assert not [w for w in caught if 'connected-components' in str(w.message)]
    assert out.is_device and out.array.dtype == torch.int32
    assert tuple(out.voxel_offset) == (1, 2, 3)
    want = equal_value_label(arr, 26)
    assert from_device(out.array, np.uint32).tobytes() == \
        want.astype(np.uint32).tobytes()


# --- B: counts and masks -----------------------------------------------------
def label_shapes():
    rng = np.random.default_rng(3)
    return [(int(rng.choice((1, 2, 3, 5))), int(rng.choice((1, 2, 3, 5))), x)
            for x in (1, 2, 15, 16, 17, 63, 64, 65, 130)]


def run_pattern(n, pool, lengths=(1, 1, 17, 3, 1, 40, 2, 9, 1, 16, 8, 1,
                                   33)):
    """Flat labels in runs of length 1, 1, 17, 3, 1, 40, 2, 9, ...: long
    runs and single voxels crossing every 8- and 16-element lane segment;
    labels recur, so a label's count is spread over many runs."""
    out, i = [], 0
    while sum(len(o) for o in out) < n:
        out.append(np.full(lengths[i % len(lengths)], pool[i % len(pool)]))
        i += 1
    return np.concatenate(out)[:n]


def label_volume(kind, shape, dtype):
    bits = np.dtype(dtype).itemsize * 8
    n = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(n + bits)
    k = rng.integers(0, 6, size=n).astype(np.uint64)
    if kind == 'distinct':
        flat = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    elif kind == 'one':
        flat = np.full(n, 77, dtype=np.uint64)
    elif kind == 'zero':
        flat = np.zeros(n, dtype=np.uint64)
    elif kind == 'runs':
        flat = run_pattern(n, (4, 0, 9, 4, 123456, 0, 7)).astype(np.uint64)
    elif kind == 'plateaus':
        # constant stretches longer than a wave's 64 segments next to short
        # runs: some waves see one label only, their neighbours do not
        flat = run_pattern(n, (6, 2, 6, 0, 11), lengths=(2500, 1, 1030, 7,
                                                         1, 4100, 3))
        flat = flat.astype(np.uint64)
    elif kind == 'same_low32':
        # 64-bit only in a meaningful way; for 32 bits the high part wraps
        # away and this is a plain few-label volume
        flat = (k << np.uint64(32)) + np.uint64(9)
    elif kind == 'top_bit':
        flat = np.where(k % 2 == 1, k | (np.uint64(1) << np.uint64(bits - 1)),
                        k)
    elif kind == 'capacity_multiples':
        # multiples of every table capacity these volumes can get
        flat = k * np.uint64(2 ** 20)
    else:
        raise AssertionError(kind)
    return flat.astype(dtype).reshape(shape)


LABEL_KINDS = ('distinct', 'one', 'zero', 'runs', 'plateaus', 'same_low32',
               'top_bit', 'capacity_multiples', 'cc_output')


def cc_output(shape, dtype):
    rng = np.random.default_rng(shape[2])
    prob = torch.from_numpy(rng.random(shape, dtype=np.float32)).cuda()
    seg = connected_component(Chunk(prob), threshold=0.45)
    assert seg.array.dtype == torch.int32
    return from_device(seg.array, np.uint32).astype(dtype)


def check_label_ops(arr, dev, bad, tag):
    """Every operation on device tensor `dev` equals the host path on the
    unsigned array `arr`."""
    dtype = arr.dtype
    before = dev.clone()
    chunk = Chunk(dev, voxel_offset=(2, 4, 6), voxel_size=(40, 4, 4))

    ids, counts = unique_counts(chunk)
    want_ids, want_counts = np.unique(arr, return_counts=True)
    assert ids.is_cuda and ids.dtype == dev.dtype
    assert counts.dtype == torch.int64
    if from_device(ids, dtype).tobytes() != want_ids.tobytes() or \
            counts.cpu().numpy().tobytes() != \
            want_counts.astype(np.int64).tobytes():
        bad.append((tag, 'unique_counts'))

    known = int(want_counts[len(want_counts) // 2])  # size of a real object
    for threshold in (0, 1, known, known - 1):
        got = mask_fragments(chunk, threshold)
        assert got.is_device and got.array.dtype == dev.dtype
        assert got.voxel_offset == chunk.voxel_offset
        assert got.voxel_size == chunk.voxel_size
        if from_device(got.array, dtype).tobytes() != \
                mask_fragments_host(arr, threshold).tobytes():
            bad.append((tag, 'mask_fragments', threshold))

    present = [int(v) for v in want_ids]
    top = int(np.iinfo(dtype).max)
    id_lists = ([], present[-1:], [top - 1, top - 5, 31337],
                [0] + present[::2],
                present + [top - 2 - i for i in range(len(present) + 7)])
    for ids_list in id_lists:
        got = mask_except(chunk, ids_list)
        assert got.is_device and got.array.dtype == dev.dtype
        if from_device(got.array, dtype).tobytes() != \
                mask_except_host(arr, ids_list).tobytes():
            bad.append((tag, 'mask_except', len(ids_list)))

    got = mask_out_objects(chunk, dust_size_threshold=known - 1,
                           selected_obj_ids=id_lists[3])
    want = mask_except_host(mask_fragments_host(arr, known - 1), id_lists[3])
    if from_device(got.array, dtype).tobytes() != want.tobytes():
        bad.append((tag, 'mask_out_objects'))
    assert torch.equal(dev, before), 'input tensor was modified'


@pytest.mark.parametrize('kind', LABEL_KINDS)
@pytest.mark.parametrize('dtype', [np.uint32, np.uint64], ids=['u32', 'u64'])
def test_counts_and_masks_equal_host(ops, dtype, kind):
    bad = []
    shapes = label_shapes()
    # (5, 33, 130): several workgroups of 256 lane segments
    cases = [(s, False) for s in shapes] + [((5, 33, 130), False),
                                            ((3, 5, 65), True)]
    for shape, misalign in cases:
        arr = (cc_output(shape, dtype) if kind == 'cc_output'
               else label_volume(kind, shape, dtype))
        check_label_ops(arr, to_device(arr, misalign=misalign), bad,
                        (shape, misalign))
    assert not bad, bad


def test_table_sizing_bound_and_load(ops):
    """The run-start bound: exact on hand-made volumes, never below the
    number of distinct labels, and the table it sizes is at most half
    full."""
    arr = np.array([[[4, 4, 0, 0, 4], [4, 7, 7, 7, 7]]], dtype=np.uint32)
    t = to_device(arr)
    # flat order 4 4 0 0 4 4 7 7 7 7: the second row starts inside a run
    assert ops.cfx.label_run_starts(t.data_ptr(), 4, arr.shape) == 4
    for kind in ('distinct', 'runs', 'one'):
        arr = label_volume(kind, (3, 5, 130), np.uint64)
        keys, vals, capacity, bound = ops.label_count_table(to_device(arr))
        flat = arr.ravel()
        assert bound == 1 + int(np.count_nonzero(flat[1:] != flat[:-1]))
        distinct = len(np.unique(arr))
        assert distinct <= bound
        assert capacity & (capacity - 1) == 0 and capacity >= 2 * bound
        assert int((keys != -1).sum()) == distinct
        assert int(vals.sum()) == arr.size


@pytest.mark.parametrize('dtype', [np.uint32, np.uint64], ids=['u32', 'u64'])
def test_mask_with_input_and_output_equally_misaligned(ops, dtype):
    """Scalar head, vector body, scalar tail: both streams start one
    element past a 16-byte boundary."""
    for shape in ((1, 1, 2), (2, 3, 17), (3, 5, 130)):
        arr = label_volume('runs', shape, dtype)
        dev = to_device(arr, misalign=True)
        out = to_device(np.zeros_like(arr), misalign=True)
        assert dev.data_ptr() % 16 == out.data_ptr() % 16 != 0
        keys, vals, capacity, _ = ops.label_count_table(dev)
        ops.cfx.label_mask(dev.data_ptr(), out.data_ptr(),
                           dev.element_size(), shape, keys.data_ptr(),
                           vals.data_ptr(), capacity, 0, 9)
        assert from_device(out, dtype).tobytes() == \
            mask_fragments_host(arr, 9).tobytes(), shape


def test_device_dtype_rejections(ops):
    seg = torch.zeros((2, 4, 8), dtype=torch.int16, device='cuda')
    for fn in (lambda c: unique_counts(c), lambda c: mask_fragments(c, 1),
               lambda c: mask_except(c, [1])):
        with pytest.raises(TypeError, match='int32 or int64'):
            fn(Chunk(seg))
        with pytest.raises(TypeError):
            fn(Chunk(seg.to(torch.float32)))
        with pytest.raises(ValueError):
            fn(Chunk(torch.zeros((2, 2, 4, 8), dtype=torch.int32,
                                 device='cuda')))


# --- C: error returns (nothing launched, or bounded by construction) --------
def test_error_returns(ops):
    from chunkflow_amd.hip import CfxError
    cfx = ops.cfx
    labels = torch.arange(1, 101, dtype=torch.int32,
                          device='cuda').view(1, 1, 100)
    out = torch.empty_like(labels)
    keys = torch.empty(64, dtype=torch.int64, device='cuda')
    vals = torch.empty(64, dtype=torch.int32, device='cuda')
    k, v, lp, op = (keys.data_ptr(), vals.data_ptr(), labels.data_ptr(),
                    out.data_ptr())
    dims = (1, 1, 100)

    # capacity not a power of two: refused before any launch
    with pytest.raises(CfxError, match='power of two'):
        cfx.label_table_clear(k, v, 48)
    with pytest.raises(CfxError, match='power of two'):
        cfx.label_count(lp, 4, dims, k, v, 48)
    with pytest.raises(CfxError, match='power of two'):
        cfx.label_mask(lp, op, 4, dims, k, v, 0, 0, 0)
    with pytest.raises(CfxError, match='power of two'):
        cfx.label_table_insert(lp, 1, 1, k, v, 12)

    # 100 distinct labels into 4 slots: every probe loop stops after
    # `capacity` steps, the entry reports it
    cfx.label_table_clear(k, v, 4)
    with pytest.raises(CfxError, match='table full'):
        cfx.label_count(lp, 4, dims, k, v, 4)
    assert int((keys[:4] != -1).sum()) == 4   # the four slots were claimed
    assert int(vals[:4].sum()) == 4           # one voxel each, none lost
    ids = torch.arange(1, 101, dtype=torch.int64, device='cuda')
    cfx.label_table_clear(k, v, 4)
    with pytest.raises(CfxError, match='table full'):
        cfx.label_table_insert(ids.data_ptr(), 100, 1, k, v, 4)
    # a table with room takes them
    cfx.label_table_clear(k, v, 64)
    cfx.label_table_insert(ids.data_ptr(), 100 - 40, 1, k, v, 64)

    # wrong element size, mode and connectivity
    for eb in (1, 2, 3, 16):
        with pytest.raises(CfxError, match='elem_bytes'):
            cfx.label_count(lp, eb, dims, k, v, 64)
        with pytest.raises(CfxError, match='elem_bytes'):
            cfx.label_mask(lp, op, eb, dims, k, v, 64, 0, 0)
        with pytest.raises(CfxError, match='elem_bytes'):
            cfx.label_run_starts(lp, eb, dims)
    with pytest.raises(CfxError, match='mode'):
        cfx.label_mask(lp, op, 4, dims, k, v, 64, 2, 0)
    scratch = torch.empty_like(labels)
    for eb in (2, 3, 16):
        with pytest.raises(CfxError, match='elem_bytes'):
            cfx.connected_components_labels(lp, eb, dims, 6, op,
                                            scratch.data_ptr())
    for connectivity in (0, 4, 7, 27):
        with pytest.raises(CfxError, match='connectivity'):
            cfx.connected_components_labels(lp, 4, dims, connectivity, op,
                                            scratch.data_ptr())

    # the reserved 64-bit label is reported, not silently miscounted
    reserved = torch.full((1, 1, 5), -1, dtype=torch.int64, device='cuda')
    cfx.label_table_clear(k, v, 64)
    with pytest.raises(CfxError, match='reserved'):
        cfx.label_count(reserved.data_ptr(), 8, (1, 1, 5), k, v, 64)


# --- D: the chain through the CLI ---------------------------------------------
def test_cli_chain_keeps_the_chunk_on_the_device(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import chunkflow_amd.segmentation as segmentation
    from chunkflow_amd.downsample import downsample
    from chunkflow_amd.flow import main

    seen = []
    real = segmentation.mask_out_objects

    def spy(chunk, **kwargs):
        out = real(chunk, **kwargs)
        seen.append((chunk.is_device, out.is_device, out.array.dtype))
        return out
    monkeypatch.setattr(segmentation, 'mask_out_objects', spy)

    aff, mip = tmp_path / 'aff.npy', tmp_path / 'mip.npy'
    result = CliRunner().invoke(main, [
        'create-chunk', '--size', '28', '100', '100', '--dtype', 'uint8',
        '--pattern', 'sin',
        'inference', '-s', '12', '32', '32',
        '--output-patch-overlap', '4', '8', '8',
        '--framework', 'identity', '--batch-size', '6',
        '--num-output-channels', '3', '--mask-output-chunk',
        'save-npy', '-f', str(aff),
        'connected-components', '-t', '0.5', '-c', '6',
        'mask-out-objects', '-d', '20000',
        'downsample', '-f', '2', '2', '2',
        'save-npy', '-f', str(mip)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    assert seen == [(True, True, torch.int32)]

    # the same chain on host chunks, from the inference output on
    host = connected_component(Chunk(np.load(aff)), threshold=0.5,
                               connectivity=6)
    n_before = len(np.unique(host.array))
    host = mask_out_objects(host, dust_size_threshold=20000)
    n_after = len(np.unique(host.array))
    assert 1 < n_after < n_before   # dust went, objects stayed
    host = downsample(host, (2, 2, 2))
    got = np.load(mip)
    assert got.shape == (14, 50, 50) and got.dtype == np.int32
    assert got.view(np.uint32).tobytes() == \
        host.array.astype(np.uint32).tobytes()
