"""evaluate-segmentation on the device against the host path: the
contingency rows are integers and must be equal, and both paths close them
with the same host function, so the score dicts must be identical — no
tolerance anywhere. (A) layouts x shapes x dtype pairs, (B) the LDS spill,
misaligned views, large labels and the grid-stride wrap, (C) the error
returns, (D) the CLI chain with the segmentation resident in HBM."""
import numpy as np
import pytest
import torch

from chunkflow_amd.chunk import Chunk
from chunkflow_amd.segmentation import (contingency, contingency_host,
                                        evaluate, scores_from_contingency)

pytestmark = pytest.mark.gpu

SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
DTYPE_PAIRS = [(np.uint32, np.uint32), (np.uint32, np.uint64),
               (np.uint64, np.uint32), (np.uint64, np.uint64)]
PAIR_IDS = ['u32-u32', 'u32-u64', 'u64-u32', 'u64-u64']
SHAPES = ((1, 1, 1), (1, 1, 70), (3, 5, 17), (5, 33, 70), (8, 16, 64))


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


def same_float(a, b) -> bool:
    a, b = np.float64(a), np.float64(b)
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


def same_scores(a: dict, b: dict) -> bool:
    if a.keys() != b.keys():
        return False
    for key in a:
        va, vb = a[key], b[key]
        if key == 'edit_distance':
            if not all(same_float(x, y) for x, y in zip(va, vb)):
                return False
        elif not same_float(va, vb):
            return False
    return True


def blocky(rng, shape, repeat, labels):
    z, y, x = shape
    coarse = rng.integers(0, labels, size=(z, y, -(-x // repeat)))
    return np.repeat(coarse, repeat, axis=2)[:, :, :x]


def layouts(shape):
    """name -> (seg, gt) of small non-negative ints."""
    rng = np.random.default_rng(sum(shape) * 17 + shape[2])
    n = shape[0] * shape[1] * shape[2]
    half = (np.arange(n) >= n // 2).reshape(shape)
    same = blocky(rng, shape, 3, 9)
    return {
        'random3': (rng.integers(0, 3, size=shape),
                    rng.integers(0, 3, size=shape)),
        'random40': (rng.integers(0, 40, size=shape),
                     rng.integers(0, 40, size=shape)),
        # 64 consecutive lane segments hold one pair: the wave-uniform add
        'constant': (np.full(shape, 7), np.full(shape, 3)),
        'zeros': (np.zeros(shape, int), np.zeros(shape, int)),
        # some waves uniform, the one across the step not
        'step': (np.full(shape, 7), np.where(half, 4, 3)),
        'blocky': (blocky(rng, shape, 3, 12), blocky(rng, shape, 5, 12)),
        'same': (same, same.copy()),
    }


_HOST = {}


def host_rows(key, seg, gt):
    """The host contingency of a pair of volumes, computed once."""
    if key not in _HOST:
        rows = contingency_host(seg, gt)
        for r in rows:
            r.setflags(write=False)
        _HOST[key] = rows
    return _HOST[key]


def rows_equal(dev_rows, rows) -> bool:
    s, g, n = dev_rows
    assert s.is_cuda and g.is_cuda and n.is_cuda
    assert s.dtype == g.dtype == n.dtype == torch.int64
    return (s.cpu().numpy().view(np.uint64).tobytes() == rows[0].tobytes()
            and g.cpu().numpy().view(np.uint64).tobytes()
            == rows[1].tobytes()
            and n.cpu().numpy().tobytes()
            == rows[2].astype(np.int64).tobytes())


# --- A: layouts x shapes x dtype pairs ----------------------------------------
@pytest.mark.parametrize('seg_dtype,gt_dtype', DTYPE_PAIRS, ids=PAIR_IDS)
def test_rows_and_scores_equal_host(ops, seg_dtype, gt_dtype):
    bad = []
    for shape in SHAPES:
        for name, (seg, gt) in layouts(shape).items():
            seg, gt = seg.astype(seg_dtype), gt.astype(gt_dtype)
            rows = host_rows((shape, name), seg, gt)
            dseg, dgt = to_device(seg), to_device(gt)
            before = dseg.clone(), dgt.clone()
            if not rows_equal(contingency(Chunk(dseg), Chunk(dgt)), rows):
                bad.append((shape, name, 'rows'))
            for thr in (0, 29):
                want = evaluate(Chunk(seg), Chunk(gt), thr)
                if not same_scores(evaluate(Chunk(dseg), Chunk(dgt), thr),
                                   want):
                    bad.append((shape, name, 'scores', thr))
            assert torch.equal(dseg, before[0]) and \
                torch.equal(dgt, before[1]), 'an input tensor was modified'
    assert not bad, bad


def test_one_chunk_on_the_host_is_uploaded(ops):
    seg, gt = layouts((5, 33, 70))['blocky']
    seg, gt = seg.astype(np.uint32), gt.astype(np.uint64)
    rows = host_rows(((5, 33, 70), 'blocky'), seg, gt)
    assert rows_equal(contingency(Chunk(to_device(seg)), Chunk(gt)), rows)
    assert rows_equal(contingency(Chunk(seg), Chunk(to_device(gt))), rows)
    # a narrow host dtype beside a device chunk
    assert rows_equal(contingency(Chunk(seg.astype(np.uint8)),
                                  Chunk(to_device(gt))), rows)


def test_table_sizes_and_profile_slot(ops):
    seg, gt = layouts((8, 16, 64))['blocky']
    seg, gt = seg.astype(np.uint32), gt.astype(np.uint32)
    rows = host_rows(((8, 16, 64), 'blocky'), seg, gt)
    ops.cfx.profile_enable(True)
    ops.cfx.profile_reset()
    try:
        _, _, keys, vals, info = ops.label_pair_table(to_device(seg),
                                                      to_device(gt))
        prof = ops.cfx.profile_get('labels')
    finally:
        ops.cfx.profile_enable(False)
    # two run-start passes, two single counts, one pair count
    assert prof['count'] == 5
    fs, fg = seg.ravel(), gt.ravel()
    pair_runs = 1 + int(np.count_nonzero((fs[1:] != fs[:-1])
                                         | (fg[1:] != fg[:-1])))
    assert info['pair_bound'] == min(
        info['seg_bound'] + info['gt_bound'] - 1, seg.size)
    assert len(rows[2]) <= pair_runs <= info['pair_bound']
    assert info['pair_capacity'] >= 2 * info['pair_bound']
    assert int((keys != -1).sum()) == len(rows[2])
    assert int(vals.sum()) == seg.size


# --- B: spill, misalignment, large labels, grid wrap --------------------------
@pytest.mark.parametrize('seg_dtype,gt_dtype', DTYPE_PAIRS, ids=PAIR_IDS)
def test_more_pairs_than_lds_slots(ops, seg_dtype, gt_dtype):
    """8192 distinct pairs within one or two workgroups' reach, far more
    than the 512 LDS slots: the rest goes straight to the HBM table."""
    shape = (4, 32, 64)
    seg = np.arange(8192).reshape(shape).astype(seg_dtype)
    gt = (np.arange(8192) // 3).reshape(shape).astype(gt_dtype)
    rows = host_rows((shape, 'arange'), seg, gt)
    assert len(rows[2]) == 8192
    assert rows_equal(contingency(Chunk(to_device(seg)),
                                  Chunk(to_device(gt))), rows)


@pytest.mark.parametrize('seg_dtype,gt_dtype', DTYPE_PAIRS, ids=PAIR_IDS)
def test_misaligned_views_give_the_same_rows(ops, seg_dtype, gt_dtype):
    bad = []
    for shape in ((1, 1, 2), (3, 5, 17), (5, 33, 70)):
        for name in ('random40', 'blocky', 'step'):
            seg, gt = layouts(shape)[name]
            seg, gt = seg.astype(seg_dtype), gt.astype(gt_dtype)
            rows = host_rows((shape, name), seg, gt)
            for mis in ((True, False), (False, True), (True, True)):
                got = contingency(Chunk(to_device(seg, misalign=mis[0])),
                                  Chunk(to_device(gt, misalign=mis[1])))
                if not rows_equal(got, rows):
                    bad.append((shape, name, mis))
    assert not bad, bad


def label_sets(dtype):
    """name -> an injective map of 0..63 with 0 -> 0."""
    k = np.arange(64, dtype=np.uint64)
    sets = {'ge_2^31': np.where(k == 0, 0, 2 ** 31 + 977 * k),
            'multiples_of_2^20': k << np.uint64(20)}
    if np.dtype(dtype) == np.uint64:
        sets['ge_2^63'] = np.where(k == 0, 0, 2 ** 63 + 31 * k)
        sets['differ_above_bit_32'] = np.where(k == 0, 0,
                                               (k << np.uint64(32)) + 5)
    return {name: m.astype(dtype) for name, m in sets.items()}


@pytest.mark.parametrize('seg_dtype,gt_dtype', DTYPE_PAIRS, ids=PAIR_IDS)
def test_large_labels(ops, seg_dtype, gt_dtype):
    shape = (5, 33, 70)
    small_seg, small_gt = layouts(shape)['random40']
    want = evaluate(Chunk(small_seg), Chunk(small_gt), 5)
    bad = []
    for sname, smap in label_sets(seg_dtype).items():
        for gname, gmap in label_sets(gt_dtype).items():
            seg, gt = smap[small_seg], gmap[small_gt]
            rows = host_rows((shape, sname, gname, seg.dtype, gt.dtype),
                             seg, gt)
            dev = contingency(Chunk(to_device(seg)), Chunk(to_device(gt)))
            if not rows_equal(dev, rows):
                bad.append((sname, gname, 'rows'))
            if not same_scores(
                    {k: v for k, v in scores_from_contingency(
                        *dev, size_threshold=5).items() if k in want}, want):
                bad.append((sname, gname, 'scores'))
    assert not bad, bad


def test_grid_stride_wrap(ops):
    """int32, 8 454 144 voxels: more than 2048 workgroups x 256 lanes x 16
    labels, so the grid-stride loop of the pair kernel takes a second trip
    (its launch bounds are those of the single count). Blocky labels keep
    the host reference quick."""
    shape = (129, 256, 256)
    assert shape[0] * shape[1] * shape[2] > 2048 * 256 * 16
    rng = np.random.default_rng(129)
    seg = blocky(rng, shape, 32, 300).astype(np.uint32)
    gt = blocky(rng, shape, 64, 200).astype(np.uint32)
    rows = contingency_host(seg, gt)
    dseg, dgt = to_device(seg), to_device(gt)
    assert rows_equal(contingency(Chunk(dseg), Chunk(dgt)), rows)
    assert same_scores(evaluate(Chunk(dseg), Chunk(dgt)),
                       evaluate(Chunk(seg), Chunk(gt)))


# --- C: error returns (nothing launched, or bounded by construction) --------
def test_error_returns(ops):
    from chunkflow_amd.hip import CfxError
    cfx = ops.cfx
    dims = (1, 1, 100)
    seg = torch.arange(1, 101, dtype=torch.int32, device='cuda').view(dims)
    gt = torch.zeros(dims, dtype=torch.int64, device='cuda')
    sk, _, scap, _ = ops.label_count_table(seg)
    gk, _, gcap, _ = ops.label_count_table(gt)
    keys = torch.empty(256, dtype=torch.int64, device='cuda')
    vals = torch.empty(256, dtype=torch.int32, device='cuda')
    k, v = keys.data_ptr(), vals.data_ptr()

    def pair(seg_t=seg, seg_dims=dims, seg_bytes=4, seg_cap=scap, gt_t=gt,
             gt_dims=dims, gt_bytes=8, capacity=256):
        cfx.label_table_clear(k, v, 256)
        cfx.label_pair_count(seg_t.data_ptr(), seg_bytes, seg_dims,
                             sk.data_ptr(), seg_cap, gt_t.data_ptr(),
                             gt_bytes, gt_dims, gk.data_ptr(), gcap, k, v,
                             capacity)

    pair()                                   # the good call
    assert int((keys != -1).sum()) == 100 and int(vals.sum()) == 100

    # 100 distinct pairs into 4 slots: every probe loop stops after
    # `capacity` steps, the entry reports it and the call comes back
    with pytest.raises(CfxError, match='table full'):
        pair(capacity=4)
    assert int((keys[:4] != -1).sum()) == 4
    assert int(vals[:4].sum()) == 4          # one voxel each, none lost
    with pytest.raises(CfxError, match='table full'):
        ops.label_pair_table(seg, gt, capacity=4)

    # refused before any launch
    with pytest.raises(CfxError, match='power of two'):
        pair(capacity=48)
    with pytest.raises(CfxError, match='differ in shape'):
        pair(gt_dims=(1, 2, 50))
    with pytest.raises(CfxError, match='differ in shape'):
        pair(seg_dims=(1, 1, 99))
    for eb in (1, 2, 16):
        with pytest.raises(CfxError, match='elem_bytes'):
            pair(seg_bytes=eb)
        with pytest.raises(CfxError, match='elem_bytes'):
            pair(gt_bytes=eb)
    with pytest.raises(CfxError, match='2\\^31'):
        pair(seg_cap=2 ** 32)
    with pytest.raises(ValueError, match='shape'):
        ops.label_contingency(seg, gt.view(1, 2, 50))
    with pytest.raises(ValueError, match='shape'):
        evaluate(Chunk(seg), Chunk(gt.view(1, 2, 50)))
    with pytest.raises(TypeError):
        evaluate(Chunk(seg), Chunk(gt.to(torch.float32)))

    # the reserved 64-bit label is reported, not silently miscounted:
    # by the single count on the way in, and by the pair kernel itself
    reserved = gt.clone()
    reserved[0, 0, 17] = -1
    with pytest.raises(CfxError, match='reserved'):
        contingency(Chunk(seg), Chunk(reserved))
    with pytest.raises(CfxError, match='reserved'):
        pair(gt_t=reserved)
    # a label its single table does not hold
    stranger = gt.clone()
    stranger[0, 0, 3] = 12345
    with pytest.raises(CfxError, match='missing from its table'):
        pair(gt_t=stranger)


# --- D: the chain through the CLI ---------------------------------------------
def test_cli_chain_scores_the_resident_segmentation(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import chunkflow_amd.runtime as runtime
    import chunkflow_amd.segmentation as segmentation
    from chunkflow_amd.flow import main

    seen = []
    real = segmentation.evaluate

    def spy(seg, gt, *args, **kwargs):
        seen.append((seg.is_device, gt.is_device, seg.array.dtype))
        return real(seg, gt, *args, **kwargs)
    monkeypatch.setattr(segmentation, 'evaluate', spy)
    task = runtime.get_initial_task()
    monkeypatch.setattr(runtime, 'get_initial_task', lambda: task)

    shape = (28, 100, 100)
    rng = np.random.default_rng(28)
    truth = blocky(rng, shape, 10, 6).astype(np.uint64)
    gt_file, seg_file = tmp_path / 'gt.npy', tmp_path / 'seg.npy'
    np.save(gt_file, truth)
    result = CliRunner().invoke(main, [
        'create-chunk', '--size', '28', '100', '100', '--dtype', 'uint8',
        '--pattern', 'sin',
        'inference', '-s', '12', '32', '32',
        '--output-patch-overlap', '4', '8', '8',
        '--framework', 'identity', '--batch-size', '6',
        '--num-output-channels', '3', '--mask-output-chunk',
        'connected-components', '-t', '0.5', '-c', '6',
        'load-npy', '-f', str(gt_file), '-o', 'groundtruth',
        'evaluate-segmentation',
        'save-npy', '-f', str(seg_file)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    assert seen == [(True, False, torch.int32)]
    assert task['chunk'].is_device        # the segmentation never left HBM

    seg = np.load(seg_file)
    assert seg.shape == shape and len(np.unique(seg)) > 2
    want = evaluate(Chunk(seg.view(np.uint32)), Chunk(truth))
    assert same_scores(task['seg_score'], want)
    assert 'Fowlkes Mallows Index: ' in result.output
