"""The affinity watershed and the region graph on the device against the
host path (chunkflow_amd/watershed.py, itself held to the definition in
tests/test_watershed.py): labels and rows are integers and must be equal.
(A) fragments over shapes x inputs, the grid-stride wrap once, guard bands;
(B) region-graph rows, large ids, the table-full return; (C) agglomerate end
to end, the CLI chain in HBM, a misaligned view."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_cases as cc  # noqa: E402
import watershed_cases as wc  # noqa: E402

from chunkflow_amd.chunk import Chunk  # noqa: E402
from chunkflow_amd.watershed import (affinity_fragments,  # noqa: E402
                                     affinity_fragments_host, agglomerate,
                                     region_graph, region_graph_host)

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (1, 1, 2), (1, 1, 70), (3, 5, 17), (5, 33, 67),
          (17, 64, 130))
WRAP_SHAPE = (8, 512, 520)


def serpentine(shape):
    """a one-voxel-wide path of strong edges through a dead volume"""
    return wc.path_edges(cc.serpentine3d(shape))


# name -> (map of a shape, low, high)
INPUTS = {
    'smooth': (wc.smooth, 0.3, 0.8),
    # thresholds exactly on a level: >= is what is tested
    'levels': (wc.levels, 0.5, 0.75),
    'levels_equal': (wc.levels, 0.75, 0.75),
    'special': (wc.special, 0.3, 0.8),
    'special_negative_low': (wc.special, -1.0, 0.5),
    'low_gt_high': (wc.levels, 0.75, 0.5),
    'all_dead': (wc.smooth, 2.0, 3.0),
    'all_strong': (wc.smooth, 0.0, 0.0),
    'serpentine': (serpentine, 0.5, 0.5),
}

_HOST = {}


def host_case(name, shape):
    """(aff, low, high, labels, n) of a case, computed once, read-only"""
    key = (name, tuple(shape))
    if key not in _HOST:
        make, low, high = INPUTS[name]
        aff = make(shape)
        labels, n = affinity_fragments_host(aff, low, high)
        aff.setflags(write=False)
        labels.setflags(write=False)
        _HOST[key] = (aff, low, high, labels, n)
    return _HOST[key]


@pytest.fixture(scope='module')
def ops():
    from chunkflow_amd.ops import HipOps
    return HipOps(0)


def upload(arr, misalign=False):
    """uint32 travels as int32; with misalign the tensor starts one element
    into its buffer"""
    arr = np.array(arr, order='C')      # a writable copy for from_numpy
    if arr.dtype == np.uint32:
        arr = arr.view(np.int32)
    t = torch.from_numpy(arr)
    if not misalign:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def labels_of(chunk):
    assert chunk.is_device and chunk.array.dtype == torch.int32
    return chunk.array.cpu().numpy().view(np.uint32)


# --- A: fragments ---------------------------------------------------------------
@pytest.mark.parametrize('name', list(INPUTS))
def test_fragments_equal_host(ops, name):
    bad = []
    for shape in SHAPES:
        aff, low, high, want, n = host_case(name, shape)
        dev = upload(aff)
        before = dev.clone()
        got, n_got = ops.affinity_fragments(dev, low, high)
        got = got.cpu().numpy().view(np.uint32)
        if n_got != n or not np.array_equal(got, want):
            bad.append((shape, n_got, n, int((got != want).sum())))
        assert torch.equal(dev.view(torch.int32), before.view(torch.int32)), \
            'the input was modified'
    assert not bad, bad


def test_the_degenerate_cases_are_what_they_say():
    for shape in SHAPES[1:]:
        assert host_case('all_dead', shape)[4] == 0
        assert host_case('all_strong', shape)[4] == 1
        _, _, _, labels, n = host_case('serpentine', shape)
        assert n == 1 and np.array_equal(labels != 0,
                                         cc.serpentine3d(shape) != 0)


def test_fragment_grid_stride_loops_wrap(ops):
    """More voxels than the fragment kernels (init, merge, compress, final;
    one voxel per lane) launch lanes, once. The region-graph rows are
    compared too, but its walk gives a lane 16 voxels and does NOT wrap
    here: test_region_graph_item_loop_wraps is the case for that."""
    assert wc.VOXEL_LANES < cc.nvox(WRAP_SHAPE) < wc.SEG * wc.REGION_LANES
    aff = wc.smooth(WRAP_SHAPE)
    want, n = affinity_fragments_host(aff, 0.3, 0.8)
    dev = upload(aff)
    got, n_got = ops.affinity_fragments(dev, 0.3, 0.8)
    assert n_got == n
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    rows = region_graph_host(want, aff)
    dev_rows = ops.region_graph(got, dev)
    for d, h in zip(dev_rows, rows):
        assert np.array_equal(d.cpu().numpy().astype(np.uint64),
                              h.astype(np.uint64))


def test_nothing_is_written_outside_the_buffers(ops):
    for name, shape in (('smooth', (5, 33, 67)), ('serpentine', (3, 5, 17)),
                        ('all_dead', (1, 1, 70))):
        aff, low, high, want, n = host_case(name, shape)
        nv = cc.nvox(shape)
        lab_buf, labels = cc.poisoned(nv, ops.device, rootlike_tail=True)
        scr_buf, scratch = cc.poisoned(nv, ops.device)
        dev = upload(aff)
        n_got = ops.cfx.affinity_fragments(dev.data_ptr(), shape, low, high,
                                           labels.data_ptr(),
                                           scratch.data_ptr())
        ops.sync()
        problems = cc.guard_problems(lab_buf, nv, 'labels',
                                     rootlike_tail=True)
        problems += cc.guard_problems(scr_buf, nv, 'scratch')
        assert not problems, (name, problems)
        assert n_got == n and np.array_equal(
            labels.cpu().numpy().view(np.uint32).reshape(shape), want)


def test_dispatch_dtypes_views_and_profile_slot(ops):
    aff, low, high, want, _ = host_case('smooth', (5, 33, 67))
    chunk = Chunk(upload(aff), voxel_offset=(7, 8, 9), voxel_size=(40, 4, 4))
    out = affinity_fragments(chunk, low, high)
    assert np.array_equal(labels_of(out), want)
    assert tuple(out.voxel_offset) == (7, 8, 9)
    assert tuple(out.voxel_size) == (40, 4, 4)
    # one element into its buffer
    mis = affinity_fragments(Chunk(upload(aff, misalign=True)), low, high)
    assert np.array_equal(labels_of(mis), want)
    # f16 and bf16 widen exactly: the host sees the same f32 values
    for dtype in (torch.float16, torch.bfloat16):
        narrow = upload(aff).to(dtype)
        ref = affinity_fragments_host(narrow.float().cpu().numpy(), low,
                                      high)[0]
        assert np.array_equal(
            labels_of(affinity_fragments(Chunk(narrow), low, high)), ref)
    # a non-contiguous view
    view = upload(np.ascontiguousarray(aff.transpose(0, 3, 2, 1))) \
        .permute(0, 3, 2, 1)
    assert not view.is_contiguous()
    assert np.array_equal(
        labels_of(affinity_fragments(Chunk(view), low, high)), want)
    # timed under the existing ids, on the context the operators share
    from chunkflow_amd.ops import shared_hip_ops
    cfx = shared_hip_ops(0).cfx
    cfx.profile_enable(True)
    cfx.profile_reset()
    try:
        region_graph(affinity_fragments(chunk, low, high), chunk)
        assert cfx.profile_get('cc')['count'] == 1
        assert cfx.profile_get('labels')['count'] == 2
    finally:
        cfx.profile_enable(False)


# --- B: region graph --------------------------------------------------------------
def rows_equal(dev_rows, rows) -> bool:
    assert all(r.is_cuda and r.dtype == torch.int64 for r in dev_rows)
    return all(np.array_equal(d.cpu().numpy().view(np.uint64),
                              h.astype(np.uint64))
               for d, h in zip(dev_rows, rows))


@pytest.mark.parametrize('name', ['smooth', 'levels', 'special',
                                  'special_negative_low', 'serpentine',
                                  'all_dead'])
def test_region_graph_rows_equal_host(ops, name):
    bad = []
    for shape in SHAPES:
        aff, _, _, frag, _ = host_case(name, shape)
        rows = region_graph_host(frag, aff)
        for mis in (False, True):
            got = ops.region_graph(upload(frag, misalign=mis),
                                   upload(aff, misalign=mis))
            if not rows_equal(got, rows):
                bad.append((shape, mis))
    assert not bad, bad


def test_region_graph_of_large_ids(ops):
    bad = []
    for shape in SHAPES:
        frag = wc.blocky_fragments(shape)
        aff = wc.special(shape)
        rows = region_graph_host(frag, aff)
        if not rows_equal(ops.region_graph(upload(frag), upload(aff)), rows):
            bad.append(shape)
        if not rows_equal(region_graph(Chunk(frag), Chunk(upload(aff))),
                          rows):
            bad.append((shape, 'host fragments uploaded'))
    assert not bad, bad
    top = region_graph_host(wc.blocky_fragments((5, 33, 67)),
                            wc.special((5, 33, 67)))
    assert int(top[1].max()) == 2 ** 32 - 1 and \
        int(top[0].max()) == 2 ** 32 - 2


def test_region_graph_item_loop_wraps(ops):
    """More 16-voxel items than the region walk launches lanes, so lanes
    take a second item (fresh runs, coordinates and left neighbour, the run
    counter carried on) in both the sizing pass and the table pass: the run
    count equals its numpy restatement and keys, counts and sums equal the
    host rows. Coarse blocks keep the host pass quick."""
    shape = wc.region_wrap_shape()
    n_items = -(-cc.nvox(shape) // wc.SEG)
    assert wc.REGION_LANES < n_items < 2 * wc.REGION_LANES
    assert cc.nvox(shape) % wc.SEG != 0
    frag, aff = wc.coarse_fragments(shape), wc.cheap_special(shape)
    rows = region_graph_host(frag, aff)
    assert len(rows[0]) > 10000 and int(rows[1].max()) == 2 ** 32 - 1
    dfrag, daff = upload(frag), upload(aff)
    assert ops.cfx.region_graph_runs(dfrag.data_ptr(), shape) == \
        wc.expected_runs(frag)
    assert rows_equal(ops.region_graph(dfrag, daff), rows)


def test_table_sizing_and_the_table_full_return(ops):
    from chunkflow_amd.hip import CfxError
    aff, _, _, frag, _ = host_case('smooth', (5, 33, 67))
    rows = region_graph_host(frag, aff)
    n_rows = len(rows[0])
    assert n_rows > 1000
    dfrag, daff = upload(frag), upload(aff)
    keys, counts, sums, info = ops.region_graph_table(dfrag, daff)
    assert n_rows <= info['bound'] == wc.expected_runs(frag)
    assert info['capacity'] >= 2 * info['bound']
    assert int((keys != -1).sum()) == n_rows
    assert int(counts.sum()) == int(rows[2].sum())
    assert int(sums.sum()) == int(rows[3].sum())
    # too small: every probe loop ends after `capacity` steps and the call
    # returns an error. The 64 slots it did fill are rows of the graph,
    # each complete: a run that found no slot added nowhere.
    keys = torch.empty(64, dtype=torch.int64, device='cuda')
    counts = torch.empty(64, dtype=torch.int32, device='cuda')
    sums = torch.empty(64, dtype=torch.int64, device='cuda')
    with pytest.raises(CfxError, match='table full'):
        ops.cfx.region_graph(dfrag.data_ptr(), daff.data_ptr(), frag.shape,
                             keys.data_ptr(), counts.data_ptr(),
                             sums.data_ptr(), 64)
    want = {(a << 32) | b: (c, s)
            for (a, b), (c, s) in wc.rows_as_dict(rows).items()}
    held = {int(k): (int(c), int(s)) for k, c, s in zip(
        keys.cpu().numpy().view(np.uint64), counts.cpu().numpy(),
        sums.cpu().numpy())}
    assert len(held) == 64 and all(want[k] == v for k, v in held.items())
    with pytest.raises(CfxError, match='table full'):
        ops.region_graph_table(dfrag, daff, capacity=64)
    with pytest.raises(CfxError, match='power of two'):
        ops.region_graph_table(dfrag, daff, capacity=48)
    # the exact fit still works
    capacity = 1 << (n_rows - 1).bit_length()
    keys, counts, _, _ = ops.region_graph_table(dfrag, daff,
                                                capacity=capacity)
    assert int((keys != -1).sum()) == n_rows
    assert int(counts.sum()) == int(rows[2].sum())
    with pytest.raises(ValueError, match='shape'):
        ops.region_graph(dfrag.view(5, 67, 33), daff)
    with pytest.raises(TypeError, match='int32'):
        ops.region_graph(dfrag.to(torch.int64), daff)


# --- C: end to end ----------------------------------------------------------------
def test_agglomerate_equals_host_and_stays_on_the_device(ops):
    for shape, threshold in (((3, 5, 17), -1.0), ((3, 5, 17), 2.0),
                             ((1, 1, 70), 0.5), ((5, 33, 67), 0.5)):
        aff = wc.smooth(shape)
        want = agglomerate(Chunk(aff), threshold, 0.3, 0.9).array
        chunk = Chunk(upload(aff), voxel_offset=(1, 2, 3),
                      voxel_size=(40, 4, 4))
        got = agglomerate(chunk, threshold, 0.3, 0.9)
        assert np.array_equal(labels_of(got), want), (shape, threshold)
        assert tuple(got.voxel_offset) == (1, 2, 3)
        mis = agglomerate(Chunk(upload(aff, misalign=True)), threshold, 0.3,
                          0.9)
        assert np.array_equal(labels_of(mis), want), (shape, threshold)
    # caller-supplied fragments, on either side
    frag = affinity_fragments_host(aff, 0.3, 0.9)[0]
    want = agglomerate(Chunk(aff), 0.5, 0.3, 0.9, fragments=frag).array
    for given in (frag, frag.view(np.int32), upload(frag)):
        got = agglomerate(Chunk(upload(aff)), 0.5, 0.3, 0.9, fragments=given)
        assert np.array_equal(labels_of(got), want)


def test_plugin_keeps_a_device_chunk_on_the_device(ops):
    from chunkflow_amd.plugin import Plugin
    aff = wc.smooth((5, 33, 67))
    args = 'threshold=0.45;aff_threshold_low=0.3;aff_threshold_high=0.95'
    want = Plugin('agglomerate')([Chunk(aff)], args=args)[0].array
    got = Plugin('agglomerate')(
        [Chunk(upload(aff), voxel_offset=(1, 2, 3))], args=args)[0]
    assert np.array_equal(labels_of(got), want)
    assert tuple(got.voxel_offset) == (1, 2, 3)


def test_cli_chain_runs_in_hbm(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import chunkflow_amd.runtime as runtime
    import chunkflow_amd.watershed as watershed
    from chunkflow_amd.flow import main
    from chunkflow_amd.segmentation import evaluate, mask_fragments_host

    seen = []
    real = watershed.affinity_fragments

    def spy(chunk, low, high):
        out = real(chunk, low, high)
        seen.append((chunk.is_device, tuple(chunk.shape), out.is_device,
                     out.array.dtype))
        affs.append(chunk.array.cpu().numpy())
        return out
    affs = []
    monkeypatch.setattr(watershed, 'affinity_fragments', spy)
    task = runtime.get_initial_task()
    monkeypatch.setattr(runtime, 'get_initial_task', lambda: task)

    shape = (28, 100, 100)
    truth = np.repeat(np.random.default_rng(28).integers(
        0, 6, size=(28, 100, 10)), 10, axis=2).astype(np.uint64)
    gt_file, seg_file = tmp_path / 'gt.npy', tmp_path / 'seg.npy'
    np.save(gt_file, truth)
    result = CliRunner().invoke(main, [
        'create-chunk', '--size', '28', '100', '100', '--dtype', 'uint8',
        '--pattern', 'sin',
        'inference', '-s', '12', '32', '32',
        '--output-patch-overlap', '4', '8', '8',
        '--framework', 'identity', '--batch-size', '6',
        '--num-output-channels', '3', '--mask-output-chunk',
        'watershed', '--low', '0.5', '--high', '0.5',
        'mask-out-objects', '-d', '20',
        'load-npy', '-f', str(gt_file), '-o', 'groundtruth',
        'evaluate-segmentation',
        'save-npy', '-f', str(seg_file)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    assert seen == [(True, (3,) + shape, True, torch.int32)]
    assert task['chunk'].is_device          # the volume never left HBM
    assert 'watershed' in task['log']['timer']

    seg = np.load(seg_file).view(np.uint32)
    want = mask_fragments_host(
        affinity_fragments_host(affs[0], 0.5, 0.5)[0], 20)
    assert np.array_equal(seg, want) and len(np.unique(seg)) > 1
    scores = evaluate(Chunk(seg), Chunk(truth))
    for key, value in scores.items():
        assert np.array_equal(np.asarray(task['seg_score'][key]),
                              np.asarray(value), equal_nan=True), key
