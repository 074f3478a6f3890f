"""The host path of the affinity watershed, the region graph, the
agglomerator and the `agglomerate` plugin (no GPU). The vectorised host
functions are the oracle of the device kernels, so they are held here to the
voxel-by-voxel restatements of tests/watershed_cases.py and to the
identities the definition implies. Everything is compared for equality."""
import inspect
import os
import sys

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse import csgraph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import watershed_cases as wc  # noqa: E402

from chunkflow_amd.agglomeration import merge_fragments  # noqa: E402
from chunkflow_amd.chunk import Chunk  # noqa: E402
from chunkflow_amd.watershed import (affinity_fragments,  # noqa: E402
                                     affinity_fragments_host, agglomerate,
                                     quantise, region_graph_host)

SMALL = ((1, 1, 1), (1, 1, 2), (1, 1, 70), (3, 5, 17), (4, 9, 13))
THRESHOLDS = (2.0, 0.6, 0.5, 0.4, -1.0)


def first_voxels_ascend(labels, n):
    uniq, first = np.unique(labels.ravel(), return_index=True)
    keep = uniq != 0
    uniq, first = uniq[keep], first[keep]
    return (uniq.tolist() == list(range(1, n + 1))
            and bool((np.diff(first) > 0).all()))


# --- fragments ----------------------------------------------------------------
@pytest.mark.parametrize('make,low,high', [
    (wc.smooth, 0.3, 0.8), (wc.levels, 0.5, 0.75), (wc.levels, 0.75, 0.5),
    (wc.special, 0.3, 0.8), (wc.special, -1.0, 0.5),
    (wc.special, -np.inf, np.inf)],
    ids=['smooth', 'levels', 'low_gt_high', 'special', 'negative_low',
         'infinite_thresholds'])
def test_fragments_equal_the_definition(make, low, high):
    for shape in SMALL:
        aff = make(shape)
        got, n = affinity_fragments_host(aff, low, high)
        want, n_want = wc.fragments_slow(aff, low, high)
        assert got.dtype == np.uint32 and got.shape == shape
        assert n == n_want and np.array_equal(got, want), shape


def test_equal_thresholds_give_edge_components():
    for shape in SMALL:
        for make, t in ((wc.smooth, 0.5), (wc.levels, 0.75),
                        (wc.special, 0.4)):
            aff = make(shape)
            got, n = affinity_fragments_host(aff, t, t)
            want, n_want = wc.edge_components_slow(aff, t)
            assert n == n_want and np.array_equal(got, want), (shape, t)


def test_edge_components_at_scale():
    """17 x 64 x 130: the partition of low == high == T against scipy on the
    thresholded edge list, built here without the host path's code."""
    shape, t = (17, 64, 130), np.float32(0.5)
    aff = wc.smooth(shape)
    got, n = affinity_fragments_host(aff, t, t)
    nvox = int(np.prod(shape))
    idx = np.arange(nvox).reshape(shape)
    ok = [aff[0][:, :, 1:] >= t, aff[1][:, 1:, :] >= t, aff[2][1:] >= t]
    src = np.concatenate([idx[:, :, 1:][ok[0]], idx[:, 1:, :][ok[1]],
                          idx[1:][ok[2]]])
    dst = np.concatenate([idx[:, :, :-1][ok[0]], idx[:, :-1, :][ok[1]],
                          idx[:-1][ok[2]]])
    graph = sparse.coo_matrix((np.ones(src.size), (src, dst)),
                              shape=(nvox, nvox))
    _, comp = csgraph.connected_components(graph, directed=False)
    touched = np.zeros(nvox, dtype=bool)
    touched[src] = touched[dst] = True
    flat = got.ravel()
    assert np.array_equal(flat != 0, touched)
    # same partition: the pairs (ours, scipy's) are one-to-one
    pairs = np.unique(np.stack([flat[touched], comp[touched]]), axis=1)
    assert pairs.shape[1] == n == len(np.unique(comp[touched]))
    assert first_voxels_ascend(got, n)


def test_no_background_when_every_edge_is_live_and_none_strong():
    for shape in SMALL[1:]:
        aff = wc.smooth(shape)
        got, n = affinity_fragments_host(aff, -1.0, 2.0)
        assert (got != 0).all() and n >= 1, shape
    # a single voxel has no edge at all
    got, n = affinity_fragments_host(wc.smooth((1, 1, 1)), -1.0, 2.0)
    assert n == 0 and got.tolist() == [[[0]]]


def test_all_dead_and_all_strong():
    aff = wc.smooth((3, 5, 17))
    got, n = affinity_fragments_host(aff, 2.0, 3.0)
    assert n == 0 and not got.any()
    got, n = affinity_fragments_host(aff, 0.0, 0.0)
    assert n == 1 and (got == 1).all()


def test_numbering_is_raster_first_encounter():
    for shape in ((3, 5, 17), (5, 33, 67)):
        for make, low, high in ((wc.smooth, 0.3, 0.8),
                                (wc.levels, 0.5, 0.75),
                                (wc.special, 0.3, 0.8)):
            got, n = affinity_fragments_host(make(shape), low, high)
            assert n > 1 and first_voxels_ascend(got, n), shape


def test_leading_faces_have_no_effect():
    for shape in ((1, 1, 70), (3, 5, 17), (5, 33, 67)):
        aff = wc.smooth(shape)
        want, n = affinity_fragments_host(aff, 0.3, 0.8)
        frag_rows = region_graph_host(want, aff)
        for value in (np.nan, 1.0):
            filled = wc.fill_leading_faces(aff, value)
            got, n_got = affinity_fragments_host(filled, 0.3, 0.8)
            assert n_got == n and np.array_equal(got, want), (shape, value)
            for r, w in zip(region_graph_host(want, filled), frag_rows):
                assert np.array_equal(r, w), (shape, value)


def test_dispatch_on_host_chunks_keeps_the_geometry():
    aff = wc.smooth((3, 5, 17))
    chunk = Chunk(aff, voxel_offset=(7, 8, 9), voxel_size=(40, 4, 4))
    out = affinity_fragments(chunk, 0.3, 0.8)
    assert not out.is_device and out.array.dtype == np.uint32
    assert tuple(out.voxel_offset) == (7, 8, 9)
    assert tuple(out.voxel_size) == (40, 4, 4)
    assert np.array_equal(out.array,
                          affinity_fragments_host(aff, 0.3, 0.8)[0])
    # f16 widens exactly; a transposed view is made contiguous
    half = aff.astype(np.float16)
    assert np.array_equal(
        affinity_fragments(Chunk(half), 0.3, 0.8).array,
        affinity_fragments_host(half.astype(np.float32), 0.3, 0.8)[0])
    view = np.ascontiguousarray(aff.transpose(0, 3, 2, 1)).transpose(
        0, 3, 2, 1)
    assert not view.flags.c_contiguous
    assert np.array_equal(affinity_fragments(Chunk(view), 0.3, 0.8).array,
                          out.array)
    with pytest.raises(ValueError, match=r'\(3, Z, Y, X\)'):
        affinity_fragments(Chunk(aff[:2]), 0.3, 0.8)


# --- region graph --------------------------------------------------------------
def test_quantise():
    w = np.array([np.nan, -np.inf, -0.5, -0.0, 0.0, 2.0 ** -25, 2.0 ** -24,
                  0.5, 1.0 - 2.0 ** -24, 1.0, 1.5, np.inf], dtype=np.float32)
    assert quantise(w).tolist() == [0, 0, 0, 0, 0, 0, 1, 2 ** 23,
                                    2 ** 24 - 1, 2 ** 24, 2 ** 24, 2 ** 24]


def test_region_graph_equals_the_definition():
    for shape in SMALL:
        for make in (wc.smooth, wc.special):
            aff = make(shape)
            frag, _ = affinity_fragments_host(aff, 0.3, 0.8)
            rows = region_graph_host(frag, aff)
            assert wc.rows_as_dict(rows) == wc.region_graph_slow(frag, aff)
            keys = (rows[0].astype(np.uint64) << np.uint64(32)) | rows[1]
            assert (np.diff(keys.astype(object)) > 0).all()
        frag = wc.blocky_fragments(shape)
        rows = region_graph_host(frag, wc.special(shape))
        assert wc.rows_as_dict(rows) == \
            wc.region_graph_slow(frag, wc.special(shape))


# --- agglomerator --------------------------------------------------------------
@pytest.fixture(scope='module')
def graph():
    """about 500 fragments and 1 700 edges from a 4 x 17 x 35 map"""
    aff = wc.smooth((4, 17, 35), seed=5)
    frag, n = affinity_fragments_host(aff, 0.3, 2.0)
    rows = region_graph_host(frag, aff)
    for r in rows:
        r.setflags(write=False)
    assert 300 < n < 900 and 1000 < len(rows[0]) < 3000, (n, len(rows[0]))
    return rows, n


@pytest.mark.parametrize('threshold', THRESHOLDS)
def test_agglomerator_equals_brute_force(graph, threshold):
    rows, n = graph
    got = merge_fragments(rows, n, threshold)
    want = wc.merge_slow(rows, n, threshold)
    assert got.dtype == np.uint32 and got.shape == (n + 1,)
    assert np.array_equal(got, want)
    # dense, and numbered by the smallest fragment of each segment
    m = int(got.max())
    assert got[0] == 0 and np.unique(got[1:]).tolist() == \
        list(range(1, m + 1))
    first = [int(np.flatnonzero(got == s)[0]) for s in range(1, m + 1)]
    assert first == sorted(first)


def test_agglomerator_end_points(graph):
    rows, n = graph
    assert merge_fragments(rows, n, 2.0).tolist() == list(range(n + 1))
    got = merge_fragments(rows, n, -1.0)
    adjacency = sparse.coo_matrix(
        (np.ones(len(rows[0])), (rows[0].astype(np.int64),
                                 rows[1].astype(np.int64))),
        shape=(n + 1, n + 1))
    ncomp, comp = csgraph.connected_components(adjacency, directed=False)
    assert int(got.max()) == ncomp - 1          # vertex 0 is its own
    pairs = np.unique(np.stack([got[1:], comp[1:]]), axis=1)
    assert pairs.shape[1] == ncomp - 1
    # in between the segments only ever grow coarser
    counts = [int(merge_fragments(rows, n, t).max()) for t in THRESHOLDS]
    assert counts == sorted(counts, reverse=True) and counts[0] == n


def test_agglomerator_does_not_depend_on_row_order(graph):
    rows, n = graph
    order = np.random.default_rng(9).permutation(len(rows[0]))
    shuffled = tuple(r[order] for r in rows)
    for threshold in (0.6, 0.5):
        assert np.array_equal(merge_fragments(shuffled, n, threshold),
                              merge_fragments(rows, n, threshold))


def test_agglomerator_refuses_bad_rows():
    one = np.array([1])
    with pytest.raises(ValueError, match='bad row'):
        merge_fragments((np.array([2]), one, one, one), 3, 0.5)
    with pytest.raises(ValueError, match='bad row'):
        merge_fragments((one, np.array([4]), one, one), 3, 0.5)
    with pytest.raises(ValueError, match='twice'):
        merge_fragments((np.array([1, 1]), np.array([2, 2]),
                         np.array([1, 1]), np.array([5, 5])), 3, 0.5)


def test_agglomerate_on_a_host_chunk():
    aff = wc.smooth((4, 17, 35), seed=5)
    chunk = Chunk(aff, voxel_offset=(1, 2, 3), voxel_size=(40, 4, 4))
    seg = agglomerate(chunk, 0.5, 0.3, 2.0)
    frag, n = affinity_fragments_host(aff, 0.3, 2.0)
    want = merge_fragments(region_graph_host(frag, aff), n, 0.5)[frag]
    assert seg.array.dtype == np.uint32 and np.array_equal(seg.array, want)
    assert tuple(seg.voxel_offset) == (1, 2, 3)
    assert first_voxels_ascend(seg.array, int(seg.array.max()))
    # caller-supplied fragments with arbitrary ids: the same partition
    spread = (frag.astype(np.uint64) * 6999997 % (2 ** 32 - 5)) \
        .astype(np.uint32)
    spread[frag == 0] = 0
    assert len(np.unique(spread)) == len(np.unique(frag))
    other = agglomerate(chunk, 0.5, 0.3, 2.0, fragments=spread).array
    pairs = np.unique(np.stack([other.ravel(), want.ravel()]), axis=1)
    assert pairs.shape[1] == len(np.unique(want))
    # the same ids in a signed dtype are read as unsigned: same numbering
    assert int(spread.max()) >= 2 ** 31
    signed = agglomerate(chunk, 0.5, 0.3, 2.0,
                         fragments=spread.view(np.int32)).array
    assert np.array_equal(signed, other)


# --- plugin, CLI, C-ABI --------------------------------------------------------
def test_plugin_loads_by_name_with_the_reference_signature():
    from chunkflow_amd.plugin import Plugin, load_plugin
    execute = load_plugin('agglomerate')
    params = inspect.signature(execute).parameters
    assert list(params) == ['affs', 'fragments', 'threshold',
                            'aff_threshold_low', 'aff_threshold_high',
                            'scoring_function', 'flip_channel']
    defaults = {k: p.default for k, p in params.items()}
    assert defaults['affs'] is inspect.Parameter.empty
    assert defaults['fragments'] is None
    assert defaults['threshold'] == 0.7
    assert defaults['aff_threshold_low'] == 0.001
    assert defaults['aff_threshold_high'] == 0.9999
    assert defaults['scoring_function'] == \
        'OneMinus<MeanAffinity<RegionGraphType, ScoreValue>>'
    assert defaults['flip_channel'] is True
    with pytest.raises(ValueError, match='OneMinus<MeanAffinity'):
        execute(Chunk(wc.smooth((1, 1, 2))),
                scoring_function='OneMinus<MaxAffinity<RegionGraphType, '
                                 'ScoreValue>>')

    aff = wc.smooth((4, 17, 35), seed=5)
    chunk = Chunk(aff, voxel_offset=(1, 2, 3), voxel_size=(40, 4, 4))
    out = execute(chunk, threshold=0.45, aff_threshold_low=0.3,
                  aff_threshold_high=0.95)
    assert isinstance(out, list) and len(out) == 1
    seg = out[0]
    want = agglomerate(chunk, 1.0 - 0.45, 0.3, 0.95).array
    assert np.array_equal(seg.array, want) and len(np.unique(want)) > 2
    assert tuple(seg.voxel_offset) == (1, 2, 3)
    assert tuple(seg.voxel_size) == (40, 4, 4)
    # a map that is in z, y, x order already
    zyx = Chunk(np.ascontiguousarray(aff[::-1]), voxel_offset=(1, 2, 3))
    out = execute(zyx, threshold=0.45, aff_threshold_low=0.3,
                  aff_threshold_high=0.95, flip_channel=False)
    assert np.array_equal(out[0].array, want)
    # through the operator's wrapper, with the reference's --args text
    got = Plugin('agglomerate')(
        [chunk], args='threshold=0.45;aff_threshold_low=0.3;'
                      'aff_threshold_high=0.95')
    assert np.array_equal(got[0].array, want)


def test_cli_watershed_operator():
    from chunkflow_amd.flow import watershed
    params = {p.name: p for p in watershed.params}
    assert params['input_chunk_name'].opts == ['--input-chunk-name', '-i']
    assert params['output_chunk_name'].opts == ['--output-chunk-name', '-o']
    assert {'low', 'high', 'name'} <= set(params)
    aff = wc.smooth((3, 5, 17))
    op = watershed.callback(name='ws', input_chunk_name='affs',
                            output_chunk_name='frag', low=0.5, high=0.5)
    task = {'affs': Chunk(aff), 'log': {'timer': {}}}
    out = list(op([None, task]))
    assert out[0] is None and 'ws' in out[1]['log']['timer']
    assert np.array_equal(out[1]['frag'].array,
                          wc.edge_components_slow(aff, 0.5)[0])


def test_new_symbols_are_exported():
    import ctypes
    from chunkflow_amd.build import build
    from chunkflow_amd.hip import KERNEL_IDS, SYMBOLS, CfxContext
    lib = ctypes.CDLL(build())
    for sym in ('cfx_affinity_fragments', 'cfx_region_graph',
                'cfx_region_graph_runs'):
        assert sym in SYMBOLS and hasattr(lib, sym), sym
    for method in ('affinity_fragments', 'region_graph',
                   'region_graph_runs'):
        assert callable(getattr(CfxContext, method))
    assert len(KERNEL_IDS) == 13      # reported under 'cc' and 'labels'
