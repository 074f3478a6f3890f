"""evaluate-segmentation on the host: the scores against the values recorded
from the reference's gala metrics (tests/golden/evaluate_cases.npz, written
by tools/gen_evaluate_golden.py), the contingency rows, invariance under
relabelling, the rejections and the command (no GPU needed)."""
import os

import numpy as np
import pytest
from click.testing import CliRunner

from chunkflow_amd.chunk import Chunk
from chunkflow_amd.segmentation import (SCORE_KEYS, contingency, evaluate,
                                        scores_from_contingency,
                                        unique_counts)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'evaluate_cases.npz')
EXACT = ('rand_index', 'adjusted_rand_index', 'fowlkes_mallows_index')
# at most 40 x 40 = 1600 non-zero pairs per case, each term O(1), float64
# rounding 2^-53 per operation: far below 1e-12
VI_TOLERANCE = 1e-12


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as f:
        data = {k: f[k] for k in f.files}
    cases = {}
    for key, value in data.items():
        name, field = key.split('/')
        cases.setdefault(name, {})[field] = value
    return cases


def same_float(a, b) -> bool:
    """Equal as float64, NaN equal to NaN."""
    a, b = np.float64(a), np.float64(b)
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


def same_scores(a: dict, b: dict) -> bool:
    if a.keys() != b.keys():
        return False
    for key in a:
        va, vb = a[key], b[key]
        if key == 'edit_distance':
            if len(va) != 2 or len(vb) != 2 or \
                    not all(same_float(x, y) for x, y in zip(va, vb)):
                return False
        elif not same_float(va, vb):
            return False
    return True


def test_scores_equal_the_reference(golden):
    bad, worst = [], 0.0
    for name, case in golden.items():
        got = evaluate(Chunk(case['seg']), Chunk(case['gt']),
                       size_threshold=int(case['size_threshold']))
        assert tuple(got) == SCORE_KEYS
        ri, ari, vi, fm, ed0, ed1 = case['scores']
        want = {'rand_index': ri, 'adjusted_rand_index': ari,
                'fowlkes_mallows_index': fm}
        for key in EXACT:
            assert isinstance(got[key], np.float64), (name, key)
            if not same_float(got[key], want[key]):
                bad.append((name, key, got[key], want[key]))
        edit = got['edit_distance']
        assert isinstance(edit, tuple) and len(edit) == 2
        assert all(isinstance(v, np.float64) for v in edit)
        if not (same_float(edit[0], ed0) and same_float(edit[1], ed1)):
            bad.append((name, 'edit_distance', edit, (ed0, ed1)))
        got_vi = got['variation_of_information']
        if np.isnan(vi) or np.isnan(got_vi):
            if not (np.isnan(vi) and np.isnan(got_vi)):
                bad.append((name, 'vi', got_vi, vi))
        else:
            worst = max(worst, abs(float(got_vi) - float(vi)))
            if abs(float(got_vi) - float(vi)) > VI_TOLERANCE:
                bad.append((name, 'vi', got_vi, vi))
    print(f'largest VI deviation over {len(golden)} cases: {worst:.3e}')
    assert not bad, bad
    assert worst <= VI_TOLERANCE


def test_fixture_holds_the_listed_cases(golden):
    """A regenerated file cannot silently lose a layout, a degenerate case
    or a threshold."""
    assert 25 <= len(golden) <= 40
    layouts = {name.split('_')[0] for name in golden}
    assert layouts == {'random', 'blocky', 'same', 'nozero', 'allzero',
                       'onelabel', 'disjoint'}
    shapes = {c['seg'].shape for c in golden.values()}
    assert (1, 1, 1) in shapes and (8, 40, 70) in shapes
    assert {int(c['size_threshold']) for c in golden.values()} == \
        {0, 5, 29, 1000}
    n_labels = set()
    for name, c in golden.items():
        assert c['seg'].dtype == np.uint8 and c['gt'].dtype == np.uint8
        assert c['seg'].shape == c['gt'].shape and c['seg'].ndim == 3
        assert c['scores'].dtype == np.float64 and c['scores'].shape == (6,)
        assert max(c['seg'].max(), c['gt'].max()) < 64
        n_labels |= {len(np.unique(c['seg'])), len(np.unique(c['gt']))}
        layout = name.split('_')[0]
        if layout == 'blocky':
            rs, rg = (int(ch) for ch in name.split('_')[1])
            for arr, rep in ((c['seg'], rs), (c['gt'], rg)):
                x = arr.shape[2] // rep * rep
                blocks = arr[:, :, :x].reshape(arr.shape[:2] + (-1, rep))
                assert (blocks == blocks[..., :1]).all(), name
        elif layout == 'same':
            assert (c['seg'] == c['gt']).all() and c['seg'].max() > 0
        elif layout == 'nozero':
            assert c['seg'].min() > 0 and c['gt'].min() > 0
        elif layout == 'allzero':
            assert not c['seg'].any() and not c['gt'].any()
        elif layout == 'onelabel':
            assert len(np.unique(c['seg'])) == 1 and c['seg'].flat[0] != 0
            assert (c['seg'] == c['gt']).all()
        elif layout == 'disjoint':
            assert c['seg'].any() and c['gt'].any()
            assert not ((c['seg'] != 0) & (c['gt'] != 0)).any()
    assert min(n_labels) == 1 and max(n_labels) == 40
    repeats = {name.split('_')[1] for name in golden if name[:6] == 'blocky'}
    assert any('3' in r for r in repeats) and any('5' in r for r in repeats)
    # the degenerate scores as the issue records them
    for name, want in (('allzero_0', (1, np.nan, np.nan, 1, 0, 0)),
                       ('onelabel_0', (1, np.nan, 0, 1, 0, 0))):
        assert all(same_float(a, b)
                   for a, b in zip(golden[name]['scores'], want)), name
    d = golden['disjoint_0']['scores']
    assert np.isnan(d[2]) and d[4] < 0 and d[5] == 0
    assert os.path.getsize(GOLDEN) < 200 * 1000


def test_contingency_rows(golden):
    for name, case in golden.items():
        seg, gt = case['seg'], case['gt']
        s, g, n = contingency(Chunk(seg), Chunk(gt))
        assert s.dtype == np.uint64 and g.dtype == np.uint64
        assert n.dtype == np.int64 and len(s) == len(g) == len(n)
        rows = list(zip(s.tolist(), g.tolist()))
        assert rows == sorted(set(rows)), name       # sorted, no duplicates
        assert (n > 0).all() and int(n.sum()) == seg.size
        for ids, vol in ((s, seg), (g, gt)):
            want_ids, want_counts = unique_counts(Chunk(vol))
            got_ids, inverse = np.unique(ids, return_inverse=True)
            got_counts = np.bincount(inverse, weights=n).astype(np.int64)
            assert got_ids.tolist() == want_ids.tolist(), name
            assert got_counts.tolist() == want_counts.tolist(), name
        # against the plain definition
        pairs, counts = np.unique(
            np.stack([seg.ravel(), gt.ravel()], axis=1).astype(np.uint64),
            axis=0, return_counts=True)
        assert pairs[:, 0].tolist() == s.tolist()
        assert pairs[:, 1].tolist() == g.tolist()
        assert counts.tolist() == n.tolist()


def test_contingency_orders_by_unsigned_value():
    seg = np.array([[[1, 2 ** 63, 1, 2 ** 64 - 2]]], dtype=np.uint64)
    gt = np.array([[[2 ** 31, 3, 7, 3]]], dtype=np.uint32)
    s, g, n = contingency(Chunk(seg), Chunk(gt))
    assert s.tolist() == [1, 1, 2 ** 63, 2 ** 64 - 2]
    assert g.tolist() == [7, 2 ** 31, 3, 3]
    assert n.tolist() == [1, 1, 1, 1]


# --- relabelling invariance -------------------------------------------------
def label_sets(dtype):
    """name -> an injective map of 0..63 with 0 -> 0 (an array indexed by
    the small label)."""
    k = np.arange(64, dtype=np.uint64)
    sets = {'ge_2^31': np.where(k == 0, 0, 2 ** 31 + 977 * k),
            'multiples_of_2^20': k << np.uint64(20)}
    if np.dtype(dtype) == np.uint64:
        sets['ge_2^63'] = np.where(k == 0, 0, 2 ** 63 + 31 * k)
        sets['differ_above_bit_32'] = np.where(k == 0, 0,
                                               (k << np.uint64(32)) + 5)
    return {name: m.astype(dtype) for name, m in sets.items()}


RELABEL_PAIRS = [(np.uint32, np.uint32), (np.uint64, np.uint64),
                 (np.uint32, np.uint64), (np.uint64, np.uint32)]


@pytest.mark.parametrize('seg_dtype,gt_dtype', RELABEL_PAIRS,
                         ids=['u32-u32', 'u64-u64', 'u32-u64', 'u64-u32'])
def test_relabelling_leaves_the_scores_unchanged(golden, seg_dtype, gt_dtype):
    bad, seen = [], set()
    for name in ('random_4', 'blocky_35_2', 'nozero_1', 'disjoint_1'):
        case = golden[name]
        thr = int(case['size_threshold'])
        want = evaluate(Chunk(case['seg']), Chunk(case['gt']), thr)
        for sname, smap in label_sets(seg_dtype).items():
            for gname, gmap in label_sets(gt_dtype).items():
                seg, gt = smap[case['seg']], gmap[case['gt']]
                assert seg.dtype == seg_dtype and gt.dtype == gt_dtype
                got = evaluate(Chunk(seg), Chunk(gt), thr)
                seen |= {sname, gname}
                if not same_scores(got, want):
                    bad.append((name, sname, gname))
    assert not bad, bad
    assert {'ge_2^31', 'multiples_of_2^20'} <= seen


def test_scores_from_contingency_extra_key_and_threshold():
    # seg 1 overlaps gt 1 (3 voxels) and gt 2 (2); seg 2 overlaps gt 2 (1)
    seg = np.array([[[1, 1, 1, 1, 1, 2, 0]]], dtype=np.uint32)
    gt = np.array([[[1, 1, 1, 2, 2, 2, 5]]], dtype=np.uint32)
    rows = contingency(Chunk(seg), Chunk(gt))
    scores = scores_from_contingency(*rows, size_threshold=0)
    assert set(scores) == set(SCORE_KEYS) | {'false_splits_by_column'}
    assert scores['edit_distance'] == (1.0, 0.0)     # 3 pairs - 2 segments
    assert scores['false_splits_by_column'] == 0.0   # 3 pairs - 3 gt labels
    scores = scores_from_contingency(*rows, size_threshold=2)
    assert scores['edit_distance'] == (-1.0, 0.0)    # 1 pair  - 2 segments
    assert scores['false_splits_by_column'] == -2.0
    assert 'false_splits_by_column' not in evaluate(Chunk(seg), Chunk(gt))


def test_any_integer_dtype_is_cast_like_the_reference(golden):
    case = golden['random_4']
    want = evaluate(Chunk(case['seg']), Chunk(case['gt']), 5)
    for dtype in (np.int8, np.uint16, np.int32, np.int64):
        got = evaluate(Chunk(case['seg'].astype(dtype)),
                       Chunk(case['gt'].astype(np.uint64)), 5)
        assert same_scores(got, want), dtype
    s, _, _ = contingency(Chunk(np.full((1, 1, 2), -1, dtype=np.int32)),
                          Chunk(np.zeros((1, 1, 2), dtype=np.uint8)))
    assert s.tolist() == [2 ** 64 - 1]   # astype(np.uint64) wraps


def test_rejections():
    seg = Chunk(np.zeros((2, 3, 4), dtype=np.uint32))
    with pytest.raises(ValueError, match='shape'):
        evaluate(seg, Chunk(np.zeros((2, 3, 5), dtype=np.uint32)))
    with pytest.raises(ValueError):
        contingency(seg, Chunk(np.zeros((1, 2, 3, 4), dtype=np.uint32)))
    with pytest.raises(TypeError, match='integer'):
        evaluate(seg, Chunk(np.zeros((2, 3, 4), dtype=np.float32)))
    with pytest.raises(TypeError, match='integer'):
        evaluate(Chunk(np.zeros((2, 3, 4), dtype=np.float32)), seg)
    # voxel offsets are not compared: the reference looks at the arrays only
    moved = Chunk(np.zeros((2, 3, 4), dtype=np.uint32),
                  voxel_offset=(5, 6, 7))
    assert evaluate(seg, moved)['rand_index'] == 1.0


# --- the command --------------------------------------------------------------
def test_cli_stores_the_scores(tmp_path, monkeypatch, golden):
    import chunkflow_amd.runtime as runtime
    from chunkflow_amd.flow import main
    case = golden['blocky_33_1']
    a, b = tmp_path / 'a.npy', tmp_path / 'b.npy'
    np.save(a, case['seg'].astype(np.uint32))
    np.save(b, case['gt'].astype(np.uint64))
    task = runtime.get_initial_task()
    monkeypatch.setattr(runtime, 'get_initial_task', lambda: task)
    result = CliRunner().invoke(main, [
        'load-npy', '-f', str(a), '-o', 'a',
        'load-npy', '-f', str(b), '-o', 'b',
        'evaluate-segmentation', '-s', 'a', '-g', 'b', '-o', 'score'],
        catch_exceptions=False)
    assert result.exit_code == 0, result.output
    # the reference's size_threshold default
    want = evaluate(Chunk(case['seg']), Chunk(case['gt']), 1000)
    assert same_scores(task['score'], want)
    for line in ('rand index: ', 'adjusted rand index: ',
                 'variation of information: ', 'edit distance: ',
                 'Fowlkes Mallows Index: '):
        assert line in result.output
    assert f'rand index: {want["rand_index"]: .3f}' in result.output


def test_cli_flags_and_none_tasks():
    from chunkflow_amd.flow import evaluate_segmentation
    params = {p.name: p for p in evaluate_segmentation.params}
    assert set(params) == {'segmentation_chunk_name',
                           'groundtruth_chunk_name', 'output'}
    assert params['segmentation_chunk_name'].opts == [
        '--segmentation-chunk-name', '-s']
    assert params['groundtruth_chunk_name'].opts == [
        '--groundtruth-chunk-name', '-g']
    assert params['output'].opts == ['--output', '-o']
    assert params['segmentation_chunk_name'].default == 'chunk'
    assert params['groundtruth_chunk_name'].default == 'groundtruth'
    assert params['output'].default == 'seg_score'
    op = evaluate_segmentation.callback(
        segmentation_chunk_name='chunk', groundtruth_chunk_name='groundtruth',
        output='seg_score')
    vol = Chunk(np.ones((1, 2, 3), dtype=np.uint32))
    out = list(op([None, {'chunk': vol, 'groundtruth': vol}]))
    assert out[0] is None and out[1]['seg_score']['rand_index'] == 1.0


def test_new_symbol_is_exported():
    import ctypes
    from chunkflow_amd.build import build
    from chunkflow_amd.hip import SYMBOLS
    assert 'cfx_label_pair_count' in SYMBOLS
    assert hasattr(ctypes.CDLL(build()), 'cfx_label_pair_count')
