"""Segmentation cleanup on the host: unique_counts / mask_fragments /
mask_except against hand-written expectations, the mask-out-objects
command, the error cases, and the new C-ABI symbols (no GPU needed)."""
import ctypes
import json

import numpy as np
import pytest
from click.testing import CliRunner

from chunkflow_amd.chunk import Chunk
from chunkflow_amd.segmentation import (mask_except, mask_fragments,
                                        mask_out_objects, parse_obj_ids,
                                        unique_counts)


def tiny(dtype=np.uint32):
    """2x3x4: label 5 has 1 voxel, 7 has 3, 9 has 4, 2**31+1 has 2 and
    zero has 14."""
    big = 2 ** 31 + 1
    return np.array([[[0, 7, 7, 0],
                      [9, 9, 0, 0],
                      [9, 9, 0, 5]],
                     [[0, 7, 0, 0],
                      [0, 0, big, big],
                      [0, 0, 0, 0]]], dtype=dtype)


def test_unique_counts_tiny():
    ids, counts = unique_counts(Chunk(tiny()))
    assert ids.tolist() == [0, 5, 7, 9, 2 ** 31 + 1]
    assert counts.tolist() == [14, 1, 3, 4, 2]
    assert ids.dtype == np.uint32


def test_mask_fragments_tiny():
    arr = tiny()
    want = arr.copy()
    want[(arr == 5) | (arr == 2 ** 31 + 1)] = 0
    got = mask_fragments(Chunk(arr), 2)
    assert got.array.dtype == arr.dtype
    assert got.array.tobytes() == want.tobytes()
    # threshold 0 removes nothing; a huge one removes everything
    assert mask_fragments(Chunk(arr), 0).array.tobytes() == arr.tobytes()
    assert not mask_fragments(Chunk(arr), 100).array.any()
    assert arr.tobytes() == tiny().tobytes()  # input untouched


def test_dust_boundary_is_less_or_equal():
    arr = tiny()
    # label 7 has exactly 3 voxels, label 9 has 3 + 1
    got = mask_fragments(Chunk(arr), 3).array
    assert not (got == 7).any()
    assert (got == 9).sum() == 4
    got = mask_fragments(Chunk(arr), 2).array
    assert (got == 7).sum() == 3


def test_mask_except_tiny():
    arr = tiny()
    want = np.where((arr == 7) | (arr == 2 ** 31 + 1), arr, 0)
    got = mask_except(Chunk(arr), [7, 2 ** 31 + 1, 1234, 0]).array
    assert got.tobytes() == want.astype(arr.dtype).tobytes()
    assert mask_except(Chunk(arr), '9').array.tobytes() == \
        np.where(arr == 9, arr, 0).astype(arr.dtype).tobytes()
    assert not mask_except(Chunk(arr), []).array.any()
    # ids outside the dtype's range match nothing
    assert not mask_except(Chunk(arr), [2 ** 40, -3]).array.any()
    same = Chunk(arr)
    assert mask_except(same, None) is same


def test_mask_out_objects_is_dust_then_selection():
    arr = tiny(np.uint64)
    got = mask_out_objects(Chunk(arr), dust_size_threshold=3,
                           selected_obj_ids=[7, 9]).array
    assert got.tobytes() == np.where(arr == 9, arr, 0).astype(
        arr.dtype).tobytes()
    same = Chunk(arr)
    assert mask_out_objects(same) is same


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.uint32,
                                   np.uint64, np.int32, np.int64])
def test_metadata_is_preserved(dtype):
    arr = (tiny() % 100).astype(dtype)
    chunk = Chunk(arr, voxel_offset=(3, 5, 7), voxel_size=(40, 4, 4))
    for out in (mask_fragments(chunk, 1), mask_except(chunk, [7]),
                mask_out_objects(chunk, 1, [7, 9])):
        assert out.array.dtype == dtype and out.shape == chunk.shape
        assert tuple(out.voxel_offset) == (3, 5, 7)
        assert tuple(out.voxel_size) == (40, 4, 4)


def test_rejections():
    with pytest.raises(TypeError):
        mask_fragments(Chunk(np.zeros((2, 3, 4), dtype=np.float32)), 1)
    with pytest.raises(TypeError):
        unique_counts(Chunk(np.zeros((2, 3, 4), dtype=bool)))
    with pytest.raises(ValueError):
        mask_except(Chunk(np.zeros((2, 2, 3, 4), dtype=np.uint32)), [1])
    with pytest.raises(ValueError):
        mask_out_objects(Chunk(np.zeros((2, 2, 3, 4), dtype=np.uint32)), 1)
    with pytest.raises(ValueError, match='protocol'):
        parse_obj_ids('gs://bucket/ids.json')
    with pytest.raises(ValueError, match='protocol'):
        parse_obj_ids('s3://bucket/ids.json')


def test_parse_obj_ids(tmp_path):
    assert parse_obj_ids(None) is None
    assert parse_obj_ids('34,56,78') == [34, 56, 78]
    assert parse_obj_ids({5}) == [5]
    path = tmp_path / 'ids.json'
    path.write_text(json.dumps([3, 2 ** 40]))
    assert parse_obj_ids(str(path)) == [3, 2 ** 40]
    assert parse_obj_ids(f'file://{path}') == [3, 2 ** 40]


def run_cli(tmp_path, *args):
    from chunkflow_amd.flow import main
    src, dst = tmp_path / 'in.npy', tmp_path / 'out.npy'
    np.save(src, tiny())
    result = CliRunner().invoke(main, [
        'load-npy', '-f', str(src), '-o', 'seg',
        'mask-out-objects', '-i', 'seg', '-o', 'clean', *args,
        'save-npy', '-i', 'clean', '-f', str(dst)])
    return result, dst


def test_cli_dust(tmp_path):
    result, dst = run_cli(tmp_path, '-d', '2')
    assert result.exit_code == 0, result.output
    want = mask_fragments(Chunk(tiny()), 2).array
    got = np.load(dst)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def test_cli_selected_ids_string(tmp_path):
    result, dst = run_cli(tmp_path, '--selected-obj-ids', '7,9')
    assert result.exit_code == 0, result.output
    arr = tiny()
    want = np.where((arr == 7) | (arr == 9), arr, 0).astype(arr.dtype)
    assert np.load(dst).tobytes() == want.tobytes()


def test_cli_selected_ids_json_and_dust(tmp_path):
    ids = tmp_path / 'ids.json'
    ids.write_text(json.dumps([5, 9]))
    result, dst = run_cli(tmp_path, '--dust-size-threshold', '1', '-s',
                          str(ids))
    assert result.exit_code == 0, result.output
    arr = tiny()
    want = np.where(arr == 9, arr, 0).astype(arr.dtype)  # 5 is dust
    assert np.load(dst).tobytes() == want.tobytes()


def test_cli_unsupported_protocol(tmp_path):
    result, dst = run_cli(tmp_path, '-s', 'gs://bucket/ids.json')
    assert result.exit_code != 0
    assert isinstance(result.exception, ValueError)
    assert 'protocol' in str(result.exception)
    assert not dst.exists()


def test_new_symbols_are_exported():
    from chunkflow_amd.build import build
    from chunkflow_amd.hip import KERNEL_IDS, SYMBOLS
    lib = ctypes.CDLL(build())
    for sym in ('cfx_connected_components_labels', 'cfx_label_run_starts',
                'cfx_label_table_clear', 'cfx_label_table_insert',
                'cfx_label_count', 'cfx_label_mask'):
        assert sym in SYMBOLS
        assert hasattr(lib, sym), sym
    assert KERNEL_IDS['labels'] == 12
