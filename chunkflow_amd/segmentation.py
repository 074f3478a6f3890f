"""Segmentation cleanup: per-label voxel counts, dust removal and object
selection (PRODUCT code) — the reference's `mask-out-objects` operator
(flow/flow.py:2015-2050) and the Segmentation methods under it
(chunk/segmentation.py:86-109).

The reference delegates to `fastremap.unique`, `fastremap.mask` and
`fastremap.mask_except`. The pin here is to those functions' DOCUMENTED
semantics expressed in numpy (the host path below), not to the fastremap
binary:

  unique_counts(chunk)       np.unique(arr, return_counts=True): ids
                             ascending, zero included
  mask_fragments(chunk, t)   every label whose voxel count is <= t becomes 0
                             (`counts <= voxel_num_threshold`, as in the
                             reference)
  mask_except(chunk, ids)    every label not in ids becomes 0; None leaves
                             the chunk unchanged, an empty list zeroes it
  mask_out_objects(...)      dust first, then selection — the operator's
                             order

Zero stays zero throughout. All of them take and return a 3-D integer Chunk
and preserve dtype, voxel_offset and voxel_size; the input is not modified.

Host chunks use numpy. Device chunks run the gfx950 kernels
(csrc/labels.hip: a label table in HBM, one table operation per run of equal
labels) with byte-identical results. Device int32 / int64 tensors carry
uint32 / uint64 labels, as in downsample: labels compare as raw bit
patterns, `unique_counts` orders them by UNSIGNED value, and ids passed to
`mask_except` are unsigned values.

Out of contract on the device: the label 2^64-1 (the table's empty-slot
key; the kernels report it as an error) and volumes of more than 2^32-1
voxels (counts are 32-bit).
"""
import json

import numpy as np

from .chunk import Chunk

try:
    import torch
except ImportError:
    torch = None


def _np_dtype(chunk: Chunk) -> np.dtype:
    dt = chunk.dtype
    if torch is not None and isinstance(dt, torch.dtype):
        return np.dtype(str(dt).split('.')[-1])
    return np.dtype(dt)


def _check(chunk: Chunk, who: str):
    if not isinstance(chunk, Chunk):
        raise TypeError(f'{who}: expected a Chunk, but got: {type(chunk)}')
    if chunk.ndim != 3:
        raise ValueError(f'{who}: 3-D segmentation only, but got shape '
                         f'{chunk.shape}')
    if not np.issubdtype(_np_dtype(chunk), np.integer):
        raise TypeError(f'{who}: integer segmentation only, but got: '
                        f'{chunk.dtype}')


_OPS = {}


def _hip_ops(device_index: int):
    from .ops import HipOps
    if device_index not in _OPS:
        _OPS[device_index] = HipOps(device_index)
    return _OPS[device_index]


def _ops_for(chunk: Chunk):
    return _hip_ops(chunk.array.device.index or 0)


def _like(chunk: Chunk, array) -> Chunk:
    return Chunk(array, voxel_offset=chunk.voxel_offset,
                 voxel_size=chunk.voxel_size)


def valid_ids(ids, lo: int, hi: int) -> list:
    """Distinct ints of `ids` within [lo, hi], ascending: an id outside a
    dtype's range matches no voxel of that dtype."""
    return sorted({int(i) for i in ids if lo <= int(i) <= hi})


def parse_obj_ids(selected_obj_ids):
    """The CLI's `--selected-obj-ids`: None, a list/set of ints, "34,56,78",
    or the path of a .json file holding a list (a local path or file://; the
    reference reads cloud paths through CloudFiles, which this project does
    not ship — any other protocol raises)."""
    if selected_obj_ids is None:
        return None
    if isinstance(selected_obj_ids, str):
        text = selected_obj_ids.strip()
        if text.endswith('.json'):
            if '://' in text:
                protocol, path = text.split('://', 1)
                if protocol != 'file':
                    raise ValueError(
                        f'selected-obj-ids: unsupported protocol '
                        f'"{protocol}://" (local paths and file:// only): '
                        f'{text}')
                text = path
            with open(text) as f:
                ids = json.load(f)
            if not isinstance(ids, list):
                raise ValueError(f'selected-obj-ids: {text} must hold a '
                                 f'JSON list of ids')
            return [int(i) for i in ids]
        if '://' in text:
            raise ValueError(f'selected-obj-ids: expected "34,56,78" or a '
                             f'.json path, but got: {text}')
        return [int(i) for i in text.split(',') if i.strip() != '']
    return [int(i) for i in selected_obj_ids]


# --- host path (numpy; the oracle of the device path) -----------------------
def unique_counts_host(arr: np.ndarray):
    return np.unique(arr, return_counts=True)


def mask_fragments_host(arr: np.ndarray, voxel_num_threshold: int):
    ids, counts = np.unique(arr, return_counts=True)
    fragments = ids[counts <= voxel_num_threshold]
    return np.where(np.isin(arr, fragments), 0, arr).astype(arr.dtype)


def mask_except_host(arr: np.ndarray, ids) -> np.ndarray:
    info = np.iinfo(arr.dtype)
    keep = np.array(valid_ids(ids, info.min, info.max), dtype=arr.dtype)
    return np.where(np.isin(arr, keep), arr, 0).astype(arr.dtype)


# --- dispatch ---------------------------------------------------------------
def unique_counts(chunk: Chunk):
    """(ids, counts) like np.unique(return_counts=True): numpy arrays for a
    host chunk, device tensors for a device chunk (ids in the chunk's dtype,
    ascending by unsigned value; counts int64)."""
    _check(chunk, 'unique_counts')
    if chunk.is_device:
        return _ops_for(chunk).label_unique_counts(chunk.array)
    return unique_counts_host(chunk.numpy().array)


def mask_fragments(chunk: Chunk, voxel_num_threshold: int) -> Chunk:
    """Remove dust: labels with at most `voxel_num_threshold` voxels -> 0."""
    _check(chunk, 'mask_fragments')
    threshold = int(voxel_num_threshold)
    if chunk.is_device:
        out = _ops_for(chunk).label_mask_fragments(chunk.array, threshold)
    else:
        out = mask_fragments_host(chunk.numpy().array, threshold)
    return _like(chunk, out)


def mask_except(chunk: Chunk, selected_obj_ids) -> Chunk:
    """Keep only the listed objects; None leaves the chunk as it is."""
    _check(chunk, 'mask_except')
    ids = parse_obj_ids(selected_obj_ids)
    if ids is None:
        return chunk
    if chunk.is_device:
        bits = 8 * chunk.array.element_size()
        # 64-bit: 2^64-1 is the table's empty key and cannot be selected
        hi = 2 ** 32 - 1 if bits == 32 else 2 ** 64 - 2
        out = _ops_for(chunk).label_mask_except(chunk.array,
                                                valid_ids(ids, 0, hi))
    else:
        out = mask_except_host(chunk.numpy().array, ids)
    return _like(chunk, out)


def mask_out_objects(chunk: Chunk, dust_size_threshold: int = None,
                     selected_obj_ids=None) -> Chunk:
    """The mask-out-objects operator: dust removal, then object selection;
    each step is skipped when its argument is None."""
    _check(chunk, 'mask_out_objects')
    if dust_size_threshold is not None:
        chunk = mask_fragments(chunk, dust_size_threshold)
    if selected_obj_ids is not None:
        chunk = mask_except(chunk, selected_obj_ids)
    return chunk
