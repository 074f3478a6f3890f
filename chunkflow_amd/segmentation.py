"""Segmentation cleanup and scoring: per-label voxel counts, dust removal,
object selection and evaluation against a ground truth (PRODUCT code).

Cleanup is the reference's `mask-out-objects` operator (flow/flow.py
:2015-2050) and the Segmentation methods under it (chunk/segmentation.py
:86-109).

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

Evaluation — the reference's `evaluate-segmentation` operator (flow/flow.py
:1519-1542 -> Segmentation.evaluate, chunk/segmentation.py:33-67 ->
lib/gala/evaluate.py):

  contingency(seg, gt)       (seg_ids, gt_ids, counts): one row per distinct
                             (seg, gt) pair of labels with its voxel count,
                             sorted by unsigned (seg, gt); zero is a label
  scores_from_contingency    the five scores from those rows, on the host
                             in float64
  evaluate(seg, gt, t)       the reference's dict of scores

Every score is a function of the contingency table alone, so the device
path only has to build the table (csrc/labels.hip, k_pair_count); both
paths then share scores_from_contingency, and equal tables give identical
floats. The reference's quirks that are reproduced are listed at
scores_from_contingency and in DESIGN.md.

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


def _hip_ops(device_index: int):
    from .ops import shared_hip_ops
    return shared_hip_ops(device_index)


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


# --- evaluation against a ground truth --------------------------------------
SCORE_KEYS = ('rand_index', 'adjusted_rand_index', 'variation_of_information',
              'fowlkes_mallows_index', 'edit_distance')


def _as_u64(arr: np.ndarray) -> np.ndarray:
    """astype(np.uint64) as the reference does (signed values wrap)."""
    return np.ascontiguousarray(arr).astype(np.uint64, copy=False)


def contingency_host(seg: np.ndarray, gt: np.ndarray):
    """Runs of equal pairs in flat order first (the device kernel's view of
    the volume), then a lexsort of the runs only."""
    s, g = _as_u64(seg).ravel(), _as_u64(gt).ravel()
    n = s.size
    start = np.ones(n, dtype=bool)
    start[1:] = (s[1:] != s[:-1]) | (g[1:] != g[:-1])
    idx = np.flatnonzero(start)
    lens = np.diff(np.append(idx, n)).astype(np.int64)
    rs, rg = s[idx], g[idx]
    order = np.lexsort((rg, rs))
    rs, rg, lens = rs[order], rg[order], lens[order]
    first = np.ones(rs.size, dtype=bool)
    first[1:] = (rs[1:] != rs[:-1]) | (rg[1:] != rg[:-1])
    fidx = np.flatnonzero(first)
    return rs[fidx], rg[fidx], np.add.reduceat(lens, fidx)


def _device_labels(chunk: Chunk, device):
    """The chunk's labels as an int32/int64 tensor on `device`, carrying
    uint32 / uint64: a host chunk is uploaded, a narrow dtype widened."""
    if chunk.is_device:
        t = chunk.array
        if t.dtype not in (torch.int32, torch.int64):
            t = t.to(torch.int64)
        return t.to(device)
    arr = np.ascontiguousarray(chunk.numpy().array)
    if arr.dtype == np.uint32:
        arr = arr.view(np.int32)
    elif arr.dtype != np.int64:
        arr = _as_u64(arr).view(np.int64)
    return torch.from_numpy(arr).to(device)


def contingency(seg: Chunk, gt: Chunk):
    """(seg_ids, gt_ids, counts): for every pair of labels (s, g) that some
    voxel carries, the number of voxels that do; rows sorted by unsigned
    (s, g), zero an ordinary label. Host chunks give numpy arrays (ids
    uint64, counts int64). If either chunk is on the device the other is
    uploaded and the gfx950 kernels build the table: device tensors, ids
    int64 carrying uint64, counts int64. Only the arrays are compared: the
    shapes must agree, the voxel offsets are not looked at (the reference
    passes the arrays alone)."""
    _check(seg, 'contingency')
    _check(gt, 'contingency')
    if tuple(seg.shape) != tuple(gt.shape):
        raise ValueError(f'contingency: segmentation {tuple(seg.shape)} and '
                         f'ground truth {tuple(gt.shape)} differ in shape')
    if seg.is_device or gt.is_device:
        anchor = seg if seg.is_device else gt
        device = anchor.array.device
        return _ops_for(anchor).label_contingency(
            _device_labels(seg, device), _device_labels(gt, device))
    return contingency_host(seg.numpy().array, gt.numpy().array)


def _host_u64(ids) -> np.ndarray:
    if torch is not None and isinstance(ids, torch.Tensor):
        ids = ids.cpu().numpy()
    ids = np.asarray(ids)
    if ids.dtype == np.int64:
        return ids.view(np.uint64)
    return ids.astype(np.uint64)


def _totals(ids: np.ndarray, counts: np.ndarray):
    """(distinct ids, index of each row's id among them, exact totals)."""
    uniq, inverse = np.unique(ids, return_inverse=True)
    totals = np.zeros(uniq.size, dtype=np.uint64)
    np.add.at(totals, inverse, counts)
    return uniq, inverse, totals


def _xlogx(x: np.ndarray) -> np.ndarray:
    y = x.copy()
    nz = y.nonzero()
    y[nz] *= np.log2(y[nz])
    return y


def scores_from_contingency(seg_ids, gt_ids, counts,
                            size_threshold: int = 1000) -> dict:
    """The reference's scores (lib/gala/evaluate.py) from contingency rows,
    on the host in float64; device triples are copied to the host first.
    Returns the five keys of `evaluate` plus `false_splits_by_column`.

    Rand, adjusted Rand and Fowlkes-Mallows use every voxel, zero being a
    label like any other (the reference passes no ignore list there). The
    four sums they need are exact integers (N < 2^32, so all fit a uint64);
    they are converted to float64 once and closed with the reference's
    expressions in its order of operations (evaluate.py:1215-1300), on
    np.float64 so that 0/0 is NaN rather than an exception.

    Variation of information uses only pairs with s != 0 and g != 0,
    normalised by their total: H(gt|seg) + H(seg|gt) in log2; NaN when
    there is no such pair, as in the reference.

    edit_distance is (false_merges, 0.0). Of the pairs with s != 0, g != 0
    and more than size_threshold voxels, false_merges = (number of such
    pairs) - (number of distinct non-zero seg labels): a segment with no
    surviving overlap contributes -1, so the value can be negative — the
    reference's arithmetic. The second element is always 0.0: the reference
    slices a 1 x N np.matrix with [1:], which empties it. The count it
    meant, pairs - distinct non-zero gt labels, is `false_splits_by_column`.
    """
    s, g = _host_u64(seg_ids), _host_u64(gt_ids)
    if torch is not None and isinstance(counts, torch.Tensor):
        counts = counts.cpu().numpy()
    n = np.asarray(counts).astype(np.uint64)
    seg_uniq, seg_inv, seg_tot = _totals(s, n)
    gt_uniq, gt_inv, gt_tot = _totals(g, n)
    f64 = np.float64
    with np.errstate(divide='ignore', invalid='ignore'):
        total = f64(int(n.sum()))
        sum1 = f64(int((n * n).sum()))
        sum2 = f64(int((seg_tot * seg_tot).sum()))
        sum3 = f64(int((gt_tot * gt_tot).sum()))
        a = (sum1 - total) / 2.0
        b = (sum2 - sum1) / 2
        c = (sum3 - sum1) / 2
        d = (sum1 + total ** 2 - sum2 - sum3) / 2
        rand_index = (a + d) / (a + b + c + d)
        nk = a + b + c + d
        chance = (a + b) * (a + c) + (c + d) * (b + d)
        adjusted_rand_index = (nk * (a + d) - chance) / (nk ** 2 - chance)
        fowlkes_mallows_index = a / (np.sqrt((a + b) * (a + c)))

        inner = (s != 0) & (g != 0)
        m = n[inner].astype(f64)
        if m.size == 0 or m.sum() == 0:
            vi = f64('nan')
        else:
            pxy = m / m.sum()
            si, gi = seg_inv[inner], gt_inv[inner]
            px = np.bincount(si, weights=pxy, minlength=seg_uniq.size)
            py = np.bincount(gi, weights=pxy, minlength=gt_uniq.size)
            lpygx = np.bincount(si, weights=_xlogx(pxy / px[si]),
                                minlength=seg_uniq.size)
            lpxgy = np.bincount(gi, weights=_xlogx(pxy / py[gi]),
                                minlength=gt_uniq.size)
            hygx = -(px * lpygx)
            hxgy = -(py * lpxgy)
            vi = np.dot(np.ones(2), np.array([hygx.sum(), hxgy.sum()]))

    survivors = int((inner & (n.astype(np.int64) > size_threshold)).sum())
    false_merges = f64(survivors - int((seg_uniq != 0).sum()))
    false_splits = f64(survivors - int((gt_uniq != 0).sum()))
    return {
        'rand_index': rand_index,
        'adjusted_rand_index': adjusted_rand_index,
        'variation_of_information': f64(vi),
        'fowlkes_mallows_index': fowlkes_mallows_index,
        'edit_distance': (false_merges, f64(0.0)),
        'false_splits_by_column': false_splits,
    }


def evaluate(seg: Chunk, gt: Chunk, size_threshold: int = 1000) -> dict:
    """Score a segmentation against a ground truth: the reference's
    Segmentation.evaluate, with exactly its keys. Device chunks are scored
    from a contingency table built on the device."""
    scores = scores_from_contingency(*contingency(seg, gt),
                                     size_threshold=size_threshold)
    return {key: scores[key] for key in SCORE_KEYS}
