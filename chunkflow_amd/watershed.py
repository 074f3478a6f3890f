"""Affinity maps to segments: watershed fragments, the region graph between
them and mean-affinity agglomeration (PRODUCT code).

The reference does this in its `agglomerate` plugin (chunkflow/plugins/
agglomerate.py), which hands the affinity map to the waterz C++ wheel.
waterz's labels are pinned by no reference test (as cc3d's),
so the semantics are defined here, order-independent and exact; the host
functions below are both the path for host chunks and the oracle of the
device path (csrc/watershed.hip), which must give the same integers.
DESIGN.md ("Watershed and agglomeration") lists the two places where this
knowingly differs from waterz.

Affinity map. f32 (3, Z, Y, X), chunkflow's channel order x, y, z: aff[c][v]
is the weight of the edge between voxel v and its predecessor along that
axis (c=0: x-1, c=1: y-1, c=2: z-1). The values on the leading face of each
axis belong to no edge and never enter a decision. Other dtypes are
converted to f32 first on either path (exact for f16 / bf16).

  affinity_fragments(chunk, low, high)
      A steepest-ascent forest. An edge is live iff w >= low and strong iff
      live and w >= high, compared in f32; NaN fails both. A voxel with a
      live incident edge picks the first one in the order -x +x -y +y -z +z
      whose weight equals the maximum over its live incident edges. The
      fragments are the connected components of the voxels under the strong
      and the picked edges, numbered 1..N by first voxel in raster order; a
      voxel with no live incident edge is background 0. With low == high ==
      T these are the connected components of the edges >= T.
  region_graph(frag, aff)
      (a, b, count, sum): one row per pair a < b of different non-zero
      fragment ids joined by at least one edge, sorted by (a, b); count is
      the number of those edges and sum the sum over them of q(w) =
      floor(c * 2^24), c = w > 0 ? min(w, 1) : 0 in f32 (NaN and negative
      weights give 0). The mean affinity of a row is sum / (count * 2^24).
  agglomerate(aff, threshold, low, high, fragments=None)
      fragments (unless given), region graph, agglomeration.merge_fragments
      with merge_threshold = threshold, and one gather through the map.

Host chunks give numpy results (labels uint32). Device chunks run the gfx950
kernels and stay on the device: labels are int32 tensors carrying uint32 as
on the connected-components paths, region-graph rows int64 tensors. Only the
region graph comes to the host for merging.
"""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

from .agglomeration import SCALE_BITS, merge_fragments
from .chunk import Chunk

try:
    import torch
except ImportError:
    torch = None

# (channel, array axis) of the three edge directions
_EDGE_AXES = ((0, 2), (1, 1), (2, 0))


def _lo_hi(axis):
    """index tuples selecting each edge's predecessor end and its own end"""
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[axis], hi[axis] = slice(None, -1), slice(1, None)
    return tuple(lo), tuple(hi)


def _host_aff(aff) -> np.ndarray:
    aff = np.ascontiguousarray(aff, dtype=np.float32)
    if aff.ndim != 4 or aff.shape[0] != 3:
        raise ValueError(f'affinity map must be (3, Z, Y, X), but got shape '
                         f'{aff.shape}')
    if aff.size == 0:
        raise ValueError('affinity map is empty')
    return aff


# --- host path (numpy / scipy; the oracle of the device path) ---------------
def affinity_fragments_host(aff, low: float, high: float):
    """(labels uint32 (Z, Y, X), number of fragments)"""
    aff = _host_aff(aff)
    low, high = np.float32(low), np.float32(high)
    shape = aff.shape[1:]
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    step = (1, shape[2], shape[1] * shape[2])
    # per voxel its six incident edges in the order -x +x -y +y -z +z
    weight = np.full((6,) + shape, -np.inf, dtype=np.float32)
    live = np.zeros((6,) + shape, dtype=bool)
    offset = np.empty(6, dtype=np.int64)
    src, dst = [], []
    for c, axis in _EDGE_AXES:
        lo, hi = _lo_hi(axis)
        w = aff[c][hi]
        ok = w >= low
        weight[2 * c][hi], live[2 * c][hi] = w, ok
        weight[2 * c + 1][lo], live[2 * c + 1][lo] = w, ok
        offset[2 * c], offset[2 * c + 1] = -step[c], step[c]
        strong = ok & (w >= high)
        src.append(idx[hi][strong])
        dst.append(idx[lo][strong])
    best = np.where(live, weight, -np.inf).max(axis=0)
    pick = (live & (weight == best)).argmax(axis=0)
    fg = live.any(axis=0)
    src.append(idx[fg])
    dst.append(idx[fg] + offset[pick[fg]])
    src, dst = np.concatenate(src), np.concatenate(dst)
    graph = sparse.coo_matrix(
        (np.ones(src.size, dtype=np.uint8), (src, dst)), shape=(n, n))
    _, comp = csgraph.connected_components(graph, directed=False)
    # number the foreground components by their first voxel in flat order
    fg = fg.ravel()
    comp = comp[fg]
    uniq, first = np.unique(comp, return_index=True)
    remap = np.zeros(int(comp.max()) + 1 if comp.size else 1,
                     dtype=np.uint32)
    remap[uniq[np.argsort(first, kind='stable')]] = \
        np.arange(1, uniq.size + 1, dtype=np.uint32)
    labels = np.zeros(n, dtype=np.uint32)
    labels[fg] = remap[comp]
    return labels.reshape(shape), int(uniq.size)


def quantise(w: np.ndarray) -> np.ndarray:
    """q(w) as uint64; the product by 2^24 is exact in f32"""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        c = np.where(w > 0, np.minimum(w, np.float32(1)), np.float32(0))
    return np.floor(c * np.float32(2 ** SCALE_BITS)).astype(np.uint64)


def region_graph_host(frag, aff):
    """(a uint32, b uint32, count int64, sum uint64), sorted by (a, b)"""
    aff = _host_aff(aff)
    frag = np.ascontiguousarray(frag)
    if frag.dtype == np.int32:
        frag = frag.view(np.uint32)
    if frag.shape != aff.shape[1:]:
        raise ValueError(f'region_graph: fragments {frag.shape} and affinity '
                         f'map {aff.shape} differ in shape')
    frag = frag.astype(np.uint64)
    keys, q = [], []
    for c, axis in _EDGE_AXES:
        lo, hi = _lo_hi(axis)
        a, b = frag[hi], frag[lo]
        sel = (a != b) & (a != 0) & (b != 0)
        a, b = a[sel], b[sel]
        keys.append((np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b))
        q.append(quantise(aff[c][hi][sel]))
    keys, q = np.concatenate(keys), np.concatenate(q)
    order = np.argsort(keys, kind='stable')
    keys, q = keys[order], q[order]
    first = np.ones(keys.size, dtype=bool)
    first[1:] = keys[1:] != keys[:-1]
    at = np.flatnonzero(first)
    rows = keys[at]
    count = np.diff(np.append(at, keys.size)).astype(np.int64)
    total = (np.add.reduceat(q, at) if keys.size
             else np.zeros(0, dtype=np.uint64))
    return ((rows >> np.uint64(32)).astype(np.uint32),
            (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), count, total)


# --- dispatch ---------------------------------------------------------------
def _ops_for(tensor):
    from .ops import shared_hip_ops
    return shared_hip_ops(tensor.device.index or 0)


def _array(x):
    return x.array if isinstance(x, Chunk) else x


def _is_device(x) -> bool:
    x = _array(x)
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


def _host(x) -> np.ndarray:
    x = _array(x)
    if torch is not None and isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.asarray(x)


def _like(chunk, array) -> Chunk:
    if isinstance(chunk, Chunk):
        return Chunk(array, voxel_offset=chunk.voxel_offset,
                     voxel_size=chunk.voxel_size)
    return Chunk(array)


def affinity_fragments(chunk, low: float, high: float) -> Chunk:
    """Watershed fragments of an affinity chunk (see the module text)."""
    if _is_device(chunk):
        labels, _ = _ops_for(_array(chunk)).affinity_fragments(
            _array(chunk), low, high)
    else:
        labels, _ = affinity_fragments_host(_host(chunk), low, high)
    return _like(chunk, labels)


def region_graph(frag, aff):
    """Rows (a, b, count, sum) of the region graph; device tensors (int64)
    when the affinity map is on the device (host fragments are uploaded),
    numpy arrays otherwise."""
    if _is_device(aff):
        aff_t = _array(aff)
        frag_t = _array(frag)
        if not _is_device(frag_t):
            host = np.ascontiguousarray(_host(frag_t))
            if host.dtype == np.uint32:
                host = host.view(np.int32)
            frag_t = torch.from_numpy(host).to(aff_t.device)
        return _ops_for(aff_t).region_graph(frag_t, aff_t)
    return region_graph_host(_host(frag), _host(aff))


def _dense_ids(frag):
    """Caller-supplied fragments may carry any ids: (volume of 0..N with 0
    staying 0, N), dense in ascending order of the ids."""
    if _is_device(frag):
        t = _array(frag)
        wide = t.to(torch.int64)
        if t.dtype == torch.int32:
            wide = wide & 0xFFFFFFFF
        ids, inverse = torch.unique(wide, return_inverse=True)
        has_zero = bool(ids[0] == 0)
        dense = inverse if has_zero else inverse + 1
        return dense.to(torch.int32), int(ids.numel()) - int(has_zero)
    arr = _host(frag)
    # int32 / int64 carry uint32 / uint64 on the host too, as on the device
    if arr.dtype in (np.int32, np.int64):
        arr = arr.view(np.uint32 if arr.dtype == np.int32 else np.uint64)
    ids, inverse = np.unique(arr, return_inverse=True)
    has_zero = bool(ids[0] == 0)
    dense = inverse.reshape(arr.shape) + (0 if has_zero else 1)
    return dense.astype(np.uint32), int(ids.size) - int(has_zero)


def agglomerate(aff, threshold: float, low: float, high: float,
                fragments=None) -> Chunk:
    """Segment an affinity chunk: fragments, region graph, then merging in
    order of decreasing mean affinity while the mean is > threshold
    (agglomeration.merge_fragments). Segment ids are dense 1..M in raster
    first-voxel order; with caller-supplied `fragments` (any integer ids,
    signed dtypes read as unsigned, host or device) in ascending order of
    each segment's smallest id. A device chunk gives a device segmentation:
    only the region graph visits the host."""
    device = _is_device(aff)
    if fragments is None:
        if device:
            frag, n_frag = _ops_for(_array(aff)).affinity_fragments(
                _array(aff), low, high)
        else:
            frag, n_frag = affinity_fragments_host(_host(aff), low, high)
    else:
        if not device:
            fragments = _host(fragments)
        frag, n_frag = _dense_ids(fragments)
        if device and not _is_device(frag):
            frag = torch.from_numpy(frag.view(np.int32)).to(
                _array(aff).device)
    rows = region_graph(frag, aff)
    if device:
        rows = tuple(r.cpu().numpy() for r in rows)
    seg_of = merge_fragments(rows, n_frag, threshold)
    if device:
        table = torch.from_numpy(seg_of.view(np.int32)).to(frag.device)
        # fragment ids are dense, far below 2^31: the int32 volume indexes
        seg = table[frag]
    else:
        seg = seg_of[frag]
    return _like(aff, seg)
