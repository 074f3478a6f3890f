"""downsample: box averaging and COUNTLESS mode pooling (PRODUCT code).

The step after inference / crop-margin / connected-components in a real
deployment: writing the result as a mip pyramid (reference flow/flow.py
:1545-1573, downsample_upload.py, save_precomputed --create-thumbnail).

Results are pinned bit-exactly to the numpy implementation the reference
ships (lib/igneous/downsample.py: downsample_with_averaging and
downsample_segmentation, called the way downsample_upload.py:67-75 calls
them) through tests/golden/downsample_cases.npz — NOT to `tinybrain`, whose
uint8 rounding was not verified. All rules below are in z,y,x order.

Averaging (uint8, float32; any positive integer factor):
  * output shape ceil(dim / f); edge cells average the voxels that exist;
  * the sum is float32 from 0, x-offset slowest, z-offset fastest;
  * the quotient is float64 sum / count, then converted to the input dtype:
    round-to-nearest for float32, TRUNCATION for uint8;
  * factor (1,1,1) returns the input unchanged.

Mode pooling (integer labels other than uint8):
  * factor a permutation of (1,2,2): COUNTLESS 2D per slice of the preserved
    axis. With a the low/low voxel, d the high/high voxel and b, c the mixed
    ones: a if a==b or a==c, else b if b==c, else d. Zero is an ordinary
    label. A pooled axis of ODD length is first extended by duplicating its
    first voxel at the front ([v0,v1,v2] -> [v0,v0,v1,v2]); the output
    length is (n+1)//2 and every block after the first is shifted by one
    voxel against an even-aligned grid. A reference quirk, replicated;
  * factor (2,2,2) on an all-even shape: COUNTLESS 3D. Over the eight voxels
    s = 4*dx + 2*dy + dz: the value of the lexicographically first all-equal
    4-combination, else of the first 3-combination, else of the first equal
    pair among s = 0..6, else voxel 7;
  * (2,2,2) on a shape with an odd dim, any factor whose product is no power
    of two, and a power-of-two factor without a 1 on a shape with an odd
    dim: plain striding arr[::fz, ::fy, ::fx], as the reference does;
  * every other power-of-two-product factor — (1,4,4), (4,4,4) on even
    shapes, (1,2,1) ... — raises ValueError: the reference's recursion
    crashes on them, so there is no behaviour to pin. Use
    downsample_pyramid, which reaches 4x by two 2x levels.

Out of contract: labels equal to the maximum value of a 64-bit or signed
dtype (the reference's internal +1 wraps there).

Device chunks run the gfx950 kernels (csrc/downsample.hip); host chunks use
the vectorised numpy below, with identical results. Device int32 / int64
tensors carry uint32 / uint64 labels: labels compare as raw bit patterns.
"""
import numpy as np

from .cartesian import Cartesian
from .chunk import Chunk

try:
    import torch
except ImportError:
    torch = None


def check_factor(factor) -> tuple:
    factor = tuple(int(f) for f in factor)
    if len(factor) != 3:
        raise ValueError(f'factor must have 3 entries (z,y,x): {factor}')
    if min(factor) <= 0:
        raise ValueError(
            f"Factors less than one don't make sense. Factor: {factor}")
    return factor


def mode_plan(shape, factor) -> tuple:
    """How the reference treats `factor` on a 3-D label volume of `shape`:
    ('identity',), ('mode2', preserved_axis), ('mode3',) or ('stride',);
    raises ValueError for the factors its recursion crashes on."""
    factor = check_factor(factor)
    if factor == (1, 1, 1):
        return ('identity',)
    prod = factor[0] * factor[1] * factor[2]
    if prod & (prod - 1):
        return ('stride',)
    if 1 in factor:
        if sorted(factor) == [1, 2, 2]:
            return ('mode2', factor.index(1))
    elif any(s % 2 for s in shape):
        return ('stride',)
    elif factor == (2, 2, 2):
        return ('mode3',)
    raise ValueError(
        f'mode pooling supports factor (2,2,2) and the permutations of '
        f'(1,2,2) only, but got {factor}; use downsample_pyramid to reach '
        f'higher factors by repeated 2x levels')


# --- host path (vectorised numpy) -------------------------------------------
def average_host(arr: np.ndarray, factor) -> np.ndarray:
    """(z,y,x) or (C,z,y,x) uint8/float32 box average."""
    fz, fy, fx = check_factor(factor)
    if (fz, fy, fx) == (1, 1, 1):
        return arr
    lead = arr.shape[:-3]
    out_shape = lead + tuple(-(-s // f) for s, f in
                             zip(arr.shape[-3:], (fz, fy, fx)))
    acc = np.zeros(out_shape, dtype=np.float32)
    count = np.zeros(out_shape[-3:], dtype=np.int64)
    for dx in range(fx):
        for dy in range(fy):
            for dz in range(fz):
                part = arr[..., dz::fz, dy::fy, dx::fx]
                nz, ny, nx = part.shape[-3:]
                acc[..., :nz, :ny, :nx] += part
                count[:nz, :ny, :nx] += 1
    return (acc.astype(np.float64) / count).astype(arr.dtype)


def _mirror_index(n: int) -> tuple:
    """(low, high) source indices of the 2-blocks along an axis of length n
    whose odd length is front-mirrored."""
    odd = n % 2
    i = np.arange((n + 1) // 2)
    return np.maximum(2 * i - odd, 0), 2 * i + 1 - odd


def _mode2_host(arr: np.ndarray, preserved_axis: int) -> np.ndarray:
    ax0, ax1 = [ax for ax in range(3) if ax != preserved_axis]
    lo0, hi0 = _mirror_index(arr.shape[ax0])
    lo1, hi1 = _mirror_index(arr.shape[ax1])
    low, high = np.take(arr, lo0, axis=ax0), np.take(arr, hi0, axis=ax0)
    a, b = np.take(low, lo1, axis=ax1), np.take(low, hi1, axis=ax1)
    c, d = np.take(high, lo1, axis=ax1), np.take(high, hi1, axis=ax1)
    return np.where((a == b) | (a == c), a, np.where(b == c, b, d))


def _mode3_host(arr: np.ndarray) -> np.ndarray:
    v = [arr[(s & 1)::2, ((s >> 1) & 1)::2, (s >> 2)::2] for s in range(8)]
    # equal-value classes are disjoint, so the first all-equal k-combination
    # belongs to the class of size >= k with the smallest lowest index
    count = [sum((v[i] == v[j]).astype(np.int8) for j in range(8))
             for i in range(8)]
    count7 = [sum((v[i] == v[j]).astype(np.int8) for j in range(7))
              for i in range(7)]
    out = v[7].copy()
    for i in range(6, -1, -1):
        out = np.where(count7[i] >= 2, v[i], out)
    for need in (3, 4):
        for i in range(7, -1, -1):
            out = np.where(count[i] >= need, v[i], out)
    return out


def mode_host(arr: np.ndarray, factor) -> np.ndarray:
    """(z,y,x) integer label volume -> mode-pooled / strided volume."""
    assert arr.ndim == 3
    plan = mode_plan(arr.shape, factor)
    if plan[0] == 'identity':
        return arr
    if plan[0] == 'mode2':
        return _mode2_host(arr, plan[1])
    if plan[0] == 'mode3':
        return _mode3_host(arr)
    fz, fy, fx = check_factor(factor)
    return np.ascontiguousarray(arr[::fz, ::fy, ::fx])


# --- dispatch ---------------------------------------------------------------
def _np_dtype(chunk: Chunk) -> np.dtype:
    dt = chunk.dtype
    if torch is not None and isinstance(dt, torch.dtype):
        return np.dtype(str(dt).split('.')[-1])
    return np.dtype(dt)


def _method(chunk: Chunk) -> str:
    """'average' or 'mode', by the reference's is_image / is_segmentation
    (chunk/base.py:495-504); float32 3-D or (C,z,y,x) chunks average too, as
    in the reference's DownsampleUploadOperator (downsample_upload.py:72)."""
    dt = _np_dtype(chunk)
    if chunk.ndim == 3 and dt == np.uint8:
        return 'average'
    if chunk.ndim == 3 and np.issubdtype(dt, np.integer):
        return 'mode'
    if chunk.ndim in (3, 4) and dt == np.float32:
        return 'average'
    raise TypeError(
        f'only support image or segmentation, but got: {chunk.dtype}')


def _hip_ops(device_index: int):
    from .ops import shared_hip_ops
    return shared_hip_ops(device_index)


def downsample(chunk: Chunk, factor=(2, 2, 2)) -> Chunk:
    """One mip level down. uint8 3-D chunks and float32 3-D / (C,z,y,x)
    chunks are averaged, other 3-D integer chunks are mode-pooled; anything
    else (bool included) raises TypeError. The result has voxel_offset //
    factor and voxel_size * factor."""
    factor = check_factor(factor)
    method = _method(chunk)
    if chunk.is_device:
        ops = _hip_ops(chunk.array.device.index or 0)
        t = chunk.array
        out = (ops.downsample_average(t, factor) if method == 'average'
               else ops.downsample_mode(t, factor))
    else:
        arr = chunk.numpy().array
        out = (average_host(arr, factor) if method == 'average'
               else mode_host(arr, factor))
    f = Cartesian(*factor)
    voxel_size = chunk.voxel_size * f if chunk.voxel_size is not None \
        else None
    return Chunk(out, voxel_offset=chunk.voxel_offset // f,
                 voxel_size=voxel_size)


def downsample_pyramid(chunk: Chunk, factor=(2, 2, 2),
                       num_mips: int = 1) -> list:
    """num_mips successive levels, each computed from the previous one
    (reference lib/igneous/tasks.py:58-60). On the device this is one launch
    per level with no host round trip or sync in between."""
    levels = []
    for _ in range(int(num_mips)):
        chunk = downsample(chunk, factor)
        levels.append(chunk)
    return levels
