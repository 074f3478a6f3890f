"""filters: per-section 2-D gaussian and 3-D median (PRODUCT code).

The two image filters the reference ships for the step before inference: the
`gaussian-filter` operator (flow/flow.py:1615-1630, Chunk.gaussian_filter_2d
at chunk/base.py:846-853, plugins/gaussian_filter.py) and the median_filter
plugin (plugins/median_filter.py), whose default size (3,1,1) is the z-median
that bridges a damaged or missing section. Both are pinned bit for bit to
scipy.ndimage, which is what the reference calls. All rules are in z,y,x
order; chunks are (z,y,x) or (C,z,y,x), uint8 or float32 on the device.

gaussian_filter_2d: every (y,x) section of every channel on its own.
  * KNOWING DIFFERENCE: on a (C,z,y,x) chunk the reference's
    Chunk.gaussian_filter_2d hands (C,y,x) to scipy and so also blurs across
    channels; the reference's own plugin filters per channel, and so do we.
    On (z,y,x) chunks the result is the reference's, bit for bit;
  * per axis, y first, then x; an axis with sigma <= 1e-15 is skipped;
  * radius r = int(4.0 * sigma + 0.5); weights in numpy float64:
    x = arange(-r, r+1); w = exp(-0.5 / (sigma*sigma) * x**2); w /= w.sum();
  * every input value is converted to float64 and the sum is built in
    scipy's symmetric order: t = v[i] * w[r], then for k = -r .. -1:
    t += (v[i+k] + v[i-k]) * w[k+r] — outermost taps first, the two
    neighbours added before the multiply, nothing fused;
  * border 'reflect', d c b a | a b c d | d c b a, period 2n; an axis
    shorter than the radius reflects several times;
  * the result of EACH pass is converted to the chunk's dtype before the
    next pass reads it: float32 rounds to nearest, uint8 TRUNCATES (a
    constant section of 255 comes out as whatever 255 * sum(w) truncates
    to). `gaussian_filter_2d_restated` below is this in plain numpy;
  * on the device the radius is at most GAUSS_MAX_RADIUS (the halo one LDS
    tile of csrc/filter.hip holds): a larger sigma raises ValueError.

median_filter: the element of rank N//2 of the N = sz*sy*sx values of the
window centred on the voxel; a (C,z,y,x) chunk is filtered per channel (an
extension: scipy raises on a 4-D array with a 3-entry size).
  * border modes 'reflect', 'nearest', 'mirror', 'constant' (value 0) and
    'wrap', each with scipy's meaning;
  * on the device every size entry is odd and N <= 125; anything beyond, or
    an unknown mode, raises ValueError; a dtype other than uint8 / float32
    raises TypeError;
  * out of contract: float NaN, and the sign of a zero result.

Host chunks call scipy.ndimage directly — it is the reference. Device chunks
run the gfx950 kernels (csrc/filter.hip) and stay on the device; there is no
host fallback.
"""
import numpy as np

from .chunk import Chunk

try:
    import torch
except ImportError:
    torch = None

MODES = ('reflect', 'nearest', 'mirror', 'constant', 'wrap')  # C-ABI codes
GAUSS_MAX_RADIUS = 24      # csrc/filter.hip's constant of the same name
MEDIAN_MAX_WINDOW = 125    # likewise
DEVICE_DTYPES = ('uint8', 'float32')


# --- argument rules (callable without a GPU) ---------------------------------
def check_sigma(sigma) -> tuple:
    """(sigma_y, sigma_x) as floats; a number means both."""
    if np.isscalar(sigma):
        sigma = (sigma, sigma)
    sigma = tuple(float(s) for s in sigma)
    if len(sigma) != 2:
        raise ValueError(f'sigma must be a number or (sigma_y, sigma_x): '
                         f'{sigma}')
    if min(sigma) < 0 or not all(np.isfinite(sigma)):
        raise ValueError(f'sigma must be finite and not negative: {sigma}')
    return sigma


def gaussian_weights(sigma: float):
    """(radius, float64 weights) of one axis as scipy computes them, or None
    for an axis that is skipped."""
    sigma = float(sigma)
    if sigma <= 1e-15:
        return None
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w /= w.sum()
    return r, w


def check_median(size, mode) -> tuple:
    """(size as 3 ints, mode code)"""
    size = tuple(int(s) for s in size)
    if len(size) != 3:
        raise ValueError(f'size must have 3 entries (z,y,x): {size}')
    if min(size) <= 0:
        raise ValueError(f'size entries must be positive: {size}')
    if mode not in MODES:
        raise ValueError(f'mode must be one of {MODES}, but got {mode!r}')
    return size, MODES.index(mode)


def _np_dtype(dtype) -> np.dtype:
    if torch is not None and isinstance(dtype, torch.dtype):
        return np.dtype(str(dtype).split('.')[-1])
    return np.dtype(dtype)


def _check_device_dtype(who: str, dtype):
    if _np_dtype(dtype).name not in DEVICE_DTYPES:
        raise TypeError(f'{who}: uint8 or float32 only, but got: {dtype}')


def check_gaussian_device(dtype, sigma) -> list:
    """The device path's rules: per axis (radius, weights) or None; raises
    TypeError / ValueError for what the kernel does not hold."""
    _check_device_dtype('gaussian_filter_2d', dtype)
    plan = [gaussian_weights(s) for s in check_sigma(sigma)]
    for axis in plan:
        if axis is not None and axis[0] > GAUSS_MAX_RADIUS:
            raise ValueError(
                f'gaussian_filter_2d: sigma {sigma} needs radius {axis[0]}, '
                f'above the device cap of {GAUSS_MAX_RADIUS} (sigma up to '
                f'{(GAUSS_MAX_RADIUS + 0.49) / 4.0:.2f})')
    return plan


def check_median_device(dtype, size, mode) -> tuple:
    """The device path's rules: (size, mode code)"""
    _check_device_dtype('median_filter', dtype)
    size, code = check_median(size, mode)
    if any(s % 2 == 0 for s in size):
        raise ValueError(f'median_filter: every size entry must be odd on '
                         f'the device: {size}')
    if size[0] * size[1] * size[2] > MEDIAN_MAX_WINDOW:
        raise ValueError(f'median_filter: a window of {size} is above the '
                         f'device cap of {MEDIAN_MAX_WINDOW} voxels')
    return size, code


# --- the arithmetic, restated in numpy ---------------------------------------
def border_index(i: np.ndarray, n: int, mode: str) -> np.ndarray:
    """Source index on an axis of length n of the positions i, which may lie
    outside it by any distance; -1 marks the constant border."""
    i = np.asarray(i)
    if mode == 'reflect':
        m = np.mod(i, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    if mode == 'nearest':
        return np.clip(i, 0, n - 1)
    if mode == 'mirror':
        if n == 1:
            return np.zeros_like(i)
        m = np.mod(i, 2 * n - 2)
        return np.where(m < n, m, 2 * n - 2 - m)
    if mode == 'wrap':
        return np.mod(i, n)
    if mode == 'constant':
        return np.where((i >= 0) & (i < n), i, -1)
    raise ValueError(f'mode must be one of {MODES}, but got {mode!r}')


def _symmetric_pass(arr: np.ndarray, axis: int, r: int,
                    w: np.ndarray) -> np.ndarray:
    n = arr.shape[axis]
    pos = np.arange(n)
    v = arr.astype(np.float64)

    def tap(k):
        return np.take(v, border_index(pos + k, n, 'reflect'), axis=axis)

    t = tap(0) * w[r]
    for k in range(-r, 0):
        t = t + (tap(k) + tap(-k)) * w[k + r]
    if arr.dtype == np.uint8:
        return np.trunc(t).astype(np.uint8)
    return t.astype(arr.dtype)


def gaussian_filter_2d_restated(arr: np.ndarray, sigma=1) -> np.ndarray:
    """What the kernel must compute: the rules of the module docstring over
    the last two axes of a uint8 / float32 array, a new array."""
    arr = np.asarray(arr)
    out = arr.copy()
    for axis, plan in zip((-2, -1),
                          (gaussian_weights(s) for s in check_sigma(sigma))):
        if plan is not None:
            out = _symmetric_pass(out, axis, *plan)
    return out


def median_filter_restated(arr: np.ndarray, size=(3, 1, 1),
                           mode: str = 'reflect') -> np.ndarray:
    """Rank-N//2 element of the centred window over the last three axes,
    with the border rules of `border_index`."""
    size, _ = check_median(size, mode)
    arr = np.asarray(arr)
    index, outside = [], []
    for n, s in zip(arr.shape[-3:], size):
        i = border_index(np.arange(n)[None, :]
                         + np.arange(s)[:, None] - s // 2, n, mode)
        outside.append(i < 0)
        index.append(np.maximum(i, 0))
    window = []
    for dz in range(size[0]):
        for dy in range(size[1]):
            for dx in range(size[2]):
                v = arr[..., index[0][dz][:, None, None],
                        index[1][dy][None, :, None],
                        index[2][dx][None, None, :]]
                out = (outside[0][dz][:, None, None]
                       | outside[1][dy][None, :, None]
                       | outside[2][dx][None, None, :])
                window.append(np.where(out, arr.dtype.type(0), v))
    return np.sort(np.stack(window), axis=0)[len(window) // 2]


# --- dispatch ----------------------------------------------------------------
def _hip_ops(device_index: int):
    from .ops import shared_hip_ops
    return shared_hip_ops(device_index)


def _as_chunk(chunk, who: str) -> Chunk:
    if not isinstance(chunk, Chunk):
        chunk = Chunk(chunk)
    if chunk.ndim not in (3, 4):
        raise ValueError(f'{who}: (z,y,x) or (C,z,y,x) only, but got '
                         f'{chunk.ndim} dimensions')
    return chunk


def gaussian_filter_2d(chunk, sigma=1, inplace: bool = False) -> Chunk:
    """Gaussian blur of every (y,x) section of a Chunk, numpy array or torch
    tensor; sigma is a number or (sigma_y, sigma_x). With inplace the
    chunk's own array is overwritten and returned, otherwise a new one."""
    chunk = _as_chunk(chunk, 'gaussian_filter_2d')
    sigma = check_sigma(sigma)
    if chunk.is_device:
        t = chunk.array
        out = _hip_ops(t.device.index or 0).gaussian_filter_2d(t, sigma)
        if inplace:
            out = t.copy_(out)
    else:
        import scipy.ndimage
        src = chunk.numpy().array
        out = src if inplace else np.empty_like(src)
        for section in np.ndindex(*src.shape[:-2]):
            out[section] = scipy.ndimage.gaussian_filter(src[section],
                                                         sigma=sigma)
        if inplace:
            out = chunk.array
    return Chunk(out, voxel_offset=chunk.voxel_offset,
                 voxel_size=chunk.voxel_size)


def median_filter(chunk, size=(3, 1, 1), mode: str = 'reflect') -> Chunk:
    """Median over the size (z,y,x) window centred on each voxel of a Chunk,
    numpy array or torch tensor, per channel for (C,z,y,x); a new array.
    Float NaN and the sign of a zero result are out of contract."""
    chunk = _as_chunk(chunk, 'median_filter')
    if chunk.is_device:
        t = chunk.array
        out = _hip_ops(t.device.index or 0).median_filter(t, size, mode)
    else:
        import scipy.ndimage
        size, _ = check_median(size, mode)
        src = chunk.numpy().array
        if src.ndim == 3:
            out = scipy.ndimage.median_filter(src, size=size, mode=mode)
        else:
            out = np.stack([
                scipy.ndimage.median_filter(c, size=size, mode=mode)
                for c in src]) if len(src) else src.copy()
    return Chunk(out, voxel_offset=chunk.voxel_offset,
                 voxel_size=chunk.voxel_size)
