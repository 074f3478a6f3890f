"""ctypes binding to the in-tree HIP C-ABI extension (libchunkflow_amd.so).

The product GPU path calls exclusively through this module; if the extension
is missing on a machine with a GPU, every entry raises — there is no silent
eager/CPU fallback (DESIGN.md 'no fallback' rule).
"""
import ctypes
import os

import numpy as np

from .build import SO_PATH, build

# the C-ABI, declared once: symbol -> (restype, argtypes), position by
# position what include/chunkflow_amd.h declares (tests/test_abi.py checks
# every entry against the header text). Every pointer parameter is a
# c_void_p, host int arrays and out-parameters included: ctypes takes an
# int, None (NULL), a ctypes array or a byref() for it, and never cuts an
# address to a C int.
P, I, L, U, F = (ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong,
                 ctypes.c_uint, ctypes.c_float)
_CONV3 = (I, [P] * 6 + [I] * 7)      # ctx in wgt bias residual out, N..K flag
_STREAM = (I, [P] * 5 + [I] * 7)     # ctx in wgt bias out, N D H W C K flag
SIGNATURES = {
    'cfx_init': (P, [I]),
    'cfx_destroy': (None, [P]),
    'cfx_last_error': (ctypes.c_char_p, []),
    'cfx_version': (I, []),
    'cfx_set_stream': (I, [P, P]),
    'cfx_sync': (I, [P]),
    'cfx_make_patch_mask': (I, [P, P, P]),
    'cfx_normalize_intensity': (I, [P, P, P, L]),
    'cfx_cast_u8_f32_div': (I, [P, P, P, L, F]),
    'cfx_extract_patches': (I, [P, P, I, P, P, I, P, P]),
    'cfx_blend_accumulate': (I, [P, P, I, P, P, P, P, P]),
    'cfx_blend_batch': (I, [P, P, I, P, P, P, P, I, P]),
    'cfx_build_chunk_mask': (I, [P, P, P, P, P, P, I]),
    'cfx_reciprocal': (I, [P, P, L]),
    'cfx_multiply_mask': (I, [P, P, P, I, L]),
    'cfx_multiply_mask_max': (I, [P, P, P, I, L, P]),
    'cfx_max': (I, [P, P, L, P]),
    'cfx_crop_margin': (I, [P, P, P, I, P, P]),
    'cfx_mask_using_last_channel': (I, [P, P, P, I, P, F]),
    'cfx_threshold': (I, [P, P, P, L, F]),
    'cfx_nonzero_u8': (I, [P, P, P, L]),
    'cfx_connected_components': (I, [P, P, P, I, P, P, P]),
    'cfx_connected_components_labels': (I, [P, P, I, P, I, P, P, P]),
    'cfx_label_run_starts': (I, [P, P, I, P, P]),
    'cfx_label_table_clear': (I, [P, P, P, L]),
    'cfx_label_table_insert': (I, [P, P, L, U, P, P, L]),
    'cfx_label_count': (I, [P, P, I, P, P, P, L]),
    'cfx_label_pair_count': (I, [P, P, I, P, P, L, P, I, P, P, L, P, P, L]),
    'cfx_label_mask': (I, [P, P, P, I, P, P, P, L, I, L]),
    'cfx_affinity_fragments': (I, [P, P, P, F, F, P, P, P]),
    'cfx_region_graph_runs': (I, [P, P, P, P]),
    'cfx_region_graph': (I, [P, P, P, P, P, P, P, L]),
    'cfx_hist_u8': (I, [P, P, L, I, P]),
    'cfx_lut_apply_u8': (I, [P, P, L, I, P]),
    'cfx_gaussian2d': (I, [P, P, P, I, L, I, I, P, I, P, I]),
    'cfx_median3d': (I, [P, P, P, I, L, P, P, I]),
    'cfx_downsample_avg_u8': (I, [P, P, P, I, P, P]),
    'cfx_downsample_avg_f32': (I, [P, P, P, I, P, P]),
    'cfx_downsample_mode2': (I, [P, P, P, I, P, I]),
    'cfx_downsample_mode3': (I, [P, P, P, I, P]),
    'cfx_conv3_ndhwc': _CONV3,
    'cfx_conv3_ndhwc_w32': _CONV3,
    'cfx_conv3_ndhwc_zring': _CONV3,
    'cfx_conv3_ndhwc_bf16': _CONV3,
    'cfx_upconv_2x2': _STREAM,
    'cfx_upconv_2x2_add': _CONV3,    # ... bias skip out
    'cfx_downconv_2x2': _STREAM,
    'cfx_conv155_c1': (I, [P] * 5 + [I] * 6),    # no C: one input channel
    'cfx_conv155_out': _STREAM,
    'cfx_bias_res_elu': (I, [P, P, P, P, L, I, I]),
    'cfx_profile_enable': (I, [P, I]),
    'cfx_profile_reset': (I, [P]),
    'cfx_profile_get': (I, [P, I, P, P, P]),
}
SYMBOLS = list(SIGNATURES)

KERNEL_IDS = {
    'blend': 0, 'extract': 1, 'normalize': 2, 'cast': 3, 'reciprocal': 4,
    'maskmul': 5, 'crop': 6, 'max': 7, 'myelin': 8, 'cc': 9, 'conv': 10,
    'conv_stream': 11, 'labels': 12,
}

_lib = None


class CfxError(RuntimeError):
    pass


def _i3(v):
    return (ctypes.c_int * 3)(*[int(x) for x in v])


def _i6(v):
    return (ctypes.c_int * 6)(*[int(x) for x in v])


def _i32(a):
    """host int32 array for a `const int*` parameter (pass .ctypes.data)"""
    return np.ascontiguousarray(a, dtype=np.int32)


def load_library(build_if_missing: bool = True):
    """Load (building if needed) the extension; raises on failure."""
    global _lib
    if _lib is not None:
        return _lib
    path = SO_PATH
    if not os.path.exists(path):
        if not build_if_missing:
            raise CfxError(f'HIP extension not built: {path}')
        path = build()
    lib = ctypes.CDLL(path)
    for sym, (restype, argtypes) in SIGNATURES.items():
        if not hasattr(lib, sym):
            raise CfxError(f'{path} is missing symbol {sym}')
        fn = getattr(lib, sym)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def extension_available() -> bool:
    try:
        load_library(build_if_missing=False)
        return True
    except Exception:
        return False


class CfxContext:
    """One per GPU rank. Wraps the cfx_ctx and adopts torch's stream so
    kernels interleave correctly with the conv forward."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.ctx = self.lib.cfx_init(device)
        if not self.ctx:
            raise CfxError('cfx_init failed: '
                           + self.lib.cfx_last_error().decode())
        self.device = device

    def _call(self, name, *args, ok=(0,)):
        """lib.<name>(ctx, *args), converted by the SIGNATURES entry; a
        return code outside `ok` raises with the library's message."""
        rc = getattr(self.lib, name)(self.ctx, *args)
        if rc not in ok:
            raise CfxError(f'{name}: {self.lib.cfx_last_error().decode()}')
        return rc

    def close(self):
        if getattr(self, 'ctx', None):
            self.lib.cfx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- stream ------------------------------------------------------------
    def adopt_torch_stream(self):
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.set_stream(s)

    def set_stream(self, stream_ptr: int):
        self._call('cfx_set_stream', stream_ptr)

    def sync(self):
        self._call('cfx_sync')

    # --- kernels (device pointers are ints from tensor.data_ptr(); None is
    # NULL for the optional ones) ---------------------------------------------
    def normalize_intensity(self, in_ptr, out_ptr, n):
        self._call('cfx_normalize_intensity', in_ptr, out_ptr, n)

    def cast_u8_f32_div(self, in_ptr, out_ptr, n, divisor):
        self._call('cfx_cast_u8_f32_div', in_ptr, out_ptr, n, divisor)

    def extract_patches(self, chunk_ptr, channels, chunk_dims, starts,
                        patch_size, out_ptr):
        starts = _i32(starts)
        self._call('cfx_extract_patches', chunk_ptr, channels,
                   _i3(chunk_dims), starts.ctypes.data, starts.shape[0],
                   _i3(patch_size), out_ptr)

    def blend_accumulate(self, out_ptr, channels, out_dims, patch_ptr,
                         patch_dims, offset, mask_ptr=None):
        self._call('cfx_blend_accumulate', out_ptr, channels, _i3(out_dims),
                   patch_ptr, _i3(patch_dims), _i3(offset), mask_ptr)

    def blend_batch(self, out_ptr, channels, out_dims, patch_ptr,
                    patch_dims, items, mask_ptr=None):
        """items: (n, 4) int32 array of (batch_index, oz, oy, ox); clipped
        regions must be pairwise disjoint."""
        items = _i32(items)
        self._call('cfx_blend_batch', out_ptr, channels, _i3(out_dims),
                   patch_ptr, _i3(patch_dims), items.ctypes.data,
                   items.shape[0], mask_ptr)

    def build_chunk_mask(self, mask_out_ptr, out_dims, patch_mask_ptr,
                         patch_dims, offsets):
        offsets = _i32(offsets)
        self._call('cfx_build_chunk_mask', mask_out_ptr, _i3(out_dims),
                   patch_mask_ptr, _i3(patch_dims), offsets.ctypes.data,
                   offsets.shape[0])

    def reciprocal(self, ptr, n):
        self._call('cfx_reciprocal', ptr, n)

    def multiply_mask(self, out_ptr, mask_ptr, channels, n_voxels):
        self._call('cfx_multiply_mask', out_ptr, mask_ptr, channels,
                   n_voxels)

    def multiply_mask_max(self, out_ptr, mask_ptr, channels, n_voxels):
        """Returns the post-multiply max, or None if the fused path was
        unavailable (caller should use max())."""
        out = ctypes.c_float(0)
        rc = self._call('cfx_multiply_mask_max', out_ptr, mask_ptr,
                        channels, n_voxels, ctypes.byref(out), ok=(0, -2))
        return None if rc == -2 else out.value

    def max(self, ptr, n) -> float:
        out = ctypes.c_float(0)
        self._call('cfx_max', ptr, n, ctypes.byref(out))
        return out.value

    def crop_margin(self, in_ptr, out_ptr, channels, in_dims, margins):
        self._call('cfx_crop_margin', in_ptr, out_ptr, channels,
                   _i3(in_dims), _i6(margins))

    def mask_using_last_channel(self, in_ptr, out_ptr, channels, dims,
                                threshold):
        self._call('cfx_mask_using_last_channel', in_ptr, out_ptr, channels,
                   _i3(dims), threshold)

    # --- connected components ----------------------------------------------
    def threshold(self, in_ptr, fg_ptr, n, thresh):
        self._call('cfx_threshold', in_ptr, fg_ptr, n, thresh)

    def nonzero_u8(self, in_ptr, fg_ptr, n):
        self._call('cfx_nonzero_u8', in_ptr, fg_ptr, n)

    def connected_components(self, fg_ptr, dims, connectivity, labels_ptr,
                             scratch_ptr) -> int:
        ncomp = ctypes.c_longlong(0)
        self._call('cfx_connected_components', fg_ptr, _i3(dims),
                   connectivity, labels_ptr, scratch_ptr,
                   ctypes.byref(ncomp))
        return ncomp.value

    def connected_components_labels(self, seg_ptr, elem_bytes, dims,
                                    connectivity, labels_ptr,
                                    scratch_ptr) -> int:
        ncomp = ctypes.c_longlong(0)
        self._call('cfx_connected_components_labels', seg_ptr, elem_bytes,
                   _i3(dims), connectivity, labels_ptr, scratch_ptr,
                   ctypes.byref(ncomp))
        return ncomp.value

    # --- label tables (per-label counts, masking) ----------------------------
    def label_run_starts(self, labels_ptr, elem_bytes, dims) -> int:
        runs = ctypes.c_longlong(0)
        self._call('cfx_label_run_starts', labels_ptr, elem_bytes,
                   _i3(dims), ctypes.byref(runs))
        return runs.value

    def label_table_clear(self, keys_ptr, vals_ptr, capacity):
        self._call('cfx_label_table_clear', keys_ptr, vals_ptr, capacity)

    def label_table_insert(self, ids_ptr, n_ids, value, keys_ptr, vals_ptr,
                           capacity):
        self._call('cfx_label_table_insert', ids_ptr, n_ids, value,
                   keys_ptr, vals_ptr, capacity)

    def label_count(self, labels_ptr, elem_bytes, dims, keys_ptr, vals_ptr,
                    capacity):
        self._call('cfx_label_count', labels_ptr, elem_bytes, _i3(dims),
                   keys_ptr, vals_ptr, capacity)

    def label_pair_count(self, seg_ptr, seg_bytes, seg_dims, seg_keys_ptr,
                         seg_capacity, gt_ptr, gt_bytes, gt_dims,
                         gt_keys_ptr, gt_capacity, keys_ptr, vals_ptr,
                         capacity):
        self._call('cfx_label_pair_count', seg_ptr, seg_bytes,
                   _i3(seg_dims), seg_keys_ptr, seg_capacity, gt_ptr,
                   gt_bytes, _i3(gt_dims), gt_keys_ptr, gt_capacity,
                   keys_ptr, vals_ptr, capacity)

    def label_mask(self, in_ptr, out_ptr, elem_bytes, dims, keys_ptr,
                   vals_ptr, capacity, mode, threshold=0):
        self._call('cfx_label_mask', in_ptr, out_ptr, elem_bytes, _i3(dims),
                   keys_ptr, vals_ptr, capacity, mode, threshold)

    # --- affinity maps to segments -------------------------------------------
    def affinity_fragments(self, aff_ptr, dims, low, high, labels_ptr,
                           scratch_ptr) -> int:
        ncomp = ctypes.c_longlong(0)
        self._call('cfx_affinity_fragments', aff_ptr, _i3(dims), low, high,
                   labels_ptr, scratch_ptr, ctypes.byref(ncomp))
        return ncomp.value

    def region_graph_runs(self, frag_ptr, dims) -> int:
        runs = ctypes.c_longlong(0)
        self._call('cfx_region_graph_runs', frag_ptr, _i3(dims),
                   ctypes.byref(runs))
        return runs.value

    def region_graph(self, frag_ptr, aff_ptr, dims, keys_ptr, counts_ptr,
                     sums_ptr, capacity):
        self._call('cfx_region_graph', frag_ptr, aff_ptr, _i3(dims),
                   keys_ptr, counts_ptr, sums_ptr, capacity)

    # --- convolutions --------------------------------------------------------
    def conv3_ndhwc(self, in_ptr, wgt_ptr, bias_ptr, residual_ptr, out_ptr,
                    n, d, h, w, c, k, do_elu=False, w32=False,
                    zring=False):
        self._call('cfx_conv3_ndhwc_zring' if zring
                   else 'cfx_conv3_ndhwc_w32' if w32 else 'cfx_conv3_ndhwc',
                   in_ptr, wgt_ptr, bias_ptr, residual_ptr, out_ptr,
                   n, d, h, w, c, k, bool(do_elu))

    def conv3_ndhwc_bf16(self, in_ptr, wgt_ptr, bias_ptr, residual_ptr,
                         out_ptr, n, d, h, w, c, k, do_elu=False):
        self._call('cfx_conv3_ndhwc_bf16', in_ptr, wgt_ptr, bias_ptr,
                   residual_ptr, out_ptr, n, d, h, w, c, k, bool(do_elu))

    def upconv_2x2(self, in_ptr, wgt_ptr, bias_ptr, out_ptr, n, d, h, w,
                   c, k, bf16=False):
        self._call('cfx_upconv_2x2', in_ptr, wgt_ptr, bias_ptr, out_ptr,
                   n, d, h, w, c, k, bool(bf16))

    def upconv_2x2_add(self, in_ptr, wgt_ptr, bias_ptr, skip_ptr, out_ptr,
                       n, d, h, w, c, k, bf16=False):
        """up-conv with `skip` (f32 NDHWC, the output's shape) added in
        the kernel's epilogue; skip_ptr None is upconv_2x2."""
        self._call('cfx_upconv_2x2_add', in_ptr, wgt_ptr, bias_ptr,
                   skip_ptr, out_ptr, n, d, h, w, c, k, bool(bf16))

    def bias_res_elu(self, y_ptr, bias_ptr, res_ptr, nvox, k, do_elu=True):
        """in place on NDHWC f32 y: y = act(y + bias (+ res))"""
        self._call('cfx_bias_res_elu', y_ptr, bias_ptr, res_ptr, nvox, k,
                   bool(do_elu))

    def downconv_2x2(self, in_ptr, wgt_ptr, bias_ptr, out_ptr, n, d, h, w,
                     c, k, bf16=False):
        self._call('cfx_downconv_2x2', in_ptr, wgt_ptr, bias_ptr, out_ptr,
                   n, d, h, w, c, k, bool(bf16))

    def conv155_c1(self, in_ptr, wgt_ptr, bias_ptr, out_ptr, n, d, h, w,
                   k, bf16=False):
        self._call('cfx_conv155_c1', in_ptr, wgt_ptr, bias_ptr, out_ptr,
                   n, d, h, w, k, bool(bf16))

    def conv155_out(self, in_ptr, wgt_ptr, bias_ptr, out_ptr, n, d, h, w,
                    c, k, bf16=False):
        self._call('cfx_conv155_out', in_ptr, wgt_ptr, bias_ptr, out_ptr,
                   n, d, h, w, c, k, bool(bf16))

    # --- image normalization -------------------------------------------------
    def hist_u8(self, in_ptr, n_per_sec, nsec, hist_ptr):
        self._call('cfx_hist_u8', in_ptr, n_per_sec, nsec, hist_ptr)

    def lut_apply_u8(self, buf_ptr, n_per_sec, nsec, lut_ptr):
        self._call('cfx_lut_apply_u8', buf_ptr, n_per_sec, nsec, lut_ptr)

    # --- image filters -------------------------------------------------------
    def gaussian2d(self, in_ptr, out_ptr, is_f32, sections, height, width,
                   wy_ptr, ry, wx_ptr, rx):
        """wy_ptr / wx_ptr: device f64 weights (2*r+1 each), or None with
        radius 0 to skip that axis"""
        self._call('cfx_gaussian2d', in_ptr, out_ptr, bool(is_f32), sections,
                   height, width, wy_ptr, ry, wx_ptr, rx)

    def median3d(self, in_ptr, out_ptr, is_f32, volumes, dims, size, mode):
        self._call('cfx_median3d', in_ptr, out_ptr, bool(is_f32), volumes,
                   _i3(dims), _i3(size), mode)

    # --- downsample ----------------------------------------------------------
    def downsample_avg(self, in_ptr, out_ptr, channels, in_dims, factor,
                       is_f32=False):
        self._call('cfx_downsample_avg_f32' if is_f32
                   else 'cfx_downsample_avg_u8', in_ptr, out_ptr, channels,
                   _i3(in_dims), _i3(factor))

    def downsample_mode2(self, in_ptr, out_ptr, elem_bytes, in_dims,
                         preserved_axis):
        self._call('cfx_downsample_mode2', in_ptr, out_ptr, elem_bytes,
                   _i3(in_dims), preserved_axis)

    def downsample_mode3(self, in_ptr, out_ptr, elem_bytes, in_dims):
        self._call('cfx_downsample_mode3', in_ptr, out_ptr, elem_bytes,
                   _i3(in_dims))

    # --- profiling ----------------------------------------------------------
    def profile_enable(self, enable=True):
        self._call('cfx_profile_enable', bool(enable))

    def profile_reset(self):
        self._call('cfx_profile_reset')

    def profile_get(self, kernel: str):
        count = ctypes.c_ulonglong(0)
        ms = ctypes.c_double(0)
        bytes_ = ctypes.c_double(0)
        self._call('cfx_profile_get', KERNEL_IDS[kernel],
                   ctypes.byref(count), ctypes.byref(ms),
                   ctypes.byref(bytes_))
        return {'count': count.value, 'total_ms': ms.value,
                'bytes': bytes_.value}


def make_patch_mask_c(patch_size, overlap) -> np.ndarray:
    """Host-side C implementation of the bump patch mask (C-ABI
    completeness; the Python product path uses chunkflow_amd.patch_mask)."""
    lib = load_library()
    out = np.empty(tuple(patch_size), dtype=np.float32)
    if lib.cfx_make_patch_mask(_i3(patch_size), _i3(overlap),
                               out.ctypes.data) != 0:
        raise CfxError('cfx_make_patch_mask failed')
    return out
