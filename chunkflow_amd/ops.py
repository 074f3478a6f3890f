"""Device-op layer under the Inferencer.

Two implementations of the same small interface over torch tensors:

  * HipOps — the PRODUCT path: hand-written gfx950 kernels through the C-ABI
    extension, stream-ordered on torch's current stream. Raises loudly if
    the extension is missing; never falls back.
  * TorchOps — CPU plumbing for GPU-less machines only (BASELINE config 1 is
    explicitly a no-GPU plumbing config, and the reference itself runs on
    CPU). The Inferencer refuses to pick TorchOps when a GPU is visible, so
    the GPU path can never silently degrade.
"""
import numpy as np
import torch


class HipOps:
    is_hip = True

    def __init__(self, device_index: int = 0):
        from .hip import CfxContext
        self.cfx = CfxContext(device_index)
        self.device = f'cuda:{device_index}'
        self.cfx.adopt_torch_stream()

    def sync(self):
        self.cfx.sync()

    def cast_div(self, u8: torch.Tensor, divisor: float) -> torch.Tensor:
        out = torch.empty(u8.shape, dtype=torch.float32, device=u8.device)
        self.cfx.cast_u8_f32_div(u8.data_ptr(), out.data_ptr(), u8.numel(),
                                 divisor)
        return out

    def normalize_intensity(self, u8: torch.Tensor) -> torch.Tensor:
        out = torch.empty(u8.shape, dtype=torch.float32, device=u8.device)
        self.cfx.normalize_intensity(u8.data_ptr(), out.data_ptr(),
                                     u8.numel())
        return out

    def extract(self, chunk_f32: torch.Tensor, starts: np.ndarray,
                patch_size, out_batch: torch.Tensor):
        dims = chunk_f32.shape[-3:]
        channels = 1 if chunk_f32.ndim == 3 else chunk_f32.shape[0]
        self.cfx.extract_patches(chunk_f32.data_ptr(), channels, dims,
                                 starts, patch_size, out_batch.data_ptr())

    def blend(self, out: torch.Tensor, patch_batch: torch.Tensor,
              batch_index: int, offset, mask: torch.Tensor = None):
        channels = out.shape[0]
        pdims = patch_batch.shape[-3:]
        pvox = pdims[0] * pdims[1] * pdims[2]
        patch_ptr = (patch_batch.data_ptr()
                     + batch_index * patch_batch.shape[1] * pvox * 4)
        self.cfx.blend_accumulate(
            out.data_ptr(), channels, out.shape[-3:], patch_ptr, pdims,
            offset, mask.data_ptr() if mask is not None else None)

    def blend_batch(self, out: torch.Tensor, patch_batch: torch.Tensor,
                    items: np.ndarray, mask: torch.Tensor = None):
        """items: (n, 4) = (batch_index, oz, oy, ox), regions disjoint."""
        channels = out.shape[0]
        self.cfx.blend_batch(
            out.data_ptr(), channels, out.shape[-3:],
            patch_batch.data_ptr(), patch_batch.shape[-3:], items,
            mask.data_ptr() if mask is not None else None)

    def build_chunk_mask(self, out_dims, patch_mask: torch.Tensor,
                         offsets: np.ndarray,
                         groups=None) -> torch.Tensor:
        """Blend the patch mask at every offset then reciprocal. With
        `groups` (disjoint index groups over `offsets`), uses one launch
        per group instead of one per offset."""
        if groups is None:
            mask = torch.empty(tuple(out_dims), dtype=torch.float32,
                               device=patch_mask.device)
            self.cfx.build_chunk_mask(mask.data_ptr(), out_dims,
                                      patch_mask.data_ptr(),
                                      patch_mask.shape[-3:], offsets)
            return mask
        mask = torch.zeros(tuple(out_dims), dtype=torch.float32,
                           device=patch_mask.device)
        mask3 = mask.unsqueeze(0)  # (1, D, H, W): one "channel"
        pm = patch_mask.unsqueeze(0)  # batch of one patch
        for idx in groups:
            items = np.concatenate(
                [np.zeros((len(idx), 1), dtype=np.int32),
                 np.asarray(offsets, dtype=np.int32)[idx]], axis=1)
            self.blend_batch(mask3, pm, items)
        self.cfx.reciprocal(mask.data_ptr(), mask.numel())
        return mask

    def multiply_mask(self, out: torch.Tensor, mask: torch.Tensor):
        self.cfx.multiply_mask(out.data_ptr(), mask.data_ptr(),
                               out.shape[0], mask.numel())

    def multiply_mask_max(self, out: torch.Tensor,
                          mask: torch.Tensor) -> float:
        """Fused mask-normalize + the <1.0001 max scan."""
        m = self.cfx.multiply_mask_max(out.data_ptr(), mask.data_ptr(),
                                       out.shape[0], mask.numel())
        if m is None:
            m = self.cfx.max(out.data_ptr(), out.numel())
        return m

    def max(self, t: torch.Tensor) -> float:
        return self.cfx.max(t.data_ptr(), t.numel())

    def crop_margin(self, t: torch.Tensor, margins) -> torch.Tensor:
        channels = 1 if t.ndim == 3 else t.shape[0]
        d, h, w = t.shape[-3:]
        od = d - margins[0] - margins[3]
        oh = h - margins[1] - margins[4]
        ow = w - margins[2] - margins[5]
        shape = (channels, od, oh, ow) if t.ndim == 4 else (od, oh, ow)
        out = torch.empty(shape, dtype=t.dtype, device=t.device)
        self.cfx.crop_margin(t.data_ptr(), out.data_ptr(), channels,
                             (d, h, w), margins)
        return out

    def mask_using_last_channel(self, t: torch.Tensor,
                                threshold: float) -> torch.Tensor:
        channels = t.shape[0]
        out = torch.empty((channels - 1,) + tuple(t.shape[1:]),
                          dtype=t.dtype, device=t.device)
        self.cfx.mask_using_last_channel(t.data_ptr(), out.data_ptr(),
                                         channels, t.shape[-3:], threshold)
        return out

    def downsample_average(self, t: torch.Tensor, factor) -> torch.Tensor:
        """Box average of a uint8/float32 (z,y,x) or (C,z,y,x) tensor
        (semantics: chunkflow_amd/downsample.py)."""
        from .downsample import check_factor
        factor = check_factor(factor)
        if t.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f'downsample_average: uint8 or float32 only, '
                            f'but got: {t.dtype}')
        if t.ndim not in (3, 4):
            raise ValueError(f'downsample_average: 3-D or 4-D only: {t.shape}')
        if factor == (1, 1, 1):
            return t
        t = t.contiguous()
        dims = tuple(t.shape[-3:])
        odims = tuple(-(-s // f) for s, f in zip(dims, factor))
        out = torch.empty(tuple(t.shape[:-3]) + odims, dtype=t.dtype,
                          device=t.device)
        self.cfx.downsample_avg(t.data_ptr(), out.data_ptr(),
                                1 if t.ndim == 3 else t.shape[0], dims,
                                factor, is_f32=t.dtype == torch.float32)
        return out

    def downsample_mode(self, t: torch.Tensor, factor) -> torch.Tensor:
        """COUNTLESS mode pooling (or the reference's striding fallback) of
        a 3-D tensor of 4- or 8-byte integer labels."""
        from .downsample import check_factor, mode_plan
        if t.ndim != 3:
            raise ValueError(f'downsample_mode: 3-D only: {t.shape}')
        if t.is_floating_point() or t.dtype == torch.bool or \
                t.element_size() not in (4, 8):
            raise TypeError(f'downsample_mode: 4- or 8-byte integer labels '
                            f'only, but got: {t.dtype}')
        plan = mode_plan(t.shape, factor)
        if plan[0] == 'identity':
            return t
        if plan[0] == 'stride':
            fz, fy, fx = check_factor(factor)
            return t[::fz, ::fy, ::fx].contiguous()
        t = t.contiguous()
        dims = tuple(t.shape)
        if plan[0] == 'mode2':
            odims = tuple(s if ax == plan[1] else (s + 1) // 2
                          for ax, s in enumerate(dims))
            out = torch.empty(odims, dtype=t.dtype, device=t.device)
            self.cfx.downsample_mode2(t.data_ptr(), out.data_ptr(),
                                      t.element_size(), dims, plan[1])
        else:
            out = torch.empty(tuple(s // 2 for s in dims), dtype=t.dtype,
                              device=t.device)
            self.cfx.downsample_mode3(t.data_ptr(), out.data_ptr(),
                                      t.element_size(), dims)
        return out

    # --- image filters (semantics: chunkflow_amd/filters.py; kernels:
    # csrc/filter.hip) ---------------------------------------------------------
    def gaussian_filter_2d(self, t: torch.Tensor, sigma) -> torch.Tensor:
        """Per-section 2-D gaussian of a uint8/float32 (z,y,x) or (C,z,y,x)
        tensor, a new tensor."""
        from .filters import check_gaussian_device
        plan = check_gaussian_device(t.dtype, sigma)
        if t.ndim not in (3, 4):
            raise ValueError(f'gaussian_filter_2d: 3-D or 4-D only: '
                             f'{tuple(t.shape)}')
        t = t.contiguous()
        out = torch.empty_like(t)
        if t.numel() == 0:
            return out
        if plan[0] is None and plan[1] is None:
            return out.copy_(t)
        # the weights are scipy's float64 values, computed on the host
        weights = [None if axis is None else
                   torch.from_numpy(axis[1]).to(t.device) for axis in plan]
        (wy, ry), (wx, rx) = [
            (None, 0) if axis is None else (wt.data_ptr(), axis[0])
            for axis, wt in zip(plan, weights)]
        h, w = t.shape[-2:]
        self.cfx.gaussian2d(t.data_ptr(), out.data_ptr(),
                            t.dtype == torch.float32, t.numel() // (h * w),
                            h, w, wy, ry, wx, rx)
        return out

    def median_filter(self, t: torch.Tensor, size=(3, 1, 1),
                      mode: str = 'reflect') -> torch.Tensor:
        """3-D median of a uint8/float32 (z,y,x) or (C,z,y,x) tensor (per
        channel), a new tensor."""
        from .filters import check_median_device
        size, code = check_median_device(t.dtype, size, mode)
        if t.ndim not in (3, 4):
            raise ValueError(f'median_filter: 3-D or 4-D only: '
                             f'{tuple(t.shape)}')
        t = t.contiguous()
        out = torch.empty_like(t)
        if t.numel() == 0:
            return out
        self.cfx.median3d(t.data_ptr(), out.data_ptr(),
                          t.dtype == torch.float32,
                          1 if t.ndim == 3 else t.shape[0],
                          tuple(t.shape[-3:]), size, code)
        return out

    # --- label tables: per-label voxel counts and masking -------------------
    # (semantics: chunkflow_amd/segmentation.py; kernels: csrc/labels.hip)
    LABEL_TABLE_MIN = 64

    @staticmethod
    def _check_labels(t: torch.Tensor, who: str) -> torch.Tensor:
        if t.ndim != 3:
            raise ValueError(f'{who}: 3-D only: {tuple(t.shape)}')
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f'{who}: device labels must be int32 or int64 '
                            f'(carrying uint32 / uint64), but got: {t.dtype}')
        if t.numel() == 0:
            raise ValueError(f'{who}: empty volume')
        return t.contiguous()

    def _new_label_table(self, distinct_bound: int, device):
        """A cleared table with room for `distinct_bound` keys at a load
        factor of at most one half."""
        capacity = self.LABEL_TABLE_MIN
        while capacity < 2 * distinct_bound:
            capacity *= 2
        keys = torch.empty(capacity, dtype=torch.int64, device=device)
        vals = torch.empty(capacity, dtype=torch.int32, device=device)
        self.cfx.label_table_clear(keys.data_ptr(), vals.data_ptr(),
                                   capacity)
        return keys, vals, capacity

    def label_count_table(self, t: torch.Tensor):
        """(keys, vals, capacity, bound): the voxel count of every label of
        a contiguous int32/int64 volume, zero included.

        Sizing. In flat (z,y,x) order call voxel i a run start if i == 0 or
        label[i] != label[i-1]. Every distinct label has a first occurrence
        f in that order; either f == 0, or label[f-1] is a different label
        (it occurred earlier, and label[f] had not) — so f is a run start,
        and distinct labels map one-to-one onto some of the run starts.
        Hence #distinct <= #run starts <= n: the table is sized from the run
        starts (one streaming read), which for a real segmentation is about
        surface / x-extent per object rather than one slot per voxel, and
        can never come out too small."""
        dims, eb = tuple(t.shape), t.element_size()
        bound = self.cfx.label_run_starts(t.data_ptr(), eb, dims)
        keys, vals, capacity = self._new_label_table(bound, t.device)
        self.cfx.label_count(t.data_ptr(), eb, dims, keys.data_ptr(),
                             vals.data_ptr(), capacity)
        return keys, vals, capacity, bound

    def label_unique_counts(self, t: torch.Tensor):
        """(ids, counts): ids in t's dtype ascending by UNSIGNED value,
        counts int64 — np.unique(return_counts=True) on the uint view."""
        t = self._check_labels(t, 'label_unique_counts')
        keys, vals, _, _ = self.label_count_table(t)
        used = keys != -1
        ids, counts = keys[used], vals[used]
        # the table is small: ordering it is torch plumbing. Flipping the
        # sign bit turns signed order into unsigned order.
        order = torch.argsort(torch.bitwise_xor(ids, -2 ** 63))
        return (ids[order].to(t.dtype),
                counts[order].to(torch.int64) & 0xFFFFFFFF)

    def label_pair_table(self, seg: torch.Tensor, gt: torch.Tensor,
                         capacity: int = None):
        """(seg_keys, gt_keys, keys, vals, info): the contingency table of
        two contiguous int32/int64 volumes of equal shape. Each volume is
        counted into a table of its own; a key of the pair table is
        (slot in seg_keys << 32) | slot in gt_keys and its value the number
        of voxels that carry that pair. `info` records the bounds and
        capacities of the three tables.

        Sizing. Call voxel i a pair run start if i == 0 or (seg[i], gt[i])
        != (seg[i-1], gt[i-1]). The pair differs from its predecessor only
        if seg or gt does, so every pair run start but voxel 0 is a run
        start of seg or of gt, and voxel 0 is one of both:
            pair run starts <= run_starts(seg) + run_starts(gt) - 1.
        By the first-occurrence argument of label_count_table, applied to
        the pairs as labels, distinct pairs <= pair run starts (and <= n).
        The pair table is sized from that sum — both terms are already
        known from sizing the single tables — and can never come out too
        small. `capacity` overrides the sizing (a power of two; a table
        that is too small makes the call raise "label table full")."""
        if seg.shape != gt.shape:
            raise ValueError(f'label_pair_table: shapes differ: '
                             f'{tuple(seg.shape)} and {tuple(gt.shape)}')
        dims = tuple(seg.shape)
        seg_keys, _, seg_cap, seg_bound = self.label_count_table(seg)
        gt_keys, _, gt_cap, gt_bound = self.label_count_table(gt)
        bound = min(seg_bound + gt_bound - 1, seg.numel())
        if capacity is None:
            keys, vals, capacity = self._new_label_table(bound, seg.device)
        else:
            keys = torch.empty(capacity, dtype=torch.int64,
                               device=seg.device)
            vals = torch.empty(capacity, dtype=torch.int32,
                               device=seg.device)
            self.cfx.label_table_clear(keys.data_ptr(), vals.data_ptr(),
                                       capacity)
        self.cfx.label_pair_count(
            seg.data_ptr(), seg.element_size(), dims, seg_keys.data_ptr(),
            seg_cap, gt.data_ptr(), gt.element_size(), dims,
            gt_keys.data_ptr(), gt_cap, keys.data_ptr(), vals.data_ptr(),
            capacity)
        info = {'seg_bound': seg_bound, 'seg_capacity': seg_cap,
                'gt_bound': gt_bound, 'gt_capacity': gt_cap,
                'pair_bound': bound, 'pair_capacity': capacity}
        return seg_keys, gt_keys, keys, vals, info

    def label_contingency(self, seg: torch.Tensor, gt: torch.Tensor):
        """(seg_ids, gt_ids, counts), one row per distinct (seg, gt) pair,
        sorted lexicographically by UNSIGNED (seg, gt). Ids are int64
        carrying uint64 (32-bit labels zero-extended), counts int64."""
        seg = self._check_labels(seg, 'label_contingency')
        gt = self._check_labels(gt, 'label_contingency')
        seg_keys, gt_keys, keys, vals, _ = self.label_pair_table(seg, gt)
        used = keys != -1
        pair, counts = keys[used], vals[used]
        seg_ids = seg_keys[pair >> 32]
        gt_ids = gt_keys[pair & 0xFFFFFFFF]
        # the table is small: ordering it is torch plumbing. Two stable
        # sorts, minor key first; the sign-bit flip gives unsigned order.
        order = torch.argsort(torch.bitwise_xor(gt_ids, -2 ** 63),
                              stable=True)
        order = order[torch.argsort(
            torch.bitwise_xor(seg_ids[order], -2 ** 63), stable=True)]
        return (seg_ids[order], gt_ids[order],
                counts[order].to(torch.int64) & 0xFFFFFFFF)

    def label_mask_fragments(self, t: torch.Tensor,
                             voxel_num_threshold: int) -> torch.Tensor:
        t = self._check_labels(t, 'label_mask_fragments')
        keys, vals, capacity, _ = self.label_count_table(t)
        out = torch.empty_like(t)
        self.cfx.label_mask(t.data_ptr(), out.data_ptr(), t.element_size(),
                            tuple(t.shape), keys.data_ptr(), vals.data_ptr(),
                            capacity, 0, int(voxel_num_threshold))
        return out

    def label_mask_except(self, t: torch.Tensor, ids) -> torch.Tensor:
        """ids: distinct Python ints within the unsigned range of the
        carried dtype (segmentation.valid_ids)."""
        t = self._check_labels(t, 'label_mask_except')
        keys, vals, capacity = self._new_label_table(len(ids), t.device)
        if len(ids):
            ids_dev = torch.from_numpy(
                np.array(ids, dtype=np.uint64).view(np.int64)).to(t.device)
            self.cfx.label_table_insert(ids_dev.data_ptr(), len(ids), 1,
                                        keys.data_ptr(), vals.data_ptr(),
                                        capacity)
        out = torch.empty_like(t)
        self.cfx.label_mask(t.data_ptr(), out.data_ptr(), t.element_size(),
                            tuple(t.shape), keys.data_ptr(), vals.data_ptr(),
                            capacity, 1, 0)
        return out

    # --- affinity maps to segments (csrc/watershed.hip) ----------------------
    @staticmethod
    def _check_affinity(t: torch.Tensor, who: str) -> torch.Tensor:
        """The map as a contiguous f32 tensor: f16 / bf16 widen exactly."""
        if t.ndim != 4 or t.shape[0] != 3:
            raise ValueError(f'{who}: affinity map must be (3, Z, Y, X), '
                             f'but got shape {tuple(t.shape)}')
        if t.numel() == 0:
            raise ValueError(f'{who}: empty affinity map')
        return t.to(torch.float32).contiguous()

    def affinity_fragments(self, aff: torch.Tensor, low: float,
                           high: float):
        """(labels, n): watershed fragments of a (3, Z, Y, X) map as an
        int32 tensor carrying uint32 labels 1..n, 0 background."""
        aff = self._check_affinity(aff, 'affinity_fragments')
        dims = tuple(aff.shape[1:])
        labels = torch.empty(dims, dtype=torch.int32, device=aff.device)
        scratch = torch.empty(dims, dtype=torch.int32, device=aff.device)
        n = self.cfx.affinity_fragments(aff.data_ptr(), dims, float(low),
                                        float(high), labels.data_ptr(),
                                        scratch.data_ptr())
        return labels, n

    def region_graph_table(self, frag: torch.Tensor, aff: torch.Tensor,
                           capacity: int = None):
        """(keys, counts, sums, info): the region graph of an int32 fragment
        volume as a table, key (a << 32) | b for a < b. The table is sized
        from the number of table operations the kernel will make (a first
        pass over the fragments alone): every distinct key is sent at least
        once, so the rows cannot outnumber the operations. `capacity`
        overrides the sizing (a power of two; too small raises "label
        table full")."""
        aff = self._check_affinity(aff, 'region_graph')
        if frag.dtype != torch.int32:
            raise TypeError(f'region_graph: device fragments must be int32 '
                            f'(carrying uint32), but got: {frag.dtype}')
        if tuple(frag.shape) != tuple(aff.shape[1:]):
            raise ValueError(f'region_graph: fragments {tuple(frag.shape)} '
                             f'and affinity map {tuple(aff.shape)} differ '
                             f'in shape')
        frag = frag.contiguous()
        dims = tuple(frag.shape)
        bound = None
        if capacity is None:
            bound = self.cfx.region_graph_runs(frag.data_ptr(), dims)
            capacity = self.LABEL_TABLE_MIN
            while capacity < 2 * bound:
                capacity *= 2
        keys = torch.empty(capacity, dtype=torch.int64, device=frag.device)
        counts = torch.empty(capacity, dtype=torch.int32, device=frag.device)
        sums = torch.empty(capacity, dtype=torch.int64, device=frag.device)
        self.cfx.region_graph(frag.data_ptr(), aff.data_ptr(), dims,
                              keys.data_ptr(), counts.data_ptr(),
                              sums.data_ptr(), capacity)
        return keys, counts, sums, {'bound': bound, 'capacity': capacity}

    def region_graph(self, frag: torch.Tensor, aff: torch.Tensor):
        """(a, b, count, sum) int64 tensors, one row per pair of touching
        fragments a < b, sorted by (a, b)."""
        keys, counts, sums, _ = self.region_graph_table(frag, aff)
        used = keys != -1
        keys, counts, sums = keys[used], counts[used], sums[used]
        # a < 2^32-1, so a key's sign bit is a's top bit: flipping it turns
        # signed order into unsigned order
        order = torch.argsort(torch.bitwise_xor(keys, -2 ** 63))
        keys = keys[order]
        return ((keys >> 32) & 0xFFFFFFFF, keys & 0xFFFFFFFF,
                counts[order].to(torch.int64) & 0xFFFFFFFF, sums[order])


_SHARED = {}


def shared_hip_ops(device_index: int = 0) -> HipOps:
    """The one HipOps (context, scratch, profile counters) per device that
    the operator modules share (segmentation, downsample, watershed)."""
    if device_index not in _SHARED:
        _SHARED[device_index] = HipOps(device_index)
    return _SHARED[device_index]


class TorchOps:
    is_hip = False

    def __init__(self, device_index: int = 0):
        self.device = 'cpu'

    def sync(self):
        pass

    def cast_div(self, u8, divisor):
        return u8.to(torch.float32) / divisor

    def normalize_intensity(self, u8):
        return u8.to(torch.float32) / 127.5 - 1.0

    def extract(self, chunk_f32, starts, patch_size, out_batch):
        pz, py, px = patch_size
        for i, (z0, y0, x0) in enumerate(starts):
            src = chunk_f32[..., z0:z0 + pz, y0:y0 + py, x0:x0 + px]
            out_batch[i] = src if src.ndim == 4 else src.unsqueeze(0)

    def blend(self, out, patch_batch, batch_index, offset, mask=None):
        patch = patch_batch[batch_index]
        if mask is not None:
            patch = patch * mask
        pdims = patch.shape[-3:]
        odims = out.shape[-3:]
        dst, src = [], []
        for off, p, h in zip(offset, pdims, odims):
            lo, hi = max(off, 0), min(off + p, h)
            if hi <= lo:
                return
            dst.append(slice(lo, hi))
            src.append(slice(lo - off, hi - off))
        out[..., dst[0], dst[1], dst[2]] += patch[..., src[0], src[1],
                                                  src[2]]

    def blend_batch(self, out, patch_batch, items, mask=None):
        # CPU plumbing: sequential (order already preserved by grouping)
        for b, oz, oy, ox in items:
            self.blend(out, patch_batch, int(b), (int(oz), int(oy), int(ox)),
                       mask=mask)

    def build_chunk_mask(self, out_dims, patch_mask, offsets, groups=None):
        mask = torch.zeros(tuple(out_dims), dtype=torch.float32)
        pm = patch_mask.unsqueeze(0)  # (1,pz,py,px): one 3-D "patch"
        for off in offsets:
            self.blend(mask, pm, 0, tuple(int(v) for v in off))
        return 1.0 / mask

    def multiply_mask(self, out, mask):
        out *= mask

    def multiply_mask_max(self, out, mask):
        out *= mask
        return out.max().item()

    def max(self, t):
        return t.max().item()

    def crop_margin(self, t, margins):
        d, h, w = t.shape[-3:]
        return t[..., margins[0]:d - margins[3], margins[1]:h - margins[4],
                 margins[2]:w - margins[5]].contiguous()

    def mask_using_last_channel(self, t, threshold):
        keep = t[-1] < threshold
        return t[:-1] * keep

    # CPU plumbing: the host numpy path on the tensor's memory
    def downsample_average(self, t, factor):
        from .downsample import average_host
        if t.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f'downsample_average: uint8 or float32 only, '
                            f'but got: {t.dtype}')
        out = average_host(t.contiguous().numpy(), factor)
        return torch.from_numpy(np.ascontiguousarray(out))

    def downsample_mode(self, t, factor):
        from .downsample import mode_host
        if t.is_floating_point() or t.dtype == torch.bool:
            raise TypeError(f'downsample_mode: integer labels only, '
                            f'but got: {t.dtype}')
        out = mode_host(t.contiguous().numpy(), factor)
        return torch.from_numpy(np.ascontiguousarray(out))
