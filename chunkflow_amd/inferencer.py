"""The MI355X-native Inferencer: overlapping-patch tiler, convnet forward,
bump-weighted blend, chunk-mask normalize.

Drop-in behavioral mirror of the reference Inferencer
(chunkflow/flow/divid_conquer/inferencer.py:36-479) redesigned device-first:

  * the input chunk is uploaded ONCE; everything downstream — int->f32
    normalize, patch extraction, convnet forward, bump-weighted blend
    accumulate (patch-mask multiply fused), chunk-mask build + reciprocal,
    mask-normalize, the <1.0001 sanity scan, the optional myelin mask —
    stays resident in HBM and runs as hand-written gfx950 kernels
    (chunkflow_amd/csrc/cfx.hip) stream-ordered with the torch conv forward.
    The reference instead round-trips every patch D2H (pytorch.py:115-118).
  * accumulation is ALWAYS f32 (the reference's f16 chunk-mask reciprocal
    overflows to inf and crashes in masked mode — SURVEY.md A.1); --dtype
    float16 casts only the final output.
  * tail batches are sized exactly (the reference computes stale buffer rows
    and drops them — SURVEY.md A.3; outputs identical).

Geometry, patch ordering, tail clamping, duplicate-position double-blending,
the chunk mask rebuild per input chunk, and the all-zero shortcut all follow
the reference line-for-line semantics (citations inline).
"""
import os

import numpy as np
import torch

from .cartesian import Cartesian, to_cartesian
from .chunk import Chunk
from .engines import create_engine
from .grouping import disjoint_groups
from .ops import HipOps, TorchOps
from .patch_mask import make_patch_mask
from .transform import TransformSequences

def _blend_reforder() -> bool:
    """Dispute-resolution switch: blend one patch per launch in the
    reference's exact order; default is the
    disjoint-group batching whose reordering is bounded by the ulp
    argument in grouping.py. Covers the chunk-mask build as well as the
    output blend, so the result is the oracle's bit for bit
    (tests/test_stitch_exact.py). Read per call so tests can toggle it."""
    return os.environ.get('CFX_BLEND_REFORDER', '0') == '1'


class Inferencer:
    def __init__(self,
                 convnet_model,
                 convnet_weight_path,
                 input_patch_size,
                 output_patch_size=None,
                 patch_num=None,
                 num_input_channels: int = 1,
                 num_output_channels: int = 3,
                 output_patch_overlap=None,
                 output_crop_margin=None,
                 dtype='float32',
                 framework: str = 'universal',
                 batch_size: int = 1,
                 bump: str = 'wu',
                 input_size=None,
                 mask_output_chunk: bool = True,
                 mask_myelin_threshold=None,
                 augment: bool = False,
                 dry_run: bool = False,
                 compute_device: str = None,
                 patch_shard: tuple = None,
                 pre_normalize_hook=None):
        """patch_shard=(rank, world): intra-chunk multi-GPU (SURVEY.md §8f
        row 4) — this rank blends only patches with index % world == rank
        into its own zero buffer; pre_normalize_hook(output_tensor) runs
        before the mask normalize (dispatch.py installs an all-reduce SUM
        there, which reconstitutes the full blend: the blend is a sum over
        patches, so sharding + summing is the same accumulation up to f32
        reordering)."""
        assert input_size is None or patch_num is None
        input_patch_size = to_cartesian(input_patch_size)
        output_patch_size = to_cartesian(output_patch_size)
        patch_num = to_cartesian(patch_num)
        input_size = to_cartesian(input_size)
        output_patch_overlap = to_cartesian(output_patch_overlap)
        output_crop_margin = to_cartesian(output_crop_margin)

        # geometry defaults (reference inferencer.py:85-122)
        if output_patch_size is None:
            output_patch_size = input_patch_size
        if output_patch_overlap is None:
            output_patch_overlap = output_patch_size // 2
        self.input_patch_size = input_patch_size
        self.output_patch_size = output_patch_size
        self.output_patch_overlap = output_patch_overlap
        self.patch_num = patch_num
        self.batch_size = batch_size
        self.input_size = input_size

        if output_crop_margin is None:
            self.output_crop_margin = (Cartesian(0, 0, 0) if mask_output_chunk
                                       else output_patch_overlap)
        else:
            self.output_crop_margin = output_crop_margin
            assert self.output_crop_margin >= self.output_patch_overlap
        self.output_patch_crop_margin = \
            (input_patch_size - output_patch_size) // 2
        if self.output_patch_crop_margin != Cartesian(0, 0, 0):
            raise NotImplementedError(
                'differing input/output patch sizes: the reference skips its '
                'own test for this mode as known-buggy '
                '(test_inferencer.py:98-139); not supported')
        self.output_offset = self.output_crop_margin
        self.output_patch_stride = output_patch_size - output_patch_overlap
        self.input_patch_overlap = \
            self.output_patch_crop_margin * 2 + output_patch_overlap
        self.input_patch_stride = input_patch_size - self.input_patch_overlap

        # aligned mode needs a pre-declared size (reference :124-139)
        if not mask_output_chunk:
            assert (input_size is not None) or (patch_num is not None)
            if patch_num is None:
                self.patch_num = Cartesian(*(
                    (isz - o) // s for isz, o, s in
                    zip(input_size, self.input_patch_overlap,
                        self.input_patch_stride)))
            if self.input_size is None:
                self.input_size = (self.input_patch_stride * self.patch_num
                                   + self.input_patch_overlap)

        self.num_input_channels = num_input_channels
        self.num_output_channels = num_output_channels
        self.mask_output_chunk = mask_output_chunk
        self.dtype = dtype
        self.mask_myelin_threshold = mask_myelin_threshold
        self.dry_run = dry_run

        # device selection: cuda when visible (HIP path, loud failure when
        # the extension is missing); TorchOps only on GPU-less machines
        if compute_device is None:
            compute_device = 'cuda' if torch.cuda.is_available() else 'cpu'
        if compute_device.startswith('cuda'):
            index = int(compute_device.split(':')[1]) \
                if ':' in compute_device else 0
            self.ops = HipOps(index)  # raises CfxError if .so missing
            self.device = f'cuda:{index}'
        else:
            if torch.cuda.is_available():
                raise RuntimeError(
                    'refusing the CPU plumbing path on a machine with a GPU '
                    '(no silent fallback); pass compute_device="cuda"')
            self.ops = TorchOps()
            self.device = 'cpu'

        self.patch_mask_np = make_patch_mask(
            tuple(output_patch_size), tuple(output_patch_overlap))
        if not dry_run:
            self.engine = create_engine(
                framework, convnet_model, convnet_weight_path,
                input_patch_size, output_patch_size, output_patch_overlap,
                num_input_channels, num_output_channels, self.patch_mask_np,
                self.device, dtype=dtype, bump=bump)
        else:
            self.engine = None
        self.transform_sequences = TransformSequences() if augment else None
        self._batch_buffers = {}
        self._group_cache = {}
        self.patch_shard = patch_shard
        self.pre_normalize_hook = pre_normalize_hook

    # ------------------------------------------------------------------
    @property
    def compute_device(self):
        if self.engine is None:
            return self.device
        return self.engine.compute_device

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return None

    # ------------------------------------------------------------------
    def _check_alignment(self, input_size):
        # reference inferencer.py:243-253
        for i, s, o in zip(input_size, self.input_patch_stride,
                           self.input_patch_overlap):
            assert (i - o) % s == 0, \
                f'patches do not align with the chunk: {input_size}'

    def _patch_starts(self, input_size):
        """Tail-clamped patch start grid (reference inferencer.py:255-292,
        chunk-local coordinates; duplicates preserved)."""
        starts = []
        for dim in range(3):
            axis = []
            size = input_size[dim]
            patch = self.input_patch_size[dim]
            stride = self.input_patch_stride[dim]
            overlap = self.input_patch_overlap[dim]
            for i in range(0, size - overlap, stride):
                if i + patch > size:
                    i = size - patch
                    assert i >= 0
                axis.append(i)
            starts.append(axis)
        out = []
        for z in starts[0]:
            for y in starts[1]:
                for x in starts[2]:
                    out.append((z, y, x))
        return np.array(out, dtype=np.int32)

    def _groups(self, out_starts: np.ndarray, out_size3):
        """Disjoint order-preserving launch groups (grouping.py) for a set
        of output-local patch starts; pure geometry, cached per start set."""
        key = (out_starts.tobytes(), tuple(out_size3))
        if key not in self._group_cache:
            self._group_cache[key] = disjoint_groups(
                out_starts, tuple(self.output_patch_size), out_size3)
        return self._group_cache[key]

    def _get_batch_buffer(self, n):
        key = n
        if key not in self._batch_buffers:
            self._batch_buffers[key] = torch.empty(
                (n, self.num_input_channels, *self.input_patch_size),
                dtype=torch.float32, device=self.device)
        return self._batch_buffers[key]

    # ------------------------------------------------------------------
    def __call__(self, input_chunk: Chunk) -> Chunk:
        assert isinstance(input_chunk, Chunk)
        input_size = input_chunk.shape[-3:]
        if not self.mask_output_chunk:
            self._check_alignment(input_size)

        out_size3 = tuple(i - 2 * o for i, o in
                          zip(input_size, self.output_offset))
        out_offset = input_chunk.voxel_offset + self.output_offset
        out_shape = (self.num_output_channels,) + out_size3

        if self.dry_run:
            # reference inferencer.py:372-385
            shape = out_shape
            if self.mask_myelin_threshold:
                shape = (shape[0] - 1,) + shape[1:]
            return Chunk.create(size=shape, dtype=self.dtype,
                                voxel_offset=out_offset,
                                voxel_size=input_chunk.voxel_size)

        # move the chunk into HBM once (H2D boundary)
        if self.ops.is_hip:
            chunk = input_chunk.to_device(self.device)
        else:
            chunk = input_chunk
        t = chunk.array if isinstance(chunk.array, torch.Tensor) \
            else torch.from_numpy(np.ascontiguousarray(chunk.array))
        t = t.contiguous()

        # all-zero shortcut (reference inferencer.py:387-393)
        output = torch.zeros(out_shape, dtype=torch.float32,
                             device=self.device)
        if not bool((t != 0).any().item()):
            if self.mask_myelin_threshold:
                output = output[:-1]
            out = Chunk(output, voxel_offset=out_offset,
                        voxel_size=input_chunk.voxel_size)
            return out.astype(self.dtype) if self.dtype != 'float32' else out

        # int -> f32 normalize to [0, 1] (reference inferencer.py:395-399)
        if t.dtype == torch.uint8:
            f32 = self.ops.cast_div(t, 255.0)
        elif t.dtype in (torch.int16, torch.int32, torch.int64):
            info = torch.iinfo(t.dtype)
            f32 = t.to(torch.float32) / info.max
        else:
            f32 = t.to(torch.float32)

        in_starts = self._patch_starts(input_size)
        # output-local patch starts: out_global - out_offset
        # = in_local + chunk_offset + crop_margin(0) - chunk_offset - output_offset
        out_starts = in_starts - np.asarray(self.output_offset,
                                            dtype=np.int32)

        patch_mask_t = self.engine.patch_mask
        recip_mask = None
        if self.mask_output_chunk:
            # mask VALUES rebuilt per input chunk, like the reference
            # (:294-333); the launch grouping is cached geometry. In
            # reference-order mode the mask sum keeps the reference's order
            # too (one launch per offset): a grouped mask differs in the
            # last bit wherever three or more patches meet
            recip_mask = self.ops.build_chunk_mask(
                out_size3, patch_mask_t, out_starts,
                groups=None if _blend_reforder()
                else self._groups(out_starts, out_size3))

        if self.patch_shard is not None:
            shard_rank, shard_world = self.patch_shard
            keep = np.arange(in_starts.shape[0]) % shard_world == shard_rank
            in_starts = in_starts[keep]
            out_starts = out_starts[keep]
        n = in_starts.shape[0]
        fuse_mask = patch_mask_t if not self.engine.pre_masked else None
        for i in range(0, n, self.batch_size):
            bs = min(self.batch_size, n - i)
            batch = self._get_batch_buffer(bs)
            self.ops.extract(f32, in_starts[i:i + bs],
                             tuple(self.input_patch_size), batch)
            if self.transform_sequences is None:
                out_patch = self.engine(batch)
            else:
                variants = self.transform_sequences.forward(batch)
                results = [self.engine(v.contiguous()) for v in variants]
                results = self.transform_sequences.backward(results)
                out_patch = sum(results) / len(results)
                out_patch = out_patch.contiguous()
            bstarts = out_starts[i:i + bs]
            if _blend_reforder():
                # dispute-resolution mode (CFX_BLEND_REFORDER=1): one
                # blend per patch in the reference's exact patch order
                # (inferencer.py:436-455) instead of the disjoint-group
                # batching — bit-reproduces the reference's accumulation
                # order at the cost of ~bs launches per batch
                for bi in range(bs):
                    self.ops.blend(output, out_patch, bi,
                                   tuple(int(v) for v in bstarts[bi]),
                                   mask=fuse_mask)
            else:
                for idx in self._groups(bstarts, out_size3):
                    items = np.concatenate(
                        [idx[:, None].astype(np.int32),
                         bstarts[idx].astype(np.int32)], axis=1)
                    self.ops.blend_batch(output, out_patch, items,
                                         mask=fuse_mask)

        if self.pre_normalize_hook is not None:
            self.pre_normalize_hook(output)

        if self.mask_output_chunk:
            # mask-normalize with the <1.0001 scan fused (:460-466)
            maxv = self.ops.multiply_mask_max(output, recip_mask)
        else:
            maxv = self.ops.max(output)
        if not maxv < 1.0001:
            raise AssertionError(
                f'output buffer should not be greater than 1: max={maxv}')

        if self.mask_myelin_threshold:
            assert output.shape[0] == 4
            output = self.ops.mask_using_last_channel(
                output, self.mask_myelin_threshold)

        out = Chunk(output, voxel_offset=out_offset,
                    voxel_size=input_chunk.voxel_size)
        if self.dtype == 'float16':
            out = out.astype('float16')
        return out
