"""The profile ledger: every timed C-ABI entry, called once at a tiny shape,
pushes the rows it always pushed -- its kernel id, its number of rows and its
work figure (`bytes`: algorithmic bytes, or FLOPs for the convs). The
expected figures are literals worked out by hand from the formula quoted
beside each call; `total_ms` is a measurement and is not pinned. Every entry
is preceded by a reset, and the kernels it must not touch have to read zero.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from chunkflow_amd.hip import KERNEL_IDS, CfxContext

pytestmark = pytest.mark.gpu

DIMS = (3, 9, 17)          # the odd volume of the exact tests
NV = 459                   # 3 * 9 * 17 voxels
PATCH = (2, 3, 5)          # 30 voxels
CAP = 64                   # table slots: a power of two, > 2 x the labels


def check(ctx, name, call, expected):
    """reset, run `call` once, compare every kernel's (count, work)"""
    ctx.profile_reset()
    call()
    for kernel in KERNEL_IDS:
        got = ctx.profile_get(kernel)
        want = expected.get(kernel, (0, 0.0))
        assert (got['count'], got['bytes']) == want, (name, kernel, got)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_stream_and_segmentation_entries():
    ctx = CfxContext(0)
    ctx.adopt_torch_stream()
    rng = np.random.default_rng(7)
    u8 = dev(rng.integers(0, 256, DIMS, dtype=np.uint8))
    f1 = torch.empty(DIMS, dtype=torch.float32, device='cuda')
    pos = dev(rng.uniform(0.5, 2.0, DIMS).astype(np.float32))
    c2 = dev(rng.uniform(0.0, 1.0, (2,) + DIMS).astype(np.float32))
    c3 = dev(rng.uniform(0.0, 1.0, (3,) + DIMS).astype(np.float32))
    out2 = torch.zeros((2,) + DIMS, dtype=torch.float32, device='cuda')
    patches = dev(rng.uniform(0.0, 1.0, (2, 2) + PATCH).astype(np.float32))
    pmask = dev(rng.uniform(0.5, 1.0, PATCH).astype(np.float32))
    # 65 windows of PATCH inside DIMS: two launches (64 + 1)
    i = np.arange(65)
    starts = np.stack([i % 2, i % 7, i % 13], axis=1)
    gathered = torch.empty((65, 1) + PATCH, dtype=torch.float32,
                           device='cuda')
    cropped = torch.empty((2, 2, 6, 12), dtype=torch.float32, device='cuda')

    seg = dev(rng.integers(0, 6, DIMS, dtype=np.int32))
    gt = dev(rng.integers(0, 4, DIMS, dtype=np.int64))
    gt_ids = dev(np.arange(4, dtype=np.int64))
    fg = (seg > 2).to(torch.uint8)
    aff = dev(rng.uniform(0.0, 1.0, (3,) + DIMS).astype(np.float32))
    labels = torch.empty(DIMS, dtype=torch.int32, device='cuda')
    scratch = torch.empty(DIMS, dtype=torch.int32, device='cuda')
    seg_out = torch.empty_like(seg)

    def table():
        keys = torch.empty(CAP, dtype=torch.int64, device='cuda')
        vals = torch.empty(CAP, dtype=torch.int32, device='cuda')
        ctx.label_table_clear(keys.data_ptr(), vals.data_ptr(), CAP)
        return keys, vals

    seg_keys, seg_vals = table()
    gt_keys, gt_vals = table()
    pair_keys, pair_vals = table()
    rg_keys, rg_counts = table()
    rg_sums = torch.empty(CAP, dtype=torch.int64, device='cuda')
    # the gt table needs its keys only: inserting them is untimed
    ctx.label_table_insert(gt_ids.data_ptr(), 4, 1, gt_keys.data_ptr(),
                           gt_vals.data_ptr(), CAP)

    p = torch.Tensor.data_ptr
    entries = [
        # 1 B read + 4 B written per voxel: 459 * 5
        ('normalize_intensity',
         lambda: ctx.normalize_intensity(p(u8), p(f1), NV),
         {'normalize': (1, 2295.0)}),
        ('cast_u8_f32_div',
         lambda: ctx.cast_u8_f32_div(p(u8), p(f1), NV, 255.0),
         {'cast': (1, 2295.0)}),
        # one row per launch of <= 64 patches, n * C * 30 * 8 each:
        # 64 * 240 + 1 * 240
        ('extract_patches',
         lambda: ctx.extract_patches(p(pos), 1, DIMS, starts, PATCH,
                                     p(gathered)),
         {'extract': (2, 15600.0)}),
        # unclipped 30-voxel region, C = 2, masked: 30 * 2 * 12 + 30 * 4
        ('blend_accumulate',
         lambda: ctx.blend_accumulate(p(out2), 2, DIMS, p(patches), PATCH,
                                      (1, 2, 3), p(pmask)),
         {'blend': (1, 840.0)}),
        # two disjoint items in one launch, no mask: (0, 0, 0) keeps its 30
        # voxels, (2, 7, 14) is clipped to 1 * 2 * 3 = 6: (30 + 6) * 2 * 12
        ('blend_batch',
         lambda: ctx.blend_batch(p(out2), 2, DIMS, p(patches), PATCH,
                                 [(0, 0, 0, 0), (1, 2, 7, 14)]),
         {'blend': (1, 864.0)}),
        # read + write f32: 459 * 8
        ('reciprocal', lambda: ctx.reciprocal(p(pos), NV),
         {'reciprocal': (1, 3672.0)}),
        # two one-channel unmasked blends of 30 voxels (30 * 12 each), then
        # the reciprocal of the whole mask
        ('build_chunk_mask',
         lambda: ctx.build_chunk_mask(p(f1), DIMS, p(pmask), PATCH,
                                      [(0, 0, 0), (1, 6, 12)]),
         {'blend': (2, 720.0), 'reciprocal': (1, 3672.0)}),
        # n * (C * 8 + 4) = 459 * 20
        ('multiply_mask', lambda: ctx.multiply_mask(p(c2), p(pos), 2, NV),
         {'maskmul': (1, 9180.0)}),
        # 459 % 4 != 0: no fused max, the plain multiply's single row
        ('multiply_mask_max',
         lambda: ctx.multiply_mask_max(p(c2), p(pos), 2, NV),
         {'maskmul': (1, 9180.0)}),
        ('max', lambda: ctx.max(p(pos), NV), {'max': (1, 1836.0)}),
        # margins (0, 1, 2 | 1, 2, 3): 2 x 6 x 12 voxels, C = 2, 8 B each
        ('crop_margin',
         lambda: ctx.crop_margin(p(c2), p(cropped), 2, DIMS,
                                 (0, 1, 2, 1, 2, 3)),
         {'crop': (1, 2304.0)}),
        # 3 channels read, 2 written: 459 * 5 * 4
        ('mask_using_last_channel',
         lambda: ctx.mask_using_last_channel(p(c3), p(out2), 3, DIMS, 0.5),
         {'myelin': (1, 9180.0)}),
        # n * (3 * elem_bytes + 24): u8 459 * 27, u32 459 * 36
        ('connected_components',
         lambda: ctx.connected_components(p(fg), DIMS, 6, p(labels),
                                          p(scratch)),
         {'cc': (1, 12393.0)}),
        ('connected_components_labels',
         lambda: ctx.connected_components_labels(p(seg), 4, DIMS, 26,
                                                 p(labels), p(scratch)),
         {'cc': (1, 16524.0)}),
        # n * (12 + 8 + 24)
        ('affinity_fragments',
         lambda: ctx.affinity_fragments(p(aff), DIMS, 0.3, 0.8, p(labels),
                                        p(scratch)),
         {'cc': (1, 20196.0)}),
        # n * elem_bytes
        ('label_run_starts',
         lambda: ctx.label_run_starts(p(seg), 4, DIMS),
         {'labels': (1, 1836.0)}),
        ('label_count',
         lambda: ctx.label_count(p(seg), 4, DIMS, p(seg_keys), p(seg_vals),
                                 CAP),
         {'labels': (1, 1836.0)}),
        # n * (4 + 8); after label_count: the seg table is filled
        ('label_pair_count',
         lambda: ctx.label_pair_count(p(seg), 4, DIMS, p(seg_keys), CAP,
                                      p(gt), 8, DIMS, p(gt_keys), CAP,
                                      p(pair_keys), p(pair_vals), CAP),
         {'labels': (1, 5508.0)}),
        # read + write: 2 * n * 4
        ('label_mask',
         lambda: ctx.label_mask(p(seg), p(seg_out), 4, DIMS, p(seg_keys),
                                p(seg_vals), CAP, 0, 10),
         {'labels': (1, 3672.0)}),
        # 4 * n, both
        ('region_graph_runs',
         lambda: ctx.region_graph_runs(p(seg), DIMS),
         {'labels': (1, 1836.0)}),
        ('region_graph',
         lambda: ctx.region_graph(p(seg), p(aff), DIMS, p(rg_keys),
                                  p(rg_counts), p(rg_sums), CAP),
         {'labels': (1, 1836.0)}),
    ]
    ctx.profile_enable(True)
    try:
        for name, call, expected in entries:
            check(ctx, name, call, expected)
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
        ctx.close()


def test_conv_entries():
    from chunkflow_amd.fastconv import (CfxConv3dBF16, CfxConvIn155,
                                        CfxConvOut155, CfxDownConv3d,
                                        CfxUpConv3d, get_cfx)
    ctx = get_cfx(0)
    torch.manual_seed(7)
    cl = torch.channels_last_3d

    def vol(c, dims=DIMS, dtype=torch.float32):
        return torch.randn((1, c) + dims, device='cuda').to(dtype) \
            .contiguous(memory_format=cl)

    def conv3(c, **route):
        x, out = vol(c), vol(c)
        wtap = torch.randn(27, c, c, device='cuda')
        bias = torch.randn(c, device='cuda')
        return lambda: ctx.conv3_ndhwc(
            x.data_ptr(), wtap.data_ptr(), bias.data_ptr(), None,
            out.data_ptr(), 1, *DIMS, c, c, do_elu=True, **route)

    def module(m, *inputs):
        m = m.cuda()
        return lambda: m(*inputs)

    up = nn.ConvTranspose3d(36, 28, (1, 2, 2), (1, 2, 2))
    skip = vol(28, (3, 18, 34))
    entries = [
        # 2 * 27 * C * K * voxels: 42336 * 459 at 28, 69984 * 459 at 36
        ('conv3_ndhwc', conv3(28), {'conv': (1, 19432224.0)}),
        ('conv3_ndhwc_w32', conv3(28, w32=True), {'conv': (1, 19432224.0)}),
        ('conv3_ndhwc_zring', conv3(28, zring=True),
         {'conv': (1, 19432224.0)}),
        # two launches, one row
        ('conv3_ndhwc_zring 36', conv3(36, zring=True),
         {'conv': (1, 32122656.0)}),
        ('conv3_ndhwc_bf16',
         module(CfxConv3dBF16(nn.Conv3d(28, 28, 3, padding=1)),
                vol(28, dtype=torch.bfloat16)),
         {'conv': (1, 19432224.0)}),
        # the sliced schedule: four launches, one row
        ('conv3_ndhwc_bf16 36',
         module(CfxConv3dBF16(nn.Conv3d(36, 36, 3, padding=1)),
                vol(36, dtype=torch.bfloat16)),
         {'conv': (1, 32122656.0)}),
        # 2 * 25 * K * voxels = 1400 * 459
        ('conv155_c1',
         module(CfxConvIn155(nn.Conv3d(1, 28, (1, 5, 5), padding=(0, 2, 2))),
                vol(1)),
         {'conv_stream': (1, 642600.0)}),
        # 2 * 25 * 28 * 3 * voxels = 4200 * 459
        ('conv155_out',
         module(CfxConvOut155(nn.Conv3d(28, 3, (1, 5, 5),
                                        padding=(0, 2, 2))), vol(28)),
         {'conv_stream': (1, 1927800.0)}),
        # 2 * 4 * C * K * input voxels: MFMA route 8064 * 459, with and
        # without the skip; K = 30 takes the VALU kernel, 8640 * 459
        ('upconv_2x2 mfma', module(CfxUpConv3d(up), vol(36)),
         {'conv_stream': (1, 3701376.0)}),
        ('upconv_2x2_add', module(CfxUpConv3d(up), vol(36), skip),
         {'conv_stream': (1, 3701376.0)}),
        ('upconv_2x2 valu',
         module(CfxUpConv3d(nn.ConvTranspose3d(36, 30, (1, 2, 2),
                                               (1, 2, 2))), vol(36)),
         {'conv_stream': (1, 3965760.0)}),
        # 3 x 8 x 16 in, 2 * 4 * 28 * 36 * (3 * 4 * 8) output voxels
        ('downconv_2x2',
         module(CfxDownConv3d(nn.Conv3d(28, 36, (1, 2, 2), (1, 2, 2))),
                vol(28, (3, 8, 16))),
         {'conv_stream': (1, 774144.0)}),
    ]
    ctx.profile_enable(True)
    try:
        for name, call, expected in entries:
            check(ctx, name, call, expected)
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
