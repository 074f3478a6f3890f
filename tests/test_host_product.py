"""Product host-side tests (no GPU): Cartesian/BoundingBox grid math, Chunk
data model, product patch mask vs golden CRCs, and the full Inferencer on the
CPU plumbing path (TorchOps — only reachable on GPU-less machines) against
the reference golden fixtures."""
import os
import zlib

import numpy as np
import pytest
import torch

from chunkflow_amd import BoundingBox, BoundingBoxes, Cartesian, Chunk
from chunkflow_amd.patch_mask import make_patch_mask

GPU = torch.cuda.is_available()


def crc(arr):
    return zlib.crc32(np.ascontiguousarray(arr).tobytes())


# --- coordinates -----------------------------------------------------------
def test_cartesian_arithmetic():
    a = Cartesian(1, 2, 3)
    assert a + (1, 1, 1) == Cartesian(2, 3, 4)
    assert a * 2 == Cartesian(2, 4, 6)
    assert Cartesian(20, 256, 256) - Cartesian(4, 64, 64) == \
        Cartesian(16, 192, 192)
    assert Cartesian(10, 10, 10) // 3 == Cartesian(3, 3, 3)
    assert Cartesian(4, 64, 64) <= Cartesian(4, 64, 64)


def test_bbox_roundtrip():
    b = BoundingBox.from_delta((1, 2, 3), (10, 20, 30))
    assert b.shape == Cartesian(10, 20, 30)
    assert BoundingBox.from_string(b.string) == b
    assert b.slices == (slice(1, 11), slice(2, 22), slice(3, 33))


def test_generate_tasks_grid():
    # 8 independent 512^3 chunks (the config-3 shard unit)
    boxes = BoundingBoxes.from_manual_setup(
        (512, 512, 512), roi_size=(512, 1024, 2048))
    assert len(boxes) == 8
    assert boxes[0].start == Cartesian(0, 0, 0)
    assert boxes[-1].start == Cartesian(0, 512, 1536)
    # clamped tail grid: ceil semantics
    boxes = BoundingBoxes.from_manual_setup((64, 64, 64),
                                            roi_size=(100, 64, 64))
    assert len(boxes) == 2
    assert boxes[1].start.z == 64
    # respect_stop clips the tail box
    boxes = BoundingBoxes.from_manual_setup(
        (64, 64, 64), roi_size=(100, 64, 64), respect_chunk_size=False)
    assert boxes[1].shape == Cartesian(36, 64, 64)


# --- chunk data model ------------------------------------------------------
def test_chunk_create_sin_matches_reference(golden):
    meta, arrays = golden
    c = Chunk.create(size=(20, 68, 72), dtype='uint8', pattern='sin')
    np.testing.assert_array_equal(c.array, arrays['sin_20x68x72_u8'])
    assert crc(c.array) == meta['cases']['sin_20x68x72_u8']['crc32']


@pytest.mark.slow
def test_chunk_create_sin_512(golden):
    meta, _ = golden
    c = Chunk.create(size=(512, 512, 512), dtype='uint8', pattern='sin')
    assert crc(c.array) == meta['cases']['sin_512_u8']['crc32']


def test_chunk_cutout_blend_crop():
    arr = np.arange(4 * 5 * 6, dtype=np.float32).reshape(4, 5, 6)
    c = Chunk(arr.copy(), voxel_offset=(10, 20, 30))
    cut = c.cutout((slice(11, 13), slice(21, 24), slice(31, 35)))
    np.testing.assert_array_equal(cut.array, arr[1:3, 1:4, 1:5])
    assert cut.voxel_offset == Cartesian(11, 21, 31)

    out = Chunk(np.zeros((2, 4, 5, 6), dtype=np.float32),
                voxel_offset=(0, 0, 0))
    patch = Chunk(np.ones((2, 3, 3, 3), dtype=np.float32),
                  voxel_offset=(-1, 3, 4))  # clips on three sides
    out.blend(patch)
    assert out.array.sum() == 2 * 2 * 2 * 2
    cropped = c.crop_margin(margin_size=(1, 1, 1))
    np.testing.assert_array_equal(cropped.array, arr[1:-1, 1:-1, 1:-1])
    assert cropped.voxel_offset == Cartesian(11, 21, 31)
    cropped6 = c.crop_margin(margin_size=(1, 0, 0, 2, 1, 3))
    np.testing.assert_array_equal(cropped6.array, arr[1:-2, 0:-1, 0:-3])


def test_chunk_mask_using_last_channel():
    arr = np.random.rand(4, 3, 3, 3).astype(np.float32)
    c = Chunk(arr.copy())
    out = c.mask_using_last_channel(threshold=0.5)
    keep = arr[-1] < 0.5
    np.testing.assert_array_equal(out.array, arr[:3] * keep)


# --- product patch mask ----------------------------------------------------
def test_product_patch_mask_golden(golden):
    meta, arrays = golden
    for name in ('mask_20x256x256_ov4x64x64', 'mask_10x32x32_ov2x8x8'):
        case = meta['cases'][name]
        m = make_patch_mask(tuple(case['patch_size']), tuple(case['overlap']))
        assert crc(m) == case['crc32']


def test_c_abi_patch_mask_bitexact():
    from chunkflow_amd.hip import make_patch_mask_c
    for geom in (((10, 32, 32), (2, 8, 8)), ((20, 128, 128), (4, 32, 32))):
        c = make_patch_mask_c(*geom)
        p = make_patch_mask(*geom)
        np.testing.assert_array_equal(c, p)


# --- full inferencer, CPU plumbing path (GPU-less machines only) -----------
@pytest.mark.skipif(GPU, reason='CPU plumbing path is refused on a GPU box')
class TestInferencerCPU:
    def _run(self, golden, **kw):
        from chunkflow_amd.inferencer import Inferencer
        _, arrays = golden
        chunk = Chunk(arrays['e2e_input_u8'].copy(),
                      voxel_offset=kw.pop('voxel_offset', (0, 0, 0)))
        inf = Inferencer(kw.pop('model', None), kw.pop('weights', None),
                         (10, 32, 32), output_patch_overlap=(2, 8, 8),
                         mask_output_chunk=True, **kw)
        assert not inf.ops.is_hip
        return inf(chunk)

    def test_identity(self, golden):
        _, arrays = golden
        out = self._run(golden, framework='identity', batch_size=3)
        np.testing.assert_allclose(out.numpy().array,
                                   arrays['e2e_identity_out'],
                                   rtol=1e-6, atol=1e-7)

    def test_identity_offset(self, golden):
        _, arrays = golden
        out = self._run(golden, framework='identity', batch_size=4,
                        voxel_offset=(7, 11, 13))
        assert out.voxel_offset == Cartesian(7, 11, 13)
        np.testing.assert_allclose(out.numpy().array,
                                   arrays['e2e_identity_offset_out'],
                                   rtol=1e-6, atol=1e-7)

    def test_identity_myelin(self, golden):
        _, arrays = golden
        out = self._run(golden, framework='identity', batch_size=3,
                        num_output_channels=4, mask_myelin_threshold=0.3)
        np.testing.assert_allclose(out.numpy().array,
                                   arrays['e2e_identity_myelin_out'],
                                   rtol=1e-6, atol=1e-7)

    def test_pytorch_model_file(self, golden, golden_dir):
        _, arrays = golden
        out = self._run(
            golden, framework='pytorch', batch_size=1,
            model=os.path.join(golden_dir, 'ref_model.py'),
            weights=os.path.join(golden_dir, 'ref_model_weights.pt'))
        np.testing.assert_allclose(out.numpy().array,
                                   arrays['e2e_pytorch_out'],
                                   rtol=1e-5, atol=1e-6)

    def test_universal_plugin_contract(self, golden, tmp_path):
        # the reference universal model-file contract:
        # PatchInferencer(weight_path, mask).__call__(ndarray) -> masked ndarray
        plugin = tmp_path / 'universal_identity.py'
        plugin.write_text(
            'import numpy as np\n'
            'class PatchInferencer:\n'
            '    def __init__(self, weight_path, mask):\n'
            '        self.mask = mask\n'
            '    def __call__(self, patch):\n'
            '        out = np.repeat(patch.astype(np.float32), 3, axis=1)\n'
            '        return out * self.mask\n')
        _, arrays = golden
        out = self._run(golden, framework='universal', batch_size=3,
                        model=str(plugin))
        np.testing.assert_allclose(out.numpy().array,
                                   arrays['e2e_identity_out'],
                                   rtol=1e-6, atol=1e-7)

    def test_aligned_mode(self, golden):
        """mask_output_chunk=False: aligned chunk, engine-masked patches,
        no chunk normalize, margins cropped (vs oracle-style expectation:
        interior equals input/255 within the mask sum tolerance)."""
        from chunkflow_amd.inferencer import Inferencer
        chunk = Chunk.create(size=(18, 56, 56), dtype='uint8', pattern='sin')
        inf = Inferencer(None, None, (10, 32, 32),
                         output_patch_overlap=(2, 8, 8),
                         framework='identity', num_output_channels=1,
                         batch_size=2, mask_output_chunk=False,
                         input_size=(18, 56, 56))
        out = inf(chunk)
        assert out.shape == (1, 14, 40, 40)
        assert out.voxel_offset == Cartesian(2, 8, 8)
        expect = chunk.array.astype(np.float32)[2:-2, 8:-8, 8:-8] / 255.0
        np.testing.assert_allclose(out.numpy().array[0], expect,
                                   rtol=1e-2, atol=1e-2)

    def test_all_zero_shortcut(self, golden):
        from chunkflow_amd.inferencer import Inferencer
        chunk = Chunk.create(size=(12, 40, 40), dtype='uint8',
                             pattern='zero')
        inf = Inferencer(None, None, (10, 32, 32),
                         output_patch_overlap=(2, 8, 8),
                         framework='identity', batch_size=2,
                         mask_output_chunk=True)
        out = inf(chunk)
        assert out.numpy().array.max() == 0


@pytest.mark.skipif(GPU, reason='CPU plumbing path is refused on a GPU box')
def test_patch_num_aligned_mode():
    """patch_num mode (reference test_aligned_patch_num shape): aligned
    inference with --patch-num instead of input size, f16 output dtype."""
    from chunkflow_amd.inferencer import Inferencer
    chunk = Chunk.create(size=(18, 56, 56), dtype='uint8', pattern='sin')
    inf = Inferencer(None, None, (10, 32, 32),
                     output_patch_overlap=(2, 8, 8), framework='identity',
                     num_output_channels=2, batch_size=5, dtype='float16',
                     mask_output_chunk=False, patch_num=(2, 2, 2))
    assert tuple(inf.input_size) == (18, 56, 56)
    out = inf(chunk)
    assert out.numpy().array.dtype == np.float16
    assert out.shape == (2, 14, 40, 40)
    expect = chunk.array.astype(np.float32)[2:-2, 8:-8, 8:-8] / 255.0
    np.testing.assert_allclose(out.numpy().array[0].astype(np.float32),
                               expect, rtol=1e-3, atol=2.0 / 255.0)


@pytest.mark.skipif(GPU, reason='CPU plumbing path is refused on a GPU box')
def test_nonaligned_vs_oracle_random_geometry():
    """A fresh odd-size case: product CPU path vs the oracle directly."""
    from chunkflow_amd.inferencer import Inferencer
    from oracle import oracle_inference
    rng = np.random.RandomState(11)
    arr = rng.randint(0, 256, size=(23, 71, 66), dtype=np.uint8)
    inf = Inferencer(None, None, (12, 32, 32),
                     output_patch_overlap=(4, 8, 8), framework='identity',
                     num_output_channels=2, batch_size=7,
                     mask_output_chunk=True)
    out = inf(Chunk(arr.copy(), voxel_offset=(1, 2, 3)))
    ref = oracle_inference(arr, (12, 32, 32), (4, 8, 8),
                           num_output_channels=2, batch_size=7,
                           offset=(1, 2, 3))
    np.testing.assert_allclose(out.numpy().array, ref, rtol=1e-6, atol=1e-7)


def test_disjoint_groups_properties():
    from chunkflow_amd.grouping import disjoint_groups, clip_regions
    rng = np.random.RandomState(3)
    out_dims = (30, 40, 50)
    pd = (8, 12, 16)
    offsets = np.stack([rng.randint(-4, 28, 60), rng.randint(-4, 36, 60),
                        rng.randint(-4, 44, 60)], axis=1)
    groups = disjoint_groups(offsets, pd, out_dims)
    lo, hi = clip_regions(offsets, pd, out_dims)
    empty = (hi <= lo).any(axis=1)
    seen = np.concatenate(groups) if groups else np.array([], dtype=int)
    assert sorted(seen.tolist()) == [i for i in range(60) if not empty[i]]
    gi = {}
    for g, idx in enumerate(groups):
        for i in idx:
            gi[int(i)] = g
    for gidx in groups:
        for a in range(len(gidx)):          # pairwise disjoint within group
            for b in range(a + 1, len(gidx)):
                i, j = gidx[a], gidx[b]
                assert not ((lo[i] < hi[j]) & (lo[j] < hi[i])).all()
    # the config-2 grid: 288 patches group into ~the overlap depth
    from oracle.inference import patch_slices_list
    starts = np.array([o for _, o in patch_slices_list(
        (512, 512, 512), (20, 256, 256), (4, 64, 64))], dtype=np.int64)
    g = disjoint_groups(starts, (20, 256, 256), (512, 512, 512))
    assert 8 <= len(g) <= 27
    assert sum(len(x) for x in g) == 288


def test_normalize_contrast_product_vs_oracle():
    from chunkflow_amd.contrast import normalize_contrast
    from oracle.contrast import oracle_normalize_contrast
    rng = np.random.RandomState(9)
    for arr in ((rng.rand(6, 40, 50) * 256).astype(np.uint8),
                (rng.rand(4, 30, 30) * 80 + 100).astype(np.uint8),
                np.zeros((3, 10, 10), dtype=np.uint8)):
        ref = oracle_normalize_contrast(arr.copy())
        got = normalize_contrast(Chunk(arr.copy()))
        np.testing.assert_array_equal(got.numpy().array, ref)
        # --whole is a no-op, like the reference
        same = normalize_contrast(Chunk(arr.copy()), per_section=False)
        np.testing.assert_array_equal(same.numpy().array, arr)


@pytest.mark.skipif(GPU, reason='CPU plumbing path is refused on a GPU box')
def test_augment_identity_roundtrip():
    """--augment with the identity engine (reference
    test_test_time_augmentation): the 8 TTA variants average back to the
    un-augmented result (square patches; the reference's flips act on
    batch/channel axes — transform.py docstring)."""
    from chunkflow_amd.inferencer import Inferencer
    rng = np.random.RandomState(77)
    arr = rng.randint(0, 256, size=(16, 40, 40), dtype=np.uint8)
    kw = dict(output_patch_overlap=(2, 8, 8), framework='identity',
              num_output_channels=2, batch_size=3, mask_output_chunk=True)
    plain = Inferencer(None, None, (8, 24, 24), **kw)(Chunk(arr.copy()))
    aug = Inferencer(None, None, (8, 24, 24), augment=True,
                     **kw)(Chunk(arr.copy()))
    np.testing.assert_allclose(aug.numpy().array, plain.numpy().array,
                               rtol=1e-5, atol=1e-6)


def test_fastconv_eligibility_rules():
    """Graph-surgery eligibility (no GPU needed): only stride-1 pad-1 3^3
    convs at the widths where the hand kernel beats MIOpen."""
    import torch.nn as nn
    from chunkflow_amd.fastconv import _eligible, _resblock_like
    assert _eligible(nn.Conv3d(28, 28, 3, padding=1))
    assert _eligible(nn.Conv3d(36, 36, 3, padding=1))
    assert not _eligible(nn.Conv3d(48, 48, 3, padding=1))  # MIOpen faster
    assert not _eligible(nn.Conv3d(28, 36, 3, padding=1))  # C != K
    assert not _eligible(nn.Conv3d(28, 28, 3, padding=1, stride=2))
    assert not _eligible(nn.Conv3d(28, 28, (1, 5, 5), padding=(0, 2, 2)))
    assert not _eligible(nn.Conv3d(28, 28, 3, padding=1, groups=28))

    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rsunet_t', os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
            'examples', 'nets', 'rsunet.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    blocks = [m for m in mod.InstantiatedModel.modules()
              if _resblock_like(m)]
    assert len(blocks) == 4  # the two 28- and two 36-wide ResBlocks


def _fresh_rsunet():
    import copy
    from chunkflow_amd.model_loader import load_source
    src = load_source(os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        'examples', 'nets', 'rsunet.py'))
    return copy.deepcopy(src.InstantiatedModel).eval()


def _walk_groups(monkeypatch, net, bf16, verdict):
    """every surgery group in order on the CPU, the probe replaced by a
    stub that answers `verdict`; returns the per-group counts"""
    from chunkflow_amd import fastconv as fc
    probed = []

    def stub(orig, repl, shape, dev, bf16_, tol):
        probed.append((type(repl).__name__, tuple(shape), bf16_, tol))
        return verdict

    monkeypatch.setattr(fc, '_probe', stub)
    counts = [fc._walk(net, rules, 'cpu', 0, bf16)
              for rules in fc._groups(bf16).values()]
    return counts, probed


def _classes(net):
    return {name: type(m).__name__ for name, m in net.named_modules()}


def test_surgery_walker_f32_probe_true(monkeypatch):
    """The rule-driven walker on the RSUNet, f32 groups in the engine's
    order: 7 ResBlocks (a detached block's convs are not visited again,
    or the count would be higher), 3 up-convs, conv_in, conv_out."""
    net = _fresh_rsunet()
    keys = list(net.state_dict())
    counts, probed = _walk_groups(monkeypatch, net, False, True)
    assert counts == [7, 3, 1, 1]
    got = _classes(net)
    want = {'enc.0': 'CfxResBlock', 'enc.1': 'CfxResBlock',
            'enc.2': 'CfxMiopenResBlock', 'enc.3': 'CfxMiopenResBlock',
            'dec.0': 'CfxResBlock', 'dec.1': 'CfxResBlock',
            'dec.2': 'CfxMiopenResBlock',
            'up.0': 'CfxUpConv3d', 'up.1': 'CfxUpConv3d',
            'up.2': 'CfxUpConv3d',
            'down.0': 'Conv3d', 'down.1': 'Conv3d', 'down.2': 'Conv3d',
            'conv_in': 'CfxConvIn155', 'conv_out': 'CfxConvOut155'}
    assert {k: got[k] for k in want} == want
    assert got['enc.0.c1'] == got['dec.1.c2'] == 'CfxConv3d'
    assert [net.enc[i].c1.C for i in (0, 1)] == [28, 36]
    assert [net.enc[i].C for i in (2, 3)] == [48, 64]
    assert net.dec[2].C == 48
    # the probes each rule asks for: shape, dtype and tolerance
    assert probed == (
        [('CfxResBlock', (1, 28, 4, 18, 22), False, 1e-4),
         ('CfxResBlock', (1, 36, 4, 18, 22), False, 1e-4),
         ('CfxMiopenResBlock', (1, 48, 4, 18, 22), False, 1e-4),
         ('CfxMiopenResBlock', (1, 64, 4, 18, 22), False, 1e-4),
         ('CfxResBlock', (1, 28, 4, 18, 22), False, 1e-4),
         ('CfxResBlock', (1, 36, 4, 18, 22), False, 1e-4),
         ('CfxMiopenResBlock', (1, 48, 4, 18, 22), False, 1e-4)]
        + [('CfxUpConv3d', (1, c, 3, 12, 16), False, 1e-4)
           for c in (36, 48, 64)]
        + [('CfxConvIn155', (1, 1, 3, 14, 19), False, 1e-4),
           ('CfxConvOut155', (1, 28, 3, 14, 19), False, 1e-4)])
    # buffer names as before the walker: wtap/bias, w1/b1/w2/b2, wpack
    new_keys = set(net.state_dict())
    assert {'enc.0.c1.wtap', 'enc.0.c1.bias', 'enc.2.w1', 'enc.2.b1',
            'enc.2.w2', 'enc.2.b2', 'up.0.wpack', 'up.0.bias',
            'conv_in.wpack', 'conv_in.bias', 'conv_out.wpack',
            'conv_out.bias', 'down.0.weight'} <= new_keys
    assert len(new_keys) == len(keys)


def test_surgery_walker_bf16_probe_true(monkeypatch):
    from chunkflow_amd import fastconv as fc
    assert fc.BF16_WIDTHS == (28, 36)  # the default the counts assume
    net = _fresh_rsunet()
    counts, probed = _walk_groups(monkeypatch, net, True, True)
    assert counts == [4, 2, 1, 1]
    got = _classes(net)
    want = {'enc.0': 'CfxResBlockBF16', 'enc.1': 'CfxResBlockBF16',
            'dec.0': 'CfxResBlockBF16', 'dec.1': 'CfxResBlockBF16',
            'enc.2': 'ResBlock', 'enc.3': 'ResBlock', 'dec.2': 'ResBlock',
            'enc.0.c1': 'CfxConv3dBF16', 'enc.2.conv1': 'Conv3d',
            'up.0': 'CfxUpConv3d', 'up.1': 'CfxUpConv3d',
            'up.2': 'ConvTranspose3d',
            'conv_in': 'CfxConvIn155', 'conv_out': 'CfxConvOut155'}
    assert {k: got[k] for k in want} == want
    assert net.up[0].bf16 and net.conv_in.bf16 and net.conv_out.bf16
    assert all(p[2] is True and p[3] == 0.05 for p in probed)
    assert len(probed) == 8


def test_surgery_walker_probe_false_falls_back_to_lone_convs(monkeypatch):
    """A hand-kernel block that fails the probe keeps its own forward and
    gets its two convs swapped, unprobed; nothing else is installed."""
    net = _fresh_rsunet()
    blocks = {n: m for n, m in net.named_modules()
              if n.startswith(('enc.', 'dec.')) and n.count('.') == 1}
    counts, probed = _walk_groups(monkeypatch, net, False, False)
    assert counts == [8, 0, 0, 0]
    assert len(probed) == 12   # every probed rule asked, none installed
    got = _classes(net)
    for name, block in blocks.items():
        assert net.get_submodule(name) is block   # the original object
        # levels 0 and 1 are the 28- and 36-wide blocks
        want = 'CfxConv3d' if name[-1] in '01' else 'Conv3d'
        assert got[name + '.conv1'] == got[name + '.conv2'] == want, name
    assert sum(v == 'CfxConv3d' for v in got.values()) == 8
    for name in ('up.0', 'up.1', 'up.2'):
        assert got[name] == 'ConvTranspose3d'
    assert got['conv_in'] == got['conv_out'] == 'Conv3d'


@pytest.mark.parametrize('seed', [5, 6, 7, 11])
def test_normalize_contrast_vs_live_reference(seed):
    """The contrast oracle is BIT-EQUAL to the reference
    Image.normalize_contrast on random uint8 volumes (including the
    for-else whole-chunk second pass, chunk/image/base.py:30-132). The
    reference results were recorded from the unmodified reference by
    oracle/reference_cases.py (tests/golden/)."""
    from oracle import reference_cases as rc
    from oracle.contrast import oracle_normalize_contrast
    arr = rc.contrast_case(seed)
    ref = rc.load_recorded()[f'contrast_{seed}']
    mine = oracle_normalize_contrast(arr.copy())
    assert mine.dtype == ref.dtype and mine.shape == ref.shape
    np.testing.assert_array_equal(mine, ref)


# --- round-2 advisor fixes -------------------------------------------------
def test_equal_value_label_semantics():
    """cc3d-style equal-value CC (reference chunk/base.py:128-137): touching
    regions of DIFFERENT values stay separate components."""
    from chunkflow_amd.connected import equal_value_label
    arr = np.zeros((3, 4, 4), dtype=np.uint8)
    arr[0, :2, :2] = 5          # component 1 (first raster encounter)
    arr[0, :2, 2:] = 7          # touches the 5-region -> still separate
    arr[2, 2:, 2:] = 5          # disconnected 5-region -> third component
    lab = equal_value_label(arr, 6)
    assert lab[0, 0, 0] == 1 and lab[0, 0, 2] == 2 and lab[2, 2, 2] == 3
    assert lab[1].sum() == 0
    # binary input degenerates to plain labeling
    from scipy import ndimage
    binary = (arr == 5).astype(np.uint8)
    ref, _ = ndimage.label(binary, ndimage.generate_binary_structure(3, 1))
    assert np.array_equal(equal_value_label(binary, 6) > 0, ref > 0)


def test_connected_component_multivalue_no_threshold():
    from chunkflow_amd.connected import connected_component
    arr = np.zeros((2, 5, 5), dtype=np.uint32)
    arr[0, :, :2] = 3
    arr[0, :, 2:] = 9           # touching, different value
    out = connected_component(Chunk(arr), threshold=None)
    assert len(np.unique(out.array)) == 3  # 0 + two components, not merged


def test_create_random_integer_is_labeled():
    np.random.seed(0)
    c = Chunk.create(size=(16, 16, 16), dtype=np.uint32, pattern='random')
    a = c.array if isinstance(c.array, np.ndarray) else c.array.numpy()
    # labels are dense 1..N (plus background), not raw randints
    u = np.unique(a)
    u = u[u != 0]
    assert np.array_equal(u, np.arange(1, len(u) + 1))


def test_create_sin_uint32_is_labeled():
    c = Chunk.create(size=(16, 16, 16), dtype=np.uint32, pattern='sin')
    a = np.asarray(c.array)
    u = np.unique(a)
    u = u[u != 0]
    assert len(u) >= 1 and np.array_equal(u, np.arange(1, len(u) + 1))


def test_from_h5_negative_cutout_size(tmp_path):
    """Reference base.py:328-333: negative cutout_size entries (without an
    explicit cutout_start) are filled from the dataset shape."""
    from chunkflow_amd import h5io
    arr = np.arange(4 * 6 * 8, dtype=np.uint8).reshape(4, 6, 8)
    p = str(tmp_path / 'c.h5')
    h5io.write_h5(p, {'main': arr})
    c = Chunk.from_h5(p, cutout_size=(-1, 6, -1))
    assert c.shape == (4, 6, 8)
    assert np.array_equal(np.asarray(c.array), arr)


# --- round-2 reference-golden pins (TTA + full RSUNet) ---------------------
@pytest.mark.skipif(GPU, reason='CPU plumbing path is refused on a GPU box')
def test_augment_identity_golden(golden):
    """TTA (augment=True) pinned against the live reference
    (transform.py:114-156 semantics): identity engine, batch 3."""
    from chunkflow_amd.inferencer import Inferencer
    _, arrays = golden
    inf = Inferencer(None, None, (10, 32, 32),
                     output_patch_overlap=(2, 8, 8), framework='identity',
                     num_output_channels=3, batch_size=3,
                     mask_output_chunk=True, augment=True)
    out = inf(Chunk(arrays['e2e_input_u8'].copy()))
    np.testing.assert_allclose(out.numpy().array,
                               arrays['e2e_identity_augment_out'],
                               rtol=1e-5, atol=1e-6)


@pytest.mark.skipif(GPU, reason='CPU plumbing path is refused on a GPU box')
def test_augment_pytorch_golden(golden, golden_dir):
    """TTA through the conv engine (the transforms actually change the
    output here, unlike identity) vs the live reference."""
    from chunkflow_amd.inferencer import Inferencer
    _, arrays = golden
    inf = Inferencer(os.path.join(golden_dir, 'ref_model.py'),
                     os.path.join(golden_dir, 'ref_model_weights.pt'),
                     (10, 32, 32),
                     output_patch_overlap=(2, 8, 8), framework='pytorch',
                     num_output_channels=3, batch_size=1,
                     mask_output_chunk=True, augment=True)
    out = inf(Chunk(arrays['e2e_input_u8'].copy()))
    np.testing.assert_allclose(out.numpy().array,
                               arrays['e2e_pytorch_augment_out'],
                               rtol=1e-5, atol=1e-5)


def test_rsunet_weight_determinism(golden):
    """The committed rsunet_weights.pt matches the seeded in-repo model
    (guards the golden against silent model-file drift)."""
    meta, _ = golden
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rsunet_det', os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
            'examples', 'nets', 'rsunet.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = meta['cases']['rsunet_64x256x256']['weight_f64_sums']
    got = {k: float(v.to(torch.float64).sum())
           for k, v in mod.InstantiatedModel.state_dict().items()}
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) < 1e-6, k


@pytest.mark.skipif(GPU, reason='CPU plumbing path is refused on a GPU box')
def test_rsunet_64x256x256_cpu_plumbing_golden(golden, golden_dir):
    """Full benchmark RSUNet through the product CPU plumbing path vs the
    live-reference Inferencer output (~15-60 s
    depending on the box)."""
    import os as _os
    torch.set_num_threads(min(8, _os.cpu_count() or 8))
    from chunkflow_amd.inferencer import Inferencer
    meta, arrays = golden
    case = meta['cases']['rsunet_64x256x256']
    rs_in = Chunk.create(size=(64, 256, 256), dtype='uint8', pattern='sin')
    assert crc(np.asarray(rs_in.array)) == case['input_crc32']
    inf = Inferencer(
        os.path.join(os.path.dirname(golden_dir), '..', 'examples', 'nets',
                     'rsunet.py'),
        os.path.join(golden_dir, 'rsunet_weights.pt'),
        (20, 128, 128), output_patch_overlap=(4, 32, 32),
        framework='pytorch', num_output_channels=3, batch_size=4,
        mask_output_chunk=True)  # batch 4: same result to 1e-5 (ulp
    # argument in grouping.py), ~2x faster on the 8-core CPU box
    out = np.asarray(inf(rs_in).numpy().array)
    assert out.shape == (3, 64, 256, 256)
    np.testing.assert_allclose(out[:, ::4, ::8, ::8],
                               arrays['rsunet_64x256x256_sub'],
                               rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(
        out.ravel()[arrays['rsunet_64x256x256_sample_idx']],
        arrays['rsunet_64x256x256_sample_val'], rtol=1e-5, atol=1e-5)
    assert abs(out.astype(np.float64).sum() - case['sum_f64']) < 1.0


def test_blend_reference_order_switch(golden, monkeypatch):
    """CFX_BLEND_REFORDER=1 blends one patch per call in the reference's
    exact order; result must match the default grouped blending at 1e-6
    and the reference golden exactly as the default does."""
    if GPU:
        pytest.skip('CPU plumbing path')
    from chunkflow_amd.inferencer import Inferencer
    _, arrays = golden

    def run():
        inf = Inferencer(None, None, (10, 32, 32),
                         output_patch_overlap=(2, 8, 8),
                         framework='identity', num_output_channels=3,
                         batch_size=3, mask_output_chunk=True)
        return np.asarray(
            inf(Chunk(arrays['e2e_input_u8'].copy())).numpy().array)

    base = run()
    monkeypatch.setenv('CFX_BLEND_REFORDER', '1')
    ref_order = run()
    np.testing.assert_allclose(ref_order, base, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(ref_order, arrays['e2e_identity_out'],
                               rtol=1e-6, atol=1e-7)
