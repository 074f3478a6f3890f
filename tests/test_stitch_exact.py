"""Bit-exact pins for the chunk stitching kernels (chunkflow_amd/csrc/
cfx.hip): u8 casts, extract, blend, batched blend, reciprocal,
mask-normalize with the fused max scan, max, crop, myelin mask.

Tables, numpy references and the driver live in tests/stitch_cases.py. The
CPU tests push every case through TorchOps, which proves the tables and
the references on any machine, and check the premises the GPU tests rest
on. The GPU tests push the same cases through HipOps and compare bit
patterns, guards included; then the chunk mask and a whole identity
inference are held against the oracle voxel by voxel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stitch_cases as sc  # noqa: E402

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
U = 2.0 ** -24                      # f32 unit roundoff


def _param(cases):
    return pytest.mark.parametrize('case', cases, ids=[c['id'] for c in cases])


@pytest.fixture(scope='module')
def hip_ops():
    from chunkflow_amd.ops import HipOps
    return HipOps(0)


@pytest.fixture(scope='module')
def torch_ops():
    from chunkflow_amd.ops import TorchOps
    return TorchOps()


ALL_CASES = [c for fam in sc.FAMILIES.values() for c in fam]


# ---------------------------------------------------------------------------
# CPU: tables and references
# ---------------------------------------------------------------------------
@_param(ALL_CASES)
def test_tables_on_torch_ops(torch_ops, case):
    """TorchOps == the numpy reference, bit for bit, on every case."""
    sc.check_case(torch_ops, case)


def test_case_ids_unique_and_conditions_met():
    ids = [c['id'] for c in ALL_CASES]
    assert len(set(ids)) == len(ids)
    # the sizes the tables claim to be "just over" a launch cap
    assert sc.U8_WRAP // 4 > 8192 * 256
    assert sc.MM_BIG % 4 == 0 and (sc.MM_BIG // 4) % 2 == 1
    assert sc.MM_BIG // 4 > 8192 * 512
    assert sc.MAX_BIG > 4096 * 256
    assert sc.MAX_X4 > 4 * 4096 * 256 and sc.MAX_X9 > 8 * 4096 * 256
    by_id = {c['id']: c for c in ALL_CASES}
    c = by_id['extract-wrap']
    assert c['C'] * c['patch'][0] * c['patch'][1] > 8192 * 4 * 2
    c = by_id['extract-split-65']
    assert len(c['starts']) == 65
    assert (c['C'] * c['patch'][0] * c['patch'][1]) % 2 == 1
    c = by_id['blend-wrap-masked']
    assert c['out'][0] * c['out'][1] * c['out'][2] > 8192 * 16
    assert sc.batch_lines(by_id['blend_batch-wrap-masked']) > 8192 * 4 * 2
    assert sc.batch_lines(by_id['blend_batch-odd-lines-masked']) % 2 == 1
    c = by_id['crop-wrap']
    assert np.prod(sc._crop_shape(c)[:-1]) > 8192 * 4
    # a mid-batch and a batch-end empty item, and mixed rx within a launch
    c = by_id['blend_batch-vec-33-masked']
    assert len(c['items']) == 33 and sc.assert_batch_disjoint(c) == 30
    lo, hi = sc.batch_regions(c)
    assert len(set((hi - lo)[:, 2].tolist())) > 1
    assert ((hi - lo)[:, 2] % 4 == 0).all() and (lo[:, 2] % 4 == 0).all()


def test_batch_tables_are_disjoint():
    for case in sc.BLEND_BATCH_CASES:
        assert sc.assert_batch_disjoint(case) >= 1
    overlapping = dict(id='bad', out=(1, 4, 4, 8), patch=(1, 1, 2, 2, 8),
                       items=np.array([[0, 0, 0, 0], [0, 1, 1, 0]], np.int32))
    with pytest.raises(AssertionError, match='overlap'):
        sc.assert_batch_disjoint(overlapping)


def test_premise_contraction_is_visible():
    """On the blend inputs a fused multiply-add (one rounding; computed
    here in f64, where the product of two f32 is exact) differs from the
    two-rounding f32 result in at least 1 % of the elements — so a build
    that lost -ffp-contract=off cannot pass the bit-exact blend cases."""
    for case in (c for c in sc.BLEND_CASES + sc.BLEND_BATCH_CASES
                 if c['masked'] and 'wrap' not in c['id']):
        inp = sc.make_inputs(case)
        patch = inp['patch'][0]
        o = inp['dst'].ravel()[:patch.size].reshape(patch.shape)
        two = (patch * inp['mask']) + o
        assert two.dtype == np.float32
        fused = (patch.astype(np.float64) * inp['mask'].astype(np.float64)
                 + o.astype(np.float64)).astype(np.float32)
        share = float(np.mean(two.view(np.uint32) != fused.view(np.uint32)))
        assert share >= 0.01, (case['id'], share)


def test_premise_one_element_corruption_is_caught():
    case = next(c for c in sc.BLEND_CASES if c['id'] ==
                'blend-interior-masked')
    inp = sc.make_inputs(case)
    exp = sc.reference(case, inp)
    sc.compare(case, {k: v.copy() for k, v in exp.items()}, exp)
    for where in (0, sc.GUARD + 12345, exp['dst'].size - 1):  # guard, body
        bad = {k: v.copy() for k, v in exp.items()}
        bad['dst'].view(np.uint32)[where] ^= np.uint32(1)     # one ulp
        with pytest.raises(AssertionError, match='1 of'):
            sc.compare(case, bad, exp)
    # scalars: a dropped NaN and a wrong value
    mcase = dict(id='m')
    with pytest.raises(AssertionError):
        sc.compare(mcase, dict(max=np.float32(1.0)),
                   dict(max=np.float32(np.nan)))
    with pytest.raises(AssertionError):
        sc.compare(mcase, dict(max=np.float32(np.nan)),
                   dict(max=np.float32(1.0)))
    sc.compare(mcase, dict(max=np.float32(np.nan)),
               dict(max=np.float32(np.nan)))
    # NaN payloads are the only tolerated difference, and only when asked
    a = np.array([1.0, np.nan], np.float32)
    b = a.copy()
    b.view(np.uint32)[1] = sc.NAN_NEG
    assert sc.bits_mismatch(a, b).size == 1
    assert sc.bits_mismatch(a, b, nan_ok=True).size == 0


# ---------------------------------------------------------------------------
# GPU: the same tables through HipOps, one test per kernel family
# ---------------------------------------------------------------------------
@gpu
@_param(sc.U8_CASES)
def test_u8_to_f32_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.EXTRACT_CASES)
def test_extract_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.BLEND_CASES)
def test_blend_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.BLEND_BATCH_CASES)
def test_blend_batch_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.RECIP_CASES)
def test_reciprocal_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.MASKMUL_CASES)
def test_maskmul_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.MAX_CASES)
def test_max_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.CROP_CASES)
def test_crop_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.MYELIN_CASES)
def test_myelin_exact(hip_ops, case):
    sc.check_case(hip_ops, case)


@gpu
@_param(sc.NAN_CASES)
def test_max_scan_sees_nan(hip_ops, case):
    """cfx_max and the fused cfx_multiply_mask_max return NaN for a NaN of
    either sign at any position (the multiply itself unchanged)."""
    sc.check_case(hip_ops, case)


@gpu
def test_fused_max_unavailable_on_unaligned_view(hip_ops):
    """The C entry reports "unavailable" (None here) after doing the
    multiply, for an unaligned view as for n % 4 != 0."""
    for mis_out, mis_mask, n in ((1, 0, 4116), (0, 1, 4116), (0, 0, 4117)):
        rng = np.random.RandomState(n + mis_out)
        out, mask = sc.mixed(rng, 2 * n), sc.mixed(rng, n)
        _, o = sc._device_view(hip_ops, out, mis_out)
        _, m = sc._device_view(hip_ops, mask, mis_mask)
        assert hip_ops.cfx.multiply_mask_max(
            o.data_ptr(), m.data_ptr(), 2, n) is None
        hip_ops.sync()
        exp = (out.reshape(2, n) * mask).ravel()
        assert sc.bits_mismatch(o.cpu().numpy(), exp).size == 0


# ---------------------------------------------------------------------------
# chunk mask and whole identity inference against the oracle
# ---------------------------------------------------------------------------
# a few patches per axis, tail-clamped on every axis; 'x4' keeps every x
# start, the row length and the patch a multiple of 4 (float4 kernels),
# 'odd' has an odd row length (scalar kernels)
PATCH, OVERLAP = (4, 16, 16), (1, 4, 4)
GEOMETRIES = {'x4': (8, 44, 48), 'odd': (9, 41, 45)}
CHANNELS, BATCH = 2, 7


def _slices(size):
    from oracle.inference import patch_slices_list
    return patch_slices_list(size, PATCH, OVERLAP)


def _coverage(size):
    """Patches covering each voxel, counted from the slice list
    (duplicates from tail clamping count)."""
    cov = np.zeros(size, dtype=np.int64)
    for _, (z, y, x) in _slices(size):
        cov[z:z + PATCH[0], y:y + PATCH[1], x:x + PATCH[2]] += 1
    return cov


def reorder_bound(k):
    """Relative distance allowed between two f32 evaluations of
    out_sum * (1 / mask_sum) that add their k non-negative terms in
    different orders.

    With u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and
    Stability of Numerical Algorithms, lemma 3.1): a sum of k terms takes
    k - 1 rounded additions (the first lands on an exact zero), so each
    computed sum is S (1 + t) with |t| <= gamma_{k-1} whatever the order,
    and because all terms are non-negative S is the same positive number
    for both. Two orders of the output sum therefore stand in a ratio of at
    most (1 + gamma_{k-1}) / (1 - gamma_{k-1}), and so do two orders of the
    mask sum. The reciprocal and the final multiply add one rounding each
    to either result, a ratio of (1 + u) / (1 - u) apiece. Hence
        got / ref <= R = ((1 + g) / (1 - g))^2 ((1 + u) / (1 - u))^2,
    g = gamma_{k-1}, and |got - ref| <= (R - 1) |ref|; R - 1 is about
    (4 (k - 1) + 4) u."""
    k = np.asarray(k, dtype=np.float64)
    g = (k - 1) * U / (1 - (k - 1) * U)
    return ((1 + g) / (1 - g)) ** 2 * ((1 + U) / (1 - U)) ** 2 - 1


@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_premise_geometries_have_both_voxel_classes(name):
    size = GEOMETRIES[name]
    cov = _coverage(size)
    assert cov.min() >= 1
    assert (cov <= 2).sum() > 0 and (cov >= 3).sum() > 0
    starts = np.array([o for _, o in _slices(size)])
    assert len(starts) > BATCH           # more than one batch
    for ax in range(3):                  # tail clamping on every axis
        s = np.unique(starts[:, ax])
        stride = PATCH[ax] - OVERLAP[ax]
        assert len(s) >= 2 and (s[-1] - s[-2]) != stride
    x4 = size[2] % 4 == 0 and (starts[:, 2] % 4 == 0).all()
    assert x4 == (name == 'x4')
    # the grouped blend does reorder something here
    from chunkflow_amd.grouping import disjoint_groups
    groups = disjoint_groups(starts[:BATCH], PATCH, size)
    assert any((np.diff(np.concatenate(groups)) < 0).tolist())


@gpu
@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_build_chunk_mask_exact(hip_ops, name):
    """Per-offset path == the oracle everywhere; grouped path == the oracle
    wherever at most two patches meet (a + b == b + a in f32)."""
    from chunkflow_amd.grouping import disjoint_groups
    from oracle.inference import build_chunk_mask
    from oracle.patch_mask import make_patch_mask
    size = GEOMETRIES[name]
    slices = _slices(size)
    pm = make_patch_mask(PATCH, OVERLAP)
    ref = build_chunk_mask(size, (0, 0, 0), slices, pm)
    offsets = np.array([o for _, o in slices], dtype=np.int32)
    pm_t = torch.from_numpy(pm.copy()).cuda()
    got = hip_ops.build_chunk_mask(size, pm_t, offsets).cpu().numpy()
    assert sc.bits_mismatch(got, ref).size == 0
    groups = disjoint_groups(offsets, PATCH, size)
    got = hip_ops.build_chunk_mask(size, pm_t, offsets,
                                   groups=groups).cpu().numpy()
    cov = _coverage(size)
    low = cov <= 2
    assert sc.bits_mismatch(got[low], ref[low]).size == 0
    err = np.abs(got.astype(np.float64) - ref)
    # one sum, one reciprocal: inside the two-sum bound a fortiori
    assert (err <= reorder_bound(cov) * np.abs(ref)).all()


def _identity_inference(size, device):
    from chunkflow_amd.chunk import Chunk
    from chunkflow_amd.inferencer import Inferencer
    rng = np.random.RandomState(sum(size))
    arr = rng.randint(0, 256, size=size).astype(np.uint8)
    inf = Inferencer(None, None, PATCH, output_patch_overlap=OVERLAP,
                     framework='identity', num_output_channels=CHANNELS,
                     batch_size=BATCH, mask_output_chunk=True,
                     compute_device=device)
    return arr, inf(Chunk(arr.copy())).numpy().array


_ORACLE = {}


def _oracle(size, arr):
    """Computed once per geometry and shared; never modified."""
    from oracle import oracle_inference
    if size not in _ORACLE:
        ref = oracle_inference(arr, PATCH, OVERLAP,
                               num_output_channels=CHANNELS,
                               batch_size=BATCH)
        ref.setflags(write=False)
        _ORACLE[size] = (arr.copy(), ref)
    assert np.array_equal(_ORACLE[size][0], arr)
    return _ORACLE[size][1]


@gpu
@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_identity_inference_reference_order_exact(name, monkeypatch):
    """CFX_BLEND_REFORDER=1 reproduces the oracle bit for bit."""
    monkeypatch.setenv('CFX_BLEND_REFORDER', '1')
    size = GEOMETRIES[name]
    arr, got = _identity_inference(size, 'cuda:0')
    ref = _oracle(size, arr)
    assert got.shape == ref.shape
    assert sc.bits_mismatch(got, ref).size == 0


@gpu
@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_identity_inference_grouped_exact_up_to_two(name, monkeypatch):
    """Default grouped blend: bit-equal wherever coverage <= 2, inside
    reorder_bound(coverage) elsewhere (derivation there; not tuned)."""
    monkeypatch.delenv('CFX_BLEND_REFORDER', raising=False)
    size = GEOMETRIES[name]
    arr, got = _identity_inference(size, 'cuda:0')
    ref = _oracle(size, arr)
    cov = np.broadcast_to(_coverage(size), ref.shape)
    low = cov <= 2
    assert sc.bits_mismatch(got[low], ref[low]).size == 0
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = reorder_bound(cov) * np.abs(ref.astype(np.float64))
    worst = float((err[~low] / np.maximum(bound[~low], 1e-300)).max())
    print(f'{name}: worst error / bound at coverage >= 3: {worst:.3f}')
    assert (err <= bound).all()


@gpu
def test_blend_batch_tuning_knobs_exact():
    """CFX_BLEND_G and CFX_BLEND_NT are read once per process: run the
    batch table in a fresh child for each setting, one after the other,
    stopping at the first that fails."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          'stitch_cases.py')
    for g, nt in ((4, 0), (8, 0), (2, 1)):
        env = dict(os.environ, CFX_BLEND_G=str(g), CFX_BLEND_NT=str(nt))
        proc = subprocess.run([sys.executable, script, '--blend-batch'],
                              env=env, timeout=240, capture_output=True,
                              text=True)
        assert proc.returncode == 0, \
            f'G={g} NT={nt}: rc={proc.returncode}\n{proc.stdout[-2000:]}' \
            f'\n{proc.stderr[-2000:]}'


# ---------------------------------------------------------------------------
# a NaN in the output must trip the "< 1.0001" check
# ---------------------------------------------------------------------------
def _nan_inference(device, mask_output_chunk):
    from chunkflow_amd.chunk import Chunk
    from chunkflow_amd.inferencer import Inferencer

    def poison(output):
        output[1, 2, 3, 5] = float('nan')

    size = (7, 28, 28)                   # aligned: (size - overlap) % stride
    kw = {} if mask_output_chunk else dict(input_size=size)
    inf = Inferencer(None, None, PATCH, output_patch_overlap=OVERLAP,
                     framework='identity', num_output_channels=CHANNELS,
                     batch_size=BATCH, mask_output_chunk=mask_output_chunk,
                     compute_device=device, pre_normalize_hook=poison, **kw)
    arr = np.random.RandomState(5).randint(1, 256, size=size).astype(np.uint8)
    with pytest.raises(AssertionError, match='should not be greater than 1'):
        inf(Chunk(arr))
    # and the same run without the NaN passes the check
    inf.pre_normalize_hook = None
    inf(Chunk(arr))


@pytest.mark.skipif(HAS_GPU,
                    reason='CPU plumbing path is refused on a GPU box')
@pytest.mark.parametrize('mask_output_chunk', [True, False])
def test_nan_output_raises_cpu(mask_output_chunk):
    _nan_inference('cpu', mask_output_chunk)


@gpu
@pytest.mark.parametrize('mask_output_chunk', [True, False])
def test_nan_output_raises_gpu(mask_output_chunk):
    _nan_inference('cuda:0', mask_output_chunk)
