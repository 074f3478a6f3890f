"""Every hand-written conv kernel pinned to a float64 CPU reference.

Tier 1 (bit-exact): small-integer inputs on which f32 accumulation and
every bf16 rounding point are exact (tests/conv_exact_util.py), so each
kernel variant, in f32 and bf16, must reproduce the f64 CPU convolution bit
for bit — one wrong tap, halo column, channel or residual voxel anywhere
fails. Only the negative ELU branch (device expm1f) gets a 1-bf16-ulp /
4-f32-ulp allowance.

Tier 2 (rounding): real-valued bf16 inputs against the f64 convolution
pushed through the kernels' documented bf16 rounding points.

The reference is never a GPU library result. The CPU self-test checks the
exactness premise without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact_util as U  # noqa: E402

gpu = pytest.mark.gpu
CL = torch.channels_last_3d


def _id(v):
    if isinstance(v, tuple):
        return 'x'.join(str(i) for i in v)
    return str(v)


# --------------------------------------------------------------------------
# CPU-only: the premise
# --------------------------------------------------------------------------
def test_exactness_premise_cpu():
    """For every case in the table: (a) the f32 CPU conv of the integer
    inputs equals the f64 one exactly (f32 accumulation is exact, hence
    order-independent); (b) every value that reaches a bf16 rounding point
    — full sum, + bias, + residual, and the sliced schedule's
    first-32-channel partial sum with and without the residual — is an
    integer of magnitude <= 256; (c) both ELU branches are populated."""
    cases = U.all_cases()
    assert len(cases) == len(set(cases))
    for kind, shape, C, K in cases:
        ref = U.reference(kind, shape, C, K)
        what = f'{kind} {shape} C={C} K={K}'
        vals = set(ref.x.unique().tolist())
        assert vals <= {-2.0, -1.0, 0.0, 1.0, 2.0}, what
        assert set(ref.w.unique().tolist()) <= {-1.0, 0.0, 1.0}, what
        assert float(ref.b.abs().max()) <= 4, what
        assert float(ref.r.abs().max()) <= 8, what
        acc32 = U.cpu_conv(kind, ref.x, ref.w, torch.float32)
        np.testing.assert_array_equal(acc32.double().numpy(),
                                      ref.acc.numpy(), err_msg=what)
        assert torch.equal(ref.acc, ref.acc.round()), what
        assert ref.rounding_point_max() <= U.BF16_EXACT_MAX, \
            (what, ref.rounding_point_max())
        if ref.acc.numel() >= 1000:
            frac_neg = float((ref.pre(True, True) < 0).double().mean())
            assert 0.3 < frac_neg < 0.7, (what, frac_neg)
        # bf16 holds every input exactly
        for t in (ref.x, ref.w, ref.b, ref.r):
            assert torch.equal(t.to(torch.bfloat16).float(), t), what


def test_comparison_catches_one_wrong_element():
    """The comparison itself: one element off by one integer step, or one
    ELU element off by two bf16 ulps, fails; a clean copy passes."""
    ref = U.reference('c333', (1, 3, 18, 67), 28, 28)
    want, neg = ref.expect(True, True, True)
    good = want.float().to(torch.bfloat16)
    U.assert_exact(good, want, neg)
    flat_pos = torch.nonzero(~neg.flatten())[7].item()
    flat_neg = torch.nonzero(neg.flatten())[7].item()
    bad = good.clone()
    bad.view(-1)[flat_pos] += 1
    with pytest.raises(AssertionError):
        U.assert_exact(bad, want, neg)
    bad = good.clone()
    raw = bad.view(-1).view(torch.int16)
    raw[flat_neg] += 2
    with pytest.raises(AssertionError):
        U.assert_exact(bad, want, neg)


# --------------------------------------------------------------------------
# tier 1: bit-exact, 3x3x3 kernels
# --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', U.C333_SHAPES, ids=_id)
@pytest.mark.parametrize('path,C', U.C333_PATHS, ids=_id)
def test_conv3_exact(path, C, shape):
    """slab / w32 / f32 z-ring (28, 36 three-launch, 48 dw) / bf16 default
    ring / bf16 sliced ring: plain, ELU, bias+residual+ELU, residual without
    ELU and bias=None, each bit-equal to the f64 CPU conv."""
    U.check_c333(path, C, shape)


# --------------------------------------------------------------------------
# tier 1: bit-exact, streaming kernels (csrc/updown.hip)
# --------------------------------------------------------------------------
def _module_case(kind, shape, C, K, bf16, bias, make):
    ref = U.reference(kind, shape, C, K)
    assert ref.rounding_point_max() <= U.BF16_EXACT_MAX
    conv = make(bias)
    with torch.no_grad():
        conv.weight.copy_(ref.w)
        if bias:
            conv.bias.copy_(ref.b)
    dt = torch.bfloat16 if bf16 else torch.float32
    x = ref.x.to(dt).cuda().contiguous(memory_format=CL)
    return ref, conv, x


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', U.UP_SHAPES, ids=_id)
@pytest.mark.parametrize('C,K', U.UP_WIDTHS, ids=_id)
def test_upconv_exact(C, K, shape, bf16):
    from chunkflow_amd.fastconv import CfxUpConv3d
    for bias in (True, False):
        ref, conv, x = _module_case(
            'up', shape, C, K, bf16, bias,
            lambda b: torch.nn.ConvTranspose3d(C, K, (1, 2, 2),
                                               stride=(1, 2, 2), bias=b))
        got = CfxUpConv3d(conv, 0, bf16=bf16).cuda()(x)
        want, neg = ref.expect(bias)
        U.assert_exact(got, want, neg, f'up {C}->{K} {shape} bias={bias}')


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', U.DOWN_SHAPES, ids=_id)
@pytest.mark.parametrize('C,K', U.DOWN_WIDTHS, ids=_id)
def test_downconv_exact(C, K, shape, bf16):
    from chunkflow_amd.fastconv import CfxDownConv3d
    for bias in (True, False):
        ref, conv, x = _module_case(
            'down', shape, C, K, bf16, bias,
            lambda b: torch.nn.Conv3d(C, K, (1, 2, 2), stride=(1, 2, 2),
                                      bias=b))
        got = CfxDownConv3d(conv, 0, bf16=bf16).cuda()(x)
        want, neg = ref.expect(bias)
        U.assert_exact(got, want, neg, f'down {C}->{K} {shape} bias={bias}')


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', U.CONV_IN_SHAPES, ids=_id)
@pytest.mark.parametrize('K', U.CONV_IN_K)
def test_conv_in_exact(K, shape, bf16):
    """(1,5,5) input conv: K=28 is the compile-time-K vector-store kernel,
    K=7 the generic runtime-K one."""
    from chunkflow_amd.fastconv import CfxConvIn155
    for bias in (True, False):
        ref, conv, x = _module_case(
            'c155', shape, 1, K, bf16, bias,
            lambda b: torch.nn.Conv3d(1, K, (1, 5, 5), padding=(0, 2, 2),
                                      bias=b))
        got = CfxConvIn155(conv, 0, bf16=bf16).cuda()(x)
        want, neg = ref.expect(bias)
        U.assert_exact(got, want, neg, f'conv_in K={K} {shape} bias={bias}')


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', U.CONV_OUT_SHAPES, ids=_id)
def test_conv_out_exact(shape, bf16):
    from chunkflow_amd.fastconv import CfxConvOut155
    for bias in (True, False):
        ref, conv, x = _module_case(
            'c155', shape, 28, 3, bf16, bias,
            lambda b: torch.nn.Conv3d(28, 3, (1, 5, 5), padding=(0, 2, 2),
                                      bias=b))
        got = CfxConvOut155(conv, 0, bf16=bf16).cuda()(x)
        want, neg = ref.expect(bias)
        U.assert_exact(got, want, neg, f'conv_out {shape} bias={bias}')


# --------------------------------------------------------------------------
# tier 2: real-valued inputs, the bf16 rounding points modelled in f64
# --------------------------------------------------------------------------
# Cap on the share of elements that are not bit-identical to the f64 model.
# An f32-accumulated CPU conv pushed through the same model, in two
# summation orders, disagrees with the f64 model on 0.7-2.1e-5 of the
# elements (the reference's own noise floor: f32 accumulation error landing
# on a bf16 rounding boundary). 1e-3 is ~50x that floor and ~100x below
# what one wrong product per output would cause.
NONIDENTICAL_CAP = 1e-3
REAL_SHAPE = (2, 5, 37, 41)


def _real_case(C, seed):
    torch.manual_seed(seed)
    n, d, h, w = REAL_SHAPE
    conv = torch.nn.Conv3d(C, C, 3, padding=1)
    x = (torch.randn(n, C, d, h, w) * 0.5).to(torch.bfloat16)
    r = (torch.randn(n, C, d, h, w) * 0.5).to(torch.bfloat16)
    wq = conv.weight.detach().to(torch.bfloat16)
    return conv, x, r, wq


def _run_real(conv, x, r):
    from chunkflow_amd.fastconv import CfxConv3dBF16
    m = CfxConv3dBF16(conv, 0).cuda()
    got = m._run(x.cuda().contiguous(memory_format=CL),
                 residual=r.cuda().contiguous(memory_format=CL), elu=True)
    torch.cuda.synchronize()
    return got.cpu()


def _check_real(got, ref, scale, what):
    """Within one bf16 ulp of max(|acc+bias|, |ref|) everywhere; share of
    non-bit-identical elements under the cap."""
    g = got.double()
    err = (g - ref).abs()
    ulp = U.bf16_ulp(torch.maximum(scale.abs(), ref.abs()))
    worst = float((err / ulp).max())
    share = float((g != ref).double().mean())
    print(f'{what}: non-identical share {share:.3e} '
          f'({int((g != ref).sum())} of {g.numel()}), '
          f'worst error {worst:.3f} bf16 ulp')
    assert worst <= 1.0, f'{what}: {worst} bf16 ulps'
    assert share < NONIDENTICAL_CAP, f'{what}: share {share}'


@gpu
def test_bf16_ring_real_rounding_model():
    """Default C=28 bf16 ring, fused bias+residual+ELU, random real bf16
    inputs, vs the f64 conv of the same rounded values pushed through the
    transposed epilogue's rounding points:
        out = bf16(elu(f32(bf16(acc + bias)) + res)).
    Observed on an MI355X: 6 of 424760 elements not bit-identical (share
    1.4e-5, inside the reference's own 0.7-2.1e-5 noise floor), worst
    error exactly 1 bf16 ulp."""
    conv, x, r, wq = _real_case(28, 101)
    acc = U.cpu_conv('c333', x, wq, torch.float64)
    ab = acc + conv.bias.detach().double().view(1, -1, 1, 1, 1)
    ref = U.bf16_round(U.elu64(U.bf16_round(ab) + r.double()))
    _check_real(_run_real(conv, x, r), ref, ab, 'bf16 ring C=28')


@gpu
def test_bf16_sliced_ring_real_rounding_model():
    """Sliced C=36 bf16 ring (two input-channel halves chained through the
    bf16 output buffer), fused, random real bf16 inputs:
        p   = bf16(f32(bf16(acc[c 0..31])) + res)
        out = bf16(elu(f32(bf16(acc[c 32..35] + bias)) + p)).
    Observed on an MI355X: 1 of 546120 elements not bit-identical (share
    1.8e-6), worst error exactly 1 bf16 ulp."""
    C = 36
    conv, x, r, wq = _real_case(C, 102)
    acc_lo = U.cpu_conv('c333', x[:, :32], wq[:, :32], torch.float64)
    acc_hi = U.cpu_conv('c333', x[:, 32:], wq[:, 32:], torch.float64)
    bias = conv.bias.detach().double().view(1, -1, 1, 1, 1)
    p = U.bf16_round(U.bf16_round(acc_lo) + r.double())
    ref = U.bf16_round(U.elu64(U.bf16_round(acc_hi + bias) + p))
    _check_real(_run_real(conv, x, r), ref, acc_lo + acc_hi + bias,
                'bf16 sliced ring C=36')
