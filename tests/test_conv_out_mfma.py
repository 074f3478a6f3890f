"""The MFMA 28 -> 3 (1,5,5) output conv (csrc/updown.hip,
k_conv155_out_mfma) at every tile seam of the kernel as built.

The kernel folds the five x-taps into the MFMA's output dimension
(column j = dx*3 + k, 16th column zero) and recombines them with a shifted
sum, so the shapes below walk W across the strip seams (S = 60 outputs per
workgroup, 64 staged, 16-position MFMA tiles) and H across the row seams
(R = 6 output rows per workgroup, 10 staged).

Tier 1 is bit-exact against the f64 CPU conv on small-integer inputs
(tests/conv_exact_util.py: f32 accumulation of these inputs is exact in any
order, so a re-ordered or fused sum must still match bit for bit). Tier 2
is real-valued f32 against the f64 CPU conv, bounded by the f32 CPU conv's
own accumulation noise. The column-packing test pins every (dy, dx, k)
column of the packed weights with impulses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact_util as U  # noqa: E402

gpu = pytest.mark.gpu
CL = torch.channels_last_3d

S = 60   # CO_S: output positions per workgroup
R = 6    # CO_R: output rows per workgroup
C, K = 28, 3

W_SHAPES = [(1, 1, R + 1, w)
            for w in (1, 2, 3, 4, 5, 15, 16, 17, S - 1, S, S + 1, S + 3,
                      2 * S + 1)]
H_SHAPES = [(1, 1, h, S + 1)
            for h in (1, 2, 3, R - 1, R, R + 1, 2 * R + 1)]
# plane index and plane stride; W % 4 == 0 takes the vector-store epilogue
# across a strip seam, (2, 3, 7, 61) the scalar one
PLANE_SHAPES = [(2, 3, R + 1, S + 1), (2, 3, R + 1, S + 4)]
SHAPES = list(dict.fromkeys(W_SHAPES + H_SHAPES + PLANE_SHAPES))
REAL_SHAPE = (2, 3, 2 * R + 1, S + 3)


def _id(v):
    return 'x'.join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _conv(bias=True):
    return torch.nn.Conv3d(C, K, (1, 5, 5), padding=(0, 2, 2), bias=bias)


def _run(conv, x, bf16=False):
    from chunkflow_amd.fastconv import CfxConvOut155
    dt = torch.bfloat16 if bf16 else torch.float32
    got = CfxConvOut155(conv, 0, bf16=bf16).cuda()(
        x.to(dt).cuda().contiguous(memory_format=CL))
    torch.cuda.synchronize()
    return got.cpu()


def test_exactness_premise_cpu():
    """Every tier-1 shape of this file, without a GPU: the f32 CPU conv of
    the integer inputs equals the f64 one (f32 accumulation is exact, hence
    order-independent), every value reaching the bf16 store is an integer
    of magnitude <= 256, bf16 holds every input exactly, and the weights
    are nonzero on every (dy, dx) tap for every k, so a dropped or
    mis-shifted tap column of the packed weights has to show."""
    assert len(SHAPES) == len(W_SHAPES) + len(H_SHAPES) + len(PLANE_SHAPES) - 1
    for shape in SHAPES:
        ref = U.reference('c155', shape, C, K)
        what = f'c155 {shape}'
        assert set(ref.x.unique().tolist()) <= {-2., -1., 0., 1., 2.}, what
        assert set(ref.w.unique().tolist()) <= {-1., 0., 1.}, what
        assert bool((ref.w[:, :, 0] != 0).any(dim=1).all()), what
        acc32 = U.cpu_conv('c155', ref.x, ref.w, torch.float32)
        np.testing.assert_array_equal(acc32.double().numpy(),
                                      ref.acc.numpy(), err_msg=what)
        assert torch.equal(ref.acc, ref.acc.round()), what
        assert ref.rounding_point_max() <= U.BF16_EXACT_MAX, \
            (what, ref.rounding_point_max())
        for t in (ref.x, ref.w, ref.b):
            assert torch.equal(t.to(torch.bfloat16).float(), t), what


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_conv_out_mfma_exact(shape, bf16):
    """Bit-equal to the f64 CPU conv, bias on and off. The weights are
    nonzero on every (dy, dx) tap (asserted in the CPU premise test)."""
    ref = U.reference('c155', shape, C, K)
    assert ref.rounding_point_max() <= U.BF16_EXACT_MAX
    for bias in (True, False):
        conv = _conv(bias)
        with torch.no_grad():
            conv.weight.copy_(ref.w)
            if bias:
                conv.bias.copy_(ref.b)
        got = _run(conv, ref.x, bf16)
        want, neg = ref.expect(bias)
        U.assert_exact(got, want, neg,
                       f'conv_out mfma {shape} bf16={bf16} bias={bias}')


@gpu
def test_conv_out_mfma_real_f32():
    """Random normal input and weights at (2, 3, 2R+1, S+3), f32, against
    the f64 CPU conv. The bound is 4x the max abs error of torch's f32 CPU
    conv against the same f64 result (the reference's own accumulation
    noise over the same 700 products; 4 is the margin for a different but
    equally long summation tree).
    Observed on an MI355X: kernel 6.6e-07, f32 CPU conv 2.1e-06 (ratio
    0.32)."""
    torch.manual_seed(155)
    n, d, h, w = REAL_SHAPE
    conv = _conv(True)
    x = torch.randn(n, C, d, h, w).contiguous(memory_format=CL)
    with torch.no_grad():
        want = conv.double()(x.double())
        conv = conv.float()
        noise = float((conv(x).double() - want).abs().max())
    err = float((_run(conv, x).double() - want).abs().max())
    print(f'conv_out mfma real f32: kernel max abs err {err:.3e}, '
          f'f32 CPU conv max abs err {noise:.3e}, ratio {err / noise:.2f}')
    assert noise > 0
    assert err <= 4 * noise, (err, noise)


@gpu
def test_conv_out_mfma_column_packing():
    """One nonzero weight w[k, c, dy, dx] = 1 and one impulse in[c] = 1 at
    (y0, x0): the only nonzero output is 1 at (k, y0 - dy + 2, x0 - dx + 2).
    All 5x5 taps x 3 output channels, c in {0, 27}; pins j = dx*3 + k and
    the zero 16th column (nothing may leak into any other output). The
    impulse sits next to a strip seam and a row seam so the shifted outputs
    land in both workgroups."""
    h, w = R + 5, S + 6
    y0, x0 = R, S + 1
    for c in (0, C - 1):
        x = torch.zeros(1, C, 1, h, w)
        x[0, c, 0, y0, x0] = 1.
        xg = x.cuda().contiguous(memory_format=CL)
        for dy in range(5):
            for dx in range(5):
                for k in range(K):
                    from chunkflow_amd.fastconv import CfxConvOut155
                    conv = _conv(False)
                    with torch.no_grad():
                        conv.weight.zero_()
                        conv.weight[k, c, 0, dy, dx] = 1.
                    got = CfxConvOut155(conv, 0).cuda()(xg).cpu()
                    want = torch.zeros(1, K, 1, h, w)
                    want[0, k, 0, y0 - dy + 2, x0 - dx + 2] = 1.
                    assert torch.equal(got, want), \
                        (c, dy, dx, k, got.nonzero().tolist())
