"""The 28 -> 3 (1,5,5) output conv walking y (csrc/updown.hip,
k_conv155_out_ywalk, the f32 route of cfx_conv155_out) at every seam of the
kernel as built.

A wave owns XO output positions (16 staged) and a segment of YS rows and
walks the input rows with five rolling accumulators; NW waves make a
workgroup. So H walks the roll-in and roll-out of the accumulators and a
segment seam, W the wave and workgroup seams (and the 60/64 seams of the
fixed-tile kernel, which still serves bf16), and n*d several densely filled
planes: a halo row must be zero, never a row of the neighbouring plane.
YS, XO, NW are read from the source.

Tier 1 is bit-exact against the f64 CPU conv on small-integer inputs
(tests/conv_exact_util.py). The whole-allocation test calls the raw-pointer
C-ABI with `out` between guard bands. Tier 2 is real-valued f32 with the
bound of tests/test_conv_out_mfma.py."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact_util as U  # noqa: E402

gpu = pytest.mark.gpu
CL = torch.channels_last_3d
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(_REPO, 'chunkflow_amd', 'csrc', 'updown.hip')
C, K = 28, 3


def parse_geometry(text):
    """(CY_YS, CY_XO, CY_NW) as updown.hip states them."""
    vals = []
    for name in ('CY_YS', 'CY_XO', 'CY_NW'):
        m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
        if not m:
            raise RuntimeError(f'updown.hip: {name} not found')
        vals.append(int(m.group(1)))
    return tuple(vals)


with open(SOURCE) as _f:
    YS, XO, NW = parse_geometry(_f.read())
WG = XO * NW    # output positions per workgroup

H_SHAPES = [(1, 1, h, XO + 1)
            for h in (1, 2, 4, 5, YS - 1, YS, YS + 1, 2 * YS + 3)]
W_SHAPES = [(1, 1, 6, w)
            for w in (1, 3, XO - 1, XO, XO + 1, WG, WG + 1, 59, 60, 61, 64,
                      131)]
PLANE_SHAPE = (2, 2, YS + 1, WG + 1)     # 4 planes, filled densely
# (shape, dense)
CASES = ([(s, False) for s in dict.fromkeys(H_SHAPES + W_SHAPES)]
         + [(PLANE_SHAPE, True)])
REAL_SHAPE = (2, 2, YS + 3, WG + 3)


def _id(v):
    if isinstance(v, tuple) and isinstance(v[0], tuple):
        return 'x'.join(map(str, v[0])) + ('-dense' if v[1] else '')
    return str(v)


@functools.lru_cache(maxsize=None)
def _case(shape, dense):
    """(x, w, b, f64 conv without bias), shared and read-only. `dense`:
    every input element non-zero, in {-2, -1, 1, 2}."""
    ref = U.reference('c155', shape, C, K)
    if not dense:
        return ref.x, ref.w, ref.b, ref.acc
    n, d, h, w = shape
    g = torch.Generator().manual_seed(U.case_seed(shape, C, K) + 1)
    xs = (n, C, d, h, w)
    x = (torch.randint(1, 3, xs, generator=g).float()
         * (torch.randint(0, 2, xs, generator=g).float() * 2 - 1))
    x = x.contiguous(memory_format=CL)
    return x, ref.w, ref.b, U.cpu_conv('c155', x, ref.w, torch.float64)


def _want(case, bias):
    x, w, b, acc = _case(*case)
    return acc + b.double().view(1, -1, 1, 1, 1) if bias else acc


def _conv(bias=True):
    return torch.nn.Conv3d(C, K, (1, 5, 5), padding=(0, 2, 2), bias=bias)


def _module(w, b):
    from chunkflow_amd.fastconv import CfxConvOut155
    conv = _conv(b is not None)
    with torch.no_grad():
        conv.weight.copy_(w)
        if b is not None:
            conv.bias.copy_(b)
    return CfxConvOut155(conv, 0).cuda()


def test_geometry_and_premise_cpu():
    """The constants parse; every tier-1 case is exact in f32 on the CPU
    (integers far below 2^24, so any summation order gives the f64 sum),
    the weights are non-zero on every (dy, dx) tap for every k, and the
    dense case has no zero input element."""
    assert XO + 4 == 16 and YS >= 5 and NW >= 1
    assert {c[0][2] for c in CASES} >= {1, 2, 4, 5, YS - 1, YS, YS + 1,
                                        2 * YS + 3}
    assert {c[0][3] for c in CASES} >= {1, 3, 59, 60, 61, 64, 131}
    for case in CASES:
        x, w, b, acc = _case(*case)
        what = f'c155 {case}'
        if case[1]:
            assert bool((x != 0).all()), what
            assert case[0][0] * case[0][1] >= 4
        assert bool((w[:, :, 0] != 0).any(dim=1).all()), what
        acc32 = U.cpu_conv('c155', x, w, torch.float32)
        np.testing.assert_array_equal(acc32.double().numpy(), acc.numpy(),
                                      err_msg=what)
        assert torch.equal(acc, acc.round()), what
        assert float(_want(case, True).abs().max()) < 2 ** 20


@gpu
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_conv_out_ywalk_exact(case):
    """f32, bit-equal to the f64 CPU conv + bias, bias on and off.
    W % 4 != 0 takes the scalar stores, W % 4 == 0 the 16-byte ones."""
    x, w, b, _ = _case(*case)
    for bias in (True, False):
        got = _module(w, b if bias else None)(x.cuda())
        torch.cuda.synchronize()
        want = _want(case, bias)
        U.assert_exact(got, want, torch.zeros_like(want, dtype=torch.bool),
                       f'conv_out ywalk {case} bias={bias}')


GUARD = 64
PATTERN = 77.


@gpu
@pytest.mark.parametrize('w,off_out', [(WG + 4, 0), (WG + 4, 1),
                                       (WG + 1, 0)],
                         ids=['vector', 'out_off1', 'ragged'])
def test_conv_out_ywalk_whole_allocation(w, off_out):
    """Raw-pointer C-ABI call, `out` a view between guard bands of an
    allocation prefilled with a pattern; the whole allocation is compared.
    Dense input in 4 planes, a segment seam in y, a workgroup seam in x."""
    from chunkflow_amd.fastconv import get_cfx
    case = ((2, 2, YS + 1, w), True)
    n, d, h, _ = case[0]
    x, wt, b, _ = _case(*case)
    m = _module(wt, b)
    want = _want(case, True).permute(0, 2, 3, 4, 1).contiguous().view(-1)
    numel = want.numel()
    xg = x.cuda().contiguous(memory_format=CL)
    buf = torch.full((2 * GUARD + numel + 8,), PATTERN, device='cuda')
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + off_out
    out = buf[lo:lo + numel]
    get_cfx(0).conv155_out(xg.data_ptr(), m.wpack.data_ptr(),
                           m.bias.data_ptr(), out.data_ptr(), n, d, h, w,
                           C, K, bf16=False)
    torch.cuda.synchronize()
    expect = torch.full((buf.numel(),), PATTERN, dtype=torch.float64)
    expect[lo:lo + numel] = want
    np.testing.assert_array_equal(buf.cpu().double().numpy(),
                                  expect.numpy())


@gpu
def test_conv_out_ywalk_nonfinite_locality():
    """Real-valued input, every weight non-zero, one +inf and one NaN in
    different waves' tiles and segments: the non-finite outputs are exactly
    those of torch's CPU conv, the 5x5 window of each clipped to the image
    in all 3 channels. A staged halo column or row that is not zeroed, or a
    tile seam that leaks, would add to them."""
    torch.manual_seed(1552)
    h, w = YS + 6, WG + 9
    spots = [(1, 3, 5, float('inf')), (YS + 2, WG + 2, 20, float('nan'))]
    x = torch.randn(1, C, 2, h, w)
    for (y, xx, c, v) in spots:
        x[0, c, 1, y, xx] = v
    conv = _conv()
    with torch.no_grad():
        conv.weight.copy_(torch.where(conv.weight >= 0, 1., -1.)
                          * (conv.weight.abs() + 0.1))
        ref_bad = ~torch.isfinite(conv(x))
    window = torch.zeros(1, K, 2, h, w, dtype=torch.bool)
    for (y, xx, _, _) in spots:
        window[0, :, 1, max(y - 2, 0):y + 3, max(xx - 2, 0):xx + 3] = True
    assert torch.equal(ref_bad, window)
    got = _module(conv.weight.detach(), conv.bias.detach())(
        x.cuda().contiguous(memory_format=CL)).cpu()
    got_bad = ~torch.isfinite(got)
    assert torch.equal(got_bad, window), \
        (got_bad ^ window).nonzero()[:8].tolist()


@gpu
def test_conv_out_ywalk_real_f32():
    """Random normal input and weights, ragged W and H over a segment and a
    workgroup seam, against the f64 CPU conv. The bound is that of
    tests/test_conv_out_mfma.py: 4x the max abs error of torch's f32 CPU
    conv against the same f64 result (the same 700 products summed in a
    different but equally long tree)."""
    torch.manual_seed(155)
    n, d, h, w = REAL_SHAPE
    conv = _conv(True)
    x = torch.randn(n, C, d, h, w).contiguous(memory_format=CL)
    with torch.no_grad():
        want = conv.double()(x.double())
        conv = conv.float()
        noise = float((conv(x).double() - want).abs().max())
    got = _module(conv.weight.detach(), conv.bias.detach())(x.cuda()).cpu()
    err = float((got.double() - want).abs().max())
    print(f'conv_out ywalk real f32: kernel max abs err {err:.3e}, '
          f'f32 CPU conv max abs err {noise:.3e}, ratio {err / noise:.2f}')
    assert noise > 0
    assert err <= 4 * noise, (err, noise)
