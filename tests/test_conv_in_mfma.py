"""The MFMA 1 -> K (1,5,5) input conv (csrc/updown.hip, k_conv155_in_mfma)
at every seam of the kernel as built.

The kernel is a GEMM over the 25 taps (padded to 28 = 7 MFMA steps) with K
padded to 32 columns: a workgroup stages (R+4) x (S+4) input values of one
(n, z) plane, wave w owns the 16-position tile column w of the strip and
walks the R rows; a tile's 16*K outputs leave as one contiguous run. So the
shapes walk W across the tile and strip seams, H across the row-group
seams, K across the column tiles and the vector/scalar store paths, and
n*d over several densely filled planes (a halo row must be zero, never a
row of the neighbouring plane). R, S are read from the source.

Tier 1 is bit-exact against the f64 CPU conv on small-integer inputs
(tests/conv_exact_util.py: f32 accumulation of these inputs is exact in any
order). The whole-allocation test calls the raw-pointer C-ABI with `out`
between guard bands. The non-finite test pins the zeroed padding taps and
columns. Tier 2 is real-valued against the f64 CPU conv."""
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


def parse_geometry(text):
    """(CI_R, CI_S) as updown.hip states them."""
    vals = []
    for name in ('CI_R', 'CI_S'):
        m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
        if not m:
            raise RuntimeError(f'updown.hip: {name} not found')
        vals.append(int(m.group(1)))
    return tuple(vals)


with open(SOURCE) as _f:
    R, S = parse_geometry(_f.read())
TILE = 16

W_SHAPES = [(1, 1, R + 1, w) for w in (1, 5, 15, TILE, 17, 35, S - 1, S + 3)]
H_SHAPES = [(1, 1, h, S + 3) for h in (1, 2, 3, R - 1, R, R + 1, 2 * R + 3)]
PLANE_SHAPE = (2, 3, R + 1, S + 3)      # n*d = 6 planes, filled densely
K_SHAPES = [(2, 2, R + 1, S + 3), (1, 1, 3, 17)]
KS = (28, 1, 3, 16, 17, 32)
# (shape, K, dense)
CASES = ([(s, 28, False) for s in dict.fromkeys(W_SHAPES + H_SHAPES)]
         + [(PLANE_SHAPE, 28, True), (PLANE_SHAPE, 17, True)]
         + [(s, k, False) for k in KS[1:] for s in K_SHAPES])
REAL_SHAPE = (2, 2, 2 * R + 3, S + 3)
# the project's f32 MFMA chain bound (REAL_FACTOR of
# tests/test_zring_f32_blocks.py, derived for chains <= 1024; 28 here)
REAL_FACTOR = 4e-7


def _id(v):
    if isinstance(v, tuple) and isinstance(v[0], tuple):
        s, k, dense = v
        return 'x'.join(map(str, s)) + f'-K{k}' + ('-dense' if dense else '')
    return str(v)


@functools.lru_cache(maxsize=None)
def _case(shape, K, dense):
    """(x, w, b, f64 conv without bias) of one exact case, shared and
    read-only. `dense`: every input element non-zero, in {-2, -1, 1, 2}."""
    ref = U.reference('c155', shape, 1, K)
    if not dense:
        return ref.x, ref.w, ref.b, ref.acc
    n, d, h, w = shape
    g = torch.Generator().manual_seed(U.case_seed(shape, 1, K) + 1)
    xs = (n, 1, d, h, w)
    x = (torch.randint(1, 3, xs, generator=g).float()
         * (torch.randint(0, 2, xs, generator=g).float() * 2 - 1))
    x = x.contiguous(memory_format=CL)
    return x, ref.w, ref.b, U.cpu_conv('c155', x, ref.w, torch.float64)


def _want(case, bias):
    x, w, b, acc = _case(*case)
    return acc + b.double().view(1, -1, 1, 1, 1) if bias else acc


def _conv(K, bias=True):
    return torch.nn.Conv3d(1, K, (1, 5, 5), padding=(0, 2, 2), bias=bias)


def _run(conv, x, bf16=False):
    from chunkflow_amd.fastconv import CfxConvIn155
    dt = torch.bfloat16 if bf16 else torch.float32
    got = CfxConvIn155(conv, 0, bf16=bf16).cuda()(
        x.to(dt).cuda().contiguous(memory_format=CL))
    torch.cuda.synchronize()
    return got.cpu()


def test_geometry_and_cases_cpu():
    """The constants parse, the tile divides the strip, and the case table
    holds the seams it claims."""
    assert S % TILE == 0 and S >= 2 * TILE and R >= 4
    ws = {c[0][3] for c in CASES}
    hs = {c[0][2] for c in CASES}
    assert {1, 5, 15, 16, 17, 35, S - 1, S + 3} <= ws
    assert {1, 2, 3, R - 1, R, R + 1, 2 * R + 3} <= hs
    assert {c[1] for c in CASES} == set(KS)
    assert any(c[2] and c[0][0] * c[0][1] >= 4 for c in CASES)


def test_exactness_premise_cpu():
    """Every tier-1 case, without a GPU: the f32 CPU conv of the integer
    inputs equals the f64 one, every value reaching a store is an integer
    of magnitude <= 256, bf16 holds every input exactly, and the dense
    cases have no zero input element."""
    for case in CASES:
        x, w, b, acc = _case(*case)
        what = f'c155 {case}'
        assert set(x.unique().tolist()) <= {-2., -1., 0., 1., 2.}, what
        if case[2]:
            assert bool((x != 0).all()), what
        assert set(w.unique().tolist()) <= {-1., 0., 1.}, what
        acc32 = U.cpu_conv('c155', x, w, torch.float32)
        np.testing.assert_array_equal(acc32.double().numpy(), acc.numpy(),
                                      err_msg=what)
        assert torch.equal(acc, acc.round()), what
        for bias in (True, False):
            assert float(_want(case, bias).abs().max()) <= U.BF16_EXACT_MAX
        for t in (x, w, b):
            assert torch.equal(t.to(torch.bfloat16).float(), t), what


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_conv_in_mfma_exact(case, bf16):
    """Bit-equal to the f64 CPU conv + bias, bias on and off."""
    shape, K, dense = case
    x, w, b, _ = _case(*case)
    for bias in (True, False):
        conv = _conv(K, bias)
        with torch.no_grad():
            conv.weight.copy_(w)
            if bias:
                conv.bias.copy_(b)
        got = _run(conv, x, bf16)
        want = _want(case, bias)
        U.assert_exact(got, want, torch.zeros_like(want, dtype=torch.bool),
                       f'conv_in mfma {case} bf16={bf16} bias={bias}')


@gpu
def test_conv_in_k33_is_an_error():
    """K = 33 is refused by the C-ABI, not launched."""
    from chunkflow_amd.hip import CfxError
    x = torch.zeros(1, 1, 1, 4, 4)
    with pytest.raises(CfxError, match='K <= 32'):
        _run(_conv(33), x)


GUARD = 64      # elements before and after `out`
PATTERN = 77.   # exact in bf16, not a value the cases produce next to 0


@gpu
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('off_out,off_in', [(0, 0), (1, 0), (0, 1)],
                         ids=['aligned', 'out_off1', 'in_off1'])
def test_conv_in_mfma_whole_allocation(off_out, off_in, bf16):
    """Raw-pointer C-ABI call with `out` a view between guard bands of an
    allocation prefilled with a pattern: the whole allocation is compared,
    so a stray or a missing write shows. `out` one element off a 16-byte
    boundary takes the scalar stores; `in` one element off is read with
    element loads either way."""
    from chunkflow_amd.fastconv import get_cfx
    case = (PLANE_SHAPE, 28, True)
    shape, K, _ = case
    n, d, h, w = shape
    x, wt, b, _ = _case(*case)
    dt = torch.bfloat16 if bf16 else torch.float32
    want = _want(case, True).permute(0, 2, 3, 4, 1).contiguous().view(-1)
    numel = want.numel()

    xbuf = torch.zeros(x.numel() + 8, dtype=dt, device='cuda')
    xin = xbuf[off_in:off_in + x.numel()]
    xin.copy_(x.permute(0, 2, 3, 4, 1).contiguous().view(-1).to(dt))
    buf = torch.full((2 * GUARD + numel + 8,), PATTERN, dtype=dt,
                     device='cuda')
    assert buf.data_ptr() % 16 == 0 and xbuf.data_ptr() % 16 == 0
    lo = GUARD + off_out
    out = buf[lo:lo + numel]
    assert (out.data_ptr() % 16 == 0) == (off_out == 0)
    wg = wt.reshape(K, 25).to(dt).contiguous().cuda()
    bg = b.float().cuda()
    get_cfx(0).conv155_c1(xin.data_ptr(), wg.data_ptr(), bg.data_ptr(),
                          out.data_ptr(), n, d, h, w, K, bf16=bf16)
    torch.cuda.synchronize()
    expect = torch.full((buf.numel(),), PATTERN, dtype=torch.float64)
    expect[lo:lo + numel] = want
    np.testing.assert_array_equal(buf.cpu().double().numpy(),
                                  expect.numpy())


@gpu
@pytest.mark.parametrize('K', [28, 17])
def test_conv_in_mfma_nonfinite_locality(K):
    """Real-valued input, every weight non-zero, one +inf and one NaN
    several tiles apart: the non-finite outputs are exactly those of
    torch's CPU conv, i.e. the 5x5 window of each clipped to the image in
    all K channels. A padding tap or column multiplied by a zero weight
    instead of being zeroed would spread them over the tile."""
    torch.manual_seed(1550 + K)
    h, w = R + 3, 2 * S + 5
    spots = [(1, 3, float('inf')), (R + 1, S + TILE + 20, float('nan'))]
    x = torch.randn(1, 1, 2, h, w)
    for (y, xx, v) in spots:
        x[0, 0, 1, y, xx] = v
    conv = _conv(K)
    with torch.no_grad():
        conv.weight.copy_(torch.where(conv.weight >= 0, 1., -1.)
                          * (conv.weight.abs() + 0.1))
        ref_bad = ~torch.isfinite(conv(x))
    window = torch.zeros(1, K, 2, h, w, dtype=torch.bool)
    for (y, xx, _) in spots:
        window[0, :, 1, max(y - 2, 0):y + 3, max(xx - 2, 0):xx + 3] = True
    assert torch.equal(ref_bad, window)
    got_bad = ~torch.isfinite(_run(conv, x))
    assert torch.equal(got_bad, window), \
        (got_bad & ~window).nonzero()[:8].tolist()


def _real_case(K=28):
    torch.manual_seed(1551)
    n, d, h, w = REAL_SHAPE
    conv = _conv(K)
    x = torch.randn(n, 1, d, h, w).contiguous(memory_format=CL)
    return conv, x


@gpu
def test_conv_in_mfma_real_f32():
    """Ragged W and H, random normal data: elementwise
    |got - want64| <= 4e-7 * (sum |x*w| + |b|), the project's f32 MFMA
    chain bound (derived for chains <= 1024; the chain here is 28)."""
    conv, x = _real_case()
    with torch.no_grad():
        c64 = _conv(28).double()
        c64.load_state_dict(conv.state_dict())
        want = c64(x.double())
        mag = torch.nn.functional.conv3d(
            x.double().abs(), c64.weight.abs(), padding=(0, 2, 2)) \
            + c64.bias.abs().view(1, -1, 1, 1, 1)
    err = (_run(conv, x).double() - want).abs()
    ratio = float((err / mag).max())
    print(f'conv_in mfma real f32: max abs err {float(err.max()):.3e}, '
          f'max err / (sum|x*w| + |b|) {ratio:.3e} (bound {REAL_FACTOR})')
    assert bool((err <= REAL_FACTOR * mag).all()), ratio


@gpu
def test_conv_in_mfma_real_bf16():
    """bf16 storage: inputs and weights widened exactly, f32 accumulation,
    one rounding at the store -- every element within 1 bf16 ulp of the f64
    result rounded once to bf16. Input, weights and bias are positive here:
    a mixed-sign sum that cancels far below its terms has a bf16 ulp
    smaller than the f32 accumulation error of those terms, a bound no
    f32-accumulating kernel can meet; the signs are the exact tier's."""
    conv, x = _real_case()
    x = (x.abs() + 0.5).contiguous(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(conv.weight.abs() + 0.05)
        conv.bias.copy_(conv.bias.abs())
        c64 = _conv(28).double()
        c64.weight.copy_(conv.weight.to(torch.bfloat16).double())
        c64.bias.copy_(conv.bias.double())
        want = c64(x.to(torch.bfloat16).double())
    got = _run(conv, x, bf16=True).double()
    ulps = (got - U.bf16_round(want)).abs() / U.bf16_ulp(want.abs())
    print(f'conv_in mfma real bf16: max distance {float(ulps.max()):.3f} '
          f'bf16 ulps, {int((ulps > 0).sum())} of {ulps.numel()} differ')
    assert float(ulps.max()) <= 1.0
