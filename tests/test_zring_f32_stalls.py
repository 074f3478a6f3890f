"""The f32 z-ring conv (C = 28, 36) after its stalls were taken out: the
residual reads now cross the per-z barrier and land under the last nine
taps, the bias is read once, the outputs of a z are finished in registers
before any store is issued, the plane staging is free of control flow (a
thread past the end of the plane re-stages its previous element) and the
weight wall is staged as one batch of float4 loads, with the scalar loop
kept for a weight tensor that is not 16-byte aligned.

None of that may change a bit of the result. Tier 1 runs the exact-integer
cases of tests/conv_exact_util.py, bit for bit against the f64 CPU conv,
on shapes the table of tests/test_conv_exact.py does not reach; tier 2 is
one real-valued case against the f64 CPU conv under the f32 MFMA chain
bound."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact_util as U  # noqa: E402

gpu = pytest.mark.gpu
CL = torch.channels_last_3d

WIDTHS = [28, 36]
SHAPES = [
    (1, 5, 8, 16),    # exactly one tile; D=5: the ring wraps past a full
                      # turn while residual loads cross the barrier every z
    (2, 3, 9, 17),    # tiles with one valid row / one valid column, batch
    (1, 6, 24, 48),   # tile (y0=8, x0=16) is xy_interior, D > 3
]
UNALIGNED_SHAPE = (1, 2, 16, 32)
REAL_SHAPE = (1, 4, 11, 35)
REAL_FACTOR = 4e-7


def _id(v):
    if isinstance(v, tuple):
        return 'x'.join(str(i) for i in v)
    return str(v)


def test_new_shapes_keep_the_exactness_premise_cpu():
    """The shapes added here stay inside the exact-integer regime the
    bit-for-bit comparison rests on, and none is already in the table."""
    for shape in SHAPES + [UNALIGNED_SHAPE]:
        assert shape not in U.C333_SHAPES
        for C in WIDTHS:
            ref = U.reference('c333', shape, C, C)
            acc32 = U.cpu_conv('c333', ref.x, ref.w, torch.float32)
            assert torch.equal(acc32.double(), ref.acc), (shape, C)
            assert ref.rounding_point_max() <= U.BF16_EXACT_MAX, (shape, C)


@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
@pytest.mark.parametrize('C', WIDTHS)
def test_zring_exact(C, shape):
    """All five flag combinations, bit-exact vs the f64 CPU conv."""
    U.check_c333('zring', C, shape)


@gpu
@pytest.mark.parametrize('C', WIDTHS)
def test_zring_exact_unaligned_weights(C):
    """The weight tensor starts 4 bytes into its buffer, so it is not
    16-byte aligned: the ring takes its scalar wall staging and must still
    be bit-exact, for every flag combination."""
    from chunkflow_amd.fastconv import get_cfx
    shape = UNALIGNED_SHAPE
    n, d, h, w = shape
    ref = U.reference('c333', shape, C, C)
    x = ref.x.cuda().contiguous(memory_format=CL)
    buf = torch.zeros(27 * C * C + 1, device='cuda')
    wtap = buf[1:].view(27, C, C)
    wtap.copy_(ref.w.permute(2, 3, 4, 1, 0).reshape(27, C, C))
    assert wtap.is_contiguous() and wtap.data_ptr() % 16 == 4
    b = ref.b.cuda()
    r = ref.r.cuda().contiguous(memory_format=CL)
    for name, (bias, res, elu) in U.FLAGS.items():
        out = torch.full_like(x, float('nan'))
        get_cfx(0).conv3_ndhwc(
            x.data_ptr(), wtap.data_ptr(),
            b.data_ptr() if bias else None,
            r.data_ptr() if res else None, out.data_ptr(),
            n, d, h, w, C, C, do_elu=elu, zring=True)
        torch.cuda.synchronize()
        want, neg = ref.expect(bias, res, elu)
        U.assert_exact(out, want, neg, f'unaligned wgt C={C} {name}')


@gpu
@pytest.mark.parametrize('C', WIDTHS)
def test_zring_real_valued(C):
    """randn x, w, bias and residual with the fused flags against the f64
    CPU conv: elementwise |got - want| <= 4e-7 (sum|x w| + |b| + |r|).
    f32 MFMA chains of K <= 1024 stay within 0.75-1.5e-7 sum|a b| (here
    K = 27 C <= 972) and ELU is 1-Lipschitz, so the factor leaves about
    2.5x margin. The largest observed ratio is printed (2.3e-7 at C=28,
    1.4e-7 at C=36 when this was written)."""
    from chunkflow_amd.fastconv import get_cfx
    n, d, h, w = REAL_SHAPE
    g = torch.Generator().manual_seed(1000 + C)
    x = torch.randn(n, C, d, h, w, generator=g).contiguous(memory_format=CL)
    wt = torch.randn(C, C, 3, 3, 3, generator=g)
    b = torch.randn(C, generator=g)
    r = torch.randn(n, C, d, h, w, generator=g).contiguous(memory_format=CL)

    x64, w64 = x.double().contiguous(), wt.double().contiguous()
    pre = F.conv3d(x64, w64, padding=1) + b.double().view(1, -1, 1, 1, 1) \
        + r.double()
    want = U.elu64(pre)
    mag = F.conv3d(x64.abs(), w64.abs(), padding=1) \
        + b.double().abs().view(1, -1, 1, 1, 1) + r.double().abs()

    xg = x.cuda().contiguous(memory_format=CL)
    wtap = wt.permute(2, 3, 4, 1, 0).reshape(27, C, C).contiguous().cuda()
    bg = b.cuda()
    rg = r.cuda().contiguous(memory_format=CL)
    out = torch.full_like(xg, float('nan'))
    get_cfx(0).conv3_ndhwc(xg.data_ptr(), wtap.data_ptr(), bg.data_ptr(),
                           rg.data_ptr(), out.data_ptr(), n, d, h, w, C, C,
                           do_elu=True, zring=True)
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert tuple(got.shape) == tuple(want.shape)
    assert torch.isfinite(got).all()
    ratio = ((got - want).abs() / mag).max().item()
    print(f'zring f32 C={C} {REAL_SHAPE}: max |err| / (sum|x w|+|b|+|r|) '
          f'= {ratio:.3e} (bound {REAL_FACTOR:.1e})')
    assert ratio <= REAL_FACTOR, ratio
