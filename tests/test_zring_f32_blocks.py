"""The f32 z-ring conv with the ragged output columns of C = 36 on 4x4
MFMA blocks: columns 32..35 are computed by v_mfma_f32_4x4x1_16b_f32 out of
the 16-wide tile's A fragment, their four k-slice partial sums are added
across lanes once per z, and four consecutive lanes store one position's 16
bytes. C=36 runs as two launches (columns 0..15 + 32..35, then 16..31).
C=28 keeps its two 16-wide tiles (three block tiles for columns 16..27
measured slower) and runs the same cases through the same kernel template.

Tier 1 is exact: the integer cases of tests/conv_exact_util.py bit for bit
against the f64 CPU conv on shapes no other table holds, the scalar wall
staging of a misaligned weight tensor, and a centre-tap identity conv that
must return its input, which pins which lane owns which (position, column).
Tier 2 is one real-valued case under the project's f32 MFMA chain bound,
with the largest ratio printed per column group."""
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
# first column of the last column group: the second 16-wide tile at C=28,
# the 4-wide block tile at C=36
LAST_GROUP = {28: (16, 'second 16-wide tile'), 36: (32, 'block tile')}
SHAPES = [
    (1, 1, 3, 13),    # under one tile, D=1; W=13 leaves a position group
                      # (x = 12..15) with one valid lane
    (2, 2, 10, 19),   # batch, ragged y and x seams, D=2
    (1, 4, 24, 48),   # tile (y0=8, x0=16) is xy_interior; the ring wraps
]
UNALIGNED_SHAPE = (1, 2, 8, 20)
IDENTITY_SHAPE = (1, 2, 9, 21)
REAL_SHAPE = (1, 4, 11, 35)
REAL_FACTOR = 4e-7


def _id(v):
    if isinstance(v, tuple):
        return 'x'.join(str(i) for i in v)
    return str(v)


def test_block_shapes_keep_the_exactness_premise_cpu():
    """The shapes added here stay inside the exact-integer regime the
    bit-for-bit comparison rests on, and no other table holds them."""
    import test_zring_f32_stalls as S
    tabled = set(U.C333_SHAPES) | set(S.SHAPES) | {S.UNALIGNED_SHAPE}
    for shape in SHAPES + [UNALIGNED_SHAPE]:
        assert shape not in tabled, shape
        for C in WIDTHS:
            ref = U.reference('c333', shape, C, C)
            acc32 = U.cpu_conv('c333', ref.x, ref.w, torch.float32)
            assert torch.equal(acc32.double(), ref.acc), (shape, C)
            assert ref.rounding_point_max() <= U.BF16_EXACT_MAX, (shape, C)
    # the identity case carries distinct integers below 2^24
    n, d, h, w = IDENTITY_SHAPE
    assert n * max(WIDTHS) * d * h * w < 2 ** 24


@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
@pytest.mark.parametrize('C', WIDTHS)
def test_zring_blocks_exact(C, shape):
    """All five flag combinations, bit-exact vs the f64 CPU conv."""
    U.check_c333('zring', C, shape)


@gpu
@pytest.mark.parametrize('C', WIDTHS)
def test_zring_blocks_exact_unaligned_weights(C):
    """The weight tensor starts 4 bytes into its buffer: the ring takes
    its scalar wall staging, which fills the block wall too, and must
    still be bit-exact for every flag combination."""
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
def test_zring_blocks_column_map(C):
    """Centre-tap identity weights, no bias: every x[n, c, z, y, x] is a
    distinct integer below 2^24 and the output must equal the input bit
    for bit, so a lane that finishes or stores the wrong (position, column)
    shows up by name."""
    from chunkflow_amd.fastconv import get_cfx
    n, d, h, w = IDENTITY_SHAPE
    numel = n * C * d * h * w
    x = (torch.arange(numel, dtype=torch.float32) + 1).view(n, d, h, w, C) \
        .permute(0, 4, 1, 2, 3)               # NCDHW view of NDHWC memory
    assert x.is_contiguous(memory_format=CL)
    wt = torch.zeros(C, C, 3, 3, 3)
    wt[torch.arange(C), torch.arange(C), 1, 1, 1] = 1.0
    xg = x.cuda().contiguous(memory_format=CL)
    wtap = wt.permute(2, 3, 4, 1, 0).reshape(27, C, C).contiguous().cuda()
    out = torch.full_like(xg, float('nan'))
    get_cfx(0).conv3_ndhwc(xg.data_ptr(), wtap.data_ptr(), None, None,
                           out.data_ptr(), n, d, h, w, C, C, do_elu=False,
                           zring=True)
    torch.cuda.synchronize()
    got = out.cpu()
    bad = (got.view(torch.int32) != x.view(torch.int32)).nonzero()
    if len(bad):
        # order the report by memory position: (n, z, y, x) then column
        bn, bc, bz, by, bx = bad.T
        key = (((bn * d + bz) * h + by) * w + bx) * C + bc
        bn, bc, bz, by, bx = bad[key.argmin()].tolist()
        raise AssertionError(
            f'C={C}: {len(bad)} wrong elements, first at position '
            f'(n={bn}, z={bz}, y={by}, x={bx}) column {bc}: got '
            f'{got[bn, bc, bz, by, bx].item()!r}, want '
            f'{x[bn, bc, bz, by, bx].item()!r}')


@gpu
@pytest.mark.parametrize('C', WIDTHS)
def test_zring_blocks_real_valued(C):
    """The inputs and the derivation of test_zring_real_valued: randn x,
    w, bias and residual with the fused flags against the f64 CPU conv,
    elementwise |got - want| <= 4e-7 (sum|x w| + |b| + |r|) over all
    columns. A block column is four chains of 27 C / 4 terms plus two
    adds, inside the K <= 1024 chain bound the factor was derived from.
    The largest ratio is printed per column group (when this was written:
    C=36 1.40e-7 on the 16-wide columns 0..31 and 7.4e-8 on the block
    columns 32..35; C=28 2.32e-7 on columns 0..15 and 2.3e-7 at most on
    16..27)."""
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
    ratio = (got - want).abs() / mag
    j4, what = LAST_GROUP[C]
    r16 = ratio[:, :j4].max().item()
    r4 = ratio[:, j4:].max().item()
    print(f'zring f32 blocks C={C} {REAL_SHAPE}: max |err| / '
          f'(sum|x w|+|b|+|r|) = {r16:.3e} on the 16-wide columns '
          f'0..{j4 - 1}, {r4:.3e} on the {what} columns {j4}..{C - 1} '
          f'(bound {REAL_FACTOR:.1e})')
    assert ratio.max().item() <= REAL_FACTOR, (r16, r4)
