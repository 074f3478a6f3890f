"""The decoder skip-add fused into the f32 MFMA up-conv
(csrc/updown.hip k_upconv2_mfma, CfxUpConv3d.forward(x, skip)) and the
torch.fx pass that routes a model's `up(x) + skip` to it.

The fused add is the kernel's last f32 operation, so `up(x, skip)` must
equal `up(x) + skip` bit for bit; the exact tier pins the sum itself to the
float64 CPU reference on integer data. The fx pass is checked on the CPU
with a stand-in up module."""
import operator
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact_util as U  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
CL = torch.channels_last_3d

WIDTHS = [(36, 28), (48, 36), (64, 48)]
# (n, d, h, w): W no multiple of the 16-position tile; the degenerate
# case; a row that crosses a tile edge and, with 4 waves per workgroup
# walking tiles grid-stride, gives a wave its second tile
SHAPES = [(2, 2, 3, 21), (1, 1, 1, 1), (1, 2, 2, 67)]


def _id(v):
    if isinstance(v, tuple):
        return 'x'.join(str(i) for i in v)
    return str(v)


def _up(C, K, bias, seed):
    from chunkflow_amd.fastconv import CfxUpConv3d
    torch.manual_seed(seed)
    conv = nn.ConvTranspose3d(C, K, (1, 2, 2), stride=(1, 2, 2),
                              bias=bias).cuda()
    return conv, CfxUpConv3d(conv, 0, bf16=False).cuda()


# --------------------------------------------------------------------------
# the kernel
# --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
@pytest.mark.parametrize('C,K', WIDTHS, ids=_id)
def test_fused_equals_unfused_plus_add_bitwise(C, K, shape, bias):
    n, d, h, w = shape
    conv, up = _up(C, K, bias, 5)
    x = torch.randn(n, C, d, h, w, device='cuda').contiguous(
        memory_format=CL)
    skip = torch.randn(n, K, d, 2 * h, 2 * w, device='cuda').contiguous(
        memory_format=CL)
    assert up._fusable(skip, skip.shape)
    fused = up(x, skip)
    unfused = up(x) + skip
    assert torch.equal(fused, unfused)
    # and both are the transposed conv
    torch.testing.assert_close(fused, conv(x) + skip, rtol=1e-4, atol=1e-4)


@gpu
@pytest.mark.parametrize('shape', U.UP_SHAPES, ids=_id)
@pytest.mark.parametrize('C,K', WIDTHS, ids=_id)
def test_fused_exact_vs_f64(C, K, shape):
    """Integer inputs + the case's small-integer residual as the skip:
    every product and sum is exact in f32, so the fused output equals the
    float64 convolution + bias + skip bit for bit."""
    from chunkflow_amd.fastconv import CfxUpConv3d
    ref = U.reference('up', tuple(shape), C, K)
    for bias in (True, False):
        conv = nn.ConvTranspose3d(C, K, (1, 2, 2), stride=(1, 2, 2),
                                  bias=bias)
        with torch.no_grad():
            conv.weight.copy_(ref.w)
            if bias:
                conv.bias.copy_(ref.b)
        up = CfxUpConv3d(conv, 0, bf16=False).cuda()
        x = ref.x.cuda().contiguous(memory_format=CL)
        skip = ref.r.cuda().contiguous(memory_format=CL)
        assert up._fusable(skip, skip.shape)
        got = up(x, skip)
        want, neg = ref.expect(bias, res=True)
        U.assert_exact(got, want, neg,
                       f'up+skip {C}->{K} {shape} bias={bias}')


@gpu
def test_fallbacks_give_the_torch_result():
    """A skip the kernel does not stream (NCDHW-contiguous) and a width it
    does not take (17 -> 5) still return up(x) + skip."""
    conv, up = _up(36, 28, True, 6)
    x = torch.randn(2, 36, 2, 5, 9, device='cuda').contiguous(
        memory_format=CL)
    skip = torch.randn(2, 28, 2, 10, 18, device='cuda')  # NCDHW
    assert not up._fusable(skip, skip.shape)
    torch.testing.assert_close(up(x, skip), conv(x) + skip, rtol=1e-4,
                               atol=1e-4)

    conv, up = _up(17, 5, True, 7)
    x = torch.randn(2, 17, 2, 5, 9, device='cuda').contiguous(
        memory_format=CL)
    skip = torch.randn(2, 5, 2, 10, 18, device='cuda').contiguous(
        memory_format=CL)
    assert not up._fusable(skip, skip.shape)
    torch.testing.assert_close(up(x, skip), conv(x) + skip, rtol=1e-4,
                               atol=1e-4)


# --------------------------------------------------------------------------
# the fx pass, on the CPU with a stand-in up module
# --------------------------------------------------------------------------
class _StandInUp(nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.conv = conv

    def forward(self, x, skip=None):
        y = self.conv(x)
        return y if skip is None else y + skip


def _is_stand_in(m):
    return isinstance(m, _StandInUp)


def _rsunet():
    from chunkflow_amd.model_loader import load_source
    src = load_source(os.path.join(REPO, 'examples', 'nets', 'rsunet.py'))
    torch.manual_seed(0)
    return src.RSUNet().eval()


def _count_adds(gm):
    return sum(1 for n in gm.graph.nodes
               if (n.op == 'call_function'
                   and n.target in (operator.add, torch.add))
               or (n.op == 'call_method' and n.target == 'add'))


@torch.no_grad()
def test_fx_pass_rsunet_loses_three_adds_cpu():
    import torch.fx as fx
    from chunkflow_amd.fastconv import fuse_up_skip_adds
    net = _rsunet()
    for i in range(len(net.up)):
        net.up[i] = _StandInUp(net.up[i])
    x = torch.randn(1, 1, 2, 16, 24)
    want = net(x)

    class LeafTracer(fx.Tracer):
        def is_leaf_module(self, m, qualname):
            return not isinstance(m, nn.ModuleList)

    before = _count_adds(fx.GraphModule(net, LeafTracer().trace(net)))
    fused, count = fuse_up_skip_adds(net, _is_stand_in)
    assert count == 3 and before == 3
    assert _count_adds(fused) == 0
    for n in fused.graph.nodes:
        if n.op == 'call_module' and n.target.startswith('up.'):
            assert len(n.args) == 2
    assert torch.equal(fused(x), want)
    # a second spatial size: no shape was baked into the trace
    x2 = torch.randn(1, 1, 3, 32, 16)
    assert torch.equal(fused(x2), net(x2))


@torch.no_grad()
def test_fx_pass_leaves_an_up_output_with_a_second_user_cpu():
    from chunkflow_amd.fastconv import fuse_up_skip_adds

    class TwoUsers(nn.Module):
        def __init__(self):
            super().__init__()
            self.up = _StandInUp(nn.ConvTranspose3d(
                4, 4, (1, 2, 2), stride=(1, 2, 2)))

        def forward(self, x, s):
            u = self.up(x)
            return (u + s) * u

    class Operands(nn.Module):
        """every add spelling, both operand orders"""
        def __init__(self):
            super().__init__()
            self.a = _StandInUp(nn.ConvTranspose3d(
                4, 4, (1, 2, 2), stride=(1, 2, 2)))
            self.b = _StandInUp(nn.ConvTranspose3d(
                4, 4, (1, 2, 2), stride=(1, 2, 2)))
            self.c = _StandInUp(nn.ConvTranspose3d(
                4, 4, (1, 2, 2), stride=(1, 2, 2)))

        def forward(self, x, s):
            return torch.add(s, self.a(x)) * self.b(x).add(s) \
                + (self.c(x) + s)

    x = torch.randn(1, 4, 2, 3, 5)
    s = torch.randn(1, 4, 2, 6, 10)
    net = TwoUsers().eval()
    same, count = fuse_up_skip_adds(net, _is_stand_in)
    assert count == 0 and same is net
    net = Operands().eval()
    fused, count = fuse_up_skip_adds(net, _is_stand_in)
    assert count == 3
    assert torch.equal(fused(x, s), net(x, s))


@torch.no_grad()
def test_fx_pass_returns_untraceable_model_unchanged_cpu():
    from chunkflow_amd.fastconv import fuse_up_skip_adds

    class DataDependent(nn.Module):
        def __init__(self):
            super().__init__()
            self.up = _StandInUp(nn.ConvTranspose3d(
                4, 4, (1, 2, 2), stride=(1, 2, 2)))

        def forward(self, x, s):
            if x.sum() > 0:
                return self.up(x) + s
            return self.up(x) - s

    net = DataDependent().eval()
    same, count = fuse_up_skip_adds(net, _is_stand_in)
    assert count == 0 and same is net


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------
@gpu
@torch.no_grad()
def test_rewritten_rsunet_matches_surgery_only():
    """RSUNet after the engine's module surgery, with and without the fx
    rewrite of its skip-adds, on one 1x1x4x32x32 input."""
    from chunkflow_amd import fastconv as fc
    net = _rsunet().cuda().to(memory_format=CL)
    fc.maybe_accelerate(net, 0)
    n_up = fc.accelerate_updown(net, 0)
    fc.accelerate_conv_in(net, 0)
    fc.accelerate_conv_out(net, 0)
    x = torch.randn(1, 1, 4, 32, 32, device='cuda').contiguous(
        memory_format=CL)
    want = net(x)
    fused, count = fc.accelerate_up_skip(net, 0, in_channels=1)
    assert count == n_up == len(fc.UP_SURGERY_WIDTHS_F32)
    assert fused is not net
    torch.testing.assert_close(fused(x), want, rtol=1e-4, atol=1e-4)


@gpu
@torch.no_grad()
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_accelerate_all_is_the_five_passes_in_order(bf16):
    """accelerate_all against the public passes called one by one in the
    engine's order, on two copies of one RSUNet: equal counts, the same
    class at every module name and bit-equal outputs. 16 x 24 is the
    smallest input through all four levels; it leaves partial ring tiles
    at the top level and 2 x 3 at the bottom. Both surgeries start from
    the same generator state, so their probes see the same inputs."""
    import copy
    from chunkflow_amd import fastconv as fc
    net = _rsunet().cuda()
    if bf16:
        net = net.to(torch.bfloat16)
    net = net.to(memory_format=CL)
    one, two = copy.deepcopy(net), copy.deepcopy(net)

    torch.manual_seed(11)
    n = (fc.maybe_accelerate_bf16 if bf16 else fc.maybe_accelerate)(one, 0)
    n += fc.accelerate_updown(one, 0, bf16=bf16)
    n += fc.accelerate_conv_in(one, 0, bf16=bf16)
    n += fc.accelerate_conv_out(one, 0, bf16=bf16)
    n_add = 0
    if not bf16:
        one, n_add = fc.accelerate_up_skip(one, 0, 1)

    torch.manual_seed(11)
    two, m, m_add = fc.accelerate_all(two, 0, bf16, 1)

    assert (n, n_add) == (m, m_add) == ((8, 0) if bf16 else (12, 3))
    names = {k: type(v).__name__ for k, v in one.named_modules()}
    assert names == {k: type(v).__name__ for k, v in two.named_modules()}
    assert names['enc.0'] == ('CfxResBlockBF16' if bf16 else 'CfxResBlock')
    torch.manual_seed(12)
    x = torch.randn(1, 1, 3, 16, 24, device='cuda')
    if bf16:
        x = x.to(torch.bfloat16)
    x = x.contiguous(memory_format=CL)
    assert torch.equal(one(x), two(x))
