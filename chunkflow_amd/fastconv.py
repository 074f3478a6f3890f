"""Graph surgery: swap eligible nn.Conv3d modules for the hand-written
gfx950 MFMA conv kernel (csrc/conv.hip).

Eligible: kernel (3,3,3), stride 1, padding 1, dilation 1, groups 1,
in_channels == out_channels in {28, 36, 48, 64} — the RSUNet ResBlock
convs, ~85% of the affinity UNet's FLOPs. Everything else stays on
MIOpen. Enabled in the pytorch engine via CFX_FASTCONV (see engine);
weights are repacked once to the kernel's (27, C, K) tap-major layout.

Also here: the up/down-sampling and (1,5,5) conv swaps (csrc/updown.hip),
CfxMiopenResBlock, which gives the ResBlocks whose convs stay on MIOpen a
one-pass bias / residual / ELU epilogue, and the torch.fx pass that moves
the decoder's `up(x) + skip` add into the up-conv's epilogue
(fuse_up_skip_adds).

The surgery itself is one walker (_walk) over a table of rules (_groups):
a rule names which modules it takes, what replaces them and the input on
which the replacement has to reproduce the original (_probe) before it is
installed. accelerate_all runs every group in the engine's order.
"""
import os
from collections import namedtuple

import torch
import torch.nn as nn

_CTX = {}
_CL = torch.channels_last_3d


def get_cfx(device_index: int = 0):
    if device_index not in _CTX:
        from .hip import CfxContext
        ctx = CfxContext(device_index)
        ctx.adopt_torch_stream()
        _CTX[device_index] = ctx
    return _CTX[device_index]


def _ptr(t):
    """device address of an optional tensor (None is the C-ABI's NULL)"""
    return None if t is None else t.data_ptr()


def _empty_cl(x, shape, dtype):
    return torch.empty(shape, dtype=dtype, device=x.device,
                       memory_format=_CL)


class _CfxModule(nn.Module):
    """Base of every replacement module: the surgery never matches one."""

    def _bias_buffer(self, conv, name='bias'):
        b = conv.bias
        self.register_buffer(
            name, None if b is None else b.detach().float().contiguous())


class _CfxConv(_CfxModule):
    """Base of the single-conv drop-ins: widths, context index, dtype."""

    def __init__(self, conv, device_index, bf16):
        super().__init__()
        self.C, self.K = conv.in_channels, conv.out_channels
        self.device_index = device_index
        self.bf16 = bf16
        self.dt = torch.bfloat16 if bf16 else torch.float32

    def _in(self, x):
        """x channels-last, checked to be of the module's dtype, and its
        n, d, h, w"""
        assert x.dtype == self.dt, f'{type(self).__name__} runs {self.dt}'
        x = x.contiguous(memory_format=_CL)
        n, _, d, h, w = x.shape
        return x, n, d, h, w


# --------------------------------------------------------------------------
# eligibility
# --------------------------------------------------------------------------
# widths where the hand kernel BEATS MIOpen (the persistent-z ring:
# C=28 88.6 vs 81.9 TF, C=36 69.5 vs 64.7; 48/64 stay on MIOpen — the
# weight wall no longer fits LDS beside the ring at those widths, and
# their spatial extents are small — DESIGN.md §10 ladder)
ELIGIBLE_WIDTHS = (28, 36)
ZRING_WIDTHS = (28, 36)

# bf16 ring widths on the hand kernels (measured,
# profiles/updown_probe_r02.json): C=28 594-624 TF (4x MIOpen), C=36
# sliced 249 TF (1.31x). C=48 sliced reaches 318 vs MIOpen's 344 raw and
# even with the fused ResBlock epilogue the same-box bench A/B reads
# 292.4/293.5 (C48 on) vs 297.1/296.5 (off) MV/s -- measured-rejected,
# kernel kept callable behind CFX_BF16_WIDTHS=28,36,48.
BF16_WIDTHS = tuple(
    int(w) for w in os.environ.get('CFX_BF16_WIDTHS', '28,36').split(',')
    if w)

# up-conv surgery allowlist. bf16 (measured, profiles/updown_probe_r02.json):
# the hand up-conv wins at in_channels 36 (7.1x) and ties at 48; it loses
# at 64 (32^2 extent). f32 (profiles/upskip_probe.json, 12 x 20 patches, up
# + skip-add): the MFMA up-conv with the add in its epilogue takes 0.73 ms
# at 36 (5.6 TB/s; VALU kernel + torch add 2.0 ms), 0.26 ms at 48 (0.86)
# and 0.09 ms at 64, where MIOpen + bias pass + add took 0.31 -- all three
# levels are on. The down shapes lose to MIOpen everywhere (0.03-0.25x)
# and keep it: no rule swaps them; CfxDownConv3d stays callable and
# GPU-tested for the record.
UP_SURGERY_WIDTHS = (36, 48)
UP_SURGERY_WIDTHS_F32 = (36, 48, 64)


def _is_conv(m, cls, kernel, stride, padding) -> bool:
    """The one shape predicate: a plain (undilated, ungrouped) conv of
    class `cls` with this kernel, stride and padding."""
    return (isinstance(m, cls)
            and m.kernel_size == kernel
            and m.stride == stride
            and m.padding == padding
            and m.dilation == (1, 1, 1)
            and m.groups == 1
            and m.output_padding == (0, 0, 0))


def _conv333(m, widths=None) -> bool:
    return (_is_conv(m, nn.Conv3d, (3, 3, 3), (1, 1, 1), (1, 1, 1))
            and m.in_channels == m.out_channels
            and (widths is None or m.in_channels in widths))


def _eligible(m: nn.Module) -> bool:
    return _conv333(m, ELIGIBLE_WIDTHS)


def _eligible_bf16(m: nn.Module) -> bool:
    return _conv333(m, BF16_WIDTHS)


def _block_like(m: nn.Module, conv_ok) -> bool:
    """The RSUNet ResBlock's attributes: conv1, conv2 (both `conv_ok`) and
    an ELU(alpha=1) `act`. Whether the forward is the ResBlock's too is the
    probe's business."""
    return (hasattr(m, 'conv1') and hasattr(m, 'conv2')
            and isinstance(getattr(m, 'act', None), nn.ELU)
            and getattr(m.act, 'alpha', None) == 1.0
            and not isinstance(m, _CfxModule)
            and conv_ok(m.conv1) and conv_ok(m.conv2))


def _resblock_like(m: nn.Module) -> bool:
    return _block_like(m, _eligible)


def _miopen_resblock_like(m: nn.Module) -> bool:
    return (_block_like(m, lambda c: _conv333(c) and not _eligible(c))
            and m.conv1.in_channels == m.conv2.in_channels)


def _up_eligible(m, bf16: bool = False) -> bool:
    widths = UP_SURGERY_WIDTHS if bf16 else UP_SURGERY_WIDTHS_F32
    return (_is_conv(m, nn.ConvTranspose3d, (1, 2, 2), (1, 2, 2), (0, 0, 0))
            and m.in_channels in widths
            and m.out_channels <= 64)


def _conv155(m) -> bool:
    return _is_conv(m, nn.Conv3d, (1, 5, 5), (1, 1, 1), (0, 2, 2))


def _conv155_eligible(m) -> bool:
    return _conv155(m) and m.in_channels == 1 and m.out_channels <= 32


def _conv155_out_eligible(m) -> bool:
    return _conv155(m) and m.in_channels == 28 and m.out_channels == 3


# --------------------------------------------------------------------------
# 3x3x3 ResBlock convs
# --------------------------------------------------------------------------
class CfxConv3d(_CfxConv):
    """Drop-in for an eligible nn.Conv3d; consumes/produces channels-last
    (NDHWC) tensors, exactly the memory format the engine runs in."""

    def __init__(self, conv: nn.Conv3d, device_index: int = 0):
        super().__init__(conv, device_index, False)
        w = conv.weight.detach()  # (K, C, 3, 3, 3)
        wtap = w.permute(2, 3, 4, 1, 0).reshape(27, self.C, self.K)
        self.register_buffer('wtap', wtap.contiguous().float())
        self._bias_buffer(conv)

    def _run(self, x, residual=None, elu=False):
        x, n, d, h, w = self._in(x)
        out = _empty_cl(x, (n, self.K, d, h, w), self.dt)
        get_cfx(self.device_index).conv3_ndhwc(
            x.data_ptr(), self.wtap.data_ptr(), _ptr(self.bias),
            _ptr(residual), out.data_ptr(), n, d, h, w, self.C, self.K,
            do_elu=elu, zring=self.C in ZRING_WIDTHS)
        return out

    forward = _run


class CfxConv3dBF16(_CfxConv):
    """bf16 drop-in for an eligible nn.Conv3d (config-5 path): the bf16
    persistent-z ring kernel on v_mfma_f32_32x32x16_bf16."""

    def __init__(self, conv: nn.Conv3d, device_index: int = 0):
        super().__init__(conv, device_index, True)
        w = conv.weight.detach().float()  # (K, C, 3, 3, 3)
        # C <= 32 uses the (27, 32, 32) pack of the single-tile ring;
        # 36/48 use the (27, 64, 48) pack of the sliced 4-launch schedule
        if self.C <= 32:
            pack = torch.zeros(27, 32, 32)
        else:
            pack = torch.zeros(27, 64, 48)
        pack[:, :self.K, :self.C] = w.permute(2, 3, 4, 0, 1) \
            .reshape(27, self.K, self.C)
        self.register_buffer('wpack', pack.to(torch.bfloat16).contiguous())
        self._bias_buffer(conv)

    def _run(self, x, residual=None, elu=False):
        x, n, d, h, w = self._in(x)
        out = _empty_cl(x, (n, self.K, d, h, w), self.dt)
        get_cfx(self.device_index).conv3_ndhwc_bf16(
            x.data_ptr(), self.wpack.data_ptr(), _ptr(self.bias),
            _ptr(residual), out.data_ptr(), n, d, h, w, self.C, self.K,
            do_elu=elu)
        return out

    forward = _run


class CfxResBlock(_CfxModule):
    """Fused replacement for the RSUNet ResBlock pattern (conv1 -> ELU ->
    conv2 -> +x -> ELU): the ELU and residual-add run in the conv
    epilogues, removing three full-tensor elementwise passes per block."""
    conv_cls = CfxConv3d

    def __init__(self, block: nn.Module, device_index: int = 0):
        super().__init__()
        self.c1 = self.conv_cls(block.conv1, device_index)
        self.c2 = self.conv_cls(block.conv2, device_index)

    def forward(self, x):
        x = x.contiguous(memory_format=_CL)
        h = self.c1._run(x, elu=True)
        return self.c2._run(h, residual=x, elu=True)


class CfxResBlockBF16(CfxResBlock):
    conv_cls = CfxConv3dBF16


class CfxMiopenResBlock(_CfxModule):
    """The RSUNet ResBlock pattern at the widths whose 3x3x3 convs stay on
    MIOpen (not in ELIGIBLE_WIDTHS): the convs run without bias, so torch
    launches no bias pass, and one in-place stream kernel per conv
    (csrc/updown.hip k_bias_res_elu) does bias + ELU, resp. bias +
    residual + ELU -- instead of a bias pass, an ELU pass and an add pass
    over the full tensor. f32 only."""

    def __init__(self, block: nn.Module, device_index: int = 0):
        super().__init__()
        self.C = block.conv1.in_channels
        self.device_index = device_index
        for i, conv in ((1, block.conv1), (2, block.conv2)):
            self.register_buffer(f'w{i}', conv.weight.detach())
            self._bias_buffer(conv, f'b{i}')

    def _conv(self, x, w, b, res):
        y = torch.nn.functional.conv3d(x, w, None, padding=1)
        y = y.contiguous(memory_format=_CL)
        n, k, d, h, wd = y.shape
        get_cfx(self.device_index).bias_res_elu(
            y.data_ptr(), _ptr(b), _ptr(res), n * d * h * wd, k,
            do_elu=True)
        return y

    def forward(self, x):
        assert x.dtype == torch.float32, 'fastconv is the f32 path'
        x = x.contiguous(memory_format=_CL)
        h = self._conv(x, self.w1, self.b1, None)
        return self._conv(h, self.w2, self.b2, x)


# --------------------------------------------------------------------------
# up/down-sampling convs: the RSUNet (1,2,2)-kernel, (1,2,2)-stride shapes
# are HBM-streaming work; csrc/updown.hip replaces MIOpen's implicit GEMM
# (bf16 bwd_data runs ~20x below the stream roofline there).
# --------------------------------------------------------------------------
class CfxUpConv3d(_CfxConv):
    """Drop-in for nn.ConvTranspose3d(kernel=(1,2,2), stride=(1,2,2))."""

    def __init__(self, conv: nn.ConvTranspose3d, device_index: int = 0,
                 bf16: bool = False):
        super().__init__(conv, device_index, bf16)
        w = conv.weight.detach().float()      # (C, K, 1, 2, 2)
        pack = w[:, :, 0].permute(2, 3, 0, 1).reshape(4, self.C, self.K)
        self.register_buffer('wpack', pack.to(self.dt).contiguous())
        self._bias_buffer(conv)

    def _fusable(self, skip, out_shape) -> bool:
        """The kernel adds `skip` in its epilogue when it is what the
        f32 MFMA up-conv streams: f32, channels-last contiguous, of the
        output's shape, 16-byte aligned (csrc/updown.hip um_eligible)."""
        return (not self.bf16 and torch.is_tensor(skip)
                and skip.dtype == torch.float32
                and skip.device == self.wpack.device
                and tuple(skip.shape) == tuple(out_shape)
                and skip.is_contiguous(memory_format=_CL)
                and skip.data_ptr() % 16 == 0
                and self.C % 4 == 0 and self.K % 4 == 0
                and self.C <= 64 and self.K <= 48)

    def forward(self, x, skip=None):
        """up(x), or up(x) + skip. The sum is bit-identical either way:
        fused, the add is the kernel's last f32 operation."""
        x, n, d, h, w = self._in(x)
        out = _empty_cl(x, (n, self.K, d, 2 * h, 2 * w), self.dt)
        fuse = (skip is not None and self._fusable(skip, out.shape)
                and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0)
        get_cfx(self.device_index).upconv_2x2_add(
            x.data_ptr(), self.wpack.data_ptr(), _ptr(self.bias),
            skip.data_ptr() if fuse else None,
            out.data_ptr(), n, d, h, w, self.C, self.K, bf16=self.bf16)
        if skip is not None and not fuse:
            return out + skip
        return out


class CfxDownConv3d(_CfxConv):
    """Drop-in for nn.Conv3d(kernel=(1,2,2), stride=(1,2,2))."""

    def __init__(self, conv: nn.Conv3d, device_index: int = 0,
                 bf16: bool = False):
        super().__init__(conv, device_index, bf16)
        w = conv.weight.detach().float()      # (K, C, 1, 2, 2)
        pack = w[:, :, 0].permute(2, 3, 1, 0).reshape(4, self.C, self.K)
        self.register_buffer('wpack', pack.to(self.dt).contiguous())
        self._bias_buffer(conv)

    def forward(self, x):
        x, n, d, h, w = self._in(x)
        out = _empty_cl(x, (n, self.K, d, h // 2, w // 2), self.dt)
        get_cfx(self.device_index).downconv_2x2(
            x.data_ptr(), self.wpack.data_ptr(), _ptr(self.bias),
            out.data_ptr(), n, d, h, w, self.C, self.K, bf16=self.bf16)
        return out


# --------------------------------------------------------------------------
# the (1,5,5) input and output convs
# --------------------------------------------------------------------------
class CfxConvIn155(_CfxConv):
    """Drop-in for nn.Conv3d(1, K, (1,5,5), padding=(0,2,2)) — the RSUNet
    input conv. MIOpen's implicit GEMM degenerates on the single input
    channel (measured 38.8 ms bf16 / 6.8 ms f32 per batch-24 launch);
    csrc/updown.hip runs it as a GEMM on the f32 matrix cores (16 x of a
    row by the 25 taps, K <= 32 outputs; f32 accumulation, bf16 rounded
    once at the store): f32 12x20x256^2 0.405 ms, bf16 24x32x256^2
    1.02 ms, against 1.04 / 2.08 ms for the VALU stencil it replaces
    (profiles/conv_in_mfma.json). `wpack` is the plain [K][25] weight in
    the compute dtype; the kernel gathers its B fragments from it."""

    def __init__(self, conv: nn.Conv3d, device_index: int = 0,
                 bf16: bool = False):
        super().__init__(conv, device_index, bf16)
        w = conv.weight.detach().float()      # (K, 1, 1, 5, 5)
        self.register_buffer(
            'wpack', w.reshape(self.K, 25).to(self.dt).contiguous())
        self._bias_buffer(conv)

    def forward(self, x):
        assert x.shape[1] == 1
        x, n, d, h, w = self._in(x)
        out = _empty_cl(x, (n, self.K, d, h, w), self.dt)
        get_cfx(self.device_index).conv155_c1(
            x.data_ptr(), self.wpack.data_ptr(), _ptr(self.bias),
            out.data_ptr(), n, d, h, w, self.K, bf16=self.bf16)
        return out


class CfxConvOut155(_CfxConv):
    """Drop-in for nn.Conv3d(28, 3, (1,5,5), padding=(0,2,2)) — the
    RSUNet output conv. MIOpen's bf16 implicit GEMM degenerates on the
    tiny K (measured 38.6 ms per batch-24 launch vs 2.85 ms here;
    f32 at batch 12 x 20: 6.76 ms vs 1.29 ms, profiles/convout_mfma.json).
    28 -> 3 only: the five x-taps are folded into the MFMA's output
    dimension (csrc/updown.hip). f32 walks y with five rolling
    accumulators (1.05 ms, profiles/conv_in_mfma.json); bf16 runs the
    fixed 6-row tiles. Both use the same `wpack` and summation order."""

    def __init__(self, conv: nn.Conv3d, device_index: int = 0,
                 bf16: bool = False):
        super().__init__(conv, device_index, bf16)
        assert (self.C, self.K) == (28, 3), 'conv_out kernel is 28 -> 3'
        w = conv.weight.detach().float()      # (K, C, 1, 5, 5)
        if bf16:                              # the kernel multiplies in f32
            w = w.to(torch.bfloat16).float()
        # B fragments of the 35 K-steps: [dy*7 + c//4][(c%4)*16 + j] with
        # j = dx*3 + k and a zero 16th column
        pack = w[:, :, 0].permute(2, 1, 3, 0).reshape(5, 28, 15)
        pack = torch.nn.functional.pad(pack, (0, 1)).reshape(35, 64)
        self.register_buffer('wpack', pack.contiguous())
        self._bias_buffer(conv)

    def forward(self, x):
        assert x.shape[1] == self.C
        assert self.wpack.dtype == torch.float32
        x, n, d, h, w = self._in(x)
        out = _empty_cl(x, (n, self.K, d, h, w), self.dt)
        get_cfx(self.device_index).conv155_out(
            x.data_ptr(), self.wpack.data_ptr(), _ptr(self.bias),
            out.data_ptr(), n, d, h, w, self.C, self.K, bf16=self.bf16)
        return out


# --------------------------------------------------------------------------
# the surgery: rules, probe, walker
# --------------------------------------------------------------------------
# match(m) says whether the rule takes a module, build(m, device_index)
# makes its replacement, shape(m) is the probe input (None: installed
# unprobed). A block rule whose probe fails falls back to swapping the
# block's conv1 and conv2 for `fallback`, unprobed.
_Rule = namedtuple('_Rule', 'match build shape fallback',
                   defaults=(None, None))


def _block_shape(block):
    return (1, block.conv1.in_channels, 4, 18, 22)


def _shape155(m):
    return (1, m.in_channels, 3, 14, 19)


def _groups(bf16: bool = False):
    """The module-surgery groups in the engine's order. Each is walked on
    its own (the probes draw from the global generator in walk order); for
    a child the first matching rule of the walked group applies."""
    def of(cls):
        return lambda m, device_index: cls(m, device_index, bf16=bf16)

    if bf16:
        blocks = (_Rule(lambda m: _block_like(m, _eligible_bf16),
                        CfxResBlockBF16, _block_shape, CfxConv3dBF16),
                  _Rule(_eligible_bf16, CfxConv3dBF16))
    else:
        blocks = (_Rule(_resblock_like, CfxResBlock, _block_shape,
                        CfxConv3d),
                  _Rule(_miopen_resblock_like, CfxMiopenResBlock,
                        _block_shape),
                  _Rule(_eligible, CfxConv3d))
    return {
        'resblock': blocks,
        'updown': (_Rule(lambda m: _up_eligible(m, bf16), of(CfxUpConv3d),
                         lambda m: (1, m.in_channels, 3, 12, 16)),),
        'conv_in': (_Rule(_conv155_eligible, of(CfxConvIn155), _shape155),),
        'conv_out': (_Rule(_conv155_out_eligible, of(CfxConvOut155),
                           _shape155),),
    }


@torch.no_grad()
def _probe(orig, repl, shape, dev, bf16, tol) -> bool:
    """Functional probe at surgery time: the replacement must reproduce the
    original forward on a random input (guards against user modules that
    merely LOOK like a ResBlock, and against a kernel that is wrong on
    this machine)."""
    x = torch.randn(*shape, device=dev)
    if bf16:
        x = x.to(torch.bfloat16)
    x = x.contiguous(memory_format=_CL)
    want = orig.to(dev)(x).float()
    got = repl(x).float()
    return bool(torch.allclose(got, want, rtol=tol, atol=tol))


def _walk(model: nn.Module, rules, dev, device_index: int = 0,
          bf16: bool = False) -> int:
    """Apply one group of rules in-place; returns the replacement count."""
    tol = 0.05 if bf16 else 1e-4
    count = 0
    detached = set()  # swapped-out originals (their convs must not re-count)
    for parent in list(model.modules()):  # snapshot: we mutate the tree
        if id(parent) in detached:
            continue
        for name, child in list(parent.named_children()):
            rule = next((r for r in rules if r.match(child)), None)
            if rule is None:
                continue
            repl = rule.build(child, device_index).to(dev)
            if rule.shape is None or _probe(child, repl, rule.shape(child),
                                            dev, bf16, tol):
                setattr(parent, name, repl)
                detached.add(id(child))
                count += 1
            elif rule.fallback is not None:
                # forward does something else: swap the lone convs
                for cn in ('conv1', 'conv2'):
                    setattr(child, cn,
                            rule.fallback(getattr(child, cn),
                                          device_index).to(dev))
                    count += 1
    return count


def _surgery(model, group, device_index, bf16) -> int:
    return _walk(model, _groups(bf16)[group], f'cuda:{device_index}',
                 device_index, bf16)


def maybe_accelerate(model: nn.Module, device_index: int = 0) -> int:
    """Replace eligible ResBlocks (fused) and lone convs in-place;
    returns the replacement count."""
    return _surgery(model, 'resblock', device_index, False)


def maybe_accelerate_bf16(model: nn.Module, device_index: int = 0) -> int:
    """bf16 surgery (widths where the bf16 ring is instantiated); same
    functional-probe guard as the f32 path."""
    return _surgery(model, 'resblock', device_index, True)


def accelerate_updown(model: nn.Module, device_index: int = 0,
                      bf16: bool = False) -> int:
    """Swap eligible up-sampling convs in-place; returns count."""
    return _surgery(model, 'updown', device_index, bf16)


def accelerate_conv_in(model: nn.Module, device_index: int = 0,
                       bf16: bool = False) -> int:
    """Swap the eligible single-channel (1,5,5) input convs; returns
    count."""
    return _surgery(model, 'conv_in', device_index, bf16)


def accelerate_conv_out(model: nn.Module, device_index: int = 0,
                        bf16: bool = False) -> int:
    """Swap the eligible 28 -> 3 (1,5,5) output convs for the MFMA kernel;
    returns count. It beats MIOpen at both dtypes (13.6x bf16, 5.2x f32,
    profiles/convout_mfma.json), so callers swap unconditionally."""
    return _surgery(model, 'conv_out', device_index, bf16)


def fuse_up_skip_adds(model: nn.Module, is_up=None):
    """torch.fx pass: rewrite `up(x) + other` to `up(x, other)` so the
    decoder's skip-add runs in the up-conv's epilogue. The add lives in
    the user's forward, out of module surgery's reach, so the root is
    traced with every non-container submodule as a leaf. A node matches
    when it is operator.add / torch.add / Tensor.add of two operands (no
    alpha), one of them the output of a module `is_up` accepts (default:
    CfxUpConv3d) called with one argument, and that output has no other
    user. Returns (model, count): a GraphModule sharing the original's
    submodules, or the model itself when nothing matched or it cannot be
    traced (e.g. tensor-dependent control flow)."""
    import operator

    import torch.fx as fx

    if is_up is None:
        def is_up(m):
            return isinstance(m, CfxUpConv3d)

    class _Tracer(fx.Tracer):
        def is_leaf_module(self, m, qualname):
            return not isinstance(m, (nn.ModuleList, nn.ModuleDict,
                                      nn.Sequential))

    try:
        graph = _Tracer().trace(model)
    except Exception:
        return model, 0
    mods = dict(model.named_modules())

    def up_call(n):
        return (isinstance(n, fx.Node) and n.op == 'call_module'
                and is_up(mods.get(n.target)) and len(n.args) == 1
                and not n.kwargs and len(n.users) == 1)

    count = 0
    for node in list(graph.nodes):
        is_add = (node.op == 'call_function'
                  and node.target in (operator.add, torch.add)) or \
                 (node.op == 'call_method' and node.target == 'add')
        if not is_add or len(node.args) != 2 or node.kwargs:
            continue
        a, b = node.args
        if up_call(a) and isinstance(b, fx.Node) and b is not a:
            up, other = a, b
        elif up_call(b) and isinstance(a, fx.Node) and a is not b:
            up, other = b, a
        else:
            continue
        # the rewrite makes `other` an input of the up call: it has to
        # be computed before it
        order = {n: i for i, n in enumerate(graph.nodes)}
        if order[other] > order[up]:
            continue
        up.args = (up.args[0], other)
        node.replace_all_uses_with(up)
        graph.erase_node(node)
        count += 1
    if count == 0:
        return model, 0
    try:
        graph.lint()
        return fx.GraphModule(model, graph), count
    except Exception:
        return model, 0


@torch.no_grad()
def accelerate_up_skip(model: nn.Module, device_index: int = 0,
                       in_channels: int = 1):
    """Run fuse_up_skip_adds on an f32 model after the module surgery and
    keep the rewrite only if it reproduces the model on two small inputs
    of different spatial size (two sizes catch a trace that baked a shape
    in). Returns (model, fused add count); on any failure the model comes
    back as it was."""
    dev = f'cuda:{device_index}'
    try:
        fused, count = fuse_up_skip_adds(model)
        if count == 0:
            return model, 0
        for shape in ((2, 16, 24), (3, 32, 16)):
            x = torch.randn(1, in_channels, *shape, device=dev).contiguous(
                memory_format=_CL)
            if not torch.allclose(fused(x), model(x), rtol=1e-4,
                                  atol=1e-4):
                return model, 0
        return fused, count
    except Exception:
        return model, 0


def accelerate_all(model: nn.Module, device_index: int = 0,
                   bf16: bool = False, in_channels: int = 1):
    """The engine's whole surgery: every group of _groups in order, then
    (f32 only) the decoder's `up(x) + skip` adds move into the up-conv's
    epilogue. Returns (model, swapped module count, fused add count); the
    model comes back as a GraphModule when adds were fused."""
    count = sum(_surgery(model, group, device_index, bf16)
                for group in _groups(bf16))
    upskip = 0
    if not bf16:
        model, upskip = accelerate_up_skip(model, device_index, in_channels)
    return model, count, upskip
