"""Exact-arithmetic inputs, f64 CPU references and comparisons for the
hand-written conv kernels (used by tests/test_conv_exact.py and by the
bf16 C=28 ring test in tests/test_gpu_parity.py).

The idea: feed the kernels small-integer data. Every product and every
partial sum is then an integer far below 2^24, so f32 accumulation is exact
in ANY order, and as long as every value that passes through a bf16
rounding point is an integer of magnitude <= 256 (8 significant bits), the
bf16 roundings are identities too. The kernel output must then equal a
float64 CPU convolution bit for bit; the only inexact step left is the
device expm1f on the negative ELU branch, which gets a one-ulp-class
allowance. Nothing here touches the GPU except `run_c333`."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

CL = torch.channels_last_3d

# integers up to 2^8 are exact in bf16 (8 significant bits)
BF16_EXACT_MAX = 256

# (bias, residual, elu) combinations run for every 3x3x3 path
FLAGS = {
    'plain': (True, False, False),
    'elu': (True, False, True),
    'fused': (True, True, True),
    'res_noelu': (True, True, False),
    'nobias': (False, False, False),
}

# ---- the case table ------------------------------------------------------
# 3x3x3 kernels: ring/slab tile seams are TY in {8,4,2}, TX in {32,16}
C333_SHAPES = [
    (2, 4, 11, 35),   # ragged y and x tiles, seams, ring wrap, batch stride
    (1, 1, 1, 1),     # degenerate everything (D=1: prologue-only ring)
    (1, 2, 8, 32),    # D=2, exactly one full TX=32 tile, no ragged edge
    (1, 3, 18, 67),   # tile (y0=8, x0=32) takes the xy_interior fast path
]
C333_PATHS = [
    ('slab', 28), ('slab', 36), ('slab', 48), ('slab', 64),
    ('w32', 28),
    ('zring', 28), ('zring', 36), ('zring', 48),
    ('bf16', 28), ('bf16', 36), ('bf16', 48),
]
UP_WIDTHS = [(36, 28), (48, 36), (64, 48)]
UP_SHAPES = [(2, 2, 2, 67), (1, 1, 1, 1)]          # XI=64, 8 x per thread
DOWN_WIDTHS = [(28, 36), (36, 48)]
DOWN_SHAPES = [(2, 2, 4, 134), (1, 1, 2, 2)]       # XO=64
CONV_IN_K = [28, 7]                                # 7: the generic-K path
CONV_IN_SHAPES = [(2, 2, 3, 259), (1, 1, 1, 1)]    # XI=256, 1 row per WG
CONV_OUT_SHAPES = [(2, 2, 6, 131), (1, 1, 1, 1)]   # XI=128, 4 rows, halo 2


def all_cases():
    """Every (kind, shape, C, K) the GPU tests use, once each."""
    cases = []
    for C in sorted({c for _, c in C333_PATHS}):
        for shape in C333_SHAPES:
            cases.append(('c333', shape, C, C))
    for (C, K) in UP_WIDTHS:
        for shape in UP_SHAPES:
            cases.append(('up', shape, C, K))
    for (C, K) in DOWN_WIDTHS:
        for shape in DOWN_SHAPES:
            cases.append(('down', shape, C, K))
    for K in CONV_IN_K:
        for shape in CONV_IN_SHAPES:
            cases.append(('c155', shape, 1, K))
    for shape in CONV_OUT_SHAPES:
        cases.append(('c155', shape, 28, 3))
    return cases


def case_seed(shape, C, K):
    n, d, h, w = shape
    return ((C * 131 + K) * 131 + n * 7 + d) * 4099 + h * 521 + w


_WSHAPE = {
    'c333': lambda C, K: (K, C, 3, 3, 3),
    'c155': lambda C, K: (K, C, 1, 5, 5),
    'down': lambda C, K: (K, C, 1, 2, 2),
    'up': lambda C, K: (C, K, 1, 2, 2),       # ConvTranspose3d layout
}


def out_shape(kind, shape, K):
    n, d, h, w = shape
    if kind == 'up':
        return (n, K, d, 2 * h, 2 * w)
    if kind == 'down':
        return (n, K, d, h // 2, w // 2)
    return (n, K, d, h, w)


def exact_case(shape, C, K, seed, kind='c333'):
    """Integer-valued f32 CPU tensors (x, w, bias, residual) for one conv.

    x: values in {-2..2}, about 25% of the elements non-zero; w: dense in
    {-1, 0, 1}; bias in {-4..4}; residual (output-shaped) in {-8..8}.
    x and residual are channels-last-3d. `kind` picks the weight layout:
    'c333' / 'c155' / 'down' are nn.Conv3d weights (K, C, kd, kh, kw), 'up'
    is an nn.ConvTranspose3d weight (C, K, 1, 2, 2)."""
    n, d, h, w = shape
    g = torch.Generator().manual_seed(int(seed))

    def ri(lo, hi, size):
        return torch.randint(lo, hi + 1, size, generator=g).float()

    xs = (n, C, d, h, w)
    mag = ri(1, 2, xs) * (ri(0, 1, xs) * 2 - 1)          # {-2,-1,1,2}
    x = mag * (torch.rand(xs, generator=g) < 0.25)
    wt = ri(-1, 1, _WSHAPE[kind](C, K))
    b = ri(-4, 4, (K,))
    r = ri(-8, 8, out_shape(kind, shape, K))
    return (x.contiguous(memory_format=CL), wt, b,
            r.contiguous(memory_format=CL))


def cpu_conv(kind, x, wt, dtype):
    """The bare convolution (no bias) on the CPU in `dtype`."""
    x = x.to(dtype).contiguous()
    wt = wt.to(dtype).contiguous()
    if kind == 'c333':
        return F.conv3d(x, wt, padding=1)
    if kind == 'c155':
        return F.conv3d(x, wt, padding=(0, 2, 2))
    if kind == 'down':
        return F.conv3d(x, wt, stride=(1, 2, 2))
    if kind == 'up':
        return F.conv_transpose3d(x, wt, stride=(1, 2, 2))
    raise ValueError(kind)


class Ref:
    """Inputs + the float64 CPU accumulators of one case."""

    def __init__(self, kind, shape, C, K):
        self.kind, self.shape, self.C, self.K = kind, shape, C, K
        self.x, self.w, self.b, self.r = exact_case(
            shape, C, K, case_seed(shape, C, K), kind)
        self.acc = cpu_conv(kind, self.x, self.w, torch.float64)
        # the sliced bf16 schedule (C in {36, 48}) writes the partial sum
        # over input channels 0..31 (+ the user residual) through bf16
        self.acc_lo = None
        if kind == 'c333' and C > 32:
            self.acc_lo = cpu_conv(kind, self.x[:, :32], self.w[:, :32],
                                   torch.float64)

    def pre(self, bias, res):
        t = self.acc
        if bias:
            t = t + self.b.double().view(1, -1, 1, 1, 1)
        if res:
            t = t + self.r.double()
        return t

    def expect(self, bias=True, res=False, elu=False):
        """(f64 expected output, mask of negative-ELU-branch elements)."""
        t = self.pre(bias, res)
        if not elu:
            return t, torch.zeros_like(t, dtype=torch.bool)
        return torch.where(t > 0, t, torch.expm1(t)), t < 0

    def rounding_point_max(self):
        """Largest magnitude that reaches any bf16 rounding point, over
        every flag combination: the accumulator with and without bias,
        the final pre-activation, and for the sliced schedule the
        first-32-channel partial sum with and without the residual."""
        vals = [self.acc, self.pre(True, False), self.pre(True, True),
                self.pre(False, True)]
        if self.acc_lo is not None:
            vals += [self.acc_lo, self.acc_lo + self.r.double()]
        return max(float(v.abs().max()) for v in vals)


@functools.lru_cache(maxsize=None)
def reference(kind, shape, C, K):
    """One shared, read-only reference per case."""
    return Ref(kind, tuple(shape), C, K)


def assert_exact(got, want, neg, what=''):
    """`got` (f32 or bf16 tensor) equals the f64 `want` bit for bit, except
    where `neg` marks the negative ELU branch: there the value is expm1 of
    a negative integer and the device expm1f may differ from float64 by an
    f32 ulp, so those compare within 1 bf16 ulp (bf16) / 4 f32 ulps (f32)
    of the correctly rounded value."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape)
    bf16 = got.dtype == torch.bfloat16
    assert bf16 or got.dtype == torch.float32, got.dtype
    neg = neg.numpy()
    g64 = got.double().contiguous().numpy()
    w64 = want.contiguous().numpy()
    np.testing.assert_array_equal(g64[~neg], w64[~neg], err_msg=what)
    if not neg.any():
        return
    if bf16:
        wr = want.float().to(torch.bfloat16).contiguous()
        gb = got.contiguous().view(torch.int16).numpy().astype(np.int64)
        wb = wr.view(torch.int16).numpy().astype(np.int64)
        tol = 1
    else:
        wr = want.float().contiguous()
        gb = got.contiguous().view(torch.int32).numpy().astype(np.int64)
        wb = wr.view(torch.int32).numpy().astype(np.int64)
        tol = 4
    # same sign (both in [-1, 0)), so raw-bit distance == ulp distance
    ulps = np.abs(gb[neg] - wb[neg])
    assert ulps.max() <= tol, \
        f'{what}: negative ELU branch off by {ulps.max()} ulps (> {tol})'


def run_c333(path, ref, bias=True, res=False, elu=False):
    """Run one 3x3x3 kernel path on cuda:0 through the public Python entry
    points and return its output (NaN-poisoned first where the caller owns
    the buffer)."""
    from chunkflow_amd.fastconv import CfxConv3dBF16, get_cfx
    C = ref.C
    if path == 'bf16':
        conv = torch.nn.Conv3d(C, C, 3, padding=1, bias=bias)
        with torch.no_grad():
            conv.weight.copy_(ref.w)
            if bias:
                conv.bias.copy_(ref.b)
        m = CfxConv3dBF16(conv, 0).cuda()
        x = ref.x.to(torch.bfloat16).cuda().contiguous(memory_format=CL)
        r = ref.r.to(torch.bfloat16).cuda().contiguous(memory_format=CL) \
            if res else None
        out = m._run(x, residual=r, elu=elu)
        torch.cuda.synchronize()
        return out
    n, d, h, w = ref.shape
    x = ref.x.cuda().contiguous(memory_format=CL)
    wtap = ref.w.permute(2, 3, 4, 1, 0).reshape(27, C, C).contiguous().cuda()
    b = ref.b.cuda() if bias else None
    r = ref.r.cuda().contiguous(memory_format=CL) if res else None
    out = torch.full_like(x, float('nan'))
    get_cfx(0).conv3_ndhwc(
        x.data_ptr(), wtap.data_ptr(),
        b.data_ptr() if b is not None else None,
        r.data_ptr() if r is not None else None, out.data_ptr(),
        n, d, h, w, C, C, do_elu=elu, w32=(path == 'w32'),
        zring=(path == 'zring'))
    torch.cuda.synchronize()
    return out


def check_c333(path, C, shape, flags=None):
    """All flag combinations of one path at one shape, bit-exact vs f64."""
    ref = reference('c333', tuple(shape), C, C)
    assert ref.rounding_point_max() <= BF16_EXACT_MAX
    for name in (flags or FLAGS):
        bias, res, elu = FLAGS[name]
        got = run_c333(path, ref, bias, res, elu)
        want, neg = ref.expect(bias, res, elu)
        assert_exact(got, want, neg, f'{path} C={C} {shape} {name}')


# ---- real-valued tier: the bf16 rounding points, modelled ----------------
def bf16_round(t):
    """Round an f64 tensor the way the kernels do: to f32, then to bf16
    (round-to-nearest-even both times); returned as f64."""
    return t.float().to(torch.bfloat16).double()


def bf16_ulp(v):
    """Spacing of bf16 numbers at magnitude v (f64 tensor, v > 0)."""
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** -120)))
    return torch.exp2(e - 7)


def elu64(t):
    return torch.where(t > 0, t, torch.expm1(t))
