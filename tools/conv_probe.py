"""A/B the hand-written MFMA conv vs torch/MIOpen per RSUNet shape, and
check numerics vs a float64 CPU reference."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from chunkflow_amd.fastconv import get_cfx

torch.backends.cudnn.benchmark = True
cl = torch.channels_last_3d

def probe(C, D, H, W, N=12, iters=10, w32=False, zring=False):
    torch.manual_seed(0)
    x = torch.randn(N, C, D, H, W, device='cuda').contiguous(memory_format=cl)
    wt = torch.randn(C, C, 3, 3, 3, device='cuda') * (1.0 / (27 * C) ** 0.5)
    bias = torch.randn(C, device='cuda') * 0.1
    wtap = wt.permute(2, 3, 4, 1, 0).reshape(27, C, C).contiguous()
    out = torch.empty_like(x)
    cfx = get_cfx(0)

    # numerics vs fp64 CPU
    ref = F.conv3d(x.double().cpu(), wt.double().cpu(), bias.double().cpu(),
                   padding=1)[:2]
    cfx.conv3_ndhwc(x.data_ptr(), wtap.data_ptr(), bias.data_ptr(), None,
                    out.data_ptr(), N, D, H, W, C, C, w32=w32, zring=zring)
    torch.cuda.synchronize()
    err = (out[:2].double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()

    def t_mine():
        t0 = time.perf_counter()
        for _ in range(iters):
            cfx.conv3_ndhwc(x.data_ptr(), wtap.data_ptr(), bias.data_ptr(),
                            None, out.data_ptr(), N, D, H, W, C, C, w32=w32, zring=zring)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    wm = wt.contiguous(memory_format=cl)
    def t_torch():
        t0 = time.perf_counter()
        for _ in range(iters):
            F.conv3d(x, wm, bias, padding=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    for _ in range(3):
        t_mine(); t_torch()
    tm, tt = t_mine(), t_torch()
    flops = 2.0 * 27 * C * C * N * D * H * W
    print({'C': C, 'w32': w32, 'zring': zring, 'shape': (N, D, H, W), 'err_vs_fp64': err,
           'rel': err / scale,
           'mine_ms': tm * 1e3, 'torch_ms': tt * 1e3,
           'mine_TF': flops / tm / 1e12, 'torch_TF': flops / tt / 1e12,
           'speedup': tt / tm}, flush=True)

def probe_zring(C, D, H, W, N=12, fused=False, iters=20, tag=''):
    """Time the f32 z-ring alone (drained queue, synchronized warm-up),
    plain (bias only) or fused (bias + residual + ELU), and print one JSON
    line. For an A/B, run this in one process per library build and
    alternate the builds; `tag` names the build in the line."""
    import json
    torch.manual_seed(0)
    x = torch.randn(N, C, D, H, W, device='cuda').contiguous(memory_format=cl)
    wt = torch.randn(C, C, 3, 3, 3, device='cuda') * (1.0 / (27 * C) ** 0.5)
    bias = torch.randn(C, device='cuda') * 0.1
    wtap = wt.permute(2, 3, 4, 1, 0).reshape(27, C, C).contiguous()
    res = torch.randn_like(x) if fused else None
    out = torch.empty_like(x)
    cfx = get_cfx(0)

    def run():
        cfx.conv3_ndhwc(x.data_ptr(), wtap.data_ptr(), bias.data_ptr(),
                        res.data_ptr() if fused else None, out.data_ptr(),
                        N, D, H, W, C, C, do_elu=fused, zring=True)

    for _ in range(5):
        run()
    torch.cuda.synchronize()
    passes = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        torch.cuda.synchronize()
        passes.append((time.perf_counter() - t0) / iters * 1e3)
    ms = min(passes)
    flops = 2.0 * 27 * C * C * N * D * H * W
    # per column group: the 16-wide MFMA tiles, then the 4-wide block tiles
    groups = {28: [(0, 16), (16, 28)],
              36: [(0, 16), (16, 32), (32, 36)]}.get(C, [(0, C)])
    print(json.dumps({
        'tag': tag, 'C': C, 'shape': [N, D, H, W], 'fused': fused,
        'ms': round(ms, 4), 'ms_passes': [round(p, 4) for p in passes],
        'TF': round(flops / ms / 1e9, 2),
        'checksum': float(out.double().sum().item()),
        'checksum_cols': {f'{a}..{b - 1}':
                          float(out[:, a:b].double().sum().item())
                          for a, b in groups}}), flush=True)


if __name__ == '__main__' and '--zring-stalls' in sys.argv:
    _tag = sys.argv[sys.argv.index('--zring-stalls') + 1]
    for _fused in (False, True):
        probe_zring(28, 20, 256, 256, fused=_fused, tag=_tag)
        probe_zring(36, 20, 128, 128, fused=_fused, tag=_tag)
    sys.exit(0)

if __name__ == '__main__' and '--bf16' not in sys.argv:
    probe(28, 20, 256, 256)
    probe(28, 20, 256, 256, w32=True)
    probe(28, 20, 256, 256, zring=True)
    probe(36, 20, 128, 128, zring=True)
    probe(36, 20, 128, 128)
    probe(48, 20, 64, 64)
    probe(64, 20, 32, 32)


def probe_bf16(C=28, D=20, H=256, W=256, N=24, iters=8):
    from chunkflow_amd.fastconv import CfxConv3dBF16
    torch.manual_seed(0)
    conv = torch.nn.Conv3d(C, C, 3, padding=1).cuda()
    m = CfxConv3dBF16(conv).cuda()
    x = (torch.randn(N, C, D, H, W, device='cuda') * 0.3) \
        .to(torch.bfloat16).contiguous(memory_format=cl)
    convb = conv.to(torch.bfloat16).to(memory_format=cl)
    got = m(x).float()
    ref = torch.nn.functional.conv3d(x, convb.weight, convb.bias,
                                     padding=1).float()
    err = (got - ref).abs().max().item()

    def t(f):
        torch.cuda.synchronize()  # drain the queue: un-synced warmup work
        t0 = time.perf_counter()  # was inflating 'mine' by ~7.5 ms/iter
        for _ in range(iters):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    for _ in range(3):
        m(x); torch.nn.functional.conv3d(x, convb.weight, convb.bias,
                                         padding=1)
    torch.cuda.synchronize()
    tm = t(lambda: m(x))
    tt = t(lambda: torch.nn.functional.conv3d(x, convb.weight, convb.bias,
                                              padding=1))
    flops = 2.0 * 27 * C * C * N * D * H * W
    print({'bf16': True, 'C': C, 'shape': (N, D, H, W),
           'err_vs_torch_bf16': err, 'mine_ms': tm * 1e3,
           'torch_ms': tt * 1e3, 'mine_TF': flops / tm / 1e12,
           'torch_TF': flops / tt / 1e12, 'speedup': tt / tm}, flush=True)


if __name__ == '__main__' and '--bf16' in sys.argv:
    probe_bf16(28, 32, 256, 256, N=24)
