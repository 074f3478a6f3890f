"""A/B the round-2 kernels vs torch/MIOpen on the RSUNet shapes:
up/down-sampling convs (csrc/updown.hip) and the sliced bf16 ring
(C=36/48). Drained-queue timing (tools/conv_probe.py lesson). Writes JSON
to gpurun_out/updown_probe.json."""
# Two further modes:
# `--upskip OUT.json` instead times the decoder's up-conv + skip-add at the
# three config-2 levels: (a) the tree's up path (hand kernel where surgery
# takes the width, MIOpen otherwise) followed by the torch add, and, in a
# tree whose CfxUpConv3d takes a skip, (b) the fused call. Run it from the
# parent and the changed tree in turn for an alternated A/B.
# `--miopen-block OUT.json` times one C=48 ResBlock at 12 x 20 x 64^2 as
# torch runs it (MIOpen conv + bias pass, ELU pass, add pass) against
# CfxMiopenResBlock (bias-free conv + one in-place epilogue), alternated.
# `--conv155 OUT.json [--tree DIR]` times the two (1,5,5) convs alone at
# 12x20x256x256 f32 and 24x32x256x256 bf16, the package taken from DIR
# (another checkout, built) when given: one process per tree, alternated
# by the caller, for a kernel-alone A/B.
import json
import os
import sys
import time

_TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--tree' in sys.argv:
    _TREE = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1])
sys.path.insert(0, _TREE)
import torch
import torch.nn as nn

from chunkflow_amd.fastconv import (CfxUpConv3d, CfxDownConv3d,
                                    CfxConv3dBF16, CfxConvIn155,
                                    CfxConvOut155)

torch.backends.cudnn.benchmark = True
cl = torch.channels_last_3d
RES = {}


def timeit(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def probe_updown(kind, C, K, N, D, H, W, bf16):
    torch.manual_seed(0)
    dt = torch.bfloat16 if bf16 else torch.float32
    if kind == 'up':
        conv = nn.ConvTranspose3d(C, K, (1, 2, 2), stride=(1, 2, 2)).cuda()
        repl = CfxUpConv3d(conv, 0, bf16=bf16).cuda()
    else:
        conv = nn.Conv3d(C, K, (1, 2, 2), stride=(1, 2, 2)).cuda()
        repl = CfxDownConv3d(conv, 0, bf16=bf16).cuda()
    tconv = conv.to(dt).to(memory_format=cl)
    x = torch.randn(N, C, D, H, W, device='cuda').to(dt).contiguous(
        memory_format=cl)
    with torch.no_grad():
        want = tconv(x).float()
        got = repl(x).float()
        err = (got - want).abs().max().item()
        t_my = timeit(lambda: repl(x))
        t_to = timeit(lambda: tconv(x))
    name = f'{kind}_{C}to{K}_{"bf16" if bf16 else "f32"}_{H}x{W}'
    RES[name] = {'mine_ms': t_my * 1e3, 'torch_ms': t_to * 1e3,
                 'speedup': t_to / t_my, 'max_err': err}
    print(name, RES[name], flush=True)


def probe_sliced(C, N, D, H, W):
    torch.manual_seed(0)
    conv = nn.Conv3d(C, C, 3, padding=1).cuda()
    repl = CfxConv3dBF16(conv, 0).cuda()
    tconv = conv.to(torch.bfloat16).to(memory_format=cl)
    x = torch.randn(N, C, D, H, W, device='cuda').to(torch.bfloat16) \
        .contiguous(memory_format=cl)
    with torch.no_grad():
        want = tconv(x).float()
        got = repl._run(x).float()
        err = (got - want).abs().max().item()
        mean_err = (got - want).abs().mean().item()
        t_my = timeit(lambda: repl._run(x))
        t_to = timeit(lambda: tconv(x))
    useful_tf = 2.0 * 27 * C * C * N * D * H * W / 1e12
    RES[f'ring_bf16_C{C}_{H}x{W}'] = {
        'mine_ms': t_my * 1e3, 'torch_ms': t_to * 1e3,
        'speedup': t_to / t_my, 'useful_tf_mine': useful_tf / t_my,
        'useful_tf_torch': useful_tf / t_to,
        'max_err': err, 'mean_err': mean_err}
    print(f'ring_bf16_C{C}', RES[f'ring_bf16_C{C}_{H}x{W}'], flush=True)


def probe_conv155(N, D, H, W, bf16):
    torch.manual_seed(0)
    conv = nn.Conv3d(1, 28, (1, 5, 5), padding=(0, 2, 2)).cuda()
    repl = CfxConvIn155(conv, 0, bf16=bf16).cuda()
    dt = torch.bfloat16 if bf16 else torch.float32
    tconv = conv.to(dt).to(memory_format=cl)
    x = torch.randn(N, 1, D, H, W, device='cuda').to(dt).contiguous(
        memory_format=cl)
    with torch.no_grad():
        want = tconv(x).float()
        got = repl(x).float()
        err = (got - want).abs().max().item()
        t_my = timeit(lambda: repl(x))
        t_to = timeit(lambda: tconv(x))
    name = f'conv155_{"bf16" if bf16 else "f32"}_{N}x{D}x{H}x{W}'
    RES[name] = {'mine_ms': t_my * 1e3, 'torch_ms': t_to * 1e3,
                 'speedup': t_to / t_my, 'max_err': err}
    print(name, RES[name], flush=True)


def probe_conv155_out(N, D, H, W, bf16):
    torch.manual_seed(0)
    conv = nn.Conv3d(28, 3, (1, 5, 5), padding=(0, 2, 2)).cuda()
    repl = CfxConvOut155(conv, 0, bf16=bf16).cuda()
    dt = torch.bfloat16 if bf16 else torch.float32
    tconv = conv.to(dt).to(memory_format=cl)
    x = torch.randn(N, 28, D, H, W, device='cuda').to(dt).contiguous(
        memory_format=cl)
    with torch.no_grad():
        want = tconv(x).float()
        got = repl(x).float()
        err = (got - want).abs().max().item()
        t_my = timeit(lambda: repl(x))
        t_to = timeit(lambda: tconv(x))
    name = f'conv155_out_{"bf16" if bf16 else "f32"}_{N}x{D}x{H}x{W}'
    RES[name] = {'mine_ms': t_my * 1e3, 'torch_ms': t_to * 1e3,
                 'speedup': t_to / t_my, 'max_err': err}
    print(name, RES[name], flush=True)


def probe_conv155_alone(path, rounds=3):
    """conv_in (1 -> 28) and conv_out (28 -> 3) alone, drained-queue timing;
    GB/s is (in + out bytes) / best time."""
    res = {'tree': _TREE}
    for N, D, bf16 in ((12, 20, False), (24, 32, True)):
        dt = torch.bfloat16 if bf16 else torch.float32
        for name, C, K, cls in (('conv_in', 1, 28, CfxConvIn155),
                                ('conv_out', 28, 3, CfxConvOut155)):
            torch.manual_seed(0)
            conv = nn.Conv3d(C, K, (1, 5, 5), padding=(0, 2, 2)).cuda()
            repl = cls(conv, 0, bf16=bf16).cuda()
            x = torch.randn(N, C, D, 256, 256, device='cuda').to(dt) \
                .contiguous(memory_format=cl)
            nbytes = x.element_size() * N * D * 256 * 256 * (C + K)
            with torch.no_grad():
                ms = [timeit(lambda: repl(x), 20) * 1e3
                      for _ in range(rounds)]
                # a small slab against torch, as a sanity check of the run
                want = conv.to(dt)(x[:1, :, :2]).float()
                err = (repl(x[:1, :, :2].contiguous(memory_format=cl))
                       .float() - want).abs().max().item()
            key = f'{name}_{"bf16" if bf16 else "f32"}_{N}x{D}x256x256'
            res[key] = {'ms': ms, 'bytes_in_out': nbytes,
                        'gbps': nbytes / min(ms) / 1e6, 'max_err': err}
            print(key, res[key], flush=True)
            del x, repl, conv
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)


def probe_upskip(path, rounds=3):
    """f32 up-conv + skip-add at 12 x 20 x {128^2, 64^2, 32^2}; TB/s is
    (in + skip + out bytes) / time, the traffic the fused result needs."""
    import inspect
    import chunkflow_amd.fastconv as fc
    UP_SURGERY_WIDTHS = getattr(fc, 'UP_SURGERY_WIDTHS_F32',
                                fc.UP_SURGERY_WIDTHS)
    fusable = 'skip' in inspect.signature(CfxUpConv3d.forward).parameters
    res = {'fused_available': fusable,
           'up_surgery_widths': list(UP_SURGERY_WIDTHS)}
    N, D = 12, 20
    for C, K, H in ((36, 28, 128), (48, 36, 64), (64, 48, 32)):
        torch.manual_seed(0)
        conv = nn.ConvTranspose3d(C, K, (1, 2, 2), stride=(1, 2, 2)).cuda()
        hand = CfxUpConv3d(conv, 0, bf16=False).cuda()
        tconv = conv.to(memory_format=cl)
        x = torch.randn(N, C, D, H, H, device='cuda').contiguous(
            memory_format=cl)
        skip = torch.randn(N, K, D, 2 * H, 2 * H, device='cuda').contiguous(
            memory_format=cl)
        nbytes = 4 * (x.numel() + 2 * skip.numel())
        up = hand if C in UP_SURGERY_WIDTHS else tconv
        entry = {'bytes_in_skip_out': nbytes, 'unfused_ms': [],
                 'unfused_path': 'hand' if up is hand else 'miopen'}
        with torch.no_grad():
            want = tconv(x) + skip
            entry['unfused_max_err'] = \
                (up(x) + skip - want).abs().max().item()
            if fusable:
                entry['fused_ms'] = []
                entry['hand_unfused_ms'] = []
                got = hand(x, skip)
                entry['fused_max_err'] = (got - want).abs().max().item()
                entry['fused_bitwise_eq_hand_plus_add'] = bool(
                    torch.equal(got, hand(x) + skip))
            for _ in range(rounds):  # alternated inside the tree too
                entry['unfused_ms'].append(
                    timeit(lambda: up(x) + skip, 20) * 1e3)
                if fusable:
                    entry['fused_ms'].append(
                        timeit(lambda: hand(x, skip), 20) * 1e3)
                    entry['hand_unfused_ms'].append(
                        timeit(lambda: hand(x) + skip, 20) * 1e3)
        for key in ('unfused_ms', 'fused_ms', 'hand_unfused_ms'):
            if key in entry:
                best = min(entry[key])
                entry[key.replace('_ms', '_tbps')] = nbytes / best / 1e9
        res[f'up_{C}to{K}_{H}x{H}'] = entry
        print(f'up_{C}to{K}_{H}x{H}', entry, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)


def probe_miopen_block(path, rounds=4):
    from chunkflow_amd.fastconv import CfxMiopenResBlock

    class ResBlock(nn.Module):
        def __init__(self, c):
            super().__init__()
            self.conv1 = nn.Conv3d(c, c, 3, padding=1, bias=True)
            self.conv2 = nn.Conv3d(c, c, 3, padding=1, bias=True)
            self.act = nn.ELU(inplace=True)

        def forward(self, x):
            y = self.act(self.conv1(x))
            y = self.conv2(y)
            return self.act(x + y)

    torch.manual_seed(0)
    C, N, D, H = 48, 12, 20, 64
    block = ResBlock(C).cuda().eval().to(memory_format=cl)
    fused = CfxMiopenResBlock(block, 0).cuda()
    x = torch.randn(N, C, D, H, H, device='cuda').contiguous(
        memory_format=cl)
    res = {'shape': [N, C, D, H, H], 'torch_ms': [], 'fused_ms': []}
    with torch.no_grad():
        res['max_err'] = (fused(x) - block(x)).abs().max().item()
        for _ in range(rounds):
            res['torch_ms'].append(timeit(lambda: block(x), 20) * 1e3)
            res['fused_ms'].append(timeit(lambda: fused(x), 20) * 1e3)
    res['fused_beats_torch_in_every_pair'] = all(
        f < t for f, t in zip(res['fused_ms'], res['torch_ms']))
    print(res, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--upskip':
        probe_upskip(sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == '--conv155':
        probe_conv155_alone(sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == '--miopen-block':
        probe_miopen_block(sys.argv[2])
        return
    N, D = 12, 20  # config-2-like depth; config-5 uses N=24 D=32
    # RSUNet up/down shapes (H, W = input dims of the op)
    for bf16 in (True, False):
        probe_updown('up', 64, 48, N, D, 32, 32, bf16)
        probe_updown('up', 48, 36, N, D, 64, 64, bf16)
        probe_updown('up', 36, 28, N, D, 128, 128, bf16)
        probe_updown('down', 28, 36, N, D, 256, 256, bf16)
        probe_updown('down', 36, 48, N, D, 128, 128, bf16)
        probe_updown('down', 48, 64, N, D, 64, 64, bf16)
    probe_sliced(36, N, D, 128, 128)
    probe_sliced(48, N, D, 64, 64)
    # config-5 geometry
    probe_sliced(36, 24, 32, 128, 128)
    probe_sliced(48, 24, 32, 64, 64)
    probe_conv155(12, 20, 256, 256, False)
    probe_conv155(24, 32, 256, 256, True)
    probe_conv155_out(12, 20, 256, 256, False)
    probe_conv155_out(24, 32, 256, 256, True)
    os.makedirs('gpurun_out', exist_ok=True)
    with open('gpurun_out/updown_probe.json', 'w') as f:
        json.dump(RES, f, indent=1)


if __name__ == '__main__':
    main()
