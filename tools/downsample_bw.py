"""Achieved bandwidth of the downsample kernels on an MI355X.

Times each kernel with HIP events on inputs larger than the 256 MiB
last-level cache and writes bytes/s (input read + output written, computed
from the shapes) to profiles/downsample_bw.json, next to two references
taken in the same run on the same tensors, alternating with the kernel:

  * a plain device-to-device copy of the input (the project's "measured copy
    ceiling"; its bytes are input read + input-sized write);
  * for float32, torch.nn.functional.avg_pool3d — what a user would reach
    for today (same algorithmic bytes as the kernel).

    python tools/downsample_bw.py [--out FILE] [--iters N] [--rounds R]

Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from chunkflow_amd.downsample import average_host, mode_host  # noqa: E402
from chunkflow_amd.ops import HipOps  # noqa: E402

CASES = [
    # (kernel, dtype, shape)
    ('average', torch.uint8, (1024, 1024, 1024)),
    ('average', torch.float32, (512, 1024, 1024)),
    ('mode', torch.int32, (512, 1024, 1024)),
]
FACTORS = [(1, 2, 2), (2, 2, 2)]


def time_ms(fn, iters):
    """Per-call device times (ms) of `iters` calls, one event pair each."""
    pairs = []
    for _ in range(iters):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def summary(times, nbytes):
    med = statistics.median(times)
    return {'ms_median': med, 'ms_min': min(times), 'ms_max': max(times),
            'bytes': nbytes, 'bytes_per_s': nbytes / (med * 1e-3)}


def check_corner(kernel, t, out, factor):
    """The timed output's first block equals the host path on the same
    voxels (byte-for-byte; the suite holds the full parity tests)."""
    src = t[:8, :16, :64].cpu().numpy()
    got = out[:8 // factor[0], :16 // factor[1], :64 // factor[2]]
    got = got.cpu().numpy()
    if kernel == 'average':
        want = average_host(src, factor)
    else:
        want = mode_host(src.view(np.uint32), factor).view(np.int32)
    assert got.tobytes() == want.tobytes(), (kernel, factor)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles',
                                                  'downsample_bw.json'))
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'downsample_bw needs a GPU'
    ops = HipOps(0)
    results = []
    for kernel, dtype, shape in CASES:
        n = shape[0] * shape[1] * shape[2]
        if dtype == torch.uint8:
            t = torch.randint(0, 256, shape, dtype=dtype, device='cuda')
        elif dtype == torch.float32:
            t = torch.randn(shape, dtype=dtype, device='cuda')
        else:
            t = torch.randint(0, 1000, shape, dtype=dtype, device='cuda')
        in_bytes = n * t.element_size()
        dst = torch.empty_like(t)
        run_op = (ops.downsample_average if kernel == 'average'
                  else ops.downsample_mode)
        for factor in FACTORS:
            out_bytes = in_bytes // (factor[0] * factor[1] * factor[2])
            runs = {'kernel': lambda: run_op(t, factor),
                    'copy': lambda: dst.copy_(t)}
            if dtype == torch.float32:
                t5 = t[None, None]
                runs['avg_pool3d'] = lambda: \
                    torch.nn.functional.avg_pool3d(t5, factor, factor)
            check_corner(kernel, t, run_op(t, factor), factor)
            times = {name: [] for name in runs}
            for fn in runs.values():            # warm-up, every shape
                time_ms(fn, 3)
            for _ in range(args.rounds):        # alternate the candidates
                for name, fn in runs.items():
                    times[name] += time_ms(fn, args.iters)
            entry = {
                'case': f'{kernel}_{str(dtype).split(".")[-1]}',
                'shape': list(shape), 'factor': list(factor),
                'kernel': summary(times['kernel'], in_bytes + out_bytes),
                'copy': summary(times['copy'], 2 * in_bytes),
            }
            if 'avg_pool3d' in runs:
                entry['avg_pool3d'] = summary(times['avg_pool3d'],
                                              in_bytes + out_bytes)
            entry['kernel_over_copy_bytes_per_s'] = (
                entry['kernel']['bytes_per_s'] / entry['copy']['bytes_per_s'])
            results.append(entry)
            print(json.dumps(entry), flush=True)
        del t, dst
        torch.cuda.empty_cache()
    doc = {
        'device': torch.cuda.get_device_name(0),
        'method': 'HIP events around each call, median of rounds*iters '
                  'calls, candidates alternated per round; bytes are '
                  'algorithmic (from shapes): kernel and avg_pool3d = input '
                  'read + output written, copy = 2 * input',
        'iters': args.iters, 'rounds': args.rounds,
        'results': results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
