"""Time and achieved bandwidth of the gaussian and median filter kernels on
an MI355X.

Times each kernel with HIP events on a 512^3 uint8 and a 512^3 float32 chunk
and writes time and algorithmic bytes/s (one read and one write of the
volume) to profiles/filters_bw.json, next to what a user has today, taken in
the same run on the same tensors and alternating with the kernel:

  * a plain device-to-device copy of the input (same algorithmic bytes);
  * gaussian: a separable torch.nn.functional.conv2d in float32 over a
    reflect-padded copy (NOT bit-exact to scipy: a speed yardstick only;
    for uint8 the conversions to float32 and back are inside the timing);
  * median (3,1,1): torch.median over three shifted copies;
  * the host scipy.ndimage call on the same data, one run, host clock.

    python tools/filters_bw.py [--out FILE] [--iters N] [--rounds R]
                               [--size N] [--no-host]

Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.ndimage
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from chunkflow_amd.filters import gaussian_weights  # noqa: E402
from chunkflow_amd.ops import HipOps  # noqa: E402

GAUSS_SIGMAS = [1, 2]
MEDIAN_SIZES = [(3, 1, 1), (3, 3, 3)]


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


def conv2d_gaussian(t, sigma):
    """The torch yardstick: pad (torch's 'reflect' is scipy's 'mirror';
    torch has no padding with scipy's 'reflect' rule, and for speed the
    two cost the same), then a (2r+1,1) and a (1,2r+1) conv2d in float32."""
    r, w = gaussian_weights(sigma)
    w = torch.from_numpy(w.astype(np.float32)).to(t.device)
    x = t.to(torch.float32)[:, None]
    x = torch.nn.functional.pad(x, (r, r, r, r), mode='reflect')
    x = torch.nn.functional.conv2d(x, w.view(1, 1, -1, 1))
    x = torch.nn.functional.conv2d(x, w.view(1, 1, 1, -1))
    return x[:, 0].to(t.dtype)


def torch_median3_z(t):
    prev = torch.cat([t[:1], t[:-1]])
    nxt = torch.cat([t[1:], t[-1:]])
    return torch.stack([prev, t, nxt]).median(dim=0).values


def host_seconds(fn):
    start = time.perf_counter()
    fn()
    return time.perf_counter() - start


def measure(runs, nbytes, iters, rounds):
    times = {name: [] for name in runs}
    for fn in runs.values():            # warm-up, every candidate
        time_ms(fn, 3)
    for _ in range(rounds):             # alternate the candidates
        for name, fn in runs.items():
            times[name] += time_ms(fn, iters)
    return {name: summary(ts, nbytes) for name, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles',
                                                  'filters_bw.json'))
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--no-host', action='store_true',
                    help='skip the host scipy runs')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'filters_bw needs a GPU'
    ops = HipOps(0)
    n = args.size
    results = []
    for dtype in (torch.uint8, torch.float32):
        if dtype == torch.uint8:
            t = torch.randint(0, 256, (n, n, n), dtype=dtype, device='cuda')
        else:
            t = torch.randn((n, n, n), dtype=dtype, device='cuda')
        host = t.cpu().numpy()
        nbytes = 2 * t.numel() * t.element_size()
        dst = torch.empty_like(t)
        name = str(dtype).split('.')[-1]
        for sigma in GAUSS_SIGMAS:
            got = ops.gaussian_filter_2d(t, sigma)[:2].cpu().numpy()
            want = np.stack([scipy.ndimage.gaussian_filter(s, sigma=sigma)
                             for s in host[:2]])
            assert np.array_equal(got, want), ('gaussian', name, sigma)
            entry = {'case': f'gaussian_{name}', 'shape': [n, n, n],
                     'sigma': sigma}
            entry.update(measure({
                'kernel': lambda: ops.gaussian_filter_2d(t, sigma),
                'copy': lambda: dst.copy_(t),
                'torch_conv2d_f32': lambda: conv2d_gaussian(t, sigma),
            }, nbytes, args.iters, args.rounds))
            if not args.no_host:
                def run():
                    for s in host:
                        scipy.ndimage.gaussian_filter(s, sigma=sigma)
                entry['host_scipy_s'] = host_seconds(run)
            results.append(entry)
            print(json.dumps(entry), flush=True)
        for size in MEDIAN_SIZES:
            got = ops.median_filter(t, size)[:2].cpu().numpy()
            want = scipy.ndimage.median_filter(host[:4], size=size)[:2]
            assert np.array_equal(got, want), ('median', name, size)
            runs = {'kernel': lambda: ops.median_filter(t, size),
                    'copy': lambda: dst.copy_(t)}
            if size == (3, 1, 1):
                runs['torch_median_of_3'] = lambda: torch_median3_z(t)
            entry = {'case': f'median_{name}', 'shape': [n, n, n],
                     'size': list(size)}
            entry.update(measure(runs, nbytes, args.iters, args.rounds))
            if not args.no_host:
                entry['host_scipy_s'] = host_seconds(
                    lambda: scipy.ndimage.median_filter(host, size=size))
            results.append(entry)
            print(json.dumps(entry), flush=True)
        del t, dst, host
        torch.cuda.empty_cache()
    doc = {
        'device': torch.cuda.get_device_name(0),
        'method': 'HIP events around each call, median of rounds*iters '
                  'calls, candidates alternated per round; bytes are '
                  'algorithmic (from shapes): one read and one write of the '
                  'volume for every candidate; host_scipy_s is one run of '
                  'scipy.ndimage on the same data, host clock, seconds',
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
