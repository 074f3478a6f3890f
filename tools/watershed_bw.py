"""Time of the three device passes that turn an affinity map into segments
on an MI355X, next to two yardsticks taken in the same run. Writes
profiles/watershed_bw.json.

Input (512^3 unless --size says otherwise): a seeded random affinity map
(3, N, N, N) f32 generated on the device, smoothed and stretched to [0, 1],
twice: 'fine' (two 5-voxel box passes: fragments of a few voxels, the worst
case for the region graph) and 'coarse' (three 9-voxel passes: larger
fragments, fewer boundary edges).

Passes:
  fragments     HipOps.affinity_fragments(aff, low, high): init, merge,
                compress, rank (one host scan), final. Floor bytes: the map
                once, 12 B per voxel, plus the label volume written, 4 B.
  region_graph  HipOps.region_graph_table(frag, aff): the sizing pass over
                the fragments, the table allocation, the clear and the edge
                pass. Floor: the fragments twice, 8 B per voxel (affinities
                are read at fragment boundaries only).
  apply         the segment map gathered through the int32 fragments
                (torch indexing). The map is a seeded random one of the
                right length: merging 10^6 rows in Python is not what is
                timed here. Floor: 8 B per voxel.
Yardsticks:
  binary_cc     connected_component(channel 0, threshold): the existing
                binary labeller on the same volume, 1 B per voxel of input
                behind a 4 B per voxel threshold pass.
  torch_unique  the region graph's keys and counts written with torch ops:
                boundary-edge keys of the three axes concatenated, then
                torch.unique(return_counts=True). It computes no sums.

Method: HIP events around each call, warm-up calls first, then rounds x
iters timed calls with the candidates alternated per round; median, min and
max are reported. The device region graph is compared with the torch rows
(keys and counts) before anything is timed.

    python tools/watershed_bw.py [--out FILE] [--size N] [--iters N]
        [--rounds R] [--low L] [--high H]

Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from chunkflow_amd.chunk import Chunk  # noqa: E402
from chunkflow_amd.connected import connected_component  # noqa: E402
from chunkflow_amd.ops import HipOps  # noqa: E402


def time_ms(fn, iters):
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
            'ms_spread': max(times) - min(times), 'calls': len(times),
            'floor_bytes': nbytes, 'bytes_per_s': nbytes / (med * 1e-3)}


def compare(runs, floors, iters, rounds):
    times = {name: [] for name in runs}
    for fn in runs.values():
        time_ms(fn, 2)
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name] += time_ms(fn, iters)
    return {name: summary(times[name], floors[name]) for name in runs}


INPUTS = {'fine': (5, 2), 'coarse': (9, 3)}   # box width, passes


def smooth_affinities(size, width, passes):
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn((3, 1, size, size, size), device='cuda', generator=g)
    for _ in range(passes):
        x = torch.nn.functional.avg_pool3d(x, width, stride=1,
                                           padding=width // 2)
    x = x[:, 0]
    lo, hi = x.min(), x.max()
    return ((x - lo) / (hi - lo)).contiguous()


def torch_region_keys(frag):
    """(keys, counts) of the region graph with torch ops alone"""
    f = frag.to(torch.int64)
    keys = []
    for axis in (2, 1, 0):
        n = f.shape[axis]
        a, b = f.narrow(axis, 1, n - 1), f.narrow(axis, 0, n - 1)
        sel = (a != b) & (a != 0) & (b != 0)
        a, b = a[sel], b[sel]
        keys.append((torch.minimum(a, b) << 32) | torch.maximum(a, b))
    return torch.unique(torch.cat(keys), return_counts=True)


def measure(ops, aff, args):
    n = aff[0].numel()
    threshold = float(aff[0].median())

    frag, n_frag = ops.affinity_fragments(aff, args.low, args.high)
    keys, counts, _, info = ops.region_graph_table(frag, aff)
    used = keys != -1
    rows = int(used.sum())
    want_keys, want_counts = torch_region_keys(frag)
    order = torch.argsort(keys[used])
    assert torch.equal(keys[used][order], want_keys)
    assert torch.equal(counts[used][order].to(torch.int64), want_counts)
    del keys, counts, used, order, want_keys, want_counts
    n_cc = int(connected_component(Chunk(aff[0]),
                                   threshold=threshold).array.max())
    g = torch.Generator(device='cuda').manual_seed(2)
    seg_of = torch.randint(1, max(n_frag // 4, 2), (n_frag + 1,),
                           device='cuda', generator=g, dtype=torch.int32)
    seg_of[0] = 0
    torch.cuda.empty_cache()

    runs = {
        'fragments': lambda: ops.affinity_fragments(aff, args.low,
                                                    args.high),
        'binary_cc': lambda: connected_component(Chunk(aff[0]),
                                                 threshold=threshold),
        'region_graph': lambda: ops.region_graph_table(frag, aff),
        'torch_unique': lambda: torch_region_keys(frag),
        'apply': lambda: seg_of[frag],
    }
    floors = {'fragments': 16 * n, 'binary_cc': 9 * n,
              'region_graph': 8 * n, 'torch_unique': 8 * n, 'apply': 8 * n}
    results = compare(runs, floors, args.iters, args.rounds)
    return {
        'shape': list(aff.shape), 'low': args.low, 'high': args.high,
        'n_fragments': n_frag, 'region_graph_rows': rows,
        'region_graph_table': info,
        'binary_cc_threshold': threshold, 'binary_cc_components': n_cc,
        'results': results,
        'fragments_over_binary_cc_time':
            results['fragments']['ms_median']
            / results['binary_cc']['ms_median'],
        'torch_unique_over_region_graph_time':
            results['torch_unique']['ms_median']
            / results['region_graph']['ms_median'],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(
        REPO, 'profiles', 'watershed_bw.json'))
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--low', type=float, default=0.3)
    ap.add_argument('--high', type=float, default=0.9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'watershed_bw needs a GPU'
    ops = HipOps(0)
    inputs = {}
    for name, (width, passes) in INPUTS.items():
        aff = smooth_affinities(args.size, width, passes)
        entry = {'box_width': width, 'box_passes': passes}
        entry.update(measure(ops, aff, args))
        inputs[name] = entry
        print(json.dumps({name: entry}), flush=True)
        del aff
        torch.cuda.empty_cache()
    doc = {
        'device': torch.cuda.get_device_name(0),
        'method': 'HIP events around each call, warm-up first, median / '
                  'min / max of rounds*iters calls, candidates alternated '
                  'per round; floor_bytes is algorithmic (from shapes)',
        'iters': args.iters, 'rounds': args.rounds, 'inputs': inputs,
        'expectation': 'fragments within a small factor of binary CC: it '
                       'streams 12 B per voxel plus three forward-neighbour '
                       'reads against 1 B per voxel '
                       '(fragments_over_binary_cc_time)',
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
