"""Time and effective bandwidth of the device contingency table behind
evaluate-segmentation on an MI355X, next to the same table written with
torch ops on the same GPU and to its algorithmic floor. Writes
profiles/evaluate_bw.json.

Input (512^3 unless --size says otherwise), as int32 and as int64:
  seg  the output of connected_component on a thresholded smooth random
       volume (few large objects, much background)
  gt   the same volume with some objects merged into a neighbouring id and
       some split across the middle z plane

Candidates:
  passes   the three streaming passes alone, tables allocated beforehand:
           cfx_label_count on each volume, then cfx_label_pair_count (each
           with its own table clear and status read-back). Floor: every
           volume is read twice, 2 * (seg bytes + gt bytes).
  kernel   HipOps.label_contingency whole: the two sizing passes, table
           allocation, the three passes above, compaction and ordering of
           the rows.
  torch    the only alternative on the device: torch.unique(
           return_counts=True) on the combined key (seg << 32) | gt. The key
           exists because these labels fit 32 bits; the kernel path does
           not need that.

Method: HIP events around each call, warm-up calls first, then rounds x
iters timed calls with the candidates alternated per round; median, min and
max are reported, and max - min is the run-to-run spread the comparison is
read against. The kernel rows are compared with the torch rows
(torch.equal) before anything is timed.

    python tools/evaluate_bw.py [--out FILE] [--size N] [--iters N]
        [--rounds R]

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


def compare(runs, floor, iters, rounds):
    times = {name: [] for name in runs}
    for fn in runs.values():
        time_ms(fn, 2)
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name] += time_ms(fn, iters)
    return {name: summary(times[name], floor) for name in runs}


def smooth_volume(size):
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn((1, 1, size, size, size), device='cuda', generator=g)
    for _ in range(2):
        x = torch.nn.functional.avg_pool3d(x, 7, stride=1, padding=3)
    return x[0, 0].contiguous()


def make_pair(size):
    """(seg, gt) int32: gt merges every label with id % 7 == 3 into id - 1
    and moves the upper half (in z) of every label with id % 5 == 1 to a
    fresh id."""
    x = smooth_volume(size)
    seg = connected_component(Chunk(x), threshold=float(x.median())).array
    del x
    n_labels = int(seg.max())
    gt = torch.where(seg % 7 == 3, seg - 1, seg)
    upper = torch.zeros_like(seg, dtype=torch.bool)
    upper[size // 2:] = True
    gt = torch.where(upper & (gt % 5 == 1), gt + n_labels, gt)
    return seg.contiguous(), gt.contiguous(), n_labels


def torch_contingency(seg, gt):
    key = (seg.to(torch.int64) << 32) | gt.to(torch.int64)
    pairs, counts = torch.unique(key, return_counts=True)
    return pairs >> 32, pairs & 0xFFFFFFFF, counts


def measure(ops, seg, gt, iters, rounds):
    dims, n = tuple(seg.shape), seg.numel()
    sb, gb = seg.element_size(), gt.element_size()
    floor = 2 * n * (sb + gb)

    want = torch_contingency(seg, gt)
    got = ops.label_contingency(seg, gt)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    n_pairs = len(want[2])
    del want, got

    sk, gk, keys, vals, info = ops.label_pair_table(seg, gt)
    distinct = {'seg': int((sk != -1).sum()), 'gt': int((gk != -1).sum()),
                'pair': int((keys != -1).sum())}
    assert distinct['pair'] == n_pairs
    tables = {
        'sizing_bound': 'single tables: flat run starts; pair table: '
                        'run_starts(seg) + run_starts(gt) - 1',
        'n_labels': distinct}
    for name in ('seg', 'gt', 'pair'):
        cap = info[f'{name}_capacity']
        tables[name] = {'bound': info[f'{name}_bound'], 'capacity': cap,
                        'distinct': distinct[name],
                        'load_factor': distinct[name] / cap,
                        'table_bytes': cap * 12}
    sv = torch.empty(info['seg_capacity'], dtype=torch.int32, device='cuda')
    gv = torch.empty(info['gt_capacity'], dtype=torch.int32, device='cuda')
    cfx = ops.cfx

    def passes():
        cfx.label_table_clear(sk.data_ptr(), sv.data_ptr(),
                              info['seg_capacity'])
        cfx.label_table_clear(gk.data_ptr(), gv.data_ptr(),
                              info['gt_capacity'])
        cfx.label_table_clear(keys.data_ptr(), vals.data_ptr(),
                              info['pair_capacity'])
        cfx.label_count(seg.data_ptr(), sb, dims, sk.data_ptr(),
                        sv.data_ptr(), info['seg_capacity'])
        cfx.label_count(gt.data_ptr(), gb, dims, gk.data_ptr(),
                        gv.data_ptr(), info['gt_capacity'])
        cfx.label_pair_count(seg.data_ptr(), sb, dims, sk.data_ptr(),
                             info['seg_capacity'], gt.data_ptr(), gb, dims,
                             gk.data_ptr(), info['gt_capacity'],
                             keys.data_ptr(), vals.data_ptr(),
                             info['pair_capacity'])

    out = {'tables': tables, 'n_pairs': n_pairs}
    out.update(compare(
        {'passes': passes,
         'kernel': lambda: ops.label_contingency(seg, gt),
         'torch': lambda: torch_contingency(seg, gt)},
        floor, iters, rounds))
    assert int(vals.to(torch.int64).sum()) == n   # the timed passes counted

    # device time of the kernels alone, table clears and read-backs excluded
    cfx.profile_reset()
    cfx.profile_enable(True)
    passes()
    prof = cfx.profile_get('labels')
    cfx.profile_enable(False)
    out['passes']['kernels_only_ms'] = prof['total_ms']
    out['passes']['kernels_only_bytes_per_s'] = floor / (
        prof['total_ms'] * 1e-3)

    k, ref = out['kernel'], out['torch']
    out['torch_over_kernel_time'] = ref['ms_median'] / k['ms_median']
    out['not_slower_than_torch_beyond_spread'] = bool(
        k['ms_median'] <= ref['ms_median']
        + max(k['ms_spread'], ref['ms_spread']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(
        REPO, 'profiles', 'evaluate_bw.json'))
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'evaluate_bw needs a GPU'
    ops = HipOps(0)
    seg32, gt32, n_labels = make_pair(args.size)
    results = []
    for dtype in (torch.int32, torch.int64):
        seg, gt = seg32.to(dtype), gt32.to(dtype)
        entry = {'shape': list(seg.shape),
                 'dtype': str(dtype).split('.')[-1],
                 'n_components': n_labels}
        entry.update(measure(ops, seg, gt, args.iters, args.rounds))
        results.append(entry)
        print(json.dumps(entry), flush=True)
        del seg, gt
        torch.cuda.empty_cache()
    doc = {
        'device': torch.cuda.get_device_name(0),
        'method': 'HIP events around each call, warm-up first, median / '
                  'min / max of rounds*iters calls, candidates alternated '
                  'per round; floor_bytes is algorithmic (from shapes): '
                  'every volume read twice, 2 * (seg bytes + gt bytes); '
                  'passes = two single counts + the pair count on '
                  'preallocated tables; kernel = HipOps.label_contingency '
                  'whole; torch = unique(return_counts) on (seg << 32) | gt',
        'expectation': 'kernel not slower than torch beyond the measured '
                       'spread (not_slower_than_torch_beyond_spread)',
        'iters': args.iters, 'rounds': args.rounds, 'results': results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
