"""Time and effective bandwidth of the segmentation-cleanup kernels on an
MI355X: equal-value connected components, mask_fragments and mask_except,
each next to the same operation written with torch ops on the same GPU and
to its algorithmic floor. Writes profiles/segmentation_bw.json.

Inputs (512^3 unless --size says otherwise):
  cc_int32       the int32 output of connected_component on a thresholded
                 smooth random volume (few large objects, much background)
  blocks_int64   an int64 volume of 5x5x5 blocks, one label each (~10^6
                 labels, x-runs of 5 voxels, ids using bits above 32)
  distinct_int32 every voxel its own label: the worst table load
  quantized_u8   the smooth volume cut into four values; equal-value CC
                 only — the input on which the host fallback that device
                 chunks took before (equal_value_label after a D2H copy) is
                 timed, once, with --host-cc

Method: HIP events around each call (the calls include their own sizing
pass, table allocation and status read-back), warm-up calls first, then
rounds x iters timed calls with the candidates alternated per round; median,
min and max are reported, and max - min is the run-to-run spread the
comparison is read against. Bytes are algorithmic, from the shapes:
mask_fragments = labels read twice + written once, mask_except = read once +
written once, CC = the entry's own profile formula. Every timed device
result is compared with the torch formulation (torch.equal) before timing.

    python tools/segmentation_bw.py [--out FILE] [--size N] [--iters N]
        [--rounds R] [--inputs a,b,..] [--host-cc]

Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from chunkflow_amd.chunk import Chunk  # noqa: E402
from chunkflow_amd.connected import (connected_component,  # noqa: E402
                                     equal_value_label)
from chunkflow_amd.ops import HipOps  # noqa: E402

DUST = 100
INPUTS = ('cc_int32', 'blocks_int64', 'distinct_int32', 'quantized_u8')


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


def smooth_volume(size):
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn((1, 1, size, size, size), device='cuda', generator=g)
    for _ in range(2):
        x = torch.nn.functional.avg_pool3d(x, 7, stride=1, padding=3)
    return x[0, 0].contiguous()


def make_input(name, size):
    if name == 'cc_int32':
        x = smooth_volume(size)
        seg = connected_component(Chunk(x), threshold=float(x.median()))
        return seg.array
    if name == 'blocks_int64':
        b = torch.arange(size, device='cuda') // 5
        nb = int(b.max()) + 1
        ids = (b[:, None, None] * nb + b[None, :, None]) * nb \
            + b[None, None, :] + 1
        return (ids.to(torch.int64) * (2 ** 33 + 1)).contiguous()
    if name == 'distinct_int32':
        n = size ** 3
        return torch.arange(1, n + 1, dtype=torch.int32,
                            device='cuda').view(size, size, size)
    if name == 'quantized_u8':
        x = smooth_volume(size)
        q = torch.quantile(x.flatten()[::997].float(),
                           torch.tensor([0.25, 0.5, 0.75], device='cuda'))
        return torch.bucketize(x, q).to(torch.uint8).contiguous()
    raise ValueError(name)


def torch_mask_fragments(t, threshold):
    ids, counts = torch.unique(t, return_counts=True)
    return torch.where(torch.isin(t, ids[counts <= threshold]), 0, t)


def torch_mask_except(t, ids_dev):
    return torch.where(torch.isin(t, ids_dev), t, 0)


def compare(runs, floors, iters, rounds):
    times = {name: [] for name in runs}
    for fn in runs.values():
        time_ms(fn, 2)
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name] += time_ms(fn, iters)
    return {name: summary(times[name], floors) for name in runs}


def measure_cc(ops, t, iters, rounds):
    dims, eb, n = tuple(t.shape), t.element_size(), t.numel()
    labels = torch.empty(dims, dtype=torch.int32, device='cuda')
    scratch = torch.empty_like(labels)

    def run():
        return ops.cfx.connected_components_labels(
            t.data_ptr(), eb, dims, 6, labels.data_ptr(),
            scratch.data_ptr())
    n_components = run()
    res = compare({'kernel': run}, n * (3 * eb + 24), iters, rounds)
    res['n_components'] = n_components
    return res


def measure_masks(ops, t, iters, rounds):
    eb, n = t.element_size(), t.numel()
    out = {}
    keys, vals, capacity, bound = ops.label_count_table(t)
    distinct = int((keys != -1).sum())
    out['table'] = {
        'sizing_bound': 'flat run starts (voxels differing from their '
                        'predecessor, plus voxel 0)',
        'run_starts': bound, 'capacity': capacity,
        'distinct_labels': distinct, 'load_factor': distinct / capacity,
        'table_bytes': capacity * 12}
    del keys, vals

    want = torch_mask_fragments(t, DUST)
    assert torch.equal(ops.label_mask_fragments(t, DUST), want)
    del want
    out['mask_fragments'] = compare(
        {'kernel': lambda: ops.label_mask_fragments(t, DUST),
         'torch': lambda: torch_mask_fragments(t, DUST)},
        3 * eb * n, iters, rounds)

    # device time of the three passes alone (sizing, count, apply)
    ops.cfx.profile_reset()
    ops.cfx.profile_enable(True)
    ops.label_mask_fragments(t, DUST)
    prof = ops.cfx.profile_get('labels')
    ops.cfx.profile_enable(False)
    out['mask_fragments']['kernel_passes_ms'] = prof['total_ms']

    ids_dev = torch.unique(t.flatten()[::4099])[::2].contiguous()
    ids = [int(v) & (2 ** (8 * eb) - 1) for v in ids_dev.cpu().tolist()]
    ids = [v for v in ids if v != 2 ** 64 - 1]
    want = torch_mask_except(t, ids_dev)
    assert torch.equal(ops.label_mask_except(t, ids), want)
    del want
    out['mask_except'] = compare(
        {'kernel': lambda: ops.label_mask_except(t, ids),
         'torch': lambda: torch_mask_except(t, ids_dev)},
        2 * eb * n, iters, rounds)
    out['mask_except']['n_ids'] = len(ids)
    for op in ('mask_fragments', 'mask_except'):
        k, ref = out[op]['kernel'], out[op]['torch']
        out[op]['torch_over_kernel_time'] = ref['ms_median'] / k['ms_median']
        out[op]['not_slower_than_torch_beyond_spread'] = bool(
            k['ms_median'] <= ref['ms_median']
            + max(k['ms_spread'], ref['ms_spread']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(
        REPO, 'profiles', 'segmentation_bw.json'))
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--inputs', default=','.join(INPUTS))
    ap.add_argument('--host-cc', action='store_true',
                    help='also time equal_value_label on the host for '
                         'quantized_u8 (slow: minutes at 512^3)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'segmentation_bw needs a GPU'
    ops = HipOps(0)
    results = []
    for name in args.inputs.split(','):
        t = make_input(name, args.size)
        entry = {'input': name, 'shape': list(t.shape),
                 'dtype': str(t.dtype).split('.')[-1]}
        entry['equal_value_cc'] = measure_cc(ops, t, args.iters, args.rounds)
        if name != 'quantized_u8':
            entry.update(measure_masks(ops, t, args.iters, args.rounds))
        elif args.host_cc:
            start = time.time()
            host = t.cpu().numpy()
            ref = equal_value_label(host, 6)
            back = torch.from_numpy(ref).cuda()
            torch.cuda.synchronize()
            secs = time.time() - start
            got = connected_component(Chunk(t), connectivity=6).array
            assert torch.equal(got, back.view(torch.int32))
            entry['equal_value_cc']['host_fallback'] = {
                'what': 'D2H + equal_value_label + H2D, one call',
                'ms': secs * 1e3,
                'over_kernel_time': secs * 1e3
                / entry['equal_value_cc']['kernel']['ms_median']}
            del host, ref, back, got
        results.append(entry)
        print(json.dumps(entry), flush=True)
        del t
        torch.cuda.empty_cache()
    doc = {
        'device': torch.cuda.get_device_name(0),
        'method': 'HIP events around each call, warm-up first, median / '
                  'min / max of rounds*iters calls, candidates alternated '
                  'per round; floor_bytes are algorithmic (from shapes): '
                  'mask_fragments = 3 * labels, mask_except = 2 * labels, '
                  'equal_value_cc = n * (3 * elem + 24); the torch '
                  'formulation is unique(return_counts) + isin + where',
        'dust_threshold': DUST, 'iters': args.iters, 'rounds': args.rounds,
        'results': results,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
