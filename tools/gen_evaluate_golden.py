"""Generate tests/golden/evaluate_cases.npz from the reference's vendored
gala metrics (chunkflow/lib/gala/evaluate.py).

Runs only where a checkout of the reference is available; tests and GPU jobs
read the committed .npz alone. The reference module is loaded by path and
called the way Segmentation.evaluate does (chunk/segmentation.py:33-67):
both volumes cast with astype(np.uint64), then rand_index, adj_rand_index,
vi, fm_index and edit_distance(size_threshold=...).

Harness details (each found by running the reference here):
  * evaluate.py imports h5py at module level and never uses it on this
    path: where h5py is not installed an empty module stands in;
  * it imports skimage.segmentation.relabel_sequential, used by
    raw_edit_distance only: where skimage is not installed an
    order-preserving numpy compaction stands in (0 stays 0, the other
    labels become 1..K in ascending order). This cannot change the edit
    distance, which only counts the non-zero entries of each row;
  * the reference allocates one matrix row per label VALUE, so the inputs
    keep their labels below 64.

    python tools/gen_evaluate_golden.py [--reference DIR] [--out FILE]

Keys of the .npz: '<case>/seg', '<case>/gt' (uint8 label volumes),
'<case>/size_threshold' (int64) and '<case>/scores' (float64[6]: rand
index, adjusted rand index, variation of information, Fowlkes-Mallows
index, and the two elements of the edit distance). <case> starts with its
layout: random, blocky, same, nozero, allzero, onelabel or disjoint.
"""
import argparse
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (shape, labels in seg, labels in gt, size_threshold)
RANDOM = [
    ((1, 1, 1), 1, 1, 0), ((1, 1, 70), 3, 2, 0), ((2, 3, 1), 2, 2, 5),
    ((3, 5, 17), 3, 5, 0), ((3, 5, 17), 10, 7, 5),
    ((5, 33, 70), 3, 3, 1000), ((4, 33, 70), 40, 40, 0),
    ((3, 33, 70), 40, 25, 29), ((8, 16, 64), 12, 20, 5),
    ((8, 40, 70), 24, 24, 29), ((8, 40, 70), 5, 8, 1000),
    ((4, 16, 64), 20, 3, 0),
]
# (shape, repeat of seg along x, repeat of gt along x, labels, threshold)
BLOCKY = [
    ((3, 5, 17), 3, 3, 6, 0), ((5, 33, 70), 3, 3, 40, 5),
    ((8, 40, 70), 3, 5, 40, 29), ((5, 33, 70), 5, 5, 12, 29),
    ((8, 40, 70), 5, 3, 25, 1000), ((1, 1, 70), 5, 3, 4, 5),
]
SAME = [((3, 5, 17), 7, 0), ((5, 33, 70), 40, 29), ((8, 40, 70), 12, 1000)]
NOZERO = [((3, 5, 17), 4, 5), ((5, 33, 70), 40, 0), ((8, 40, 70), 9, 1000)]
ALLZERO = [((3, 5, 17), 0), ((8, 40, 70), 1000)]
ONELABEL = [((3, 5, 17), 5), ((8, 40, 70), 1000)]
DISJOINT = [((3, 5, 17), 3, 0), ((5, 33, 70), 9, 5)]


def _relabel_sequential(arr):
    """(relabelled,): 0 stays 0, the other labels become 1..K, ascending."""
    arr = np.asarray(arr)
    uniq = np.unique(arr[arr != 0])
    out = np.zeros(arr.shape, dtype=arr.dtype)
    nz = arr != 0
    out[nz] = (np.searchsorted(uniq, arr[nz]) + 1).astype(arr.dtype)
    return (out,)


def load_reference(root):
    for name in ('h5py',):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    try:
        importlib.import_module('skimage.segmentation')
    except ImportError:
        skimage = types.ModuleType('skimage')
        seg = types.ModuleType('skimage.segmentation')
        seg.relabel_sequential = _relabel_sequential
        skimage.segmentation = seg
        sys.modules['skimage'] = skimage
        sys.modules['skimage.segmentation'] = seg
    path = os.path.join(root, 'chunkflow', 'lib', 'gala', 'evaluate.py')
    spec = importlib.util.spec_from_file_location('ref_gala_evaluate', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ref_scores(ref, seg, gt, size_threshold):
    seg, gt = seg.astype(np.uint64), gt.astype(np.uint64)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        edit = ref.edit_distance(seg, gt, size_threshold=size_threshold)
        return np.array([ref.rand_index(seg, gt),
                         ref.adj_rand_index(seg, gt), ref.vi(seg, gt),
                         ref.fm_index(seg, gt), edit[0], edit[1]],
                        dtype=np.float64)


def blocky(rng, shape, repeat, labels):
    z, y, x = shape
    coarse = rng.integers(0, labels, size=(z, y, -(-x // repeat)))
    return np.repeat(coarse, repeat, axis=2)[:, :, :x]


def build_cases(rng):
    """name -> (seg, gt, size_threshold)."""
    cases = {}
    for i, (shape, ks, kg, thr) in enumerate(RANDOM):
        cases[f'random_{i}'] = (rng.integers(0, ks, size=shape),
                                rng.integers(0, kg, size=shape), thr)
    for i, (shape, rs, rg, k, thr) in enumerate(BLOCKY):
        cases[f'blocky_{rs}{rg}_{i}'] = (blocky(rng, shape, rs, k),
                                         blocky(rng, shape, rg, k), thr)
    for i, (shape, k, thr) in enumerate(SAME):
        seg = blocky(rng, shape, 3, k)
        cases[f'same_{i}'] = (seg, seg.copy(), thr)
    for i, (shape, k, thr) in enumerate(NOZERO):
        cases[f'nozero_{i}'] = (blocky(rng, shape, 3, k) + 1,
                                blocky(rng, shape, 5, k) + 1, thr)
    for i, (shape, thr) in enumerate(ALLZERO):
        cases[f'allzero_{i}'] = (np.zeros(shape, int), np.zeros(shape, int),
                                 thr)
    for i, (shape, thr) in enumerate(ONELABEL):
        cases[f'onelabel_{i}'] = (np.full(shape, 7), np.full(shape, 7), thr)
    for i, (shape, k, thr) in enumerate(DISJOINT):
        side = blocky(rng, shape, 5, 2).astype(bool)
        cases[f'disjoint_{i}'] = (
            np.where(side, rng.integers(1, k + 1, size=shape), 0),
            np.where(side, 0, rng.integers(1, k + 1, size=shape)), thr)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=None,
                    help='root of a checkout of the reference')
    ap.add_argument('--out', default=os.path.join(
        REPO, 'tests', 'golden', 'evaluate_cases.npz'))
    args = ap.parse_args()
    root = args.reference
    if root is None:
        sys.path.insert(0, REPO)
        from oracle.ref_harness import REFERENCE_PATH
        root = REFERENCE_PATH
    ref = load_reference(root)
    rng = np.random.default_rng(20240611)
    out = {}
    for name, (seg, gt, thr) in build_cases(rng).items():
        assert seg.shape == gt.shape and max(seg.max(), gt.max()) < 64, name
        seg, gt = seg.astype(np.uint8), gt.astype(np.uint8)
        out[f'{name}/seg'] = seg
        out[f'{name}/gt'] = gt
        out[f'{name}/size_threshold'] = np.int64(thr)
        out[f'{name}/scores'] = ref_scores(ref, seg, gt, thr)
        print(name, seg.shape, thr, out[f'{name}/scores'])
    np.savez_compressed(args.out, **out)
    print(f'{len(out) // 4} cases -> {args.out} '
          f'({os.path.getsize(args.out)} bytes)')


if __name__ == '__main__':
    main()
