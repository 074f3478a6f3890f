"""Generate tests/golden/downsample_cases.npz from the reference's vendored
numpy downsampling (chunkflow/lib/igneous/downsample.py).

Runs only where a checkout of the reference is available; tests and GPU jobs
read the committed .npz alone. The reference module is loaded by path and
called the way its own callers do (downsample_upload.py:67-75,
save_precomputed.py:128): array transposed to x,y,z order, factor reversed.

Harness details (each found by running the reference under numpy 2):
  * the reference uses np.cast, which numpy 2 removed: an equivalent is
    installed before the call;
  * its 2-D mode path needs a 4-D (x,y,z,1) input;
  * its 3-D mode path needs a plain 3-D input (a trailing channel axis trips
    its even-size assertion).

    python tools/gen_downsample_golden.py [--reference DIR] [--out FILE]

Keys of the .npz: '<case>/in', '<case>/factor', '<case>/out', where <case>
starts with 'avg_' or 'mode_'.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AVG_SHAPES = [(5, 7, 9), (4, 6, 8), (1, 3, 2), (3, 5, 70), (3, 4, 6, 10)]
AVG_FACTORS = [(2, 2, 2), (1, 2, 2), (2, 1, 2), (3, 2, 2), (2, 3, 5)]

MODE2_FACTORS = [(1, 2, 2), (2, 1, 2), (2, 2, 1)]
MODE2_SHAPES = [(3, 6, 8), (2, 5, 7), (1, 1, 1), (5, 7, 9)]
MODE3_SHAPES = [(4, 6, 8), (2, 2, 2), (6, 4, 2)]
STRIDE_CASES = [((5, 7, 9), (2, 2, 2)), ((5, 7, 9), (1, 3, 3))]


class _Cast:
    """np.cast[dtype](x) of numpy 1."""

    def __getitem__(self, dtype):
        return lambda x: np.asarray(x).astype(dtype)


def load_reference(root):
    path = os.path.join(root, 'chunkflow', 'lib', 'igneous', 'downsample.py')
    spec = importlib.util.spec_from_file_location('ref_igneous_downsample',
                                                  path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not hasattr(np, 'cast'):
        np.cast = _Cast()
    return mod


def ref_average(ref, arr, factor):
    """arr (z,y,x) or (C,z,y,x)."""
    xyz = np.transpose(arr).copy()
    if xyz.ndim == 3:
        xyz = np.expand_dims(xyz, 3)
    out = ref.downsample_with_averaging(xyz, tuple(factor[::-1]))
    out = np.transpose(out)
    if arr.ndim == 3:
        out = out[0]
    return np.ascontiguousarray(out)


def ref_mode(ref, arr, factor):
    xyz = np.transpose(arr).copy()
    prod = factor[0] * factor[1] * factor[2]
    two_d = 1 in factor and prod & (prod - 1) == 0
    if two_d:
        xyz = np.expand_dims(xyz, 3)
    out = ref.downsample_segmentation(xyz, tuple(factor[::-1]))
    if two_d:
        out = out[..., 0]
    return np.ascontiguousarray(np.transpose(out))


def alphabets(dtype):
    """Label alphabets: sizes 2 and 3 force ties, size 50 forces the
    'no match -> last voxel' branch; zero is a label; uint32 labels reach
    above 2**31; uint64 labels differ only in their high 32 bits."""
    if dtype == np.uint32:
        return {
            'a2': np.array([0, 2**31 + 5], dtype=dtype),
            'a3': np.array([0, 7, 2**32 - 2], dtype=dtype),
            'a50': np.concatenate([
                np.arange(25), 2**31 + np.arange(25)]).astype(dtype),
        }
    return {
        'a2': np.array([(1 << 32) + 5, (2 << 32) + 5], dtype=dtype),
        'a3': np.array([0, 5, (1 << 32) + 5], dtype=dtype),
        'a50': np.concatenate([
            np.arange(25), (np.arange(25) << 32) + 3]).astype(dtype),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=None,
                    help='root of a checkout of the reference')
    ap.add_argument('--out', default=os.path.join(
        REPO, 'tests', 'golden', 'downsample_cases.npz'))
    args = ap.parse_args()
    root = args.reference
    if root is None:
        sys.path.insert(0, REPO)
        from oracle.ref_harness import REFERENCE_PATH
        root = REFERENCE_PATH
    ref = load_reference(root)
    rng = np.random.default_rng(20240517)
    cases = {}

    def add(name, arr, factor, out):
        assert out.dtype == arr.dtype, (name, out.dtype)
        cases[f'{name}/in'] = arr
        cases[f'{name}/factor'] = np.asarray(factor, dtype=np.int64)
        cases[f'{name}/out'] = out

    for si, shape in enumerate(AVG_SHAPES):
        u8 = rng.integers(0, 256, size=shape, dtype=np.uint8)
        u8.flat[:4] = [0, 255, 255, 254]
        # mixed signs and magnitudes so the summation order shows
        f32 = (rng.standard_normal(shape)
               * 10.0 ** rng.integers(-3, 6, size=shape)).astype(np.float32)
        for fi, factor in enumerate(AVG_FACTORS):
            add(f'avg_u8_s{si}_f{fi}', u8, factor,
                ref_average(ref, u8, factor))
            add(f'avg_f32_s{si}_f{fi}', f32, factor,
                ref_average(ref, f32, factor))

    mode_cases = [(s, f) for f in MODE2_FACTORS for s in MODE2_SHAPES]
    mode_cases += [(s, (2, 2, 2)) for s in MODE3_SHAPES]
    mode_cases += STRIDE_CASES
    for dtype in (np.uint32, np.uint64):
        for aname, alphabet in alphabets(dtype).items():
            for ci, (shape, factor) in enumerate(mode_cases):
                arr = alphabet[rng.integers(0, len(alphabet), size=shape)]
                add(f'mode_{np.dtype(dtype).name}_{aname}_c{ci}', arr,
                    factor, ref_mode(ref, arr, factor))

    np.savez_compressed(args.out, **cases)
    print(f'{len(cases) // 3} cases -> {args.out} '
          f'({os.path.getsize(args.out)} bytes)')


if __name__ == '__main__':
    main()
