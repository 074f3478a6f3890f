"""Seeded oracle-vs-reference cases and their recorded reference outputs.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py). The case builders below
are shared by the tests (tests/test_oracle_golden.py,
tests/test_host_product.py) and by the recorder, so both always see the same
inputs. The recorder runs the UNMODIFIED reference on every case and stores
what it returned in tests/golden/reference_cases.npz; run it from the repo
root where the reference checkout is available (oracle/ref_harness.py):

    python -m oracle.reference_cases
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, '..', 'tests', 'golden', 'reference_cases.npz')

FUZZ_SEEDS = (101, 202, 303)
CONTRAST_SEEDS = (5, 6, 7, 11)


def identity_case():
    """Fixed non-aligned masked identity inference with a voxel offset."""
    rng = np.random.RandomState(42)
    arr = rng.randint(0, 256, size=(24, 70, 66), dtype=np.uint8)
    return dict(arr=arr, patch=(12, 32, 32), ov=(4, 8, 8), off=(3, 4, 5),
                nch=2, bs=5)


def fuzz_case(seed: int):
    """Randomized geometry: chunk/patch/overlap/offset/channels/batch drawn
    per seed, identity engine, masked mode."""
    rng = np.random.RandomState(seed)
    patch = tuple(int(rng.randint(6, 13) * 2) for _ in range(3))
    ov = tuple(max(2, (p // 4) // 2 * 2) for p in patch)
    chunk = tuple(p + int(rng.randint(0, 3)) * (p - o)
                  + int(rng.randint(0, 4))
                  for p, o in zip(patch, ov))
    off = tuple(int(v) for v in rng.randint(0, 9, size=3))
    nch = int(rng.randint(1, 4))
    bs = int(rng.randint(1, 5))
    arr = rng.randint(0, 256, size=chunk).astype(np.uint8)
    return dict(arr=arr, patch=patch, ov=ov, off=off, nch=nch, bs=bs)


def contrast_case(seed: int) -> np.ndarray:
    """Random small uint8 volume for normalize_contrast."""
    rng = np.random.RandomState(seed)
    shape = tuple(int(v) for v in rng.randint(3, 20, size=3))
    return rng.randint(0, 256, size=shape).astype(np.uint8)


def load_recorded():
    """The recorded reference outputs, keyed 'identity', 'fuzz_<seed>',
    'contrast_<seed>'."""
    return np.load(FIXTURE)


def _run_reference_identity(Inferencer, Chunk, case) -> np.ndarray:
    with Inferencer(None, None, case['patch'],
                    output_patch_overlap=case['ov'], framework='identity',
                    num_output_channels=case['nch'],
                    batch_size=case['bs'],
                    mask_output_chunk=True) as inf:
        out = inf(Chunk(case['arr'].copy(), voxel_offset=case['off']))
    return np.asarray(out.array)


def main():
    import sys
    from .ref_harness import (import_reference, install_stubs,
                              reference_available, REFERENCE_PATH)
    assert reference_available(), 'recording needs the reference checkout'
    Inferencer, Chunk, _ = import_reference()
    install_stubs()
    if REFERENCE_PATH not in sys.path:
        sys.path.insert(0, REFERENCE_PATH)
    from chunkflow.chunk.image import Image as RefImage

    arrays = {'identity': _run_reference_identity(Inferencer, Chunk,
                                                  identity_case())}
    for seed in FUZZ_SEEDS:
        arrays[f'fuzz_{seed}'] = _run_reference_identity(
            Inferencer, Chunk, fuzz_case(seed))
    for seed in CONTRAST_SEEDS:
        img = RefImage(contrast_case(seed).copy())
        img.normalize_contrast()
        arrays[f'contrast_{seed}'] = np.asarray(img.array)
    np.savez_compressed(FIXTURE, **arrays)
    for k, v in arrays.items():
        print(k, v.dtype, v.shape)
    print(f'wrote {os.path.getsize(FIXTURE) / 1e6:.2f} MB to {FIXTURE}')


if __name__ == '__main__':
    main()
