"""Case tables, plain numpy f32 references and one driver for the chunk
stitching kernels of chunkflow_amd/csrc/cfx.hip (used by
tests/test_stitch_exact.py; not collected by pytest).

Every kernel here moves or combines f32 values with at most two IEEE
operations per element, so a numpy restatement in f32 is not "close" to the
kernel, it IS the kernel's arithmetic: the comparison is on the bit
patterns. `reference(case, inputs)` is numpy slicing and f32 ufuncs only;
`run_case(ops, case)` drives the same case through `TorchOps` (any machine)
or `HipOps` (the product path) and returns the same dictionary of arrays.

Buffers. Every destination is a view into a larger allocation with guard
bands of a multiple of 4 floats on both sides (so the view keeps the
16-byte alignment of the allocation), the guards hold a sentinel bit
pattern, and the destination is prefilled with random non-zero data. What
is compared is the WHOLE allocation: the reference works on a copy of the
same allocation, so guards and voxels outside the written region must come
back bit-unchanged and the written region bit-equal. A case may shift a
buffer by one element (`mis`), which makes its base pointer unaligned: the
kernels must then take their scalar path and give the same bits.

Run as `python tests/stitch_cases.py --blend-batch` it drives the batched
blend table through HipOps in this process (the CFX_BLEND_G / CFX_BLEND_NT
knobs are read once per process) and exits non-zero on any mismatch.
"""
import os
import sys
import zlib

import numpy as np

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _REPO not in sys.path:
    sys.path.insert(0, _REPO)

SENTINEL = np.uint32(0xCDCDCDCD)       # a finite f32; compared as bits
GUARD = 8                              # floats before and after; 8 % 4 == 0
NAN_POS = np.uint32(0x7FC00000)
NAN_NEG = np.uint32(0xFFC00000)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def case_rng(case):
    return np.random.RandomState(zlib.crc32(case['id'].encode()) & 0x7FFFFFFF)


def mixed(rng, shape, emin=-6, emax=6):
    """Non-zero f32 of both signs, magnitudes over 2^emin..2^emax with full
    random mantissas (so products and sums round)."""
    mant = 1.0 + rng.random_sample(shape)
    expo = rng.randint(emin, emax + 1, size=shape)
    sign = np.where(rng.random_sample(shape) < 0.5, -1.0, 1.0)
    return (sign * mant * np.exp2(expo)).astype(np.float32)


def guarded(values, mis=0):
    """(allocation, lo, hi): a flat f32 allocation whose [lo, hi) holds
    `values` between sentinel guards. mis=1 starts the view one float past
    a 16-byte boundary."""
    flat = np.ascontiguousarray(values, dtype=np.float32).ravel()
    lo = GUARD + mis
    alloc = np.empty(lo + flat.size + GUARD, dtype=np.float32)
    alloc.view(np.uint32)[:] = SENTINEL
    alloc[lo:lo + flat.size] = flat
    return alloc, lo, lo + flat.size


def bits_mismatch(got, exp, nan_ok=False):
    """Flat indices at which two f32 (or u32-viewable) arrays differ as bit
    patterns. nan_ok: a NaN matches a NaN of any sign and payload (the one
    documented exception: an invalid operation such as inf * 0 makes a
    NaN whose sign differs between x86 and the GPU)."""
    got = np.ascontiguousarray(got)
    exp = np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, \
        (got.shape, exp.shape, got.dtype, exp.dtype)
    bad = got.view(np.uint32).ravel() != exp.view(np.uint32).ravel()
    if nan_ok:
        bad &= ~(np.isnan(got.ravel()) & np.isnan(exp.ravel()))
    return np.nonzero(bad)[0]


def scalar_mismatch(got, exp):
    """A max result: NaN must meet NaN; numbers compare by value (numpy's
    max, like the kernel's, does not order -0.0 against +0.0)."""
    if np.isnan(exp):
        return not np.isnan(got)
    return not (np.float32(got) == np.float32(exp))


def compare(case, got, exp):
    """Raises AssertionError naming the first differing entry."""
    assert sorted(got) == sorted(exp), (sorted(got), sorted(exp))
    for key in sorted(exp):
        if np.ndim(exp[key]) == 0:
            if scalar_mismatch(got[key], exp[key]):
                raise AssertionError(
                    f'{case["id"]}: {key}: got {got[key]!r}, '
                    f'expected {exp[key]!r}')
            continue
        bad = bits_mismatch(got[key], exp[key], case.get('nan_ok', False))
        if bad.size:
            i = int(bad[0])
            g = np.ascontiguousarray(got[key]).view(np.uint32).ravel()[i]
            e = np.ascontiguousarray(exp[key]).view(np.uint32).ravel()[i]
            raise AssertionError(
                f'{case["id"]}: {key}: {bad.size} of {np.size(exp[key])} '
                f'elements differ, first at flat index {i}: '
                f'got 0x{int(g):08x}, expected 0x{int(e):08x}')


# ---------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------
def _ids(prefix, cases):
    for c in cases:
        c['id'] = f'{prefix}-{c["id"]}'
        c['kind'] = prefix
    assert len({c['id'] for c in cases}) == len(cases)
    return cases


# k_u8_to_f32: n in 1..5 is "tail only" and "n4 = 1 plus tail"; 259 holds
# every byte value; 8192 * 256 * 4 + 5 wraps the grid-stride loop
U8_WRAP = 8192 * 256 * 4 + 5
U8_CASES = _ids('u8', [
    dict(id=f'{entry}-n{n}', entry=entry, n=n)
    for entry in ('normalize', 'cast') for n in (1, 2, 3, 4, 5, 259, U8_WRAP)
] + [
    dict(id='normalize-unaligned-src', entry='normalize', n=1031, mis_in=1),
    dict(id='cast-unaligned-dst', entry='cast', n=1031, mis_out=1),
])


def _starts(rng, n, dims, patch, xstep):
    hi = [d - p for d, p in zip(dims, patch)]
    s = np.stack([rng.randint(0, hi[0] + 1, n), rng.randint(0, hi[1] + 1, n),
                  rng.randint(0, hi[2] // xstep + 1, n) * xstep], axis=1)
    s[n // 2] = s[0]                   # a duplicate start
    return s.astype(np.int32)


def _extract_cases():
    rng = np.random.RandomState(1)
    return _ids('extract', [
        # vectorised, px/4 = 66 > 64: second trip of the x loop; C > 1
        dict(id='vec-px264', C=2, dims=(5, 9, 272), patch=(3, 3, 264),
             starts=np.array([[0, 0, 0], [2, 6, 8], [1, 3, 4], [1, 3, 4],
                              [2, 5, 4]], np.int32)),
        # 64 + 1 split; the second launch has 1 * 1 * 3 * 3 = 9 lines (odd)
        dict(id='split-65', C=1, dims=(4, 5, 16), patch=(3, 3, 8),
             starts=_starts(rng, 65, (4, 5, 16), (3, 3, 8), 4)),
        # each scalar trigger alone
        dict(id='scalar-px70', C=2, dims=(4, 5, 80), patch=(2, 3, 70),
             starts=_starts(rng, 5, (4, 5, 80), (2, 3, 70), 4)),
        dict(id='scalar-x0', C=2, dims=(4, 5, 16), patch=(2, 3, 8),
             starts=np.array([[0, 0, 0], [1, 1, 2], [2, 2, 8]], np.int32)),
        dict(id='scalar-W', C=2, dims=(4, 5, 18), patch=(2, 3, 8),
             starts=_starts(rng, 5, (4, 5, 18), (2, 3, 8), 4)),
        # 2 * 8 * 4100 = 65600 lines > 8192 * 4 * 2: grid-stride wrap
        dict(id='wrap', C=2, dims=(8, 4100, 8), patch=(8, 4100, 4),
             starts=np.array([[0, 0, 4]], np.int32)),
        dict(id='unaligned-chunk', C=2, dims=(4, 5, 16), patch=(2, 3, 8),
             starts=np.array([[0, 0, 0], [2, 2, 8], [1, 1, 4]], np.int32),
             mis_chunk=1),
        dict(id='unaligned-out', C=2, dims=(4, 5, 16), patch=(2, 3, 8),
             starts=np.array([[0, 0, 0], [2, 2, 8], [1, 1, 4]], np.int32),
             mis_out=1),
    ])


EXTRACT_CASES = _extract_cases()

# k_blend: out (C, D, H, W), patch (B, C, pz, py, px), calls of
# (batch_index, offset) applied in order. Each base case runs masked and
# unmasked, so vec/scalar x masked/unmasked = the 4 instantiations.
_B_OUT, _B_PATCH = (2, 6, 10, 272), (2, 2, 3, 5, 264)
_BLEND_BASE = [
    # rx = 264 vectorised (66 float4: second x trip); 2*3*5 = 30 lines, %4 = 2
    dict(id='interior', out=_B_OUT, patch=_B_PATCH, calls=[(1, (1, 2, 4))]),
    # low side of every axis, x clipped by 4: stays vectorised, rx = 260
    dict(id='clip-low', out=_B_OUT, patch=_B_PATCH,
         calls=[(0, (-1, -2, -4))]),
    # high side of every axis, x by 4
    dict(id='clip-high', out=_B_OUT, patch=_B_PATCH,
         calls=[(1, (4, 7, 12))]),
    # x clipped by 2 on either side: scalar, rx = 262
    dict(id='clip-x2', out=_B_OUT, patch=_B_PATCH,
         calls=[(0, (1, 2, -2)), (1, (2, 3, 10))]),
    # odd x offset: scalar at full rx = 264 (five 64-lane trips)
    dict(id='odd-x', out=_B_OUT, patch=_B_PATCH, calls=[(1, (1, 2, 3))]),
    dict(id='OW-not-x4', out=(2, 6, 10, 270), patch=_B_PATCH,
         calls=[(1, (1, 2, 4))]),
    # rx = 70 scalar (second trip of the scalar loop), PW % 4 != 0 alone
    dict(id='px70', out=(2, 4, 6, 80), patch=(1, 2, 2, 3, 70),
         calls=[(0, (1, 1, 4))]),
    # C = 3: 27 lines (%4 = 3), then z clipped to one plane: 9 lines (%4 = 1)
    dict(id='lines-27', out=(3, 4, 6, 16), patch=(1, 3, 3, 3, 8),
         calls=[(0, (0, 1, 4))]),
    dict(id='lines-9', out=(3, 4, 6, 16), patch=(1, 3, 3, 3, 8),
         calls=[(0, (-2, 2, 8))]),
    # the same voxels twice and an overlapping neighbour: += not =
    dict(id='accumulate', out=_B_OUT, patch=_B_PATCH,
         calls=[(0, (1, 2, 4)), (1, (1, 2, 4)), (0, (2, 4, 8))]),
    # fully outside and edge-touching on either side: no write at all
    dict(id='outside', out=_B_OUT, patch=_B_PATCH,
         calls=[(0, (6, 0, 0)), (1, (-3, 0, 0)), (0, (0, 10, 0)),
                (1, (0, -5, 0)), (0, (0, 0, 272)), (1, (0, 0, -264)),
                (0, (100, 100, 100))]),
    # 3 * 32 * 1400 = 134400 lines > 8192 * 16: grid-stride wrap
    dict(id='wrap', out=(3, 32, 1400, 4), patch=(1, 3, 32, 1400, 4),
         calls=[(0, (0, 0, 0))]),
]
_BLEND_UNALIGNED = [
    dict(id=f'unaligned-{which}', out=_B_OUT, patch=_B_PATCH,
         calls=[(1, (1, 2, 4)), (0, (-1, -2, -4))], masked=True,
         **{f'mis_{which}': 1})
    for which in ('out', 'patch', 'mask')]
BLEND_CASES = _ids('blend', [
    dict(c, id=f'{c["id"]}-{"masked" if m else "plain"}', masked=m)
    for c in _BLEND_BASE for m in (True, False)] + _BLEND_UNALIGNED)


# k_blend_batch: items (batch_index, oz, oy, ox) on a grid of z-y cells so
# the clipped regions are pairwise disjoint; EMPTY items clip to nothing.
def _cell_items(n, grid, cell, x_of, empty_at=(), clip=True, nbatch=3):
    """One item per (z, y) cell in raster order. A cell on the low or high
    border of an axis gets an offset one voxel outside it when `clip`, so
    the patch is clipped there (the region stays inside its cell)."""
    items, k = [], 0
    for i in range(n):
        if i in empty_at:
            # alternately far outside and edge-touching
            items.append((i % nbatch,) + ((-cell[0], 0, 0) if i % 2 else
                                          (1000, 1000, 1000)))
            continue
        cz, cy = divmod(k, grid[1])
        assert cz < grid[0], 'grid too small'
        oz, oy = cz * cell[0], cy * cell[1]
        if clip and cz == 0:
            oz -= 1
        if clip and cz == grid[0] - 1:
            oz += 1
        if clip and cy == 0:
            oy -= 1
        if clip and cy == grid[1] - 1:
            oy += 1
        items.append((i % nbatch, oz, oy, x_of(k)))
        k += 1
    return np.array(items, dtype=np.int32)


_BB_OUT, _BB_PATCH = (2, 8, 30, 272), (3, 2, 2, 3, 264)   # 4 x 10 cells
_BB_GRID, _BB_CELL = (4, 10), (2, 3)
_BB_BASE = [
    # 33 items = 32 + 1; empties first, middle and last (the second launch
    # is all-empty and must be skipped); rx 264 and 260 in one launch, all
    # x offsets multiples of 4: vectorised
    dict(id='vec-33', out=_BB_OUT, patch=_BB_PATCH,
         items=_cell_items(33, _BB_GRID, _BB_CELL,
                           lambda k: (4, -4, 12, 8, 0)[k % 5],
                           empty_at=(0, 16, 32))),
    # 35 items: the second launch holds two real items and a trailing empty
    dict(id='vec-35', out=_BB_OUT, patch=_BB_PATCH,
         items=_cell_items(35, _BB_GRID, _BB_CELL,
                           lambda k: (8, 4, -4)[k % 3],
                           empty_at=(0, 17, 34))),
    # odd offsets and clips by 2: scalar, rx in {264, 262, 261}
    dict(id='scalar-mixed-rx', out=_BB_OUT, patch=_BB_PATCH,
         items=_cell_items(33, _BB_GRID, _BB_CELL,
                           lambda k: (3, -2, 10, 4, 11)[k % 5],
                           empty_at=(0, 16, 32))),
    dict(id='OW-not-x4', out=(2, 8, 30, 270), patch=_BB_PATCH,
         items=_cell_items(7, _BB_GRID, _BB_CELL, lambda k: (4, 0)[k % 2])),
    dict(id='px70', out=(2, 8, 30, 80), patch=(3, 2, 2, 3, 70),
         items=_cell_items(9, _BB_GRID, _BB_CELL,
                           lambda k: (4, -4, 12)[k % 3], empty_at=(4,))),
    # C = 3, first grid row (z clipped to one plane): 3 * 2 lines for the
    # y-clipped corner cell + 5 * 9 = 51 lines, odd: the G = 2 group tail
    # (51 % 4 = 3, 51 % 8 = 3); asserted below
    dict(id='odd-lines', out=(3, 8, 30, 16), patch=(3, 3, 2, 3, 8),
         items=_cell_items(6, _BB_GRID, _BB_CELL, lambda k: (4, 8)[k % 2]),
         lines=51),
    # 134400 lines > 8192 * 4 * 2: grid-stride wrap at G = 2
    dict(id='wrap', out=(3, 32, 1400, 4), patch=(1, 3, 32, 1400, 4),
         items=np.array([[0, 5000, 0, 0], [0, 0, 0, 0]], np.int32)),
]
_BB_UNALIGNED = [
    dict(id=f'unaligned-{which}', out=_BB_OUT, patch=_BB_PATCH,
         items=_cell_items(6, _BB_GRID, _BB_CELL, lambda k: (4, -4)[k % 2]),
         masked=True, **{f'mis_{which}': 1})
    for which in ('out', 'patch', 'mask')]
BLEND_BATCH_CASES = _ids('blend_batch', [
    dict(c, id=f'{c["id"]}-{"masked" if m else "plain"}', masked=m)
    for c in _BB_BASE for m in (True, False)] + _BB_UNALIGNED)


def batch_regions(case):
    """(lo, hi) of the non-empty clipped regions of a batch case."""
    from chunkflow_amd.grouping import clip_regions
    lo, hi = clip_regions(case['items'][:, 1:], case['patch'][-3:],
                          case['out'][-3:])
    keep = (hi > lo).all(axis=1)
    return lo[keep], hi[keep]


def assert_batch_disjoint(case):
    lo, hi = batch_regions(case)
    for i in range(len(lo)):
        ov = ((lo[i] < hi[:i]) & (lo[:i] < hi[i])).all(axis=1)
        assert not ov.any(), f'{case["id"]}: item regions overlap'
    return len(lo)


def batch_lines(case):
    lo, hi = batch_regions(case)
    r = hi - lo
    return int(case['out'][0] * (r[:, 0] * r[:, 1]).sum())


for _c in BLEND_BATCH_CASES:
    assert_batch_disjoint(_c)
    assert batch_lines(_c) == _c.get('lines', batch_lines(_c)), _c['id']

# k_reciprocal: 2097155 = 8192 * 256 + 3 wraps
RECIP_CASES = _ids('reciprocal', [
    dict(id=f'n{n}', n=n) for n in (1, 257, 8192 * 256 + 3)])

# k_maskmul and the fused max. 512 float4 per block per trip (256 threads,
# U = 2), 8192 blocks: MM_WRAP4 float4s wrap; MM_WRAP4 + 5 is odd, its last
# float4 is a lone U tail in the wrapped part.
MM_WRAP4 = 8192 * 512
MM_BIG = (MM_WRAP4 + 5) * 4
MASKMUL_CASES = _ids('maskmul', [
    # n4 = 3 (odd, one U tail); peak in the last channel
    dict(id='C3-n12-last-channel', C=3, n=12, fused=True, peak=2 * 12 + 5),
    # n4 = 1029 (odd, three blocks); peak in the U tail (last float4)
    dict(id='C3-n4116-tail', C=3, n=4116, fused=True, peak=4116 + 4114),
    dict(id='C1-n4116', C=1, n=4116, fused=True, peak=700),
    dict(id='C3-n4116-plain', C=3, n=4116, fused=False),
    # n % 4 != 0: fused reports "unavailable", ops falls back to cfx_max
    dict(id='C3-n4117-fallback', C=3, n=4117, fused=True, peak=4117 + 4116),
    dict(id='C1-n4117-plain', C=1, n=4117, fused=False),
    dict(id='C3-all-negative', C=3, n=4116, fused=True, negative=True),
    dict(id='C3-inf', C=3, n=4116, fused=True, peak=2 * 4116 + 131,
         peak_value=np.inf),
    # wrapped part, not the tail / the lone tail float4
    dict(id='C1-wrap-peak-wrapped', C=1, n=MM_BIG, fused=True,
         peak=(MM_WRAP4 + 2) * 4 + 1),
    dict(id='C1-wrap-peak-tail', C=1, n=MM_BIG, fused=True,
         peak=MM_BIG - 2),
    # unaligned views: scalar multiply, fused max unavailable (-2)
    dict(id='C3-unaligned-out', C=3, n=4116, fused=True, peak=4116 + 9,
         mis_out=1),
    dict(id='C3-unaligned-mask', C=3, n=4116, fused=True, peak=4116 + 9,
         mis_mask=1),
    dict(id='C3-unaligned-out-plain', C=3, n=4116, fused=False, mis_out=1),
])

# k_max: 256 threads, 4096 blocks: n > MAX_WRAP wraps; element MAX_WRAP + k
# is read by thread k of block 0. A lane takes its elements four at a time
# (i, i + MAX_WRAP, ...), then one at a time: MAX_X4 gives threads below 257
# one four-element trip and the rest four single ones; MAX_X9 gives every
# thread two four-element trips and threads below 3 a single one after.
MAX_WRAP = 4096 * 256
MAX_BIG = MAX_WRAP + 257
MAX_X4 = 4 * MAX_WRAP + 257
MAX_X9 = 8 * MAX_WRAP + 3
MAX_CASES = _ids('max', [
    dict(id='n1', n=1, peak=0),
    dict(id='n63', n=63, peak=62),
    dict(id='n65-lane0', n=65, peak=64),
    dict(id='n65-lane17', n=65, peak=17),
    dict(id='wrap-peak-wrapped-lane37', n=MAX_BIG, peak=MAX_WRAP + 37),
    dict(id='wrap-peak-last', n=MAX_BIG, peak=MAX_BIG - 1),
    dict(id='wrap-peak-body', n=MAX_BIG, peak=123457),
    dict(id='x4-peak-slot2', n=MAX_X4, peak=2 * MAX_WRAP + 100),
    dict(id='x4-peak-single', n=MAX_X4, peak=3 * MAX_WRAP + 300),
    dict(id='x9-peak-second-trip', n=MAX_X9, peak=5 * MAX_WRAP + 70000),
    dict(id='x9-peak-last', n=MAX_X9, peak=MAX_X9 - 1),
    dict(id='x9-all-negative', n=MAX_X9, negative=True),
    dict(id='all-negative', n=1000, negative=True),
    dict(id='all-negative-wrap', n=MAX_BIG, negative=True),
    dict(id='zeros-neg-vs-pos', n=1000, zeros=True, peak=333,
         peak_value=0.0),
    dict(id='zeros-all-negative', n=1000, zeros=True),
])


# NaN in the sanity scan: both quiet-NaN signs at the first element, the
# last, a lane other than 0, the wrapped part and the U tail
def _nan_cases():
    out = []
    for name, bits in (('pos', NAN_POS), ('neg', NAN_NEG)):
        for where, n, at in (('first', 1000, 0), ('last', 1000, 999),
                             ('lane5', 1000, 64 + 5),
                             ('wrapped', MAX_BIG, MAX_WRAP + 70),
                             ('wrap-last', MAX_BIG, MAX_BIG - 1),
                             ('x4-slot3', MAX_X4, 3 * MAX_WRAP + 77),
                             ('x9-slot1', MAX_X9, 5 * MAX_WRAP + 12345),
                             ('x9-last', MAX_X9, MAX_X9 - 1)):
            out.append(dict(kind='max', id=f'max-nan-{name}-{where}', n=n,
                            nan_at=at, nan_bits=bits))
        for where, C, n, at in (('first', 3, 4116, 0),
                                ('last', 3, 4116, 3 * 4116 - 1),
                                ('lane5', 3, 4116, 4116 + (64 + 5) * 8 + 2),
                                ('tail', 3, 4116, 4116 + 4113),
                                ('fallback', 3, 4117, 2 * 4117 + 4116),
                                ('wrapped', 1, MM_BIG, (MM_WRAP4 + 3) * 4),
                                ('wrap-tail', 1, MM_BIG, MM_BIG - 3)):
            out.append(dict(kind='maskmul', id=f'maskmul-nan-{name}-{where}',
                            C=C, n=n, fused=True, nan_at=at, nan_bits=bits,
                            nan_ok=True))
    return out


NAN_CASES = _nan_cases()

# k_crop: (C, D, H, W) -> margins (-z, -y, -x, +z, +y, +x)
CROP_CASES = _ids('crop', [
    # vectorised, oW = 260 (65 float4: second x trip)
    dict(id='vec-oW260', shape=(2, 5, 7, 272), margins=(1, 2, 4, 1, 0, 8)),
    dict(id='vec-zero-low', shape=(2, 5, 7, 272),
         margins=(0, 0, 0, 2, 3, 12)),
    dict(id='no-margins', shape=(2, 3, 4, 16), margins=(0, 0, 0, 0, 0, 0)),
    dict(id='3d', shape=(5, 7, 24), margins=(1, 0, 4, 0, 2, 4)),
    # each scalar trigger alone (oW stays 260 where it is not the trigger)
    dict(id='scalar-W', shape=(2, 5, 7, 270), margins=(1, 2, 4, 1, 0, 6)),
    dict(id='scalar-oW', shape=(2, 5, 7, 272), margins=(1, 2, 4, 1, 0, 6)),
    dict(id='scalar-m2', shape=(2, 5, 7, 272), margins=(1, 2, 2, 1, 0, 10)),
    # 2 * 40 * 419 = 33520 lines > 8192 * 4: grid-stride wrap
    dict(id='wrap', shape=(2, 40, 420, 4), margins=(0, 1, 0, 0, 0, 0)),
    dict(id='unaligned-in', shape=(2, 5, 7, 32), margins=(1, 2, 4, 1, 0, 8),
         mis_in=1),
    dict(id='unaligned-out', shape=(2, 5, 7, 32), margins=(1, 2, 4, 1, 0, 8),
         mis_out=1),
    # empty output: raises, writes nothing
    dict(id='empty', shape=(2, 5, 7, 32), margins=(3, 0, 0, 2, 0, 0),
         empty=True),
])

# k_myelin: in (channels, dims) -> out (channels - 1, dims); the threshold
# is exactly representable so "equal to the threshold" means the same in
# every implementation (strict <: such voxels are dropped)
MYELIN_THR = 0.375
MYELIN_CASES = _ids('myelin', [
    dict(id='C4-small', channels=4, dims=(3, 5, 7), nan_ok=True),
    dict(id='C2-small', channels=2, dims=(1, 1, 300), nan_ok=True),
    dict(id='C2-wrap', channels=2, dims=(1, 1, 8192 * 256 + 3),
         nan_ok=True),
    dict(id='C4-wrap', channels=4, dims=(1, 1, 8192 * 256 + 3),
         nan_ok=True),
])

FAMILIES = {
    'u8': U8_CASES, 'extract': EXTRACT_CASES, 'blend': BLEND_CASES,
    'blend_batch': BLEND_BATCH_CASES, 'reciprocal': RECIP_CASES,
    'maskmul': MASKMUL_CASES, 'max': MAX_CASES, 'crop': CROP_CASES,
    'myelin': MYELIN_CASES, 'nan': NAN_CASES,
}


# ---------------------------------------------------------------------------
# inputs per case (host numpy; deterministic)
# ---------------------------------------------------------------------------
def make_inputs(case):
    rng = case_rng(case)
    kind = case['kind']
    if kind == 'u8':
        n = case['n']
        src = rng.randint(0, 256, size=n).astype(np.uint8)
        if n >= 256:
            src[:256] = np.arange(256, dtype=np.uint8)
        return dict(src=src, dst=mixed(rng, n))
    if kind == 'extract':
        pz, py, px = case['patch']
        n = len(case['starts'])
        return dict(chunk=mixed(rng, (case['C'],) + tuple(case['dims'])),
                    dst=mixed(rng, (n, case['C'], pz, py, px)))
    if kind in ('blend', 'blend_batch'):
        # magnitudes around 1 on every side so that the product's rounding
        # is visible in the sum (see the contraction premise test)
        return dict(dst=mixed(rng, case['out'], -2, 2),
                    patch=mixed(rng, case['patch'], -2, 2),
                    mask=mixed(rng, case['patch'][-3:], -2, 2))
    if kind == 'reciprocal':
        n = case['n']
        buf = mixed(rng, n, -20, 20)
        # reciprocals that are denormal, overflow, or hit +-inf
        special = np.array([3e38, -2.5e38, 1e-39, -1e-40, 0.0, -0.0, 1e38,
                            np.inf, -np.inf, 1.1754944e-38, 2.0 ** 126,
                            2.0 ** 127], dtype=np.float32)
        k = min(n, special.size)
        at = rng.choice(n, k, replace=False)
        buf[at] = special[:k]
        return dict(dst=buf)
    if kind in ('maskmul', 'max'):
        n = case['n']
        C = case.get('C', 1)
        dst = mixed(rng, C * n)
        mask = mixed(rng, n)
        if kind == 'maskmul' and case.get('negative'):
            dst, mask = -np.abs(dst), np.abs(mask)
        if kind == 'max' and case.get('negative'):
            dst = -np.abs(dst)
        if case.get('zeros'):
            dst[:] = -0.0
        if 'peak' in case:
            # products are below 2^14; the peak stands clear of them
            dst[case['peak']] = case.get('peak_value', 3.0e5)
            mask[case['peak'] % n] = 1.0
        if 'nan_at' in case:
            dst.view(np.uint32)[case['nan_at']] = case['nan_bits']
        out = dict(dst=dst)
        if kind == 'maskmul':
            out['mask'] = mask
        return out
    if kind == 'crop':
        shape = case['shape']
        oshape = _crop_shape(case)
        nout = int(np.prod(oshape)) if not case.get('empty') else 64
        return dict(src=mixed(rng, shape), dst=mixed(rng, nout))
    if kind == 'myelin':
        ch, dims = case['channels'], tuple(case['dims'])
        src = mixed(rng, (ch,) + dims, -3, 1)
        n = int(np.prod(dims))
        flat = src.reshape(ch, n)
        k = max(1, n // 16)
        flat[-1, rng.choice(n, k, replace=False)] = MYELIN_THR
        flat[-1, rng.choice(n, k, replace=False)] = np.nan
        flat[-1, rng.choice(n, k, replace=False)] = -np.inf
        assert (flat[-1] == np.float32(MYELIN_THR)).any()
        for c in range(ch - 1):
            flat[c, rng.choice(n, k, replace=False)] = np.nan
            flat[c, rng.choice(n, k, replace=False)] = np.inf
            flat[c, rng.choice(n, k, replace=False)] = -np.inf
        return dict(src=src, dst=mixed(rng, (ch - 1,) + dims))
    raise KeyError(kind)


def _crop_shape(case):
    shape, m = case['shape'], case['margins']
    d, h, w = shape[-3:]
    return tuple(shape[:-3]) + (d - m[0] - m[3], h - m[1] - m[4],
                                w - m[2] - m[5])


# ---------------------------------------------------------------------------
# numpy references
# ---------------------------------------------------------------------------
def _clip(offset, pdims, odims):
    dst, src = [], []
    for off, p, h in zip(offset, pdims, odims):
        lo, hi = max(off, 0), min(off + p, h)
        if hi <= lo:
            return None, None
        dst.append(slice(lo, hi))
        src.append(slice(lo - off, hi - off))
    return tuple(dst), tuple(src)


def _ref_blend(out, patch, mask, offset):
    """out[region] += patch[region'] * mask[region'] in f32: the product is
    rounded to f32, then the sum is (two roundings, no fused multiply-add)."""
    dst, src = _clip(offset, patch.shape[-3:], out.shape[-3:])
    if dst is None:
        return
    term = patch[(slice(None),) + src]
    if mask is not None:
        term = term * mask[src]
    assert term.dtype == np.float32
    out[(slice(None),) + dst] += term


def reference(case, inputs):
    """The expected result dictionary: whole allocations (guards included)
    as flat f32 arrays, and scalars."""
    kind = case['kind']
    alloc, lo, hi = guarded(inputs['dst'], case.get('mis_out', 0))
    view = alloc[lo:hi]
    res = {}
    if kind == 'u8':
        x = inputs['src'].astype(np.float32)
        if case['entry'] == 'normalize':
            view[:] = x / np.float32(127.5) - np.float32(1.0)
        else:
            view[:] = x / np.float32(255.0)
    elif kind == 'extract':
        pz, py, px = case['patch']
        out = view.reshape(inputs['dst'].shape)
        for i, (z0, y0, x0) in enumerate(case['starts']):
            out[i] = inputs['chunk'][:, z0:z0 + pz, y0:y0 + py, x0:x0 + px]
    elif kind == 'blend':
        out = view.reshape(case['out'])
        mask = inputs['mask'] if case['masked'] else None
        for b, off in case['calls']:
            _ref_blend(out, inputs['patch'][b], mask, off)
    elif kind == 'blend_batch':
        out = view.reshape(case['out'])
        mask = inputs['mask'] if case['masked'] else None
        for b, oz, oy, ox in case['items']:
            _ref_blend(out, inputs['patch'][b], mask,
                       (int(oz), int(oy), int(ox)))
    elif kind == 'reciprocal':
        with np.errstate(all='ignore'):
            view[:] = np.float32(1.0) / view
    elif kind == 'maskmul':
        with np.errstate(all='ignore'):
            out = view.reshape(case['C'], case['n'])
            out *= inputs['mask']
            if case['fused']:
                res['max'] = np.float32(np.max(out))   # propagates NaN
    elif kind == 'max':
        res['max'] = np.float32(np.max(view))
    elif kind == 'crop':
        if not case.get('empty'):
            m = case['margins']
            d, h, w = case['shape'][-3:]
            view[:] = inputs['src'][..., m[0]:d - m[3], m[1]:h - m[4],
                                    m[2]:w - m[5]].ravel()
    elif kind == 'myelin':
        src = inputs['src']
        with np.errstate(all='ignore'):
            keep = src[-1] < np.float32(MYELIN_THR)
            view[:] = (src[:-1] * keep).ravel()
            assert (src[:-1] * keep).dtype == np.float32
    else:
        raise KeyError(kind)
    res['dst'] = alloc
    return res


# ---------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------
def _device_view(ops, values, mis=0, dtype=np.float32):
    """Upload `values` into a guarded allocation on ops.device; returns
    (allocation tensor, view tensor shaped like values)."""
    import torch
    values = np.asarray(values)
    if dtype == np.uint8:
        # u8 source: 4-byte alignment is what matters; shift by one byte
        lo = 16 + mis
        alloc = np.full(lo + values.size + 16, 0xCD, dtype=np.uint8)
        alloc[lo:lo + values.size] = values.ravel()
        hi = lo + values.size
    else:
        alloc, lo, hi = guarded(values, mis)
    t = torch.from_numpy(alloc).to(ops.device)
    return t, t[lo:hi].view(values.shape)


def run_case(ops, case, inputs=None):
    """Run one case through `ops` (TorchOps or HipOps); returns the same
    dictionary as reference(). Where HipOps allocates its own result
    (u8 casts, crop, myelin) the kernel is called through ops.cfx with a
    guarded destination, which is what the HipOps method does with a fresh
    tensor; TorchOps results are copied into the guarded view."""
    import torch
    if inputs is None:
        inputs = make_inputs(case)
    kind = case['kind']
    alloc, dst = _device_view(ops, inputs['dst'], case.get('mis_out', 0))
    res = {}
    with np.errstate(all='ignore'):
        if kind == 'u8':
            _, src = _device_view(ops, inputs['src'], case.get('mis_in', 0),
                                  dtype=np.uint8)
            if ops.is_hip:
                if case['entry'] == 'normalize':
                    ops.cfx.normalize_intensity(src.data_ptr(),
                                                dst.data_ptr(), src.numel())
                else:
                    ops.cfx.cast_u8_f32_div(src.data_ptr(), dst.data_ptr(),
                                            src.numel(), 255.0)
            elif case['entry'] == 'normalize':
                dst.copy_(ops.normalize_intensity(src))
            else:
                dst.copy_(ops.cast_div(src, 255.0))
        elif kind == 'extract':
            _, chunk = _device_view(ops, inputs['chunk'],
                                    case.get('mis_chunk', 0))
            ops.extract(chunk, case['starts'], tuple(case['patch']), dst)
        elif kind in ('blend', 'blend_batch'):
            _, patch = _device_view(ops, inputs['patch'],
                                    case.get('mis_patch', 0))
            mask = None
            if case['masked']:
                _, mask = _device_view(ops, inputs['mask'],
                                       case.get('mis_mask', 0))
            if kind == 'blend':
                for b, off in case['calls']:
                    ops.blend(dst, patch, b, off, mask=mask)
            else:
                ops.blend_batch(dst, patch, case['items'], mask=mask)
        elif kind == 'reciprocal':
            if ops.is_hip:
                ops.cfx.reciprocal(dst.data_ptr(), dst.numel())
            else:
                dst.copy_(1.0 / dst)     # as TorchOps.build_chunk_mask does
        elif kind == 'maskmul':
            out = dst.view(case['C'], case['n'])
            _, mask = _device_view(ops, inputs['mask'],
                                   case.get('mis_mask', 0))
            if case['fused']:
                res['max'] = np.float32(ops.multiply_mask_max(out, mask))
            else:
                ops.multiply_mask(out, mask)
        elif kind == 'max':
            res['max'] = np.float32(ops.max(dst))
        elif kind == 'crop':
            _, src = _device_view(ops, inputs['src'], case.get('mis_in', 0))
            shape, m = case['shape'], case['margins']
            if ops.is_hip:
                from chunkflow_amd.hip import CfxError
                try:
                    ops.cfx.crop_margin(
                        src.data_ptr(), dst.data_ptr(),
                        1 if len(shape) == 3 else shape[0], shape[-3:], m)
                    raised = False
                except CfxError:
                    raised = True
                assert raised == bool(case.get('empty')), \
                    f'{case["id"]}: empty-output error raised={raised}'
            else:
                got = ops.crop_margin(src, m)
                if case.get('empty'):
                    assert got.numel() == 0
                else:
                    dst.copy_(got.reshape(-1))
        elif kind == 'myelin':
            _, src = _device_view(ops, inputs['src'])
            if ops.is_hip:
                ops.cfx.mask_using_last_channel(
                    src.data_ptr(), dst.data_ptr(), case['channels'],
                    case['dims'], MYELIN_THR)
            else:
                dst.copy_(ops.mask_using_last_channel(src, MYELIN_THR))
        else:
            raise KeyError(kind)
    ops.sync()
    res['dst'] = alloc.cpu().numpy()
    return res


def check_case(ops, case):
    inputs = make_inputs(case)
    compare(case, run_case(ops, case, inputs), reference(case, inputs))


# ---------------------------------------------------------------------------
# child-process entry for the blend tuning knobs
# ---------------------------------------------------------------------------
def main(argv):
    if argv != ['--blend-batch']:
        print('usage: stitch_cases.py --blend-batch', file=sys.stderr)
        return 2
    from chunkflow_amd.ops import HipOps
    ops = HipOps(0)
    failed = 0
    for case in BLEND_BATCH_CASES:
        try:
            check_case(ops, case)
        except AssertionError as e:
            failed += 1
            print(f'MISMATCH {e}')
    print(f'blend-batch table: {len(BLEND_BATCH_CASES)} cases, '
          f'{failed} mismatches (CFX_BLEND_G='
          f'{os.environ.get("CFX_BLEND_G", "")!r} CFX_BLEND_NT='
          f'{os.environ.get("CFX_BLEND_NT", "")!r})')
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
