"""Bit-exact pins for the union-find labeller (chunkflow_amd/csrc/cc.hip)
at the scales where it can go wrong: volumes above one trip of the
grid-stride loops, volumes around the borders of the rank chunks, one chain
through a whole volume, trees joined only at the end of raster order, the
complete truth table of the neighbour predicate, and the threshold step of
the operator in every chunk dtype.

Shapes, generators, references and the driver live in tests/cc_cases.py.
The CPU tests hold the references against a flood fill that shares no code
with them and check the premises the GPU tests rest on; the GPU tests
compare bytes. Every labelling here writes into buffers prefilled with
0xA5A5A5A5 between guard bands (cc_cases.run_case)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_cases as cc  # noqa: E402

gpu = pytest.mark.gpu

# all 256 2x2x2 patterns plus 512 seeded random 3x3x3 patterns
# (cc_cases.cells); counted by the flood fill, confirmed by scipy below
CELLS_COUNTS = {6: 1594, 18: 828, 26: 787}


@pytest.fixture(scope='module')
def ops():
    from chunkflow_amd.ops import HipOps
    return HipOps(0)


# ---------------------------------------------------------------------------
# CPU: constants, shapes, references
# ---------------------------------------------------------------------------
def test_parsed_constants():
    with open(cc.CC_SOURCE) as f:
        text = f.read()
    scan_chunk, cap, block = cc.parse_geometry(text)
    assert (scan_chunk, cap, block) == (cc.SCAN_CHUNK, cc.GRID_CAP, cc.BLOCK)
    assert cc.WRAP == cap * block
    # one 64-lane wave ranks a chunk in whole ballots; 256-thread blocks
    assert scan_chunk % 64 == 0 and block % 64 == 0 and cap >= 1
    # a retune that hides a constant from the parser must not pass quietly
    for broken in (text.replace('SCAN_CHUNK =', 'SCAN_CHUNK_2 ='),
                   text.replace('want < ', 'want <= '),
                   text.replace('dim3(grid_for(n, 256)), dim3(256)',
                                'dim3(grid_for(n, 256)), dim3(128)', 1),
                   text.replace('grid_for(n, 256)', 'grid_of(n)')):
        assert broken != text
        with pytest.raises(RuntimeError):
            cc.parse_geometry(broken)


def test_big_shape_properties():
    n = cc.nvox(cc.BIG)
    assert n > cc.WRAP                       # a second grid-stride trip
    assert n - cc.WRAP < cc.WRAP // 64       # ... of a small part only
    assert n % 64 != 0                       # a partial last ballot
    assert 1 < n % cc.SCAN_CHUNK < cc.SCAN_CHUNK   # a partial last chunk
    assert cc.big_ok(cc.BIG)
    assert not cc.big_ok((32, 256, 256))     # exactly WRAP today: no wrap
    assert n < 2 ** 31


def test_shape_tables():
    sc = cc.SCAN_CHUNK
    assert set(cc.RANK_NS) == {1, 63, 64, 65, sc - 1, sc, sc + 1,
                               2 * sc + 64, 3 * sc + 1}
    flat = [s for s in cc.RANK_SHAPES if s[:2] == (1, 1)]
    assert sorted(cc.nvox(s) for s in flat) == sorted(cc.RANK_NS)
    folded = [s for s in cc.RANK_SHAPES if s[:2] != (1, 1)]
    assert {cc.nvox(s) for s in folded} <= set(cc.RANK_NS)
    # the chunk border falls inside a plane of a genuinely 3-D volume for
    # the chunk size itself and its two neighbours
    for n in (sc - 1, sc, sc + 1):
        s = cc.fold3(n)
        assert s is not None and cc.nvox(s) == n and s in cc.RANK_SHAPES, n
    assert cc.fold3(sc)[0] >= 2 and cc.fold3(sc - 1)[0] >= 2
    assert cc.fold3(1) is None and cc.fold3(7) is None
    assert cc.fold3(65) == (1, 5, 13) and cc.fold3(64) == (4, 4, 4)
    for s in cc.DEGENERATE_SHAPES:
        assert s in cc.EDGE_SHAPES
    assert all(cc.nvox(s) <= 5000 for s in cc.SMALL_SHAPES)


def test_label_mappings_keep_values_distinct():
    vol = np.arange(8).reshape(2, 2, 2)
    for dtype in cc.LABEL_DTYPES:
        out = cc.as_dtype(vol, dtype)
        assert out.dtype == dtype and len(np.unique(out)) == 8
        assert out.ravel()[0] == 0
    u64 = cc.as_dtype(vol, np.uint64).ravel()[1:]
    assert len(np.unique(u64 & np.uint64(0xFFFFFFFF))) == 1


@pytest.mark.parametrize('connectivity', cc.CONNECTIVITIES)
def test_references_equal_flood_fill_on_small_cases(connectivity):
    """scipy, equal_value_label and its vectorised restatement against the
    independent flood fill, labels and counts."""
    from chunkflow_amd.connected import equal_value_label
    bad = []
    for shape in cc.SMALL_SHAPES:
        for name in cc.GENERATORS_ALL:
            vol = cc.volume(name, shape)
            flood, n_flood = cc.flood_label(vol, connectivity)
            ref, n_ref = cc.binary_reference(vol, connectivity)
            if flood.tobytes() != ref.tobytes() or n_flood != n_ref:
                bad.append((shape, name, 'binary', n_flood, n_ref))
            bad += [(shape, name, p) for p in
                    cc.invariant_problems(vol != 0, ref, n_ref)]
            lvol = cc.volume(name, shape, labels=True)
            flood, n_flood = cc.flood_label(lvol, connectivity,
                                            equal_value=True)
            slow = equal_value_label(np.ascontiguousarray(lvol),
                                     connectivity).astype(np.uint32)
            fast, n_fast = cc.equal_value_fast(lvol, connectivity)
            if not (flood.tobytes() == slow.tobytes() == fast.tobytes()) \
                    or not (n_flood == n_fast == int(slow.max())):
                bad.append((shape, name, 'labels', n_flood, n_fast))
    assert not bad, bad


def test_truth_table_references_and_counts():
    vol = cc.cells()
    assert vol.shape == (44, 32, 32)
    # every 2x2x2 pattern is there, in cell order
    for p in (0, 1, 0x96, 255):
        cz, cy, cx = p // 64, (p // 8) % 8, p % 8
        block = vol[3 * cz:3 * cz + 2, 3 * cy:3 * cy + 2, 3 * cx:3 * cx + 2]
        assert sum(int(b) << i for i, b in enumerate(block.ravel())) == p
    for connectivity in cc.CONNECTIVITIES:
        flood, n = cc.flood_label(vol, connectivity)
        ref, n_ref = cc.binary_reference(vol, connectivity)
        assert flood.tobytes() == ref.tobytes()
        assert n == n_ref == CELLS_COUNTS[connectivity]
        _, n = cc.flood_label(cc.stairs(), connectivity)
        assert n == cc.STAIRS_COUNTS[connectivity]
        assert cc.binary_reference(cc.stairs(), connectivity)[1] == n
    assert len(set(cc.STAIRS_COUNTS.values())) == 3
    assert len(set(CELLS_COUNTS.values())) == 3


def test_generator_structure():
    """The structure the volumes were built for, stated directly."""
    shape = (5, 8, 9)
    # serpentine: one 6-component rooted at voxel 0, one voxel wide (every
    # path voxel has at most two path neighbours, exactly two ends)
    serp = cc.serpentine3d(shape)
    lab, n = cc.flood_label(serp, 6)
    assert n == 1 and lab.ravel()[0] == 1
    pad = np.pad(serp, 1)
    deg = sum(np.roll(pad, s, axis=a) for a in range(3) for s in (1, -1))
    deg = deg[1:-1, 1:-1, 1:-1][serp == 1]
    assert deg.max() == 2 and (deg == 1).sum() == 2
    assert serp[0::2, 0::2, :].all() and serp[1::2].sum() == shape[0] // 2
    assert set(np.unique(cc.serpentine3d(shape, labels=True))) == {1, 2}
    # combs: (H + 1) // 2 teeth, separate at every connectivity until the
    # spine joins them; the spine lies in the last (first) plane only
    teeth = cc.comb_teeth(shape)
    for connectivity in cc.CONNECTIVITIES:
        assert cc.flood_label(teeth, connectivity)[1] == (shape[1] + 1) // 2
        assert cc.flood_label(cc.late_comb(shape), connectivity)[1] == 1
        assert cc.flood_label(cc.early_comb(shape), connectivity)[1] == 1
    late, early = cc.late_comb(shape), cc.early_comb(shape)
    assert (late[:-1] == teeth[:-1]).all() and (late != teeth).any()
    assert early.ravel()[0] == 1 and late.ravel()[-1] == 1
    assert (early == late[::-1, ::-1, ::-1]).all()
    # stairs: the stated counts
    for gen, counts in ((cc.stair18, cc.stair18_counts),
                        (cc.stair26, cc.stair26_counts)):
        for connectivity in cc.CONNECTIVITIES:
            assert cc.flood_label(gen(shape), connectivity)[1] == \
                counts(shape)[connectivity]
    assert cc.stair18_counts(shape) == {6: 24, 18: 3, 26: 3}
    assert cc.stair26_counts(shape)[26] < cc.stair26_counts(shape)[18]
    # checkerboard: all roots at 6, one component otherwise
    board = cc.checkerboard(shape)
    assert cc.flood_label(board, 6)[1] == int(board.sum())
    assert cc.flood_label(board, 18)[1] == cc.flood_label(board, 26)[1] == 1


def test_invariant_checker_catches_wrong_labellings():
    vol = cc.volume('random_p50', (5, 7, 9))
    ref, n = cc.binary_reference(vol, 6)
    assert n >= 3 and cc.invariant_problems(vol != 0, ref, n) == []
    swapped = ref.copy()
    swapped[ref == 1], swapped[ref == 2] = 2, 1
    assert cc.invariant_problems(vol != 0, swapped, n)
    poisoned = ref.copy()
    poisoned.ravel()[np.flatnonzero(vol.ravel())[0]] = cc.POISON
    assert cc.invariant_problems(vol != 0, poisoned, n)
    leaked = ref.copy()
    leaked.ravel()[np.flatnonzero(vol.ravel() == 0)[0]] = 1
    assert cc.invariant_problems(vol != 0, leaked, n)
    assert cc.invariant_problems(vol != 0, ref, n + 1)


# ---------------------------------------------------------------------------
# GPU: wrap scale
# ---------------------------------------------------------------------------
def _check(ops, bad, tag, vol, connectivity, entry, want, n_want,
           dtype=np.uint8, invariants=False):
    """One labelling against its reference; returns the labels."""
    got, n, problems = cc.run_case(ops, vol, connectivity, entry, dtype)
    if n != n_want:
        bad.append((tag, 'n_components', n, n_want))
    if got.tobytes() != want.tobytes():
        wrong = np.flatnonzero(got.ravel() != want.ravel())
        bad.append((tag, 'labels', f'{wrong.size} voxels differ, first at '
                    f'{int(wrong[0])}: got {int(got.ravel()[wrong[0]])}, '
                    f'expected {int(want.ravel()[wrong[0]])}'))
    bad += [(tag, p) for p in problems]
    if invariants:
        bad += [(tag, p) for p in cc.invariant_problems(vol != 0, got, n)]
        # the labelling is a fixed point of the equal-value entry
        again, n_again, problems = cc.run_case(ops, got, connectivity,
                                               'labels')
        if again.tobytes() != got.tobytes() or n_again != n:
            bad.append((tag, 'relabelling its own output', n_again, n))
        bad += [(tag, 'relabel', p) for p in problems]
    return got


def _wrap_connectivities(name):
    return (6, 18, 26) if name in ('checkerboard', 'random_p50',
                                   'random_p31') else (6, 26)


@gpu
@pytest.mark.parametrize('name', sorted(cc.GENERATORS))
def test_wrap_scale_binary(ops, name):
    """cfx_connected_components above one grid-stride trip == scipy."""
    bad = []
    vol = cc.volume(name, cc.BIG)
    for connectivity in _wrap_connectivities(name):
        want, n_want = cc.reference(name, cc.BIG, connectivity, 'binary')
        _check(ops, bad, (name, connectivity), vol, connectivity, 'binary',
               want, n_want, invariants=True)
    assert not bad, bad


@gpu
@pytest.mark.parametrize('dtype', cc.LABEL_DTYPES, ids=['u8', 'u32', 'u64'])
@pytest.mark.parametrize('name', ['serpentine3d', 'late_comb', 'random_k2',
                                  'checkerboard'])
def test_wrap_scale_equal_value(ops, name, dtype):
    """cfx_connected_components_labels above one trip == the equal-value
    reference; on a volume of one value also == the binary entry."""
    bad = []
    vol = cc.volume(name, cc.BIG, labels=True)
    for connectivity in _wrap_connectivities(name):
        want, n_want = cc.reference(name, cc.BIG, connectivity, 'labels')
        got = _check(ops, bad, (name, connectivity), vol, connectivity,
                     'labels', want, n_want, dtype=dtype, invariants=True)
        if vol.max() == 1:
            binary, n, _ = cc.run_case(ops, vol, connectivity, 'binary')
            if binary.tobytes() != got.tobytes() or n != n_want:
                bad.append((name, connectivity, 'binary entry differs'))
    assert not bad, bad


@gpu
def test_same_answer_every_time(ops):
    """Three labellings of the same volume into fresh poisoned buffers."""
    bad = []
    for name, connectivity in (('late_comb', 6), ('random_p31', 26),
                               ('all_foreground', 26)):
        vol = cc.volume(name, cc.BIG)
        want, n_want = cc.reference(name, cc.BIG, connectivity, 'binary')
        runs = [_check(ops, bad, (name, connectivity, k), vol, connectivity,
                       'binary', want, n_want) for k in range(3)]
        if not (runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()):
            bad.append((name, connectivity, 'runs differ'))
    assert not bad, bad


@gpu
def test_context_scratch_reuse():
    """Large, small, large on one context: the per-chunk count array grows
    once and is reused by the smaller call."""
    from chunkflow_amd.ops import HipOps
    own = HipOps(0)
    bad = []
    for name, shape, connectivity in (('random_p50', cc.BIG, 6),
                                      ('checkerboard', (1, 1, 65), 6),
                                      ('random_k7', cc.BIG, 26)):
        want, n_want = cc.reference(name, shape, connectivity, 'binary')
        _check(own, bad, (name, shape), cc.volume(name, shape),
               connectivity, 'binary', want, n_want)
        want, n_want = cc.reference(name, shape, connectivity, 'labels')
        _check(own, bad, (name, shape, 'labels'),
               cc.volume(name, shape, labels=True), connectivity, 'labels',
               want, n_want, dtype=np.uint32)
    assert not bad, bad


# ---------------------------------------------------------------------------
# GPU: rank-chunk borders, degenerate extents, the truth table
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('connectivity', cc.CONNECTIVITIES)
def test_rank_edges_and_degenerate_extents(ops, connectivity):
    bad = []
    k = 0
    for shape in cc.EDGE_SHAPES:
        for name in cc.EDGE_GENERATORS:
            want, n_want = cc.reference(name, shape, connectivity, 'binary')
            _check(ops, bad, (shape, name, 'binary'), cc.volume(name, shape),
                   connectivity, 'binary', want, n_want)
            want, n_want = cc.reference(name, shape, connectivity, 'labels')
            _check(ops, bad, (shape, name, 'labels'),
                   cc.volume(name, shape, labels=True), connectivity,
                   'labels', want, n_want, dtype=cc.LABEL_DTYPES[k % 3])
            k += 1
    assert not bad, bad


@gpu
def test_neighbour_truth_table(ops):
    """Every 2x2x2 pattern and 512 random 3x3x3 patterns in one call per
    connectivity, and the edge and corner stairs."""
    bad = []
    for vol, counts, tag in ((cc.cells(), CELLS_COUNTS, 'cells'),
                             (cc.stairs(), cc.STAIRS_COUNTS, 'stairs')):
        for connectivity in cc.CONNECTIVITIES:
            want, n_want = cc.binary_reference(vol, connectivity)
            assert n_want == counts[connectivity]
            for entry in ('binary', 'labels'):
                _check(ops, bad, (tag, connectivity, entry), vol,
                       connectivity, entry, want, n_want, dtype=np.uint32)
    for gen, counts in ((cc.stair18, cc.stair18_counts),
                        (cc.stair26, cc.stair26_counts)):
        shape = (9, 12, 14)
        for connectivity in cc.CONNECTIVITIES:
            want, n_want = cc.binary_reference(gen(shape), connectivity)
            assert n_want == counts(shape)[connectivity]
            _check(ops, bad, (gen.__name__, connectivity), gen(shape),
                   connectivity, 'binary', want, n_want)
    assert not bad, bad


# ---------------------------------------------------------------------------
# GPU: cfx_threshold and cfx_nonzero_u8
# ---------------------------------------------------------------------------
THRESHOLDS = (0.0, -0.0, 0.7, 0.5)
MASK_NS = (1, 255, 256, 257, cc.WRAP + 257)


def _specials():
    out = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    for thr in THRESHOLDS:
        t = np.float32(thr)
        out += [t, np.nextafter(t, np.float32(np.inf)),
                np.nextafter(t, np.float32(-np.inf))]
    return np.array(out, dtype=np.float32)


def _threshold_input(n, rot):
    """Random values in [-1, 2) with a special value at every other
    position, cycling through all of them from `rot` on."""
    sp = _specials()
    vals = (np.random.default_rng(n).random(n) * 3 - 1).astype(np.float32)
    at = np.arange(0, n, 2)
    vals[at] = sp[(at // 2 + rot) % len(sp)]
    return vals


def _mask_call(ops, call, n):
    """Run `call(fg_ptr)` on a poisoned, guarded u8 buffer of n bytes."""
    buf = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=ops.device)
    call(buf[64:64 + n].data_ptr())
    ops.sync()
    out = buf.cpu().numpy()
    assert (out[:64] == 0xA5).all() and (out[64 + n:] == 0xA5).all(), \
        'guard bytes written'
    return out[64:64 + n]


@gpu
def test_threshold_exact(ops):
    """cfx_threshold == numpy `in > float32(threshold)` byte for byte, with
    NaN, infinities, both zeros, the threshold and its two neighbours in
    the first trip and in the wrapped tail."""
    bad = []
    n_special = len(_specials())
    for n in MASK_NS:
        for rot in (range(n_special) if n == 1 else (0,)):
            vals = _threshold_input(n, rot)
            if n > cc.WRAP:
                tail = vals[cc.WRAP:]
                assert np.isnan(tail).any() and np.isinf(tail).any()
                assert all((tail == np.float32(t)).any() for t in THRESHOLDS)
            dev = torch.from_numpy(vals).to(ops.device)
            for thr in THRESHOLDS:
                got = _mask_call(ops, lambda p: ops.cfx.threshold(
                    dev.data_ptr(), p, n, thr), n)
                with np.errstate(invalid='ignore'):
                    want = (vals > np.float32(thr)).astype(np.uint8)
                if got.tobytes() != want.tobytes():
                    bad.append((n, rot, thr,
                                int(np.flatnonzero(got != want)[0])))
            assert dev.cpu().numpy().tobytes() == vals.tobytes()
    assert not bad, bad


@gpu
def test_nonzero_u8_exact(ops):
    bad = []
    for n in MASK_NS:
        vals = np.random.default_rng(n).integers(0, 3, n).astype(np.uint8)
        vals[vals == 2] = np.random.default_rng(n + 1).integers(
            1, 256, int((vals == 2).sum()))
        if n >= 255:
            vals[n - 255:] = np.arange(1, 256)[::-1]     # every byte value
            vals[n - 3] = 0
        if n == 1:
            vals[0] = 128
        dev = torch.from_numpy(vals).to(ops.device)
        got = _mask_call(ops, lambda p: ops.cfx.nonzero_u8(
            dev.data_ptr(), p, n), n)
        if got.tobytes() != (vals != 0).astype(np.uint8).tobytes():
            bad.append(n)
        assert dev.cpu().numpy().tobytes() == vals.tobytes()
    zero = torch.zeros(1, dtype=torch.uint8, device=ops.device)
    assert _mask_call(ops, lambda p: ops.cfx.nonzero_u8(
        zero.data_ptr(), p, 1), 1)[0] == 0
    assert not bad, bad


# ---------------------------------------------------------------------------
# GPU: the operator on device chunks of every dtype
# ---------------------------------------------------------------------------
OP_SHAPE = (5, 33, 70)


def _straddling(dtype):
    """(threshold, values): values on both sides of the threshold in the
    dtype's own grid, with the voxels an f32 round trip would move across
    it: float16(0.7) > float32(0.7) although it is not > 0.7 in f16;
    0.7 + 1e-12 and 2**24 + 1 are above their thresholds but round onto
    them in f32."""
    if dtype in (np.float16, np.float32, np.float64):
        t = dtype(0.7)
        vals = [t, np.nextafter(t, dtype(1)), np.nextafter(t, dtype(0)),
                dtype(np.float32(0.7)), dtype(0), dtype(1), dtype(np.nan),
                dtype(np.inf), dtype(-np.inf)]
        if dtype == np.float64:
            vals += [0.7 + 1e-12, 0.7 - 1e-12]
        return 0.7, np.array(vals, dtype=dtype)
    if dtype == np.uint8:
        return 127.0, np.array([0, 126, 127, 128, 255], dtype=dtype)
    assert dtype == np.int32
    return float(2 ** 24), np.array(
        [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 0, -5,
         2 ** 31 - 1, -2 ** 31], dtype=dtype)


def _operator_volume(dtype):
    threshold, vals = _straddling(dtype)
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    arr = vals[rng.integers(0, len(vals), size=OP_SHAPE)]
    assert arr.dtype == dtype
    with np.errstate(invalid='ignore'):
        fg = arr > threshold
    assert 0.2 < fg.mean() < 0.8
    return threshold, arr


def _operator_equals_host(arr, dev, threshold, connectivity):
    from chunkflow_amd.chunk import Chunk
    from chunkflow_amd.connected import connected_component
    with np.errstate(invalid='ignore'):
        host = connected_component(Chunk(arr), threshold=threshold,
                                   connectivity=connectivity)
    got = connected_component(Chunk(dev), threshold=threshold,
                              connectivity=connectivity)
    assert got.is_device and got.array.dtype == torch.int32
    assert dev.cpu().numpy().tobytes() == arr.tobytes(), \
        'input chunk was modified'
    assert tuple(got.array.shape) == host.array.shape
    want = host.array.astype(np.uint32)
    assert int(want.max()) >= 2           # more than one component
    return got.array.cpu().numpy().view(np.uint32).tobytes() == \
        want.tobytes()


@gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float16, np.float64,
                                   np.uint8, np.int32],
                         ids=['f32', 'f16', 'f64', 'u8', 'i32'])
def test_operator_threshold_in_chunk_dtype(dtype):
    """connected_component on a device chunk == the host path on the same
    array, for voxels straddling the threshold in the chunk's own dtype
    (f16, f64 and int32 differed while the device path compared an f32
    copy against the f32 threshold)."""
    threshold, arr = _operator_volume(dtype)
    for connectivity in (6, 26):
        dev = torch.from_numpy(arr.copy()).cuda()
        assert _operator_equals_host(arr, dev, threshold, connectivity), \
            (np.dtype(dtype).name, connectivity)


@gpu
def test_operator_4d_and_non_contiguous_chunks():
    # a (1, D, H, W) chunk
    threshold, arr = _operator_volume(np.float16)
    dev = torch.from_numpy(arr[None].copy()).cuda()
    assert _operator_equals_host(arr[None], dev, threshold, 18)
    # every other voxel along x of a wider f64 volume, and a transposed
    # int32 volume: views, not copies
    threshold, arr = _operator_volume(np.float64)
    wide = np.repeat(arr, 2, axis=2)
    wide[:, :, 1::2] = 1.0                    # the skipped voxels: foreground
    dev = torch.from_numpy(wide.copy()).cuda()[:, :, ::2]
    assert not dev.is_contiguous()
    assert _operator_equals_host(wide[:, :, ::2], dev, threshold, 6)
    threshold, arr = _operator_volume(np.int32)
    dev = torch.from_numpy(arr.copy()).cuda().permute(2, 1, 0)
    assert not dev.is_contiguous()
    assert _operator_equals_host(arr.transpose(2, 1, 0), dev, threshold, 26)
