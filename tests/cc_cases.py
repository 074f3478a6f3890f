"""Shapes, generators, references and one driver for the union-find
labeller of chunkflow_amd/csrc/cc.hip (used by tests/test_cc_exact.py; not
collected by pytest).

Everything here is integer: a labelling is right when its bytes equal the
reference's bytes. Three references are kept apart:
  * `binary_reference`: scipy.ndimage.label with the project's structuring
    elements (the pin of the binary entry);
  * `connected.equal_value_label` and its vectorised restatement
    `equal_value_fast` (the pin of the equal-value entry; the restatement
    only replaces the per-component Python renumbering loop, and the CPU
    tests hold it equal to the original on every small case);
  * `flood_label`: a plain Python flood fill over an explicit neighbour
    list, numbered by first raster encounter. It shares no code with the
    other two and checks them on every small case.

Geometry. The shapes are derived from constants parsed out of cc.hip (the
rank chunk SCAN_CHUNK, the grid cap and the block size of `grid_for`), so
that a retune of the kernels moves the shapes with it or fails loudly.
WRAP voxels fill one trip of every grid-stride loop; BIG is just above it.

Buffers. `run_case` hands the kernels views into larger allocations:
`labels` and `scratch` are prefilled with 0xA5A5A5A5, as are the guard
bands around them, except the band after `labels`, which holds its own
flat indices: to a kernel that looks one element too far these read as
union-find roots. All four bands must come back unchanged.
"""
import os
import re
import sys

import numpy as np

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _REPO not in sys.path:
    sys.path.insert(0, _REPO)

CC_SOURCE = os.path.join(_REPO, 'chunkflow_amd', 'csrc', 'cc.hip')
CONNECTIVITIES = (6, 18, 26)
POISON = 0xA5A5A5A5
GUARD = 64          # u32 elements before and after labels / scratch


# ---------------------------------------------------------------------------
# geometry parsed from the kernel source
# ---------------------------------------------------------------------------
def parse_geometry(text):
    """(SCAN_CHUNK, grid cap, block size) as cc.hip states them. Raises
    when a pattern is not found or the launches disagree on the block."""
    m = re.search(r'constexpr\s+int\s+SCAN_CHUNK\s*=\s*(\d+)\s*;', text)
    if not m:
        raise RuntimeError('cc.hip: SCAN_CHUNK not found')
    scan_chunk = int(m.group(1))
    m = re.search(r'inline\s+int\s+grid_for\s*\([^)]*\)\s*\{[^}]*?'
                  r'want\s*<\s*(\d+)\s*\?\s*want\s*:\s*(\d+)\s*\)\s*;', text)
    if not m or m.group(1) != m.group(2):
        raise RuntimeError('cc.hip: the grid cap of grid_for not found')
    cap = int(m.group(1))
    launches = re.findall(
        r'dim3\(grid_for\(n,\s*(\d+)\)\),\s*dim3\((\d+)\)', text)
    blocks = {int(v) for pair in launches for v in pair}
    if len(launches) < 6 or len(blocks) != 1:
        raise RuntimeError(f'cc.hip: grid-stride launches not found or not '
                           f'of one block size: {launches}')
    return scan_chunk, cap, blocks.pop()


with open(CC_SOURCE) as _f:
    SCAN_CHUNK, GRID_CAP, BLOCK = parse_geometry(_f.read())
WRAP = GRID_CAP * BLOCK             # voxels in one trip of a grid-stride loop


def nvox(shape):
    return int(shape[0]) * int(shape[1]) * int(shape[2])


def big_ok(shape):
    """Just above one trip, not a multiple of the wave size, and with a
    partial last rank chunk."""
    n = nvox(shape)
    return (WRAP < n <= WRAP + WRAP // 64 and n % 64 != 0
            and n % SCAN_CHUNK not in (0, 1))


def choose_big():
    """(33, 252, 254) while it has the three properties; otherwise the
    first 33 x 252 x W that does."""
    if big_ok((33, 252, 254)):
        return (33, 252, 254)
    for w in range(WRAP // (33 * 252), WRAP // (33 * 252) + 64):
        if big_ok((33, 252, w)):
            return (33, 252, w)
    raise RuntimeError('no wrap-scale shape for the parsed constants')


BIG = choose_big()
assert big_ok(BIG), BIG


def fold3(n):
    """n as (d, h, w), d <= h <= w, with the largest possible d, then h;
    None when n has no factor (1 and primes)."""
    best = None
    for d in range(1, int(round(n ** (1 / 3))) + 2):
        if n % d:
            continue
        m = n // d
        for h in range(d, int(m ** 0.5) + 1):
            if m % h == 0 and h >= 2:
                best = (d, h, m // h)
    return best


RANK_NS = (1, 63, 64, 65, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1,
           2 * SCAN_CHUNK + 64, 3 * SCAN_CHUNK + 1)
RANK_SHAPES = tuple((1, 1, n) for n in RANK_NS) + tuple(
    s for s in (fold3(n) for n in RANK_NS) if s is not None)
DEGENERATE_SHAPES = ((1, 1, 1), (1, 70, 1), (70, 1, 1), (2, 1, 300),
                     (1, 2, 300))
EDGE_SHAPES = tuple(dict.fromkeys(RANK_SHAPES + DEGENERATE_SHAPES))
# small enough for the Python flood fill
SMALL_SHAPES = tuple(s for s in EDGE_SHAPES if nvox(s) <= 5000) + (
    (5, 7, 9), (4, 6, 11), (2, 2, 2), (6, 9, 17), (3, 3, 3))


# ---------------------------------------------------------------------------
# label mappings (shared with tests/test_segmentation_gpu.py)
# ---------------------------------------------------------------------------
def as_dtype(vol, dtype):
    """Distinct small ints -> distinct labels of `dtype`; the uint64 labels
    share their low 32 bits and differ only above bit 32."""
    vol = vol.astype(np.uint64)
    if dtype == np.uint8:
        return (vol * np.uint64(31)).astype(np.uint8)
    if dtype == np.uint32:
        return (vol * np.uint64(2 ** 31 // 4)).astype(np.uint32)
    return (vol << np.uint64(32)) + (vol != 0) * np.uint64(9)


LABEL_DTYPES = (np.uint8, np.uint32, np.uint64)


# ---------------------------------------------------------------------------
# generators: small ints, 0 is background. `labels=True` gives the form
# meant for the equal-value entry where that differs.
# ---------------------------------------------------------------------------
def serpentine_end(shape):
    """(y, x) at which the in-plane path that starts at (0, 0) ends."""
    ylast = (shape[1] - 1) // 2 * 2
    return ylast, (shape[2] - 1 if (ylast // 2) % 2 == 0 else 0)


def serpentine3d(shape, labels=False):
    """One one-voxel-wide path: every even row of every even plane, rows
    joined by a single voxel at alternating ends of the odd rows, planes
    joined by a single voxel in the odd plane between them, alternately
    above the end and above the start of the in-plane path. One 6-component
    whose root is voxel 0; every voxel of it has to compress to voxel 0.
    With labels the path holds 1 and everything else 2."""
    D, H, W = shape
    vol = np.zeros(shape, dtype=np.int64)
    vol[0::2, 0::2, :] = 1
    for y in range(1, H - 1, 2):
        vol[0::2, y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    ye, xe = serpentine_end(shape)
    for z in range(1, D - 1, 2):
        if (z // 2) % 2 == 0:
            vol[z, ye, xe] = 1
        else:
            vol[z, 0, 0] = 1
    if labels:
        vol = np.where(vol == 1, 1, 2)
    return vol


def comb_teeth(shape):
    """The teeth of the combs: every other row (even y), full length along
    x, in every plane, so each tooth is an x-z sheet of D * W voxels and
    reaches the last plane. (Teeth confined to inner planes could only be
    joined by voxels next to them, that is early in raster order.)"""
    vol = np.zeros(shape, dtype=np.int64)
    vol[:, 0::2, :] = 1
    return vol


def late_comb(shape, labels=False):
    """The teeth joined only by a spine in the last plane: the last voxel
    of every row there. Every tooth is a provisional tree of its own until
    the last row-ends of raster order unite them all."""
    vol = comb_teeth(shape)
    vol[-1, :, -1] = 1
    return vol


def early_comb(shape, labels=False):
    """late_comb mirrored in all three axes: the spine starts at voxel 0."""
    return np.ascontiguousarray(late_comb(shape)[::-1, ::-1, ::-1])


def checkerboard(shape, labels=False):
    """(z + y + x) % 2: at 6-connectivity every foreground voxel is a root
    (every rank ballot is half full); at 18 and 26 it is one component.
    With labels both colours are foreground (1 and 2)."""
    z, y, x = np.indices(shape)
    return (z + y + x) % 2 + (1 if labels else 0)


def all_foreground(shape, labels=False):
    return np.ones(shape, dtype=np.int64)


def all_background(shape, labels=False):
    return np.zeros(shape, dtype=np.int64)


def _rng(shape, salt):
    return np.random.default_rng([salt, *shape])


def random_p(p):
    def gen(shape, labels=False):
        return (_rng(shape, int(p * 1000)).random(shape) < p).astype(np.int64)
    gen.__name__ = f'random_p{int(round(p * 100)):02d}'
    return gen


def random_k(k):
    def gen(shape, labels=False):
        return _rng(shape, 7000 + k).integers(0, k + 1, size=shape)
    gen.__name__ = f'random_k{k}'
    return gen


def stair18(shape, labels=False):
    """In every even plane the diagonal y == x: neighbours along it touch
    only along an edge. Odd planes are empty."""
    z, y, x = np.indices(shape)
    return ((z % 2 == 0) & (y == x)).astype(np.int64)


def stair18_counts(shape):
    planes, steps = (shape[0] + 1) // 2, min(shape[1], shape[2])
    return {6: planes * steps, 18: planes, 26: planes}


def stair26(shape, labels=False):
    """Space diagonals (k, k, k + c) for every c divisible by 3: neighbours
    along one touch only at a corner, and two diagonals never touch."""
    z, y, x = np.indices(shape)
    return ((z == y) & ((x - z) % 3 == 0)).astype(np.int64)


def stair26_counts(shape):
    vol = stair26(shape)
    z, _, x = np.nonzero(vol)
    voxels = int(vol.sum())
    return {6: voxels, 18: voxels, 26: len(np.unique(x - z))}


def stairs(shape=(9, 12, 14)):
    """An edge stair of 5 voxels and a corner stair of 4 in one volume, far
    apart: 9, 1 + 4 and 2 components at 6, 18 and 26."""
    vol = np.zeros(shape, dtype=np.int64)
    for k in range(5):
        vol[0, k, k] = 1
    for k in range(4):
        vol[4 + k, 6 + k, 8 + k] = 1
    return vol


STAIRS_COUNTS = {6: 9, 18: 5, 26: 2}


def cells():
    """The truth table of the neighbour predicate in one volume: all 256
    patterns of a 2 x 2 x 2 block, each in its own 3 x 3 x 3 cell (a
    4 x 8 x 8 grid of cells, padded to 12 x 32 x 32), on top of 512 seeded
    random 3 x 3 x 3 patterns in 4 x 4 x 4 cells (8 x 8 x 8 of them).
    Cells never touch, not even at a corner."""
    top = np.zeros((12, 32, 32), dtype=np.int64)
    for p in range(256):
        cz, cy, cx = p // 64, (p // 8) % 8, p % 8
        bits = [(p >> b) & 1 for b in range(8)]
        top[3 * cz:3 * cz + 2, 3 * cy:3 * cy + 2, 3 * cx:3 * cx + 2] = \
            np.array(bits).reshape(2, 2, 2)
    rng = np.random.default_rng(26)
    bottom = np.zeros((32, 32, 32), dtype=np.int64)
    for c in range(512):
        cz, cy, cx = c // 64, (c // 8) % 8, c % 8
        bottom[4 * cz:4 * cz + 3, 4 * cy:4 * cy + 3, 4 * cx:4 * cx + 3] = \
            rng.integers(0, 2, size=(3, 3, 3))
    return np.concatenate([top, bottom], axis=0)


GENERATORS = {g.__name__: g for g in (
    serpentine3d, late_comb, early_comb, checkerboard, all_foreground,
    random_p(0.5), random_p(0.31), random_k(2), random_k(7), stair18,
    stair26)}
EDGE_GENERATORS = ('checkerboard', 'all_foreground', 'random_p50',
                   'all_background')
GENERATORS_ALL = dict(GENERATORS, all_background=all_background)

_VOLUMES = {}


def volume(name, shape, labels=False):
    """Generated once per (name, shape, form), shared, read-only."""
    key = (name, tuple(shape), bool(labels))
    if key not in _VOLUMES:
        vol = np.ascontiguousarray(
            GENERATORS_ALL[name](tuple(shape), labels=labels),
            dtype=np.int64)
        assert vol.shape == tuple(shape)
        vol.setflags(write=False)
        _VOLUMES[key] = vol
    return _VOLUMES[key]


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def binary_reference(vol, connectivity):
    """(labels u32, n): scipy.ndimage.label of vol != 0."""
    from scipy import ndimage
    from chunkflow_amd.connected import _STRUCTS
    lab, n = ndimage.label(vol != 0, structure=_STRUCTS[connectivity])
    return lab.astype(np.uint32), int(n)


def equal_value_fast(vol, connectivity):
    """(labels u32, n): connected.equal_value_label with its renumbering
    loop vectorised. Per value a scipy labelling, offsets added, then the
    components are renumbered by the flat index of their first voxel."""
    from scipy import ndimage
    from chunkflow_amd.connected import _STRUCTS
    out = np.zeros(vol.shape, dtype=np.int64)
    offset = 0
    for v in np.unique(vol):
        if v == 0:
            continue
        lab, n = ndimage.label(vol == v, structure=_STRUCTS[connectivity])
        sel = lab > 0
        out[sel] = lab[sel].astype(np.int64) + offset
        offset += n
    flat = out.ravel()
    uniq, first = np.unique(flat, return_index=True)
    keep = uniq != 0
    uniq, first = uniq[keep], first[keep]
    remap = np.zeros(offset + 1, dtype=np.uint32)
    remap[uniq[np.argsort(first, kind='stable')]] = \
        np.arange(1, len(uniq) + 1, dtype=np.uint32)
    return remap[flat].reshape(vol.shape), int(len(uniq))


def neighbour_offsets(connectivity):
    """The explicit neighbour list: offsets in {-1, 0, 1}^3 that change at
    most 1 (6), 2 (18) or 3 (26) coordinates."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1)
            for dx in (-1, 0, 1)
            if 0 < (dz != 0) + (dy != 0) + (dx != 0) <= most]


def flood_label(vol, connectivity, equal_value=False):
    """(labels u32, n): plain flood fill in raster order. A neighbour joins
    when it is foreground (binary) or holds the same non-zero value
    (equal_value). The k-th component is the one whose first voxel in
    raster order comes k-th."""
    D, H, W = vol.shape
    offs = neighbour_offsets(connectivity)
    val = vol.tolist()
    lab = [[[0] * W for _ in range(H)] for _ in range(D)]
    n = 0
    for z in range(D):
        for y in range(H):
            for x in range(W):
                if val[z][y][x] == 0 or lab[z][y][x]:
                    continue
                n += 1
                v = val[z][y][x]
                lab[z][y][x] = n
                stack = [(z, y, x)]
                while stack:
                    cz, cy, cx = stack.pop()
                    for dz, dy, dx in offs:
                        az, ay, ax = cz + dz, cy + dy, cx + dx
                        if not (0 <= az < D and 0 <= ay < H and 0 <= ax < W):
                            continue
                        w = val[az][ay][ax]
                        if lab[az][ay][ax] or w == 0:
                            continue
                        if equal_value and w != v:
                            continue
                        lab[az][ay][ax] = n
                        stack.append((az, ay, ax))
    return np.array(lab, dtype=np.uint32).reshape(vol.shape), n


_REFS = {}


def reference(name, shape, connectivity, entry):
    """(labels u32, n) of a generated volume, computed once and shared,
    read-only. entry 'binary': the volume as a mask; 'labels': its label
    form under equal-value semantics."""
    key = (name, tuple(shape), connectivity, entry)
    if key not in _REFS:
        if entry == 'binary':
            lab, n = binary_reference(volume(name, shape), connectivity)
        else:
            lab, n = equal_value_fast(volume(name, shape, labels=True),
                                      connectivity)
        lab.setflags(write=False)
        _REFS[key] = (lab, n)
    return _REFS[key]


def invariant_problems(foreground, labels, n):
    """What a labelling must satisfy whatever the reference says:
    background 0 and foreground in 1..n, every label used, and the first
    flat index of label k strictly increasing in k."""
    out = []
    fg = np.asarray(foreground, dtype=bool)
    if labels[~fg].any():
        out.append('background voxel with a label')
    if fg.any() and (labels[fg].min() < 1 or labels[fg].max() > n):
        out.append(f'foreground label outside 1..{n}')
    uniq, first = np.unique(labels.ravel(), return_index=True)
    keep = uniq != 0
    uniq, first = uniq[keep], first[keep]
    if len(uniq) != n or (n and (uniq[0] != 1 or uniq[-1] != n)):
        out.append(f'{len(uniq)} distinct labels for n_components {n}')
    if (np.diff(first) <= 0).any():
        out.append('first voxels of the labels not in raster order')
    return out


# ---------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------
def upload(arr, device):
    """Host array -> device tensor; uint32/uint64 travel as int32/int64."""
    import torch
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    arr = np.ascontiguousarray(arr)
    if arr.dtype in signed:
        arr = arr.view(signed[arr.dtype])
    return torch.from_numpy(arr).to(device)


def poisoned(n, device, rootlike_tail=False):
    """A u32 allocation of GUARD + n + GUARD elements filled with POISON;
    with rootlike_tail the band after the body holds n, n + 1, ... (what
    the body's own index would be there). Returns (allocation, body)."""
    import torch
    buf = torch.full((n + 2 * GUARD,), POISON - (1 << 32),
                     dtype=torch.int32, device=device)
    if rootlike_tail:
        buf[GUARD + n:] = torch.arange(n, n + GUARD, dtype=torch.int32,
                                       device=device)
    return buf, buf[GUARD:GUARD + n]


def guard_problems(buf, n, name, rootlike_tail=False):
    head = buf[:GUARD].cpu().numpy().view(np.uint32)
    tail = buf[GUARD + n:].cpu().numpy().view(np.uint32)
    want = (np.arange(n, n + GUARD, dtype=np.uint32) if rootlike_tail
            else np.full(GUARD, POISON, dtype=np.uint32))
    out = []
    if (head != np.uint32(POISON)).any():
        out.append(f'{name}: guard before the buffer was written')
    if (tail != want).any():
        out.append(f'{name}: guard after the buffer was written')
    return out


def run_case(ops, vol, connectivity, entry='binary', dtype=np.uint8):
    """Label `vol` on ops' device. entry 'binary': cfx_connected_components
    on the mask vol != 0; 'labels': cfx_connected_components_labels on
    as_dtype(vol, dtype), or on vol itself when it already is unsigned.
    Returns (labels u32 of vol's shape, n_components, problems): problems
    lists touched guard bands and a modified input."""
    import torch
    shape = tuple(vol.shape)
    n = nvox(shape)
    if entry == 'binary':
        src = upload((vol != 0).astype(np.uint8), ops.device)
    elif vol.dtype.kind == 'u':
        src = upload(vol, ops.device)
    else:
        src = upload(as_dtype(vol, dtype), ops.device)
    before = src.clone()
    lab_buf, labels = poisoned(n, ops.device, rootlike_tail=True)
    scr_buf, scratch = poisoned(n, ops.device)
    if entry == 'binary':
        count = ops.cfx.connected_components(
            src.data_ptr(), shape, connectivity, labels.data_ptr(),
            scratch.data_ptr())
    else:
        count = ops.cfx.connected_components_labels(
            src.data_ptr(), src.element_size(), shape, connectivity,
            labels.data_ptr(), scratch.data_ptr())
    ops.sync()
    problems = guard_problems(lab_buf, n, 'labels', rootlike_tail=True)
    problems += guard_problems(scr_buf, n, 'scratch')
    if not torch.equal(src, before):
        problems.append('input modified')
    got = labels.cpu().numpy().view(np.uint32).reshape(shape)
    return got, int(count), problems
