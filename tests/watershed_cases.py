"""Inputs and slow references for the affinity watershed, the region graph
and the agglomerator (used by tests/test_watershed.py and
tests/test_watershed_gpu.py; not collected by pytest).

The slow references restate the definitions of chunkflow_amd/watershed.py
and agglomeration.py literally, one voxel or one edge at a time in plain
Python, and share no code with the vectorised host path they check.
Everything is integer: a result is right when it is equal.
"""
import numpy as np
from scipy import ndimage

# (channel, dz, dy, dx) of each voxel's six incident edges in pick order
# -x +x -y +y -z +z; the weight of a forward edge is stored at its far end
PICK_ORDER = ((0, 0, 0, -1), (0, 0, 0, 1), (1, 0, -1, 0), (1, 0, 1, 0),
              (2, -1, 0, 0), (2, 1, 0, 0))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def smooth(shape, seed=0):
    """Seeded noise smoothed over 3 voxels, stretched to [0, 1], f32."""
    rng = np.random.default_rng([seed, *shape])
    a = rng.random((3,) + tuple(shape))
    a = ndimage.uniform_filter(a, size=(1, 3, 3, 3), mode='nearest')
    lo, hi = a.min(), a.max()
    a = (a - lo) / (hi - lo) if hi > lo else np.full_like(a, 0.5)
    return np.ascontiguousarray(a, dtype=np.float32)


def levels(shape, seed=1):
    """Four levels 0.25, 0.5, 0.75, 1.0: ties between directions wherever
    one looks."""
    rng = np.random.default_rng([seed, *shape])
    return (rng.integers(1, 5, size=(3,) + tuple(shape)) / 4.0) \
        .astype(np.float32)


def special(shape, seed=2):
    """smooth() with NaN, +inf, -inf and negative entries sprinkled in."""
    a = smooth(shape, seed)
    rng = np.random.default_rng([seed + 100, *shape])
    r = rng.random(a.shape)
    a[r < 0.04] = np.nan
    a[(r >= 0.04) & (r < 0.07)] = np.inf
    a[(r >= 0.07) & (r < 0.10)] = -np.inf
    a[(r >= 0.10) & (r < 0.16)] *= -1
    return a


def path_edges(mask):
    """Affinity 1.0 on the edges that join two voxels of `mask`, 0.0 on
    every other edge."""
    m = mask.astype(bool)
    a = np.zeros((3,) + m.shape, dtype=np.float32)
    a[0][:, :, 1:] = m[:, :, 1:] & m[:, :, :-1]
    a[1][:, 1:, :] = m[:, 1:, :] & m[:, :-1, :]
    a[2][1:, :, :] = m[1:, :, :] & m[:-1, :, :]
    return a


def fill_leading_faces(aff, value):
    out = aff.copy()
    out[0][:, :, 0] = value
    out[1][:, 0, :] = value
    out[2][0, :, :] = value
    return out


def blocky_fragments(shape, seed=3):
    """A hand-made label volume: blocks of 3 voxels along x, ids drawn from
    0, a few small ones and the top of the u32 range."""
    rng = np.random.default_rng([seed, *shape])
    ids = np.array([0, 1, 2, 3, 7, 2 ** 31, 2 ** 32 - 3, 2 ** 32 - 2,
                    2 ** 32 - 1], dtype=np.uint32)
    z, y, x = shape
    coarse = rng.integers(0, ids.size, size=(z, y, -(-x // 3)))
    return ids[np.repeat(coarse, 3, axis=2)[:, :, :x]]


# ---------------------------------------------------------------------------
# the region-graph walk at scale: geometry parsed from the kernel source, so
# that a retune moves the shapes with it or fails loudly
# ---------------------------------------------------------------------------
def _constant(name):
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), 'chunkflow_amd', 'csrc',
        'watershed.hip')
    with open(path) as f:
        m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name,
                      f.read())
    if not m:
        raise RuntimeError(f'watershed.hip: {name} not found')
    return int(m.group(1))


SEG = _constant('SEG')                      # voxels per lane and item
VOXEL_LANES = _constant('kGridCap') * _constant('kBlock')
REGION_LANES = _constant('kRegionGrid') * _constant('kBlock')


def region_wrap_shape():
    """(129, 255, W): a few percent more SEG-voxel items than the region
    walk has lanes, so some lanes take a second item and most do not; the
    last item is partial."""
    for w in range(8, 4096):
        n = 129 * 255 * w
        if n > 1.03 * SEG * REGION_LANES and n % SEG:
            return (129, 255, w)
    raise RuntimeError('no wrap shape for the parsed constants')


def coarse_fragments(shape, seed=4):
    """Blocks of 4 x 8 x 32 voxels with ids from 0, small ones and the top
    of the u32 range: few enough boundary edges for a quick host pass at
    millions of voxels, runs that span lanes, and many distinct pairs."""
    rng = np.random.default_rng([seed, *shape])
    ids = np.concatenate([[0], np.arange(1, 200),
                          2 ** 32 - 1 - np.arange(200)]).astype(np.uint32)
    z, y, x = shape
    coarse = rng.integers(0, ids.size,
                          size=(-(-z // 4), -(-y // 8), -(-x // 32)))
    vol = np.repeat(np.repeat(np.repeat(coarse, 4, 0), 8, 1), 32, 2)
    return ids[vol[:z, :y, :x]]


def cheap_special(shape, seed=6):
    """Unsmoothed f32 noise in [-0.25, 1.25) with NaN and inf sprinkled in:
    what special() is for, at a cost that suits millions of voxels."""
    rng = np.random.default_rng([seed, *shape])
    a = rng.random((3,) + tuple(shape), dtype=np.float32) * np.float32(1.5) \
        - np.float32(0.25)
    r = rng.integers(0, 64, size=a.shape, dtype=np.uint8)
    a[r == 0] = np.nan
    a[r == 1] = np.inf
    a[r == 2] = -np.inf
    return a


def expected_runs(frag):
    """The number of table operations the device walk makes, restated with
    numpy: per channel, within each item of SEG consecutive voxels, the
    voxels that have an edge whose key differs from that of the previous
    voxel WITH an edge in the same item (or that are the first such)."""
    f = np.ascontiguousarray(frag).astype(np.uint64)
    n = f.size
    item = np.arange(n, dtype=np.int64).reshape(f.shape) // SEG
    total = 0
    for axis in (2, 1, 0):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        a, b = f[tuple(hi)], f[tuple(lo)]
        sel = (a != b) & (a != 0) & (b != 0)
        key = (np.minimum(a, b)[sel] << np.uint64(32)) | np.maximum(a, b)[sel]
        it = item[tuple(hi)][sel]            # selection keeps flat order
        start = np.ones(key.size, dtype=bool)
        start[1:] = (key[1:] != key[:-1]) | (it[1:] != it[:-1])
        total += int(start.sum())
    return total


# ---------------------------------------------------------------------------
# slow references
# ---------------------------------------------------------------------------
def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def _number_by_first_voxel(parent, fg):
    """labels 1..N by first voxel in flat order, 0 where fg is False"""
    out = np.zeros(len(parent), dtype=np.uint32)
    seen = {}
    for i in range(len(parent)):
        if fg[i]:
            r = _find(parent, i)
            if r not in seen:
                seen[r] = len(seen) + 1
            out[i] = seen[r]
    return out, len(seen)


def fragments_slow(aff, low, high):
    """(labels u32, n) by the definition, voxel by voxel."""
    aff = np.asarray(aff, dtype=np.float32)
    low, high = np.float32(low), np.float32(high)
    _, D, H, W = aff.shape
    parent = list(range(D * H * W))
    fg = [False] * (D * H * W)

    def union(i, j):
        ri, rj = _find(parent, i), _find(parent, j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)

    for z in range(D):
        for y in range(H):
            for x in range(W):
                i = (z * H + y) * W + x
                best = None
                for c, dz, dy, dx in PICK_ORDER:
                    nz, ny, nx = z + dz, y + dy, x + dx
                    if not (0 <= nz < D and 0 <= ny < H and 0 <= nx < W):
                        continue
                    # the edge's weight sits at its later end
                    w = aff[c, max(z, nz), max(y, ny), max(x, nx)]
                    if not w >= low:
                        continue
                    j = (nz * H + ny) * W + nx
                    if w >= high:
                        union(i, j)
                    if best is None or w > best[0]:
                        best = (w, j)
                if best is not None:
                    fg[i] = True
                    union(i, best[1])
    labels, n = _number_by_first_voxel(parent, fg)
    return labels.reshape(D, H, W), n


def edge_components_slow(aff, threshold):
    """(labels u32, n): components of the voxels under the edges with
    w >= threshold; a voxel with no such edge is 0."""
    aff = np.asarray(aff, dtype=np.float32)
    t = np.float32(threshold)
    _, D, H, W = aff.shape
    parent = list(range(D * H * W))
    fg = [False] * (D * H * W)
    for z in range(D):
        for y in range(H):
            for x in range(W):
                i = (z * H + y) * W + x
                for c, j, ok in ((0, i - 1, x > 0), (1, i - W, y > 0),
                                 (2, i - H * W, z > 0)):
                    if ok and aff[c, z, y, x] >= t:
                        fg[i] = fg[j] = True
                        ri, rj = _find(parent, i), _find(parent, j)
                        if ri != rj:
                            parent[max(ri, rj)] = min(ri, rj)
    labels, n = _number_by_first_voxel(parent, fg)
    return labels.reshape(D, H, W), n


def region_graph_slow(frag, aff):
    """{(a, b): [count, sum]} edge by edge, q(w) in Python arithmetic."""
    aff = np.asarray(aff, dtype=np.float32)
    D, H, W = frag.shape
    rows = {}
    for z in range(D):
        for y in range(H):
            for x in range(W):
                a = int(frag[z, y, x])
                for c, (pz, py, px) in enumerate(((z, y, x - 1),
                                                  (z, y - 1, x),
                                                  (z - 1, y, x))):
                    if min(pz, py, px) < 0:
                        continue
                    b = int(frag[pz, py, px])
                    if a == 0 or b == 0 or a == b:
                        continue
                    w = float(aff[c, z, y, x])
                    clamped = min(w, 1.0) if w > 0 else 0.0
                    row = rows.setdefault((min(a, b), max(a, b)), [0, 0])
                    row[0] += 1
                    row[1] += int(clamped * 2 ** 24)   # exact; floor
    return rows


def rows_as_dict(rows):
    a, b, count, total = rows
    return {(int(p), int(q)): [int(c), int(s)]
            for p, q, c, s in zip(a, b, count, total)}


def merge_slow(rows, n_fragments, merge_threshold):
    """The agglomerator by rescanning every edge at every step."""
    edges = {k: tuple(v) for k, v in rows_as_dict(rows).items()}
    rep = list(range(n_fragments + 1))
    while edges:
        best = None
        for (a, b), (c, s) in edges.items():
            if best is None:
                best = (a, b, c, s)
                continue
            lhs, rhs = s * best[2], best[3] * c
            if lhs > rhs or (lhs == rhs and (a, b) < best[:2]):
                best = (a, b, c, s)
        a, b, c, s = best
        if not s / (c << 24) > merge_threshold:
            break
        merged = {}
        for (u, v), (cu, su) in edges.items():
            u, v = (a if u == b else u), (a if v == b else v)
            if u == v:
                continue
            key = (min(u, v), max(u, v))
            have = merged.get(key, (0, 0))
            merged[key] = (have[0] + cu, have[1] + su)
        edges = merged
        rep = [a if r == b else r for r in rep]
    reps = sorted(set(rep[1:]))
    rank = {r: i + 1 for i, r in enumerate(reps)}
    return np.array([0] + [rank[r] for r in rep[1:]], dtype=np.uint32)
