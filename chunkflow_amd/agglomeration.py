"""Mean-affinity agglomeration of a region graph, on the host.

The graph is small next to the volume it came from (one row per pair of
touching fragments), so it is merged here in Python with a heap while the
volume stays where it is; `watershed.agglomerate` applies the resulting map
with one gather.

Rows are (a, b, count, sum) with a < b fragment ids, `count` the number of
voxel edges between the two fragments and `sum` the sum of their affinities
quantised to 24 fractional bits (watershed.region_graph), so the mean
affinity of a row is sum / (count * 2^24) and everything below is integer
arithmetic: the result does not depend on the order of the rows.

  * The edge with the largest mean goes first. Means are compared exactly,
    sum_i * count_j against sum_j * count_i in Python ints; ties go to the
    smaller (a, b) of the current representatives.
  * It is merged while `sum / (count << 24) > merge_threshold` holds, and
    the first edge for which it does not ends the run (no later edge has a
    larger mean).
  * The representative of a merged pair is its smaller id. Parallel edges
    that a merge creates combine by adding counts and sums.
  * A fragment's segment id is the rank of its representative among the
    representatives: dense 1..M, and still ordered by first voxel when the
    fragment ids were. 0 maps to 0.
"""
import heapq

import numpy as np

SCALE_BITS = 24


class _Edge:
    """Heap entry: larger mean first, then smaller (a, b)."""
    __slots__ = ('a', 'b', 'count', 'sum')

    def __init__(self, a, b, count, total):
        self.a, self.b, self.count, self.sum = a, b, count, total

    def __lt__(self, other):
        mine, theirs = self.sum * other.count, other.sum * self.count
        if mine != theirs:
            return mine > theirs
        return (self.a, self.b) < (other.a, other.b)


def _int_rows(rows):
    a, b, count, total = rows
    return zip((int(v) for v in a), (int(v) for v in b),
               (int(v) for v in count), (int(v) for v in total))


def merge_fragments(rows, n_fragments: int,
                    merge_threshold: float) -> np.ndarray:
    """uint32 map of length n_fragments + 1 from fragment id to segment id.

    rows: four equally long sequences a, b, count, sum (numpy arrays or
    lists) with 1 <= a < b <= n_fragments, each pair at most once."""
    n_fragments = int(n_fragments)
    adj = [None] * (n_fragments + 1)   # rep -> {neighbour rep: (count, sum)}
    heap = []
    for a, b, count, total in _int_rows(rows):
        if not 1 <= a < b <= n_fragments:
            raise ValueError(f'merge_fragments: bad row ({a}, {b}) for '
                             f'{n_fragments} fragments')
        if count <= 0:
            raise ValueError(f'merge_fragments: row ({a}, {b}) has no edges')
        for u, v in ((a, b), (b, a)):
            if adj[u] is None:
                adj[u] = {}
            if v in adj[u]:
                raise ValueError(f'merge_fragments: row ({a}, {b}) twice')
            adj[u][v] = (count, total)
        heap.append(_Edge(a, b, count, total))
    heapq.heapify(heap)
    parent = list(range(n_fragments + 1))

    while heap:
        e = heapq.heappop(heap)
        # an entry is current iff both ends still stand for themselves and
        # the pair's totals are the entry's (totals only ever grow)
        if adj[e.a] is None or adj[e.a].get(e.b) != (e.count, e.sum):
            continue
        if not e.sum / (e.count << SCALE_BITS) > merge_threshold:
            break
        a, b = e.a, e.b            # a < b: a stays
        del adj[a][b]
        del adj[b][a]
        parent[b] = a
        for c, (count, total) in adj[b].items():
            del adj[c][b]
            if c in adj[a]:
                have = adj[a][c]
                count, total = count + have[0], total + have[1]
            adj[a][c] = adj[c][a] = (count, total)
            heapq.heappush(heap, _Edge(min(a, c), max(a, c), count, total))
        adj[b] = None

    # parents are smaller than their children: one ascending pass resolves
    seg = [0] * (n_fragments + 1)
    next_id = 0
    for f in range(1, n_fragments + 1):
        if parent[f] == f:
            next_id += 1
            seg[f] = next_id
        else:
            seg[f] = seg[parent[f]]
    return np.array(seg, dtype=np.uint32)
