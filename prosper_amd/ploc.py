"""The PLOC method of the GPU hierarchy build, stated once in NumPy.

pt_bvh_ploc.hip meets this file bit for bit: the same rounds, the same merges, the same leaf order, the same numbering.
Nothing here is fast; it is the rule.  The binary tree comes from parallel locally-ordered clustering (Meister and
Bittner 2018) over the Morton order of prosper_amd/lbvh.py; everything behind the binary tree is lbvh.py's own code.

    flat world triangles -> boxes, centroids, 63-bit Morton codes, order by (code, triangle index)      (lbvh.py)
    -> clusters in that order, merged round by round with their nearest neighbour within `radius` positions
    -> ranges from the root down: the leaf order -> cut at leaf_size -> 4-wide collapse by box cost, numbering,
    stack bound, heights, the refit's tables                                                                (lbvh.py)

The rule in full (s[p] is the triangle at ordered position p; vertices are finite):

* Clusters: a list of binary nodes.  At the start position p holds leaf p, whose box is the fp32 min / max box of
  triangle s[p] and whose size is 1.
* Cost of a pair of boxes: per axis lo = min, hi = max, e = hi - lo; cost = (e.x * e.y + e.y * e.z) + e.z * e.x, every
  operation one fp32 operation, nothing contracted.  The cost is never negative: its bits without the sign bit (a zero
  may carry one), compared as unsigned integers, compare as the floats do.  The cost of a box is the same expression
  over its own extent.
* A round over m > 1 clusters at positions 0 .. m - 1.  Every search reads the state from the start of the round.  For
  position i the candidates are every j != i with |j - i| <= radius and 0 <= j < m; nn(i) is the candidate with the least
  key (cost, |j - i|, min(i, j) & 1, min(i, j)), compared lexicographically.  That is a total order on unordered pairs:
  the least pair overall is mutual, so every round merges at least one pair; and among equal boxes the neighbours
  (0, 1), (2, 3), .. pair up, which keeps duplicates balanced (with "lowest cost, then lowest index" identical
  triangles become a comb of depth n - 1, which the stack bound refuses).  For a fixed i the last component comes down to
  "is j below i", so the packed key is  cost bits << 32 | |j - i| << 2 | (min(i, j) & 1) << 1 | (j > i).
* Merge: the pair (i, j), i < j, merges iff nn(nn(i)) == i.  The merged cluster takes position i; its left child is the
  cluster that was at i, its right child the one at j, its box the exact union, its size the sum.  Position j is
  removed; survivors keep their order.  Rounds repeat until m = 1; their number is part of the result.
* Ranges: the root starts at 0; a node's left child takes [first, first + size(left)), its right child the rest;
  permutation[q] = s[p] for the leaf p that lands at q.  Every binary node's triangles are contiguous in leaf order.
* A node of at most leaf_size (1 .. 4) triangles is a leaf, ~ref = first << 3 | count - 1.  A scene of at most leaf_size
  triangles and the empty scene are the linear statement's.
* 4-wide collapse: the linear statement's, but the slot to open is the inner node with the LARGEST COST OF ITS OWN BOX;
  on equal cost the one with the larger range, then the first such slot.  (The range decides among equal boxes: with
  "the first slot" alone a block of duplicates opens one side only and comes out deeper than the linear tree's.)
  Numbering, `reserved`, stack bound and refusal, heights, order, level offsets and leaf positions are lbvh.py's.
* The numbering of the binary nodes is internal (here: leaves 0 .. n - 1 by ordered position, merged nodes from n in the
  order of rounds and, within a round, of positions).
"""
from collections import namedtuple

import numpy as np

from . import lbvh

DEFAULT_RADIUS = 8
MAX_RADIUS = 32
# the leaf size of a PLOC build when the caller names none (DESIGN.md f26 says how it and the radius were chosen)
DEFAULT_LEAF_SIZE = 2
# cluster count from which the GPU build runs all remaining rounds in one workgroup (same rounds, same result)
SINGLE_WORKGROUP_CLUSTERS = 512

# rounds: how many; round_counts: the clusters every round started with (the GPU build runs those that start with at most
# SINGLE_WORKGROUP_CLUSTERS in its one-workgroup launch)
Ploc = namedtuple("Ploc", lbvh.Lbvh._fields + ("rounds", "round_counts"))
Binary = namedtuple("Binary", "left right lo hi sizes root rounds order round_counts")


def boxes(v):
    """fp32 min / max boxes of (n, 3, 3) vertices."""
    return np.minimum(np.minimum(v[:, 0], v[:, 1]), v[:, 2]), np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 2])


def box_cost(lo, hi):
    e = (hi - lo).astype(np.float32)
    return ((e[..., 0] * e[..., 1]).astype(np.float32) + (e[..., 1] * e[..., 2]).astype(np.float32)).astype(np.float32) + \
        (e[..., 2] * e[..., 0]).astype(np.float32)


def pair_cost(lo_a, hi_a, lo_b, hi_b):
    return box_cost(np.minimum(lo_a, lo_b), np.maximum(hi_a, hi_b))


def cost_bits(cost):
    return np.ascontiguousarray(cost, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def nearest(lo, hi, radius):
    """nn(i) of every position of one round's clusters."""
    m = len(lo)
    i = np.arange(m, dtype=np.int64)
    best = np.full(m, np.iinfo(np.uint64).max, np.uint64)
    nn = np.full(m, -1, np.int64)
    for d in range(1, min(radius, m - 1) + 1):
        for above in (0, 1):
            j = i + d if above else i - d
            inside = (j >= 0) & (j < m)
            jj = np.clip(j, 0, m - 1)
            bits = cost_bits(pair_cost(lo, hi, lo[jj], hi[jj])).astype(np.uint64)
            key = (bits << np.uint64(32)) | np.uint64(d << 2) | ((np.minimum(i, jj) & 1).astype(np.uint64) << np.uint64(1)) | np.uint64(above)
            take = inside & (key < best)
            best = np.where(take, key, best)
            nn = np.where(take, j, nn)
    return nn


def binary_tree(flat, radius=DEFAULT_RADIUS, order=None):
    """The binary tree of the rounds over n >= 1 triangles: left / right child of the inner nodes n .. 2 n - 2 (indexed
    from 0), the boxes and sizes of all 2 n - 1 nodes, the root, the round count and the order s the leaves stand for."""
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError("radius is 1 .. %d" % MAX_RADIUS)
    v = lbvh.vertices(flat)
    n = len(v)
    if order is None:
        order = np.lexsort((np.arange(n), lbvh.morton_codes(v))).astype(np.uint32)
    lo, hi = boxes(v[order])
    node_lo, node_hi = [lo], [hi]
    left, right, sizes = [], [], [np.ones(n, np.int64)]
    ids, size = np.arange(n, dtype=np.int64), np.ones(n, np.int64)
    made, rounds, round_counts = n, 0, []
    while len(ids) > 1:
        m = len(ids)
        round_counts.append(m)
        nn = nearest(lo, hi, radius)
        i = np.arange(m, dtype=np.int64)
        mutual = nn[nn] == i
        merges, removed = mutual & (i < nn), mutual & (nn < i)
        assert merges.any()
        a, b = i[merges], nn[merges]
        union_lo, union_hi = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
        left.append(ids[a])
        right.append(ids[b])
        node_lo.append(union_lo)
        node_hi.append(union_hi)
        sizes.append(size[a] + size[b])
        lo, hi, ids, size = lo.copy(), hi.copy(), ids.copy(), size.copy()
        lo[a], hi[a], size[a] = union_lo, union_hi, size[a] + size[b]
        ids[a] = made + np.arange(len(a))
        made += len(a)
        keep = ~removed
        lo, hi, ids, size = lo[keep], hi[keep], ids[keep], size[keep]
        rounds += 1
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return Binary(cat(left, np.int64), cat(right, np.int64), np.concatenate(node_lo), np.concatenate(node_hi),
                  cat(sizes, np.int64), int(ids[0]), rounds, order, tuple(round_counts))


def ranges(tree):
    """first leaf position of every binary node, from the root down."""
    n = (len(tree.sizes) + 1) // 2
    first = np.zeros(len(tree.sizes), np.int64)
    for node in range(len(tree.sizes) - 1, n - 1, -1):  # a merged node is made after its children
        l, r = tree.left[node - n], tree.right[node - n]
        first[l] = first[node]
        first[r] = first[node] + tree.sizes[l]
    return first


def build(flat, leaf_size=DEFAULT_LEAF_SIZE, radius=DEFAULT_RADIUS, max_stack_bound=lbvh.MAX_STACK_BOUND):
    """The whole statement over flat world triangles ((n, 12) uint32 words or (n, 3, 3) float32 vertices)."""
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError("radius is 1 .. %d" % MAX_RADIUS)
    rounds = [0, ()]

    def binary(v, order):
        tree = binary_tree(v, radius, order)
        n = len(order)
        rounds[:] = tree.rounds, tree.round_counts
        start = ranges(tree)
        permutation = np.zeros(n, np.uint32)
        permutation[start[:n]] = order
        # the radix tree's form: the root is node 0, a left child is numbered by its last position, a right child by
        # its first (a binary tree over contiguous ranges has exactly one such numbering)
        first, last, split = (np.zeros(n - 1, np.uint32) for _ in range(3))
        key = np.zeros(n - 1, np.float32)
        number = {tree.root: 0}
        cost = box_cost(tree.lo, tree.hi)
        for node in range(2 * n - 2, n - 1, -1):
            l, r = int(tree.left[node - n]), int(tree.right[node - n])
            a, b = int(start[node]), int(start[node] + tree.sizes[node] - 1)
            s = a + int(tree.sizes[l]) - 1
            number[l], number[r] = s, s + 1
            t = number[node]
            first[t], last[t], split[t], key[t] = a, b, s, cost[node]
        return permutation, first, last, split, key

    return Ploc(*lbvh.build(flat, leaf_size, max_stack_bound, binary=binary), *rounds)
