"""The linear BVH the GPU hierarchy build makes, stated once in NumPy.

pt_bvh_build.hip meets this file bit for bit: the same codes, the same order, the same tree, the same numbering.  Nothing
here is fast; it is the rule.

    flat world triangles -> primitive boxes, centroids -> 63-bit Morton codes -> order by (code, triangle index)
    -> Karras' binary radix tree over the ordered keys -> cut at ranges of at most leaf_size triangles
    -> collapse to 4-wide nodes, numbered breadth-first -> stack bound, heights, the refit's tables

The rule in full:

* Box of a triangle: fp32 min / max over its three vertices.  Centroid: 0.5f * (lo + hi), fp32.  The centroid bounds are
  the exact min / max of the centroids.  Vertices are finite.
* Quantisation, per axis, every step one fp32 operation, nothing contracted:
      ext = hi - lo;  ext > 0 is false: 0
      v = ((c - lo) / ext) * 2097152.0f;  v >= 2097151: 2097151;  v > 0: trunc(v);  otherwise 0
* Code: bit 3 i + 2 is bit i of x, bit 3 i + 1 of y, bit 3 i of z (i = 0 .. 20): 63 bits.
* Order: ascending (code, triangle index).  The leaf order IS this order: the permutation is the ordered triangle indices.
* Radix tree: Karras 2012 over the ordered keys; the common prefix of two positions with equal codes is
  64 + clz32(i ^ j), so equal codes split by position and give a balanced subtree.
* A radix node whose range holds at most leaf_size (1 .. 4) triangles is a leaf, ~ref = first << 3 | count - 1.
* 4-wide collapse of an inner radix node: its slots start as [left, right]; while fewer than four slots are in use and
  some slot holds an inner radix node, the one with the LARGEST RANGE (the first such slot on a tie) is replaced by its left
  child and its right child is appended.  `reserved` is the number of slots in use; unused slots hold -1.
* Numbering: the root is node 0; the nodes of one 4-wide depth are numbered in the order of their parents and, under one
  parent, of their slots.  A scene of at most leaf_size triangles is a root with one leaf child; an empty scene a root
  with no child.
* Stack bound: 1 + the largest sum of (reserved - 1) over the nodes of a root-to-leaf path.
"""
from collections import namedtuple

import numpy as np

CODE_BITS = 21
MAX_LEAF_TRIANGLES = 4
MAX_STACK_BOUND = 96
# the leaf size of a GPU build when the caller names none (DESIGN.md f24 says how it was chosen)
DEFAULT_LEAF_SIZE = 2

Lbvh = namedtuple("Lbvh", "codes permutation child reserved stack_bound heights order level_offsets leaf_position levels depths")


class Refused(Exception):
    """The tree's stack bound exceeds what the traversal can hold; nothing is built."""


def vertices(flat):
    """(n, 3, 3) float32 vertices of flat world triangles given as (n, 12) uint32 words (48-byte WorldTriangle)."""
    flat = np.ascontiguousarray(flat)
    if flat.dtype == np.float32 and flat.ndim == 3:
        return flat
    words = flat.view(np.uint32).reshape(-1, 12)
    return np.ascontiguousarray(words.reshape(-1, 3, 4)[:, :, :3]).view(np.float32)


def centroids(v):
    lo = np.minimum(np.minimum(v[:, 0], v[:, 1]), v[:, 2])
    hi = np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 2])
    return (np.float32(0.5) * (lo + hi)).astype(np.float32)


def quantise(c, lo, hi):
    """(n, 3) uint32 cells of centroids c inside the centroid bounds [lo, hi]."""
    c, lo, hi = np.asarray(c, np.float32), np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    with np.errstate(all="ignore"):
        ext = (hi - lo).astype(np.float32)
        v = (((c - lo).astype(np.float32) / ext).astype(np.float32) * np.float32(2097152.0)).astype(np.float32)
    top = np.float32((1 << CODE_BITS) - 1)
    q = np.where(v >= top, top, np.where(v > 0, np.trunc(v), np.float32(0))).astype(np.uint32)
    return np.where(np.broadcast_to(ext > 0, q.shape), q, np.uint32(0)).astype(np.uint32)


def interleave(q):
    """(n, 3) cells -> uint64 codes of 63 bits, x in the highest bit of every triple."""
    q = np.asarray(q, np.uint64)
    code = np.zeros(q.shape[0], np.uint64)
    for i in range(CODE_BITS):
        for axis in range(3):
            code |= ((q[:, axis] >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + 2 - axis)
    return code


def morton_codes(v):
    c = centroids(v)
    if len(c) == 0:
        return np.zeros(0, np.uint64)
    return interleave(quantise(c, c.min(axis=0), c.max(axis=0)))


def _bit_length(x):
    """Bits needed for every element of a uint64 array (0 for 0)."""
    x = np.array(x, np.uint64)
    bits = np.zeros(x.shape, np.int64)
    for step in (32, 16, 8, 4, 2, 1):
        high = x >= (np.uint64(1) << np.uint64(step))
        bits += np.where(high, step, 0)
        x = np.where(high, x >> np.uint64(step), x)
    return bits + (x > 0)


def radix_tree(codes):
    """Karras' tree over ordered codes (n >= 2): first, last, split of the n - 1 inner nodes.  The children of node i
    are the ranges [first, split] and [split + 1, last]; a child of more than one key is inner node `split` (left) or
    `split + 1` (right).  Every node runs Karras' searches on its own; here all nodes take each step together."""
    codes = np.asarray(codes, np.uint64)
    n = len(codes)
    i = np.arange(n - 1, dtype=np.int64)

    def delta(j):
        """Common prefix of the keys at i and j (-1 outside the array): of the codes, or, for equal codes, 64 + that of
        the positions as 32-bit numbers."""
        inside = (j >= 0) & (j < n)
        jj = np.clip(j, 0, n - 1)
        x = codes[i] ^ codes[jj]
        prefix = np.where(x != 0, 64 - _bit_length(x), 64 + 32 - _bit_length((i ^ jj).astype(np.uint64)))
        return np.where(inside, prefix, -1)

    d = np.where(delta(i + 1) > delta(i - 1), 1, -1).astype(np.int64)
    dmin = delta(i - d)
    lmax = np.full(n - 1, 2, np.int64)
    while True:
        grow = delta(i + lmax * d) > dmin
        if not grow.any():
            break
        lmax[grow] *= 2
    length, t = np.zeros(n - 1, np.int64), lmax // 2
    while (t >= 1).any():
        take = (t >= 1) & (delta(i + (length + t) * d) > dmin)
        length[take] += t[take]
        t //= 2
    j = i + length * d
    dnode = delta(j)
    s, t = np.zeros(n - 1, np.int64), length.copy()
    while (t > 1).any():
        live = t > 1
        t = np.where(live, (t + 1) // 2, t)
        take = live & (delta(i + (s + t) * d) > dnode)
        s[take] += t[take]
        t = np.where(live, t, 0)
    split = i + s * d + np.minimum(d, 0)
    return np.minimum(i, j).astype(np.uint32), np.maximum(i, j).astype(np.uint32), split.astype(np.uint32)


def build(flat, leaf_size=DEFAULT_LEAF_SIZE, max_stack_bound=MAX_STACK_BOUND, binary=None):
    """The whole statement over flat world triangles ((n, 12) uint32 words or (n, 3, 3) float32 vertices).

    `binary` is the hook of another method of the same builder (prosper_amd/ploc.py): called with the vertices and the
    order by (code, index) of a scene of more than leaf_size triangles, it returns the leaf order and a binary tree over
    it in the radix tree's own form (first, last, split), plus a key per inner node; the collapse then opens the slot
    with the largest (key, range) instead of the largest range.  Without it nothing here changes."""
    if not 1 <= leaf_size <= MAX_LEAF_TRIANGLES:
        raise ValueError("leaf_size is 1 .. %d" % MAX_LEAF_TRIANGLES)
    v = vertices(flat)
    n = len(v)
    codes = morton_codes(v)
    permutation = np.lexsort((np.arange(n), codes)).astype(np.uint32)
    ordered = codes[permutation]

    child_rows, reserved, path = [], [], []
    if n <= leaf_size:
        child_rows.append([~((0 << 3) | (n - 1)) if n else -1, -1, -1, -1])
        reserved.append(1 if n else 0)
        path.append(0)
        level_starts = [0, 1]
    else:
        key = None
        if binary is None:
            first, last, split = radix_tree(ordered)
        else:
            permutation, first, last, split, key = binary(v, permutation)

        def kids_of(t):
            return [(int(first[t]), int(split[t]), int(split[t])), (int(split[t]) + 1, int(last[t]), int(split[t]) + 1)]

        level, path_of, level_starts = [0], {0: 0}, [0]
        numbered = 1
        while level:
            following = []
            for t in level:
                kids = kids_of(t)
                while len(kids) < 4:
                    best, best_key = -1, None
                    for c, (a, b, radix) in enumerate(kids):
                        if b - a + 1 <= leaf_size:
                            continue
                        kid_key = b - a + 1 if key is None else (key[radix], b - a + 1)
                        if best < 0 or kid_key > best_key:
                            best, best_key = c, kid_key
                    if best < 0:
                        break
                    opened = kids_of(kids[best][2])
                    kids[best] = opened[0]
                    kids.append(opened[1])
                row = [-1, -1, -1, -1]
                for c, (a, b, radix) in enumerate(kids):
                    if b - a + 1 > leaf_size:
                        row[c] = numbered
                        numbered += 1
                        following.append(radix)
                        path_of[radix] = path_of[t] + len(kids) - 1
                    else:
                        row[c] = ~((a << 3) | (b - a))
                child_rows.append(row)
                reserved.append(len(kids))
                path.append(path_of[t])
            level_starts.append(level_starts[-1] + len(level))
            level = following

    child = np.array(child_rows, np.int32).reshape(-1, 4)
    reserved = np.array(reserved, np.uint32)
    stack_bound = 1 + max(int(p) + max(int(k), 1) - 1 for p, k in zip(path, reserved))
    if stack_bound > max_stack_bound:
        raise Refused("stack bound %d exceeds %d" % (stack_bound, max_stack_bound))

    count = len(child)
    heights = np.zeros(count, np.uint32)
    for i in range(count - 1, -1, -1):  # every child is numbered after its parent
        inner = child[i][child[i] >= 0]
        if len(inner):
            heights[i] = heights[inner].max() + 1
    levels = int(heights[0]) + 1
    order = np.lexsort((np.arange(count), heights)).astype(np.uint32)
    level_offsets = np.concatenate([[0], np.cumsum(np.bincount(heights, minlength=levels))]).astype(np.uint32)
    leaf_position = np.zeros(n, np.uint32)
    leaf_position[permutation] = np.arange(n, dtype=np.uint32)
    return Lbvh(codes, permutation, child, reserved, stack_bound, heights, order, level_offsets, leaf_position, levels,
                len(level_starts) - 1)


def recursive_stack_bound(child, reserved):
    """The same bound by a plain walk from the root (what a test compares build()'s with)."""
    def need(i):
        k = int(reserved[i])
        deepest = max([need(int(c)) for c in child[i][:k] if c >= 0], default=0)
        return max(k, 1) - 1 + deepest
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    return need(0) + 1


def decode_boxes(nodes):
    """Child boxes of (n, 20) uint32 node words as exact float64 (lo, hi), each (n, 4, 3): the fp32 origin plus the
    binary16 offsets, which the encoder rounded outward."""
    nodes = np.ascontiguousarray(nodes, np.uint32)
    origin = nodes[:, 0:3].view(np.float32).astype(np.float64)
    halves = nodes[:, 4:16].view(np.float16).reshape(-1, 2, 3, 4).astype(np.float64)  # [lo | hi][axis][child]
    lo = origin[:, None, :] + np.transpose(halves[:, 0], (0, 2, 1))
    hi = origin[:, None, :] + np.transpose(halves[:, 1], (0, 2, 1))
    return lo, hi
