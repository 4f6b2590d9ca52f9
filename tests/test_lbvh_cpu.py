"""prosper_amd/lbvh.py alone: the NumPy statement of the linear BVH the GPU hierarchy build makes.
tests/test_gpu_hierarchy.py holds the kernels to it; here the statement is held to what a valid tree is."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lbvh_sets
from prosper_amd import lbvh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = lbvh_sets.sets()
LEAF_SIZES = (1, 2, 4)


@pytest.fixture(scope="module")
def built():
    return {(name, leaf): lbvh.build(v, leaf_size=leaf) for name, v in SETS.items() for leaf in LEAF_SIZES}


def _leaves(tree):
    """(first, count) of every leaf child, and every inner child reference with its parent."""
    leaves, inner = [], []
    for i, (row, k) in enumerate(zip(tree.child, tree.reserved)):
        assert (row[k:] == -1).all()
        for ref in row[:k]:
            if ref < 0:
                leaves.append(((~int(ref)) >> 3, ((~int(ref)) & 7) + 1))
            else:
                inner.append((i, int(ref)))
    return leaves, inner


@pytest.mark.parametrize("leaf", LEAF_SIZES)
@pytest.mark.parametrize("name", sorted(SETS))
def test_the_statement_gives_a_valid_tree(built, name, leaf):
    tree, n = built[(name, leaf)], len(SETS[name])
    count = len(tree.child)
    leaves, inner = _leaves(tree)
    # the leaf ranges tile [0, n) exactly once, no leaf is longer than the leaf size (at most 4)
    covered = np.zeros(n, np.int64)
    for first, length in leaves:
        assert 1 <= length <= leaf <= lbvh.MAX_LEAF_TRIANGLES
        covered[first:first + length] += 1
    assert (covered == 1).all()
    # node 0 is the root and is inner; every child is numbered after its parent; every node but the root has one parent
    assert count >= 1 and (tree.reserved <= 4).all()
    assert all(child > parent for parent, child in inner)
    assert sorted(child for _, child in inner) == list(range(1, count))
    if n == 0:
        assert count == 1 and tree.reserved[0] == 0
    elif n <= leaf:
        assert count == 1 and tree.reserved[0] == 1 and tree.child[0][0] == ~(n - 1)
    else:
        assert (tree.reserved >= 2).all()
    # the stack bound is a plain recursive walk's, and the traversal can hold it
    assert tree.stack_bound == lbvh.recursive_stack_bound(tree.child, tree.reserved) <= lbvh.MAX_STACK_BOUND
    # heights, the nodes by height and the level offsets agree
    for parent, child in inner:
        assert tree.heights[parent] > tree.heights[child]
    for i in range(count):
        below = [tree.heights[c] for c in tree.child[i] if c >= 0]
        assert tree.heights[i] == (max(below) + 1 if below else 0)
    assert tree.levels == tree.heights[0] + 1 == len(tree.level_offsets) - 1
    assert tree.level_offsets[0] == 0 and tree.level_offsets[-1] == count
    assert sorted(tree.order) == list(range(count))
    for level in range(tree.levels):
        members = tree.order[tree.level_offsets[level]:tree.level_offsets[level + 1]]
        assert (tree.heights[members] == level).all() and (np.diff(members.astype(np.int64)) > 0).all()
    # the permutation is one, ordered by (code, index), and the leaf position is its inverse
    assert sorted(tree.permutation) == list(range(n))
    keys = list(zip(tree.codes[tree.permutation].tolist(), tree.permutation.tolist()))
    assert keys == sorted(keys)
    assert (tree.permutation[tree.leaf_position] == np.arange(n)).all()


def test_two_runs_give_identical_results():
    for name in ("soup", "identical70", "spread"):
        a, b = lbvh.build(SETS[name]), lbvh.build(SETS[name].copy())
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_equal_codes_give_a_balanced_subtree():
    for n in (9, 70):
        tree = lbvh.build(SETS["identical%d" % n], leaf_size=1)
        assert (tree.codes == 0).all() and (tree.permutation == np.arange(n)).all()
        # binary depth ceil(log2 n); the collapse takes two binary levels per 4-wide depth
        assert tree.levels <= (int(np.ceil(np.log2(n))) + 1) // 2 + 1


def test_zero_extent_axes_quantise_to_zero():
    x_bits = sum(1 << (3 * i + 2) for i in range(lbvh.CODE_BITS))
    z_bits = sum(1 << (3 * i) for i in range(lbvh.CODE_BITS))
    line, plane, point = (lbvh.morton_codes(lbvh.vertices(SETS[k])) for k in ("line", "plane", "point"))
    assert (line & ~np.uint64(x_bits) == 0).all() and len(np.unique(line)) > 8
    assert (plane & ~np.uint64(x_bits | z_bits) == 0).all() and (plane & np.uint64(z_bits)).any()
    assert (point == 0).all()


def test_hand_computed_codes():
    lo, hi = np.float32([0.0, -1.0, 2.0]), np.float32([8.0, 1.0, 2.0])
    top = (1 << 21) - 1
    cells = lbvh.quantise(np.float32([[0.0, -1.0, 2.0], [8.0, 1.0, 2.0], [4.0, 0.0, 2.0], [1.0, -0.5, 2.0], [8.0, -1.0, 2.0]]), lo, hi)
    # the minimum is cell 0, the maximum is clamped to the top cell, the middle is 2^20; z has no extent
    assert cells.tolist() == [[0, 0, 0], [top, top, 0], [1 << 20, 1 << 20, 0], [1 << 18, 1 << 19, 0], [top, 0, 0]]
    codes = lbvh.interleave(cells)
    all_x = sum(1 << (3 * i + 2) for i in range(21))
    all_y = sum(1 << (3 * i + 1) for i in range(21))
    assert codes.tolist() == [0, all_x | all_y, (1 << 62) | (1 << 61), (1 << 56) | (1 << 58), all_x]
    assert int(lbvh.interleave(np.uint32([[top, top, top]]))[0]) == (1 << 63) - 1
    assert int(lbvh.interleave(np.uint32([[1, 0, 0]]))[0]) == 4 and int(lbvh.interleave(np.uint32([[0, 0, 1 << 20]]))[0]) == 1 << 60
    # a third of the way is not a binary fraction: fl(fl(1 / 3) * 2^21) truncated
    third = lbvh.quantise(np.float32([[1.0, 0.0, 0.0]]), np.float32([0.0, 0.0, 0.0]), np.float32([3.0, 1.0, 1.0]))
    assert third[0].tolist() == [int(np.float32(1.0) / np.float32(3.0) * np.float32(2097152.0)), 0, 0] == [699050, 0, 0]


def test_spread_coordinates_keep_distinct_cells():
    tree = lbvh.build(SETS["spread"], leaf_size=1)
    assert len(np.unique(tree.codes)) > len(tree.codes) // 2


def test_the_refusal():
    """No input that a test can hold exceeds the traversal's 96 entries (the deepest path of n triangles
    needs at most about 64 + 1.5 log2 n entries, so upwards of two million triangles), so the check itself is tested with
    the limit lowered, on the deepest tree a few hundred triangles give: one triangle per code bit in geometric
    sequence on the three axes, and a balanced block of identical ones below the last split."""
    deep = lbvh_sets.deep_comb()
    tree = lbvh.build(deep, leaf_size=1)
    assert len(np.unique(tree.codes)) == 65  # every code bit is used once: the comb is 63 splits deep
    assert 75 <= tree.stack_bound <= lbvh.MAX_STACK_BOUND
    assert tree.stack_bound == lbvh.recursive_stack_bound(tree.child, tree.reserved)
    assert lbvh.build(deep, leaf_size=1, max_stack_bound=tree.stack_bound).stack_bound == tree.stack_bound
    with pytest.raises(lbvh.Refused):
        lbvh.build(deep, leaf_size=1, max_stack_bound=tree.stack_bound - 1)
    assert lbvh.build(deep, leaf_size=4).stack_bound < tree.stack_bound
    with pytest.raises(ValueError):
        lbvh.build(deep, leaf_size=5)


def test_decode_boxes_reads_the_node_layout():
    node = np.zeros((1, 20), np.uint32)
    node[0, 0:3] = np.float32([1.0, 2.0, 3.0]).view(np.uint32)
    halves = np.zeros((2, 3, 4), np.float16)
    halves[0, 0, 1], halves[1, 0, 1], halves[1, 2, 3] = 0.5, 1.5, 4.0  # lo.x of child 1, hi.x of child 1, hi.z of child 3
    node[0, 4:16] = halves.reshape(-1).view(np.uint32)
    lo, hi = lbvh.decode_boxes(node)
    assert lo[0, 1].tolist() == [1.5, 2.0, 3.0] and hi[0, 1].tolist() == [2.5, 2.0, 3.0] and hi[0, 3].tolist() == [1.0, 2.0, 7.0]


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    """tests/lbvh_rule_main.cpp: the functions the kernels call (pt_bvh_rule.hpp), built for the host without contraction,
    under AddressSanitizer + UBSan."""
    gxx = shutil.which("g++")
    assert gxx, "the host C++ compiler (g++) is needed"
    exe = str(tmp_path_factory.mktemp("lbvh_rule") / "lbvh_rule")
    subprocess.check_call([
        gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "prosper_amd", "csrc"),
        os.path.join(ROOT, "tests", "lbvh_rule_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("leaf", (1, 4))
@pytest.mark.parametrize("name", sorted(SETS) + ["deep"])
def test_the_kernels_arithmetic_meets_the_statement_on_a_cpu(rule_program, built, tmp_path, name, leaf):
    v = lbvh_sets.deep_comb() if name == "deep" else SETS[name]
    want = lbvh.build(v, leaf_size=leaf) if name == "deep" else built[(name, leaf)]
    flat = np.zeros((len(v), 12), np.uint32)
    flat.reshape(-1, 3, 4)[:, :, :3] = v.view(np.uint32)
    flat[:, 3] = 7  # (the words between the vertices are not coordinates)
    assert np.array_equal(lbvh.vertices(flat), v)
    src, dst = str(tmp_path / "triangles.bin"), str(tmp_path / "tree.bin")
    flat.tofile(src)
    out = subprocess.run([rule_program, src, str(leaf), dst], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "lbvh rule ok" in text and "runtime error" not in text, text[-3000:]
    words = np.fromfile(dst, np.uint32)
    n, count, bound = (int(x) for x in words[:3])
    assert n == len(v) and count == len(want.child) and bound == want.stack_bound
    at = 3
    assert np.array_equal(words[at:at + 2 * n].view(np.uint64), want.codes)
    at += 2 * n
    assert np.array_equal(words[at:at + n], want.permutation)
    at += n
    nodes = words[at:].reshape(count, 5)
    assert np.array_equal(nodes[:, :4].view(np.int32), want.child) and np.array_equal(nodes[:, 4], want.reserved)
