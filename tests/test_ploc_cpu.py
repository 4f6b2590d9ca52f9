"""prosper_amd/ploc.py alone: the NumPy statement of the PLOC method of the GPU hierarchy build, held to
what a valid tree is, to rounds computed by hand, to its tie rule and to the tree cost it is there for; and
tests/ploc_rule_main.cpp, the kernels' own rule functions run on a CPU under sanitizers, held to the statement.
tests/test_gpu_hierarchy_ploc.py holds the kernels to it.  The nested comb (tests/ploc_sets.py) puts the statement's stack
bound on the limit and one beyond it: the facts tests/test_gpu_hierarchy_refusal.py leans on are derived here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lbvh_sets
import ploc_sets
from prosper_amd import lbvh, ploc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF_SIZES = (1, 2, 4)
RADII = (1, 16, 32)


SETS = ploc_sets.sets()


@pytest.fixture(scope="module")
def built():
    return {(name, leaf, radius): ploc.build(v, leaf_size=leaf, radius=radius)
            for name, v in SETS.items() for leaf in LEAF_SIZES for radius in RADII}


def _leaves(tree):
    leaves, inner = [], []
    for i, (row, k) in enumerate(zip(tree.child, tree.reserved)):
        assert (row[k:] == -1).all()
        for ref in row[:k]:
            if ref < 0:
                leaves.append(((~int(ref)) >> 3, ((~int(ref)) & 7) + 1))
            else:
                inner.append((i, int(ref)))
    return leaves, inner


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("leaf", LEAF_SIZES)
@pytest.mark.parametrize("name", sorted(SETS))
def test_the_statement_gives_a_valid_tree(built, name, leaf, radius):
    tree, n = built[(name, leaf, radius)], len(SETS[name])
    count = len(tree.child)
    leaves, inner = _leaves(tree)
    # every triangle is in exactly one leaf; leaves are contiguous ranges of at most leaf_size triangles
    covered = np.zeros(n, np.int64)
    for first, length in leaves:
        assert 1 <= length <= leaf
        covered[first:first + length] += 1
    assert (covered == 1).all()
    assert sorted(tree.permutation) == list(range(n)) and (tree.permutation[tree.leaf_position] == np.arange(n)).all()
    # children are numbered after their parents, every node but the root has one parent
    assert count >= 1 and (tree.reserved <= 4).all()
    assert all(child > parent for parent, child in inner)
    assert sorted(child for _, child in inner) == list(range(1, count))
    if n == 0:
        assert count == 1 and tree.reserved[0] == 0 and tree.rounds == 0
    elif n <= leaf:
        assert count == 1 and tree.reserved[0] == 1 and tree.child[0][0] == ~(n - 1) and tree.rounds == 0
        assert np.array_equal(tree.permutation, lbvh.build(SETS[name], leaf_size=leaf).permutation)
    else:
        assert (tree.reserved >= 2).all() and 1 <= tree.rounds <= n - 1
        # every round merges at least one pair, and none more than every second cluster
        counts = tree.round_counts + (1,)
        assert len(tree.round_counts) == tree.rounds and counts[0] == n
        assert all(a > b >= (a + 1) // 2 for a, b in zip(counts, counts[1:]))
    assert tree.stack_bound == lbvh.recursive_stack_bound(tree.child, tree.reserved) <= lbvh.MAX_STACK_BOUND
    # heights, the nodes by height and the level offsets agree (lbvh.py's code, over this tree)
    for i in range(count):
        below = [tree.heights[c] for c in tree.child[i] if c >= 0]
        assert tree.heights[i] == (max(below) + 1 if below else 0)
    assert tree.levels == tree.heights[0] + 1 == len(tree.level_offsets) - 1
    assert tree.level_offsets[0] == 0 and tree.level_offsets[-1] == count and sorted(tree.order) == list(range(count))
    for level in range(tree.levels):
        members = tree.order[tree.level_offsets[level]:tree.level_offsets[level + 1]]
        assert (tree.heights[members] == level).all() and (np.diff(members.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("name", ["soup", "n257", "t_plus_1"])
def test_every_binary_node_is_contiguous_and_holds_its_children(name):
    tree = ploc.binary_tree(SETS[name], 16)
    n = len(SETS[name])
    first = ploc.ranges(tree)
    assert tree.root == 2 * n - 2 and tree.sizes[tree.root] == n and sorted(first[:n]) == list(range(n))
    lo, hi = ploc.boxes(SETS[name][tree.order])
    for node in range(n, 2 * n - 1):
        l, r = tree.left[node - n], tree.right[node - n]
        assert l < node and r < node and tree.sizes[node] == tree.sizes[l] + tree.sizes[r]
        assert first[l] == first[node] and first[r] == first[node] + tree.sizes[l]
        assert np.array_equal(tree.lo[node], np.minimum(tree.lo[l], tree.lo[r]))
        assert np.array_equal(tree.hi[node], np.maximum(tree.hi[l], tree.hi[r]))
    assert np.array_equal(tree.lo[:n], lo) and np.array_equal(tree.hi[:n], hi)


def test_two_runs_give_identical_results():
    for name in ("soup", "identical70", "spread", "t_plus_1"):
        a, b = ploc.build(SETS[name]), ploc.build(SETS[name].copy())
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def _on_a_line(xs):
    """Triangles whose boxes are [x, x + 1] x [0, 1] x [0, 0]: the cost of a pair is its extent along x."""
    return np.float32([[[x, 0, 0], [x + 1, 0, 0], [x, 1, 0]] for x in xs])


def test_hand_computed_rounds():
    assert ploc.pair_cost(*(np.float32(c) for c in ([4, 0, 0], [5, 1, 0], [20, 0, 0], [21, 1, 0]))) == 17.0
    # four triangles A B C D at x = 0, 4, 5, 20, handed over as C A D B.  Costs: AB 5, AC 6, AD 21, BC 2, BD 17, CD 16.
    #   round 1: nn(A) = B, nn(B) = C, nn(C) = B, nn(D) = C: only (B, C) is mutual; A, whose nearest neighbour is not,
    #            and D are left over -> A, BC = [4, 6], D
    #   round 2: A-BC 6, BC-D 17, A-D 21: nn(A) = BC, nn(BC) = A, nn(D) = BC -> (A, BC); D is left over again
    #   round 3: the last pair.  The tree is ((A, (B, C)), D), the leaf order A B C D.
    four = ploc.binary_tree(_on_a_line([5, 0, 20, 4]), 16)
    assert four.order.tolist() == [1, 3, 0, 2] and four.rounds == 3 and four.root == 6
    assert four.left.tolist() == [1, 0, 5] and four.right.tolist() == [2, 4, 3] and four.sizes.tolist() == [1, 1, 1, 1, 2, 3, 4]
    assert four.lo[4:, 0].tolist() == [4, 0, 0] and four.hi[4:, 0].tolist() == [6, 6, 21]
    tree = ploc.build(_on_a_line([5, 0, 20, 4]), leaf_size=1, radius=16)
    assert tree.permutation.tolist() == [1, 3, 0, 2] and tree.rounds == 3
    # the collapse: [A(BC), D] -> [A, D, BC] -> [A, D, B, C]
    assert tree.child.tolist() == [[~(0 << 3), ~(3 << 3), ~(1 << 3), ~(2 << 3)]] and tree.reserved.tolist() == [4]
    two = ploc.build(_on_a_line([5, 0, 20, 4]), leaf_size=2, radius=16)
    assert two.child.tolist() == [[~(0 << 3), ~(3 << 3), ~(1 << 3 | 1), -1]] and two.reserved.tolist() == [3]
    # the nearest neighbour of position 0 with radius 1 is position 1 whatever lies beyond: same first round
    assert ploc.nearest(*ploc.boxes(_on_a_line([0, 4, 5, 20])), 1).tolist() == [1, 2, 1, 2]

    # five triangles at x = 0, 1, 10, 11, 13.  Costs: AB 2, BC 10, CD 2, DE 3, CE 4.
    #   round 1: (A, B) and (C, D) are mutual; nn(E) = D is not, E is left over -> AB = [0, 2], CD = [10, 12], E
    #   round 2: AB-CD 12, CD-E 4, AB-E 14: nn(AB) = CD is not mutual, (CD, E) is -> AB, CDE
    #   round 3: the last pair.  ((A, B), ((C, D), E)).
    five = ploc.binary_tree(_on_a_line([0, 1, 10, 11, 13]), 16)
    assert five.order.tolist() == [0, 1, 2, 3, 4] and five.rounds == 3
    assert five.left.tolist() == [0, 2, 6, 5] and five.right.tolist() == [1, 3, 4, 7]
    assert ploc.ranges(five).tolist() == [0, 1, 2, 3, 4, 0, 2, 2, 0]
    # with radius 1 position 0 never sees beyond its neighbour: the same tree here
    assert ploc.binary_tree(_on_a_line([0, 1, 10, 11, 13]), 1).left.tolist() == [0, 2, 6, 5]

    # equal costs at equal distance: the pair whose lower position is even wins, so (0, 1) and (2, 3) pair up
    even = ploc.binary_tree(_on_a_line([0, 1, 2, 3]), 16)
    assert even.rounds == 2 and even.left.tolist() == [0, 2, 4] and even.right.tolist() == [1, 3, 5]


def test_the_key_packs_the_order_on_pairs():
    lo, hi = ploc.boxes(_on_a_line([0, 1, 2, 3, 4]))
    # position 2: costs 2 at distance 1 on either side; (1, 2) has an odd lower position, (2, 3) an even one
    assert ploc.nearest(lo, hi, 16).tolist() == [1, 0, 3, 2, 3]
    # a zero cost with a sign bit is a zero
    assert ploc.cost_bits(np.float32([-0.0, 0.0, 1.0])).tolist() == [0, 0, 0x3F800000]


@pytest.mark.parametrize("name", ["identical9", "identical70", "point"])
def test_the_tie_rule_keeps_duplicates_balanced(built, name):
    n = len(SETS[name])
    for leaf in LEAF_SIZES:
        for radius in RADII:
            tree = built[(name, leaf, radius)]
            assert tree.rounds <= int(np.ceil(np.log2(n)))
            assert tree.depths == lbvh.build(SETS[name], leaf_size=leaf).depths


def test_a_radius_beyond_the_cluster_count():
    tree = ploc.build(SETS["n5"], leaf_size=1, radius=16)
    assert tree.rounds >= 2 and sorted(tree.permutation) == list(range(5))
    # every position sees every other: radius 4 is the same search
    for x, y in zip(tree, ploc.build(SETS["n5"], leaf_size=1, radius=4)):
        assert np.array_equal(x, y)
    for radius in (0, 33):
        with pytest.raises(ValueError):
            ploc.build(SETS["n5"], radius=radius)
    with pytest.raises(ValueError):
        ploc.build(SETS["n5"], leaf_size=5)


def test_the_refusal(built):
    tree = built[("soup", 1, 16)]
    assert ploc.build(SETS["soup"], leaf_size=1, radius=16, max_stack_bound=tree.stack_bound).stack_bound == tree.stack_bound
    with pytest.raises(lbvh.Refused):
        ploc.build(SETS["soup"], leaf_size=1, radius=16, max_stack_bound=tree.stack_bound - 1)


def _cut_cost(children, box, size, root):
    """The tree cost of a binary tree cut at leaves of 2: the box cost of every inner node plus, per leaf, its box cost
    times its triangles, over the root's box cost.  Exact sums of the fp32 boxes' costs in double."""
    def cost(node):
        lo, hi = (x.astype(np.float64) for x in box(node))
        e = hi - lo
        return e[0] * e[1] + e[1] * e[2] + e[2] * e[0]
    total, stack = 0.0, [root]
    while stack:
        node = stack.pop()
        if size(node) <= 2:
            total += cost(node) * size(node)
        else:
            total += cost(node)
            stack.extend(children(node))
    return total / cost(root) if cost(root) > 0.0 else total


def _ploc_cost(v, radius):
    tree = ploc.binary_tree(v, radius)
    n = len(v)
    return _cut_cost(lambda x: (int(tree.left[x - n]), int(tree.right[x - n])), lambda x: (tree.lo[x], tree.hi[x]),
                     lambda x: int(tree.sizes[x]), tree.root)


def _linear_cost(v):
    """The same measure over lbvh.radix_tree with exact boxes; a node is its range (first, last) of ordered positions."""
    codes = lbvh.morton_codes(v)
    order = np.lexsort((np.arange(len(v)), codes))
    first, last, split = lbvh.radix_tree(codes[order])
    lo, hi = ploc.boxes(v[order])
    inner = {(int(a), int(b)): int(s) for a, b, s in zip(first, last, split)}

    def children(node):
        s = inner[node]
        return (node[0], s), (s + 1, node[1])
    return _cut_cost(children, lambda x: (lo[x[0]:x[1] + 1].min(axis=0), hi[x[0]:x[1] + 1].max(axis=0)),
                     lambda x: x[1] - x[0] + 1, (0, len(v) - 1))


def test_the_cost_condition():
    for name, bound in (("soup", 0.85), ("spread", 0.85), ("identical70", 1.0), ("point", 1.0)):
        got, linear = _ploc_cost(SETS[name], 16), _linear_cost(SETS[name])
        print("%s: tree cost PLOC radius 16 %.4f, linear %.4f, ratio %.3f" % (name, got, linear, got / linear))
        assert got <= bound * linear, name


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    """tests/ploc_rule_main.cpp: the functions the kernels call (pt_bvh_ploc_rule.hpp, pt_bvh_rule.hpp), built for the host
    without contraction, under AddressSanitizer + UBSan."""
    gxx = shutil.which("g++")
    assert gxx, "the host C++ compiler (g++) is needed"
    exe = str(tmp_path_factory.mktemp("ploc_rule") / "ploc_rule")
    subprocess.check_call([
        gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "prosper_amd", "csrc"),
        os.path.join(ROOT, "tests", "ploc_rule_main.cpp"), "-o", exe])
    return exe


def _check_rule_program(rule_program, tmp_path, v, want, leaf, radius):
    flat = np.zeros((len(v), 12), np.uint32)
    flat.reshape(-1, 3, 4)[:, :, :3] = v.view(np.uint32)
    flat[:, 3] = 7  # (the words between the vertices are not coordinates)
    src, dst = str(tmp_path / "triangles.bin"), str(tmp_path / "tree.bin")
    flat.tofile(src)
    out = subprocess.run([rule_program, src, str(leaf), str(radius), dst], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    text = out.stdout + out.stderr
    assert out.returncode == 0 and "ploc rule ok" in text and "runtime error" not in text, text[-3000:]
    words = np.fromfile(dst, np.uint32)
    n, count, bound, rounds = (int(x) for x in words[:4])
    assert n == len(v) and count == len(want.child) and bound == want.stack_bound and rounds == want.rounds
    at = 4
    assert np.array_equal(words[at:at + 2 * n].view(np.uint64), want.codes)
    at += 2 * n
    assert np.array_equal(words[at:at + n], want.permutation)
    at += n
    nodes = words[at:].reshape(count, 5)
    assert np.array_equal(nodes[:, :4].view(np.int32), want.child) and np.array_equal(nodes[:, 4], want.reserved)


@pytest.mark.parametrize("leaf,radius", [(1, 16), (4, 16), (1, 1), (4, 32)])
@pytest.mark.parametrize("name", ["soup", "identical70", "spread", "n257", "t_plus_1", "n2", "n0"])
def test_the_kernels_arithmetic_meets_the_statement_on_a_cpu(rule_program, built, tmp_path, name, leaf, radius):
    _check_rule_program(rule_program, tmp_path, SETS[name], built[(name, leaf, radius)], leaf, radius)


# ---- the nested comb (ploc_sets.nested_comb): trees on the traversal's stack limit and beyond it ----
HUGE = 1 << 20
COMB_RADII = (1, 8, 32)


@pytest.fixture(scope="module")
def combs():
    """The statement over every comb with no limit on the stack bound: what the device computes before it decides."""
    return {(n, leaf, radius): ploc.build(ploc_sets.nested_comb(n), leaf_size=leaf, radius=radius, max_stack_bound=HUGE)
            for n in ploc_sets.COMB_SIZES for leaf in LEAF_SIZES for radius in COMB_RADII}


def test_the_nested_comb_is_exact_and_nested():
    for n in ploc_sets.COMB_SIZES:
        v = ploc_sets.nested_comb(n)
        s = np.exp2(np.arange(n, dtype=np.float64) - n // 2)
        want = np.zeros((n, 3, 3))
        want[:, 0], want[:, 1], want[:, 2] = (np.stack([-s, 0 * s, s / 16], 1), np.stack([s, 0 * s + 0.0625, s / 16], 1),
                                              np.stack([0 * s, 0 * s + 0.0625, s / 16], 1))
        assert v.dtype == np.float32 and np.array_equal(v.astype(np.float64), want)  # every value is exact in fp32
        lo, hi = ploc.boxes(v)
        assert (lo[1:, :2] <= lo[:-1, :2]).all() and (hi[1:, :2] >= hi[:-1, :2]).all()  # boxes nest in x and y
        assert (lo[:, 2] == hi[:, 2]).all() and (np.diff(lo[:, 2]) > 0).all()  # one plane each, all different


@pytest.mark.parametrize("leaf", LEAF_SIZES)
@pytest.mark.parametrize("n", ploc_sets.COMB_SIZES)
def test_the_nested_comb_reaches_the_stack_limit_one_triangle_apart(combs, n, leaf):
    v = ploc_sets.nested_comb(n)
    bounds = set()
    for radius in COMB_RADII:
        tree = combs[(n, leaf, radius)]
        assert tree.stack_bound == lbvh.recursive_stack_bound(tree.child, tree.reserved)
        assert tree.rounds == n - 1  # a comb: one merge a round
        bounds.add(tree.stack_bound)
        # under the default limit the statement refuses exactly the trees beyond it
        if tree.stack_bound > lbvh.MAX_STACK_BOUND:
            with pytest.raises(lbvh.Refused):
                ploc.build(v, leaf_size=leaf, radius=radius)
        else:
            for x, y in zip(ploc.build(v, leaf_size=leaf, radius=radius), tree):
                assert np.array_equal(x, y)
    assert len(bounds) == 1  # (the search radius does not matter: the nearest neighbour is the next position)
    bound = bounds.pop()
    print("nested_comb(%d), leaf %d: PLOC stack bound %d (%s), linear %d" % (
        n, leaf, bound, "refused" if bound > lbvh.MAX_STACK_BOUND else "accepted", lbvh.build(v, leaf_size=leaf).stack_bound))
    if leaf == 1:
        assert bound == n
    # the linear method's tree over the same set is nowhere near the limit (lbvh.build raises Refused beyond it)
    assert lbvh.build(v, leaf_size=leaf).stack_bound <= lbvh.MAX_STACK_BOUND


def test_the_nested_comb_sits_on_the_limit_or_is_refused(combs):
    """The facts tests/test_gpu_hierarchy_refusal.py leans on, with the default radius: 96 triangles at leaf 1 and 97 at
    leaf 2 sit exactly on the limit; 97 at leaf 1 and 101 at every leaf size are beyond it."""
    bound = lambda n, leaf: combs[(n, leaf, ploc.DEFAULT_RADIUS)].stack_bound
    assert lbvh.MAX_STACK_BOUND == 96 and ploc.DEFAULT_RADIUS in COMB_RADII
    assert bound(96, 1) == 96 and bound(97, 2) == 96
    assert bound(97, 1) == 97
    assert all(bound(101, leaf) > 96 for leaf in LEAF_SIZES)


@pytest.mark.parametrize("leaf", [1, ploc.DEFAULT_LEAF_SIZE])
@pytest.mark.parametrize("n", ploc_sets.COMB_SIZES)
def test_the_kernels_arithmetic_meets_the_statement_on_the_nested_comb(rule_program, combs, tmp_path, n, leaf):
    """The program computes the stack bound and does not decide on it: compared with the statement without a limit."""
    radius = ploc.DEFAULT_RADIUS
    _check_rule_program(rule_program, tmp_path, ploc_sets.nested_comb(n), combs[(n, leaf, radius)], leaf, radius)
