"""The hierarchy built on the GPU (prosper_pt_build_hierarchy_gpu) against its NumPy statement
(prosper_amd/lbvh.py) and against the hit contract: any valid tree gives the host tree's image, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import lbvh_sets
from conftest import default_pc, same_bits
from prosper_amd import capi, gltf, lbvh, scenes, structs as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = lbvh_sets.sets()
W = H = 48


def _sponza_small():
    return scenes.sponza_class(lights=True, foliage=True, texture_size=64, sky_size=32, detail=0.25)


SCENES = {
    "cornell": lambda: scenes.cornell(),
    "tiny_gltf": lambda: gltf.load_gltf(os.path.join(HERE, "golden", "tiny_scene.gltf")),
    "sponza_small": _sponza_small,
    "alpha_wall": scenes.alpha_wall,
}


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            made[name] = SCENES[name]() if name in SCENES else lbvh_sets.world_of(SETS[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def own_ctx():
    """A context of this module's own: the builder selection must not leak into the session's."""
    ctx = capi.Context(device=0)
    yield ctx
    ctx.close()


@pytest.fixture
def ctx(own_ctx):
    own_ctx.set_hierarchy_builder(S.BUILDER_HOST)
    yield own_ctx
    own_ctx.set_hierarchy_builder(S.BUILDER_HOST)


def _image(ctx, oracle, world, frames=2, draw="Default"):
    c = world.camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], W, H)
    ctx.render(default_pc(S, fl, max_bounces=4, ibl=world.skybox is not None, draw_type=S.DrawType[draw]), cam, W, H, frames=frames)
    return ctx.read_hdr()


def _images(ctx, oracle, world):
    """All bounces, and the primitive ids the camera rays hit (whatever the lighting)."""
    return np.stack([_image(ctx, oracle, world), _image(ctx, oracle, world, draw="PrimitiveID")])


def _tree_words(nodes):
    return nodes[:, 16:20].view(np.int32), nodes[:, 3]


def _check_against_statement(ctx, leaf):
    flat, perm = ctx.read_hierarchy_arrays()
    want = lbvh.build(flat, leaf_size=leaf)
    nodes = ctx.read_nodes()
    child, reserved = _tree_words(nodes)
    assert np.array_equal(perm, want.permutation)
    assert np.array_equal(reserved, want.reserved) and np.array_equal(child, want.child)
    info, stats, state = ctx.hierarchy_build_info(), ctx.scene_stats(), ctx.hierarchy_state()
    assert info.builder == S.BUILDER_GPU and info.leafSize == leaf
    assert info.nodeCount == stats.nodeCount == state.nodeCount == len(want.child)
    assert info.levels == state.levels == want.levels and info.depths == want.depths
    assert info.stackBound == stats.maxDepth == want.stack_bound
    stage_ms = list(info.stageMs)
    assert all(ms >= 0.0 for ms in stage_ms) and abs(info.totalMs - sum(stage_ms)) <= 1e-3 * max(1.0, info.totalMs) and info.totalMs > 0.0
    return flat, perm, nodes, want


def _check_containment(flat, perm, nodes, tree):
    """Every leaf child's box contains its triangles; every inner child's box contains every triangle below that child,
    that is the exact boxes of the child's own children - what the traversal needs of a stored box.  (The STORED boxes of
    the child's children: _stored_boxes_sticking_out.)"""
    lo, hi = lbvh.decode_boxes(nodes)
    v = lbvh.vertices(flat)[perm].astype(np.float64)  # leaf order
    below_lo, below_hi = np.zeros((len(nodes), 3)), np.zeros((len(nodes), 3))
    for i in range(len(nodes) - 1, -1, -1):  # children are numbered after their parent
        k = int(tree.reserved[i])
        exact_lo, exact_hi = np.full((k, 3), np.inf), np.full((k, 3), -np.inf)
        for c in range(k):
            ref = int(tree.child[i, c])
            if ref < 0:
                first, count = (~ref) >> 3, ((~ref) & 7) + 1
                inside = v[first:first + count].reshape(-1, 3)
                exact_lo[c], exact_hi[c] = inside.min(axis=0), inside.max(axis=0)
            else:
                exact_lo[c], exact_hi[c] = below_lo[ref], below_hi[ref]
        assert (exact_lo >= lo[i, :k]).all() and (exact_hi <= hi[i, :k]).all(), i
        below_lo[i], below_hi[i] = exact_lo.min(axis=0), exact_hi.max(axis=0)


def _stored_boxes_sticking_out(nodes):
    """(node, slot) pairs whose stored box does not contain the stored boxes of that child's own children, and the
    largest excess as a fraction of the containing box's largest side."""
    lo, hi = lbvh.decode_boxes(nodes)
    child, reserved = _tree_words(nodes)
    out, worst = 0, 0.0
    for i in range(len(nodes)):
        for c in range(int(reserved[i])):
            ref = int(child[i, c])
            if ref < 0:
                continue
            k = int(reserved[ref])
            excess = max(float((lo[i, c] - lo[ref, :k]).max()), float((hi[ref, :k] - hi[i, c]).max()))
            if excess > 0.0:
                out += 1
                worst = max(worst, excess / float((hi[i, c] - lo[i, c]).max()))
    return out, worst


CASES = [(name, leaf) for name in sorted(SETS) if name != "n0" for leaf in (1, 4)] + \
        [(name, leaf) for name in ("cornell", "tiny_gltf") for leaf in (2, 4)] + [("sponza_small", 4)]


@pytest.mark.parametrize("name,leaf", CASES)
def test_gpu_tree_equals_the_statement_and_its_boxes_contain(ctx, worlds, name, leaf):
    capi.debug(leafSize=leaf)
    ctx.upload_scene(worlds(name))
    assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST
    before = ctx.hierarchy_state()
    ctx.build_hierarchy_gpu()
    after = ctx.hierarchy_state()
    assert after.rebuilds == before.rebuilds + 1 and after.costRatio == 1.0 and after.geometryInstalls == before.geometryInstalls
    assert ctx.scene_stats().bvhBuildSeconds > 0.0
    flat, perm, nodes, want = _check_against_statement(ctx, leaf)
    assert len(flat) == worlds(name).triangle_count()
    _check_containment(flat, perm, nodes, want)
    assert _stored_boxes_sticking_out(nodes)[0] == 0


def test_default_leaf_size_is_the_statements(ctx, worlds):
    ctx.upload_scene(worlds("n257"))
    ctx.build_hierarchy_gpu()
    _check_against_statement(ctx, lbvh.DEFAULT_LEAF_SIZE)


@pytest.mark.parametrize("name", ["alpha_wall", "sponza_small", "soup"])
def test_hit_contract_gpu_tree_gives_the_host_trees_image(ctx, oracle, worlds, name):
    """MASK and BLEND triangles included (alpha_wall, the foliage of sponza_small): the any-hit records follow the
    triangles through the new leaf order."""
    world = worlds(name)
    ctx.upload_scene(world)
    host = _images(ctx, oracle, world)
    assert np.isfinite(host).all() and len(np.unique(host[1].reshape(-1, 4), axis=0)) > 2  # primitives are in view
    for leaf in (1, 4):
        capi.debug(leafSize=leaf)
        ctx.build_hierarchy_gpu()
        assert same_bits(_images(ctx, oracle, world), host).all(), leaf
    fresh = capi.Context(device=0)
    try:
        fresh.upload_scene(world)
        fresh.build_hierarchy_gpu()
        assert fresh.hierarchy_build_info().builder == S.BUILDER_GPU
        assert same_bits(_images(fresh, oracle, world), host).all()
    finally:
        fresh.close()


def _moved(k):
    from prosper_amd.world import rotate_y, translate
    world = scenes.sponza_class(lights=(4, 4), foliage=True, texture_size=64, sky_size=32, detail=0.25)
    for i, delta in ((3, translate((0.4 * k, 0.25 * k, -0.3 * k)) @ rotate_y(0.6 * k)), (7, translate((-0.2 * k, 0.0, 0.5 * k)))):
        model, m = world.model_instances[i]
        world.model_instances[i] = (model, delta @ m)
    return world


def test_refit_after_a_gpu_build_equals_a_fresh_upload(ctx, oracle):
    poses = [_moved(k) for k in range(3)]
    ctx.upload_scene(poses[0])
    ctx.build_hierarchy_gpu()
    nodes = ctx.read_nodes()
    fresh = capi.Context(device=0)
    try:
        for world in poses[1:] + poses[:1]:
            ctx.update_transforms(world)
            got = _image(ctx, oracle, world)
            fresh.upload_scene(world)
            assert same_bits(got, _image(fresh, oracle, world)).all()
        state = ctx.hierarchy_state()
        assert state.refits == 3 and ctx.hierarchy_build_info().builder == S.BUILDER_GPU
        # the refits kept the GPU tree's topology and, back in the first pose, wrote its bytes again
        assert np.array_equal(ctx.read_nodes(), nodes)
    finally:
        fresh.close()


def test_host_rebuild_after_a_gpu_build_splits_every_instance_again(ctx, oracle):
    still, moved = _moved(0), _moved(1)
    ctx.upload_scene(still)
    nodes_at_upload = ctx.read_nodes()
    first = _image(ctx, oracle, still)
    ctx.build_hierarchy_gpu()
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    ctx.rebuild_hierarchy()  # HOST mode: the host builder, with no subtree to keep
    info, state = ctx.hierarchy_build_info(), ctx.hierarchy_state()
    assert info.builder == S.BUILDER_HOST and info.depths == 0 and info.totalMs == 0.0
    assert state.rebuilds == 2 and abs(state.costRatio - 1.0) < 1e-6
    # the same state built the same way: the node array of the upload (the identity the rebuild test asserts for uploads)
    assert np.array_equal(ctx.read_nodes(), nodes_at_upload)
    # ... and after a move, a GPU build and a host rebuild: a fresh upload's image and node array
    ctx.update_transforms(moved)
    ctx.build_hierarchy_gpu()
    ctx.rebuild_hierarchy()
    got = _image(ctx, oracle, moved)
    fresh = capi.Context(device=0)
    try:
        fresh.upload_scene(moved)
        assert same_bits(got, _image(fresh, oracle, moved)).all()
        assert np.array_equal(ctx.read_nodes(), fresh.read_nodes())
    finally:
        fresh.close()
    # the kept subtrees are the host's own again: a rebuild after a move re-splits only what moved, same image
    ctx.update_transforms(still)
    ctx.rebuild_hierarchy()
    assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST
    assert same_bits(_image(ctx, oracle, still), first).all()


def test_gpu_mode_routes_the_rebuild_and_the_drift_trigger(ctx, oracle):
    """The scenario of test_drifting_instances_trigger_the_rebuild_with_frames_in_flight with the builder set to GPU: an
    update rebuilds by itself, on the device and inside the call (no background geometry is installed), and every frame
    shows its own pose."""
    from prosper_amd.world import translate

    def pose(k):
        world = scenes.sponza_class(lights=(4, 4), texture_size=64, sky_size=32, detail=0.25)
        for i in (3, 5, 7):
            model, m = world.model_instances[i]
            world.model_instances[i] = (model, translate((1.5 * k, 0.2 * k, 0.4 * k)) @ m)
        return world
    poses = [pose(k) for k in range(14)]
    c = poses[0].camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], W, H)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    ctx.upload_scene(poses[0])
    ctx.set_hierarchy_builder(S.BUILDER_GPU)
    assert ctx.hierarchy_build_info().selectedBuilder == S.BUILDER_GPU and ctx.hierarchy_build_info().builder == S.BUILDER_HOST
    ctx.rebuild_hierarchy()  # GPU mode: the GPU build
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    before = ctx.hierarchy_state()
    images = []
    for world in poses[1:]:
        ctx.update_transforms(world)
        ctx.render(pc, cam, W, H, frames=4, flags=S.RENDER_PIPELINED)
        images.append(ctx.read_hdr())
    after = ctx.hierarchy_state()
    assert after.rebuilds > before.rebuilds, "refits %d, rebuilds %d, measure x%.3f" % (after.refits, after.rebuilds, after.costRatio)
    assert after.geometryInstalls == 0 and after.geometryBuildRunning == 0
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    fresh = capi.Context(device=0)
    try:
        for world, got in zip(poses[1:], images):
            fresh.upload_scene(world)
            fresh.render(pc, cam, W, H, frames=4)
            assert same_bits(got, fresh.read_hdr()).all()
    finally:
        fresh.close()


def test_two_gpu_builds_give_identical_bytes(ctx, worlds):
    for name in ("soup", "sponza_small"):
        ctx.upload_scene(worlds(name))
        ctx.build_hierarchy_gpu()
        nodes, (_, perm) = ctx.read_nodes(), ctx.read_hierarchy_arrays()
        ctx.build_hierarchy_gpu()
        assert np.array_equal(ctx.read_nodes(), nodes) and np.array_equal(ctx.read_hierarchy_arrays()[1], perm)


def test_empty_scene_does_what_the_host_path_does(ctx, oracle, worlds):
    world = worlds("n0")
    ctx.upload_scene(world)
    nodes = ctx.read_nodes()
    before = ctx.hierarchy_state()
    ctx.build_hierarchy_gpu()
    after = ctx.hierarchy_state()
    assert after.rebuilds == before.rebuilds + 1 and after.nodeCount == 1
    assert np.array_equal(ctx.read_nodes(), nodes) and nodes[0, 3] == 0
    flat, perm = ctx.read_hierarchy_arrays()
    assert len(flat) == 0 and len(perm) == 0
    assert np.isfinite(_image(ctx, oracle, world)).all()


def test_refusals(ctx, worlds):
    lib = capi.lib()
    assert lib.prosper_pt_build_hierarchy_gpu(None) == -1 and b"null" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_set_hierarchy_builder(None, 0) == -1
    assert lib.prosper_pt_get_hierarchy_build_info(None, None) == -1
    assert lib.prosper_pt_debug_read_hierarchy_arrays(None, None, 0, None, 0) == -1
    bare = capi.Context(device=0)
    try:
        info = S.HierarchyBuildInfo()
        buf = np.zeros(64, np.uint32)
        assert lib.prosper_pt_build_hierarchy_gpu(bare._h) == -4 and b"no scene" in lib.prosper_pt_last_error()
        assert lib.prosper_pt_get_hierarchy_build_info(bare._h, C.byref(info)) == -4
        assert lib.prosper_pt_debug_read_hierarchy_arrays(bare._h, buf.ctypes.data, buf.nbytes, buf.ctypes.data, buf.nbytes) == -4
        bare.set_hierarchy_builder(S.BUILDER_GPU)  # (a selection needs no scene)
        assert lib.prosper_pt_set_hierarchy_builder(bare._h, 2) == -1 and b"unknown builder" in lib.prosper_pt_last_error()
    finally:
        bare.close()
    ctx.upload_scene(worlds("n65"))
    ctx.build_hierarchy_gpu()
    nodes = ctx.read_nodes()
    with pytest.raises(capi.ProsperPtError) as e:
        ctx.set_hierarchy_builder(7)
    assert e.value.code == -1
    assert ctx.hierarchy_build_info().selectedBuilder == S.BUILDER_HOST
    tris, perm = np.zeros((65, 12), np.uint32), np.zeros(65, np.uint32)
    assert lib.prosper_pt_debug_read_hierarchy_arrays(ctx._h, tris.ctypes.data, tris.nbytes - 4, perm.ctypes.data, perm.nbytes) == -1
    assert b"too small" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_debug_read_hierarchy_arrays(ctx._h, tris.ctypes.data, tris.nbytes, perm.ctypes.data, perm.nbytes - 4) == -1
    assert not tris.any() and not perm.any()
    assert np.array_equal(ctx.read_nodes(), nodes)


def test_stored_child_boxes_nest(ctx, oracle, worlds):
    """Every inner child's DECODED box contains the decoded boxes of that child's own children - after a GPU build and
    after every refit of its tree.  The encoder alone does not give this (bvh_encode.hpp pads every stored box from the
    exact bounds below it and rounds outward on its own node's binary16 grid, so a grandchild's box can stick out of the
    child's by a fraction of a grid step: the host builder's trees, which are left as they are, show it); behind the
    refit of a GPU-built tree lbvh_nest_boxes_kernel grows the boxes that need it, lowest nodes first."""
    ctx.upload_scene(worlds("soup"))
    host = _stored_boxes_sticking_out(ctx.read_nodes())
    ctx.build_hierarchy_gpu()
    gpu = _stored_boxes_sticking_out(ctx.read_nodes())
    print("stored boxes sticking out of their parent's (pairs, worst excess / side): host tree %d %.3g, GPU tree %d %.3g" % (host + gpu))
    assert gpu[0] == 0
    still, moved = _moved(0), _moved(1)
    ctx.upload_scene(still)
    ctx.build_hierarchy_gpu()
    assert _stored_boxes_sticking_out(ctx.read_nodes())[0] == 0
    ctx.update_transforms(moved)
    _image(ctx, oracle, moved)  # (the refit runs at the head of the render)
    flat, perm = ctx.read_hierarchy_arrays()
    nodes = ctx.read_nodes()
    assert _stored_boxes_sticking_out(nodes)[0] == 0
    _check_containment(flat, perm, nodes, lbvh.build(ctx.read_hierarchy_arrays()[0][:0], leaf_size=1)._replace(
        child=_tree_words(nodes)[0], reserved=_tree_words(nodes)[1]))
