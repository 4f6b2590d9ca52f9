"""The PLOC method of the GPU hierarchy build (prosper_pt_set_gpu_hierarchy_method) against its NumPy
statement (prosper_amd/ploc.py) and against the hit contract: any valid tree gives the host tree's image, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import ploc_sets
import test_gpu_hierarchy as linear
from conftest import same_bits
from prosper_amd import capi, lbvh, ploc, scenes, structs as S

pytestmark = pytest.mark.gpu

SETS = ploc_sets.sets()
T = ploc_sets.T
PLOC, LINEAR = S.GPU_HIERARCHY_PLOC, S.GPU_HIERARCHY_LINEAR


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            made[name] = linear.SCENES[name]() if name in linear.SCENES else ploc_sets.lbvh_sets.world_of(SETS[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def own_ctx():
    """A context of this module's own: neither selection must leak into the session's."""
    ctx = capi.Context(device=0)
    yield ctx
    ctx.close()


@pytest.fixture
def ctx(own_ctx):
    own_ctx.set_hierarchy_builder(S.BUILDER_HOST)
    own_ctx.set_gpu_hierarchy_method(LINEAR)
    capi.debug(leafSize=None)
    yield own_ctx
    own_ctx.set_hierarchy_builder(S.BUILDER_HOST)
    own_ctx.set_gpu_hierarchy_method(LINEAR)
    capi.debug(leafSize=None)


def _check_against_statement(ctx, leaf, radius):
    flat, perm = ctx.read_hierarchy_arrays()
    want = ploc.build(flat, leaf_size=leaf, radius=radius)
    nodes = ctx.read_nodes()
    child, reserved = linear._tree_words(nodes)
    assert np.array_equal(perm, want.permutation)
    assert np.array_equal(reserved, want.reserved) and np.array_equal(child, want.child)
    info, stats, state, method = ctx.hierarchy_build_info(), ctx.scene_stats(), ctx.hierarchy_state(), ctx.gpu_hierarchy_method_info()
    assert info.builder == S.BUILDER_GPU and info.leafSize == leaf
    assert info.nodeCount == stats.nodeCount == state.nodeCount == len(want.child)
    assert info.levels == state.levels == want.levels and info.depths == want.depths
    assert info.stackBound == stats.maxDepth == want.stack_bound
    assert method.method == method.selectedMethod == PLOC and method.radius == method.selectedRadius == radius
    assert method.rounds == want.rounds
    # the rounds that start with at most T clusters run in the one-workgroup launch
    assert method.finishRounds == sum(1 for m in want.round_counts if m <= T)
    stage_ms = list(info.stageMs)
    assert all(ms >= 0.0 for ms in stage_ms) and abs(info.totalMs - sum(stage_ms)) <= 1e-3 * max(1.0, info.totalMs) and info.totalMs > 0.0
    return flat, perm, nodes, want


CASES = [(name, leaf, 16) for name in sorted(SETS) if name != "n0" for leaf in (1, 4)] + \
        [(name, leaf, radius) for name in ("n257", "soup", "t", "t_plus_1", "two_t_plus_1") for leaf in (1, 4) for radius in (1, 32)] + \
        [(name, 2, 16) for name in ("cornell", "tiny_gltf", "sponza_small")]


@pytest.mark.parametrize("name,leaf,radius", CASES)
def test_ploc_tree_equals_the_statement_and_its_boxes_contain(ctx, worlds, name, leaf, radius):
    capi.debug(leafSize=leaf)
    ctx.upload_scene(worlds(name))
    ctx.set_gpu_hierarchy_method(PLOC, radius)
    before = ctx.hierarchy_state()
    assert ctx.gpu_hierarchy_method_info().method == LINEAR and ctx.gpu_hierarchy_method_info().rounds == 0  # (nothing built yet)
    ctx.build_hierarchy_gpu()
    after = ctx.hierarchy_state()
    assert after.rebuilds == before.rebuilds + 1 and after.costRatio == 1.0
    flat, perm, nodes, want = _check_against_statement(ctx, leaf, radius)
    assert len(flat) == worlds(name).triangle_count()
    linear._check_containment(flat, perm, nodes, want)
    assert linear._stored_boxes_sticking_out(nodes)[0] == 0


def test_the_threshold_sets_split_their_rounds_as_meant(ctx, worlds):
    """T triangles: every round in the one-workgroup launch; T + 1: exactly one before it; 2 T + 1: several."""
    outside = {}
    for name in ("t", "t_plus_1", "two_t_plus_1"):
        ctx.upload_scene(worlds(name))
        ctx.set_gpu_hierarchy_method(PLOC, 16)
        ctx.build_hierarchy_gpu()
        info = ctx.gpu_hierarchy_method_info()
        outside[name] = info.rounds - info.finishRounds
    assert outside["t"] == 0 and outside["t_plus_1"] == 1 and outside["two_t_plus_1"] >= 2


def test_default_radius_and_leaf_size_are_the_statements(ctx, worlds):
    ctx.upload_scene(worlds("n257"))
    ctx.set_gpu_hierarchy_method(PLOC)
    assert ctx.gpu_hierarchy_method_info().selectedRadius == ploc.DEFAULT_RADIUS
    ctx.build_hierarchy_gpu()
    _check_against_statement(ctx, ploc.DEFAULT_LEAF_SIZE, ploc.DEFAULT_RADIUS)


def test_nothing_selected_is_the_linear_method(ctx, worlds):
    ctx.upload_scene(worlds("n257"))
    info = ctx.gpu_hierarchy_method_info()
    assert info.selectedMethod == LINEAR and info.method == LINEAR and info.rounds == 0
    ctx.build_hierarchy_gpu()
    linear._check_against_statement(ctx, lbvh.DEFAULT_LEAF_SIZE)
    info = ctx.gpu_hierarchy_method_info()
    assert info.method == LINEAR and info.radius == 0 and info.rounds == 0 and info.finishRounds == 0


@pytest.mark.parametrize("name", ["alpha_wall", "sponza_small", "soup"])
def test_hit_contract_ploc_tree_gives_the_host_trees_image(ctx, oracle, worlds, name):
    world = worlds(name)
    ctx.upload_scene(world)
    host = linear._images(ctx, oracle, world)
    assert np.isfinite(host).all() and len(np.unique(host[1].reshape(-1, 4), axis=0)) > 2  # primitives are in view
    for leaf, radius in ((1, 16), (4, 8), (2, 32)):
        capi.debug(leafSize=leaf)
        ctx.set_gpu_hierarchy_method(PLOC, radius)
        ctx.build_hierarchy_gpu()
        assert ctx.gpu_hierarchy_method_info().rounds > 0
        assert same_bits(linear._images(ctx, oracle, world), host).all(), (leaf, radius)


def test_refit_after_a_ploc_build_equals_a_fresh_upload_and_its_boxes_nest(ctx, oracle):
    poses = [linear._moved(k) for k in range(3)]
    ctx.upload_scene(poses[0])
    ctx.set_gpu_hierarchy_method(PLOC, 16)
    ctx.build_hierarchy_gpu()
    nodes = ctx.read_nodes()
    assert linear._stored_boxes_sticking_out(nodes)[0] == 0
    fresh = capi.Context(device=0)
    try:
        for world in poses[1:] + poses[:1]:
            ctx.update_transforms(world)
            got = linear._image(ctx, oracle, world)
            fresh.upload_scene(world)
            assert same_bits(got, linear._image(fresh, oracle, world)).all()
            # after a refit of moved instances: the stored boxes contain what lies below them, and nest
            flat, perm = ctx.read_hierarchy_arrays()
            moved = ctx.read_nodes()
            assert linear._stored_boxes_sticking_out(moved)[0] == 0
            child, reserved = linear._tree_words(moved)
            linear._check_containment(flat, perm, moved, lbvh.build(flat[:0], leaf_size=1)._replace(child=child, reserved=reserved))
        assert ctx.hierarchy_state().refits == 3 and ctx.gpu_hierarchy_method_info().method == PLOC
        # the refits kept the PLOC tree's topology and, back in the first pose, wrote its bytes again
        assert np.array_equal(ctx.read_nodes(), nodes)
    finally:
        fresh.close()


def test_repeatability(ctx, worlds):
    for name in ("soup", "sponza_small"):
        ctx.upload_scene(worlds(name))
        at_upload = ctx.read_nodes()
        ctx.build_hierarchy_gpu()
        first_linear, (_, linear_perm) = ctx.read_nodes(), ctx.read_hierarchy_arrays()
        ctx.set_gpu_hierarchy_method(PLOC, 16)
        ctx.build_hierarchy_gpu()
        nodes, (_, perm) = ctx.read_nodes(), ctx.read_hierarchy_arrays()
        assert not np.array_equal(perm, linear_perm)
        ctx.build_hierarchy_gpu()
        assert np.array_equal(ctx.read_nodes(), nodes) and np.array_equal(ctx.read_hierarchy_arrays()[1], perm)
        ctx.set_gpu_hierarchy_method(LINEAR)
        ctx.build_hierarchy_gpu()
        assert np.array_equal(ctx.read_nodes(), first_linear) and np.array_equal(ctx.read_hierarchy_arrays()[1], linear_perm)
        # a host rebuild after a PLOC build: a fresh upload's node array
        ctx.set_gpu_hierarchy_method(PLOC, 16)
        ctx.build_hierarchy_gpu()
        ctx.rebuild_hierarchy()
        assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST and ctx.gpu_hierarchy_method_info().rounds == 0
        assert np.array_equal(ctx.read_nodes(), at_upload)
        ctx.set_gpu_hierarchy_method(LINEAR)


def test_gpu_mode_routes_the_rebuild_and_the_drift_trigger_to_the_selected_method(ctx, oracle):
    from conftest import default_pc
    from prosper_amd.world import translate

    def pose(k):
        world = scenes.sponza_class(lights=(4, 4), texture_size=64, sky_size=32, detail=0.25)
        for i in (3, 5, 7):
            model, m = world.model_instances[i]
            world.model_instances[i] = (model, translate((1.5 * k, 0.2 * k, 0.4 * k)) @ m)
        return world
    poses = [pose(k) for k in range(14)]
    c = poses[0].camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], linear.W, linear.H)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    ctx.upload_scene(poses[0])
    ctx.set_hierarchy_builder(S.BUILDER_GPU)
    ctx.set_gpu_hierarchy_method(PLOC, 8)
    ctx.rebuild_hierarchy()  # GPU mode: the GPU build, by the selected method
    info = ctx.gpu_hierarchy_method_info()
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU and info.method == PLOC and info.radius == 8 and info.rounds > 0
    before = ctx.hierarchy_state()
    images = []
    for world in poses[1:]:
        ctx.update_transforms(world)
        ctx.render(pc, cam, linear.W, linear.H, frames=4, flags=S.RENDER_PIPELINED)
        images.append(ctx.read_hdr())
    after = ctx.hierarchy_state()
    assert after.rebuilds > before.rebuilds, "refits %d, rebuilds %d, measure x%.3f" % (after.refits, after.rebuilds, after.costRatio)
    info = ctx.gpu_hierarchy_method_info()
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU and info.method == PLOC and info.rounds > 0
    fresh = capi.Context(device=0)
    try:
        for world, got in zip(poses[1:], images):
            fresh.upload_scene(world)
            fresh.render(pc, cam, linear.W, linear.H, frames=4)
            assert same_bits(got, fresh.read_hdr()).all()
    finally:
        fresh.close()


def test_empty_scene_does_what_the_host_path_does(ctx, oracle, worlds):
    world = worlds("n0")
    ctx.upload_scene(world)
    nodes = ctx.read_nodes()
    ctx.set_gpu_hierarchy_method(PLOC, 16)
    before = ctx.hierarchy_state()
    ctx.build_hierarchy_gpu()
    after = ctx.hierarchy_state()
    assert after.rebuilds == before.rebuilds + 1 and after.nodeCount == 1
    assert np.array_equal(ctx.read_nodes(), nodes) and nodes[0, 3] == 0
    info = ctx.gpu_hierarchy_method_info()
    assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST and info.method == LINEAR and info.rounds == 0
    assert np.isfinite(linear._image(ctx, oracle, world)).all()


def test_refusals(ctx, worlds):
    lib = capi.lib()
    info = S.GpuHierarchyMethodInfo()
    assert lib.prosper_pt_set_gpu_hierarchy_method(None, PLOC, 16) == -1 and b"null" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_get_gpu_hierarchy_method_info(None, C.byref(info)) == -1
    bare = capi.Context(device=0)
    try:
        assert lib.prosper_pt_get_gpu_hierarchy_method_info(bare._h, None) == -1 and b"null" in lib.prosper_pt_last_error()
        bare.set_gpu_hierarchy_method(PLOC, 32)  # (a selection needs no scene, and neither does reading it)
        for method, radius in ((2, 16), (PLOC, 33), (7, 0), (LINEAR, 0xFFFFFFFF)):
            assert lib.prosper_pt_set_gpu_hierarchy_method(bare._h, method, radius) == -1
            got = bare.gpu_hierarchy_method_info()
            assert got.selectedMethod == PLOC and got.selectedRadius == 32 and got.method == LINEAR and got.rounds == 0
        assert b"radius" in lib.prosper_pt_last_error()
        # the method is a property of the GPU builder, not a third builder
        assert lib.prosper_pt_set_hierarchy_builder(bare._h, 2) == -1
    finally:
        bare.close()
    ctx.upload_scene(worlds("n65"))
    ctx.set_gpu_hierarchy_method(PLOC, 4)
    ctx.build_hierarchy_gpu()
    nodes = ctx.read_nodes()
    with pytest.raises(capi.ProsperPtError) as e:
        ctx.set_gpu_hierarchy_method(PLOC, 33)
    assert e.value.code == -1
    got = ctx.gpu_hierarchy_method_info()
    assert got.selectedRadius == 4 and got.radius == 4 and np.array_equal(ctx.read_nodes(), nodes)
