"""The GPU builder's build sites (prosper_pt_set_gpu_hierarchy_sites): the scene's first tree, the worker
thread's generations and the drift re-split made on the device - against the NumPy statements (prosper_amd/lbvh.py,
ploc.py), against an upload followed by prosper_pt_build_hierarchy_gpu (the fused flatten launch writes the existing
kernels' bytes) and against the hit contract: any valid tree gives the host tree's image, bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest

import lbvh_sets
import test_gpu_hierarchy as linear
from conftest import default_pc, same_bits
from prosper_amd import capi, lbvh, ploc, scenes, structs as S
from prosper_amd.world import translate

pytestmark = pytest.mark.gpu

UPLOAD, MESH_UPDATES, DRIFT = S.GPU_BUILD_SITE_UPLOAD, S.GPU_BUILD_SITE_MESH_UPDATES, S.GPU_BUILD_SITE_DRIFT
PLOC, LINEAR = S.GPU_HIERARCHY_PLOC, S.GPU_HIERARCHY_LINEAR
SETS = lbvh_sets.sets()
# the borders of the fused launch's reduction - a wave is 64 triangles, a workgroup 256 - beside the sets' 64, 65 and 257
BORDERS = {"b%d" % n: n for n in (255, 256, 513)}


def _border_set(n):
    rng = np.random.default_rng(1000 + n)
    c = rng.uniform(-3.0, 3.0, (n, 1, 3)).astype(np.float32)
    v = c + rng.uniform(-0.125, 0.125, (n, 3, 3)).astype(np.float32)
    return v.astype(np.float16).astype(np.float32)  # (binary16 values: the scene holds exactly these triangles)


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            if name in linear.SCENES:
                made[name] = linear.SCENES[name]()
            elif name in BORDERS:
                made[name] = lbvh_sets.world_of(_border_set(BORDERS[name]))
            else:
                made[name] = lbvh_sets.world_of(SETS[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def own_ctx():
    """A context of this module's own: no selection must leak into the session's."""
    ctx = capi.Context(device=0)
    yield ctx
    ctx.close()


def _reset(ctx):
    ctx.set_gpu_hierarchy_sites(0)
    ctx.set_hierarchy_builder(S.BUILDER_HOST)
    ctx.set_gpu_hierarchy_method(LINEAR)
    ctx.set_debug()
    capi.debug(leafSize=None)


@pytest.fixture
def ctx(own_ctx):
    _reset(own_ctx)
    yield own_ctx
    _reset(own_ctx)


@pytest.fixture
def other():
    """A second context, with nothing selected."""
    c = capi.Context(device=0)
    yield c
    c.close()


def _sited_upload(ctx, world, sites=UPLOAD):
    ctx.set_gpu_hierarchy_sites(sites)
    ctx.upload_scene(world)


# ---- 1. upload equals the statement ----
CASES = [(name, leaf) for name in sorted(SETS) if name != "n0" for leaf in (1, 4)] + \
        [(name, leaf) for name in sorted(BORDERS) for leaf in (1, 4)] + \
        [(name, leaf) for name in ("cornell", "tiny_gltf") for leaf in (2, 4)] + [("sponza_small", 4)]


def _check_first_tree(ctx, world, flat, perm, nodes, want):
    assert len(flat) == world.triangle_count()
    linear._check_containment(flat, perm, nodes, want)
    assert linear._stored_boxes_sticking_out(nodes)[0] == 0
    state, stats = ctx.hierarchy_state(), ctx.scene_stats()
    assert state.rebuilds == 0 and state.costRatio == 1.0
    assert stats.bvhBuildSeconds > 0.0 and stats.buildSeconds >= stats.bvhBuildSeconds
    assert ctx.hierarchy_build_info().totalMs > 0.0


@pytest.mark.parametrize("name,leaf", CASES)
def test_sited_upload_equals_the_statement_and_its_boxes_contain(ctx, worlds, name, leaf):
    capi.debug(leafSize=leaf)
    _sited_upload(ctx, worlds(name))
    flat, perm, nodes, want = linear._check_against_statement(ctx, leaf)
    _check_first_tree(ctx, worlds(name), flat, perm, nodes, want)
    method = ctx.gpu_hierarchy_method_info()
    assert method.method == LINEAR and method.rounds == 0


@pytest.mark.parametrize("name", ["soup", "identical70", "n257"])
@pytest.mark.parametrize("radius", [1, 8])
def test_sited_upload_with_the_ploc_method_equals_its_statement(ctx, worlds, name, radius):
    leaf = ploc.DEFAULT_LEAF_SIZE
    ctx.set_gpu_hierarchy_method(PLOC, radius)
    _sited_upload(ctx, worlds(name))
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
    assert method.method == PLOC and method.radius == radius and method.rounds == want.rounds
    _check_first_tree(ctx, worlds(name), flat, perm, nodes, want)


# ---- 2. upload equals upload-then-build: the fused launch's triangles and bounds are the existing kernels' ----
@pytest.mark.parametrize("name", ["soup", "sponza_small", "alpha_wall"])
def test_sited_upload_equals_an_upload_followed_by_a_gpu_build(ctx, other, worlds, name):
    world = worlds(name)
    _sited_upload(ctx, world)
    other.upload_scene(world)
    assert other.hierarchy_build_info().builder == S.BUILDER_HOST
    other.build_hierarchy_gpu()
    flat, perm = ctx.read_hierarchy_arrays()
    flat2, perm2 = other.read_hierarchy_arrays()
    assert len(flat) == world.triangle_count() and np.array_equal(flat, flat2)
    assert np.array_equal(perm, perm2)
    assert np.array_equal(ctx.read_nodes(), other.read_nodes())
    a, b = ctx.hierarchy_build_info(), other.hierarchy_build_info()
    assert (a.builder, a.leafSize, a.nodeCount, a.levels, a.depths, a.stackBound) == (b.builder, b.leafSize, b.nodeCount, b.levels, b.depths, b.stackBound)


# ---- 3. the hit contract ----
def _oracle_image(oracle, world, **pc):
    c = world.camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], linear.W, linear.H)
    osc = oracle.OracleScene(world)
    want = None
    for f in (1, 2):
        want, _ = osc.render(default_pc(S, fl, frame_index=f, skip_history=(f == 1), **pc), cam, linear.W, linear.H, history=want)
    return want


@pytest.mark.parametrize("name", ["cornell", "tiny_gltf", "sponza_small", "alpha_wall"])
def test_hit_contract_sited_upload_gives_the_host_trees_image(ctx, other, oracle, worlds, name):
    """alpha_wall and the foliage of sponza_small: the any-hit records are the fused launch's."""
    world = worlds(name)
    other.upload_scene(world)
    host = linear._images(other, oracle, world)
    assert np.isfinite(host).all() and len(np.unique(host[1].reshape(-1, 4), axis=0)) > 2  # primitives are in view
    _sited_upload(ctx, world)
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    assert ctx.scene_stats().alphaTriangleCount == other.scene_stats().alphaTriangleCount
    assert same_bits(linear._images(ctx, oracle, world), host).all()
    if name == "cornell":
        assert same_bits(host[0], _oracle_image(oracle, world, max_bounces=4, ibl=world.skybox is not None)).all()


# ---- 4. what follows a sited upload ----
def test_refits_after_a_sited_upload_equal_fresh_uploads(ctx, other, oracle):
    poses = [linear._moved(k) for k in range(3)]
    _sited_upload(ctx, poses[0])
    nodes = ctx.read_nodes()
    for world in poses[1:] + poses[:1]:
        ctx.update_transforms(world)
        got = linear._image(ctx, oracle, world)
        other.upload_scene(world)
        assert same_bits(got, linear._image(other, oracle, world)).all()
    state = ctx.hierarchy_state()
    assert state.refits == 3 and state.rebuilds == 0 and ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    # the refits kept the GPU tree's topology and, back in the first pose, wrote its bytes again: nest pass included
    assert np.array_equal(ctx.read_nodes(), nodes)
    assert linear._stored_boxes_sticking_out(ctx.read_nodes())[0] == 0


def test_host_rebuild_after_a_sited_upload_gives_a_fresh_host_uploads_nodes(ctx, other, oracle):
    """No host copy of the triangles and no subtree exists after a sited upload: the host builder splits every instance
    as a fresh upload does."""
    world = linear._moved(1)
    _sited_upload(ctx, world)
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    ctx.rebuild_hierarchy()  # HOST mode
    info, state = ctx.hierarchy_build_info(), ctx.hierarchy_state()
    assert info.builder == S.BUILDER_HOST and info.depths == 0 and info.totalMs == 0.0
    assert state.rebuilds == 1 and abs(state.costRatio - 1.0) < 1e-6
    other.upload_scene(world)
    assert np.array_equal(ctx.read_nodes(), other.read_nodes())
    assert same_bits(linear._image(ctx, oracle, world), linear._image(other, oracle, world)).all()


def test_two_sited_uploads_give_identical_bytes(ctx, worlds):
    for name in ("soup", "sponza_small"):
        _sited_upload(ctx, worlds(name))
        nodes, (flat, perm) = ctx.read_nodes(), ctx.read_hierarchy_arrays()
        _sited_upload(ctx, worlds(name))
        again = ctx.read_hierarchy_arrays()
        assert np.array_equal(ctx.read_nodes(), nodes) and np.array_equal(again[0], flat) and np.array_equal(again[1], perm)


# ---- 5. empty and loading scenes take the host's path ----
def test_scenes_without_triangles_take_the_host_path(ctx, oracle, worlds):
    loading = scenes.sponza_class(texture_size=32, sky_size=16, detail=0.25).with_meshes_loaded([])
    for world in (worlds("n0"), loading):
        _sited_upload(ctx, world, UPLOAD | MESH_UPDATES | DRIFT)
        info = ctx.hierarchy_build_info()
        assert info.builder == S.BUILDER_HOST and info.nodeCount == 1 and ctx.scene_stats().triangleCount == 0
        assert len(ctx.read_nodes()) == 1
        assert np.isfinite(linear._images(ctx, oracle, world)).all()


# ---- 6. mesh adoption ----
def _moved(world, instance, offset):
    w = copy.copy(world)
    w._frozen = None
    w.model_instances = list(world.model_instances)
    model, m = w.model_instances[instance]
    w.model_instances[instance] = (model, translate(offset) @ m)
    return w


def test_meshes_stream_in_through_the_gpu_builder(ctx, other, oracle):
    """The scenario of test_mesh_adoption.test_meshes_stream_in_over_frames_in_flight with the first tree and every
    generation of the worker thread from the GPU builder."""
    full = scenes.sponza_class(texture_size=32, sky_size=16, detail=0.25)
    meshes = len(full.metadatas)
    order = list(range(meshes))
    steps = [0, 4, 9, 10, 18, 27, meshes]
    w, h = 240, 136
    c = full.camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    base = full
    _sited_upload(ctx, base.with_meshes_loaded([]), UPLOAD | MESH_UPDATES)
    assert ctx.scene_stats().triangleCount == 0 and ctx.hierarchy_build_info().builder == S.BUILDER_HOST
    states, got = [], []
    for k, loaded in enumerate(steps):
        if k == 3:
            base = _moved(base, 2, (0.4, 0.1, -0.3))
            ctx.update_transforms(base)
        if k == 5:
            base = _moved(base, 7, (-0.2, 0.0, 0.5))
            ctx.update_transforms(base)
        if k:
            ctx.update_meshes(base, order[steps[k - 1]:loaded])
        states.append(base.with_meshes_loaded(order[:loaded]))
        ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_PIPELINED)
        got.append(ctx.read_hdr())
    ctx.finish_mesh_updates()
    assert ctx.scene_stats().triangleCount == full.triangle_count()
    for k, state in enumerate(states):
        other.upload_scene(state)
        other.render(pc, cam, w, h, frames=2)
        assert same_bits(got[k], other.read_hdr()).all(), "frame %d (%d meshes)" % (k, steps[k])
    assert not same_bits(got[1], got[-1]).all()
    state = ctx.hierarchy_state()
    assert state.geometryInstalls >= 1 and state.geometryBuildRunning == 0
    flat, perm, nodes, want = linear._check_against_statement(ctx, lbvh.DEFAULT_LEAF_SIZE)  # (builder == GPU among it)
    linear._check_containment(flat, perm, nodes, want)


def test_a_failed_gpu_generation_leaves_the_scene_as_it_was(ctx, other, oracle, cornell_world):
    """Debug option failNextUpdate under MESH_UPDATES: the scene stays, what the worker allocated is given back, and the
    next build - again the GPU builder's - takes the meshes."""
    full = cornell_world
    meshes = len(full.metadatas)
    w, h = 96, 64
    c = full.camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)
    pc = default_pc(S, fl, max_bounces=2)
    _sited_upload(ctx, full.with_meshes_loaded(range(meshes - 2)), UPLOAD | MESH_UPDATES)
    ctx.render(pc, cam, w, h)
    before = ctx.read_hdr()
    nodes_before, bytes_before = ctx.read_nodes(), ctx.scene_stats().deviceBytes
    ctx.set_debug(failNextUpdate=1)
    ctx.update_meshes(full, [meshes - 2, meshes - 1], wait=False)
    with pytest.raises(capi.ProsperPtError) as e:
        ctx.finish_mesh_updates()
    assert e.value.code == -6 and "background build" in str(e.value)
    ctx.set_debug(failNextUpdate=None)
    ctx.render(pc, cam, w, h)
    assert same_bits(before, ctx.read_hdr()).all() and np.array_equal(ctx.read_nodes(), nodes_before)
    assert ctx.scene_stats().deviceBytes == bytes_before
    assert ctx.hierarchy_state().geometryBuildRunning == 1  # the meshes still wait
    ctx.finish_mesh_updates()
    ctx.render(pc, cam, w, h)
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU and ctx.hierarchy_state().geometryInstalls >= 1
    other.upload_scene(full)
    other.render(pc, cam, w, h)
    assert same_bits(ctx.read_hdr(), other.read_hdr()).all()


# ---- 7. drift in the background ----
def _drift_pose(k):
    world = scenes.sponza_class(lights=(4, 4), texture_size=64, sky_size=32, detail=0.25)
    for i in (3, 5, 7):
        model, m = world.model_instances[i]
        world.model_instances[i] = (model, translate((1.5 * k, 0.2 * k, 0.4 * k)) @ m)
    return world


@pytest.fixture(scope="module")
def drift(oracle):
    """The poses of test_gpu_hierarchy.test_gpu_mode_routes_the_rebuild_and_the_drift_trigger and a fresh upload's image of
    each, made once for both selected builders."""
    poses = [_drift_pose(k) for k in range(14)]
    c = poses[0].camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], linear.W, linear.H)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    fresh = capi.Context(device=0)
    want = []
    try:
        for world in poses[1:]:
            fresh.upload_scene(world)
            fresh.render(pc, cam, linear.W, linear.H, frames=4)
            want.append(fresh.read_hdr())
    finally:
        fresh.close()
    return poses, cam, pc, want


@pytest.mark.parametrize("builder", [S.BUILDER_HOST, S.BUILDER_GPU])
def test_drift_trigger_starts_a_background_gpu_generation(ctx, drift, builder):
    poses, cam, pc, want = drift
    ctx.upload_scene(poses[0])
    ctx.set_hierarchy_builder(builder)
    ctx.set_gpu_hierarchy_sites(DRIFT)
    before = ctx.hierarchy_state()
    assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST and before.rebuilds == 0
    images = []
    for world in poses[1:]:
        ctx.update_transforms(world)
        ctx.render(pc, cam, linear.W, linear.H, frames=4, flags=S.RENDER_PIPELINED)
        images.append(ctx.read_hdr())
    ctx.finish_mesh_updates()
    after = ctx.hierarchy_state()
    installs = after.geometryInstalls - before.geometryInstalls
    assert installs > 0, "refits %d, rebuilds %d, measure x%.3f" % (after.refits, after.rebuilds, after.costRatio)
    # every re-split came through the worker thread: none was a synchronous rebuild inside an update
    assert after.rebuilds - before.rebuilds == installs and after.geometryBuildRunning == 0
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    for k, (got, fresh) in enumerate(zip(images, want)):
        assert same_bits(got, fresh).all(), "pose %d" % (k + 1)


# ---- 8. refusals ----
def test_refusals(ctx, worlds):
    lib = capi.lib()
    sites = C.c_uint32(77)
    assert lib.prosper_pt_set_gpu_hierarchy_sites(None, 0) == -1 and b"null" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_get_gpu_hierarchy_sites(None, C.byref(sites)) == -1
    assert lib.prosper_pt_get_gpu_hierarchy_sites(ctx._h, None) == -1 and b"null" in lib.prosper_pt_last_error()
    assert sites.value == 77
    bare = capi.Context(device=0)
    try:
        assert bare.gpu_hierarchy_sites() == 0  # (the default; neither call needs a scene)
        bare.set_gpu_hierarchy_sites(UPLOAD | DRIFT)
        assert bare.gpu_hierarchy_sites() == UPLOAD | DRIFT
        for mask in (8, 0xFFFFFFFF):
            assert lib.prosper_pt_set_gpu_hierarchy_sites(bare._h, mask) == -1 and b"unknown build site" in lib.prosper_pt_last_error()
            assert bare.gpu_hierarchy_sites() == UPLOAD | DRIFT
        bare.set_gpu_hierarchy_sites(0)
        assert bare.gpu_hierarchy_sites() == 0
    finally:
        bare.close()
    ctx.set_gpu_hierarchy_sites(UPLOAD | MESH_UPDATES)
    ctx.upload_scene(worlds("n65"))
    assert ctx.gpu_hierarchy_sites() == UPLOAD | MESH_UPDATES  # (survives the upload)
    with pytest.raises(capi.ProsperPtError) as e:
        ctx.set_gpu_hierarchy_sites(8)
    assert e.value.code == -1 and ctx.gpu_hierarchy_sites() == UPLOAD | MESH_UPDATES
    # independent of the builder selection, which keeps its own contract
    assert ctx.hierarchy_build_info().selectedBuilder == S.BUILDER_HOST and ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    assert lib.prosper_pt_set_hierarchy_builder(ctx._h, 2) == -1 and b"unknown builder" in lib.prosper_pt_last_error()
