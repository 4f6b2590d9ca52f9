"""The GPU builder's refusal and its limit: a tree whose stack bound exceeds kMaxStackBound (96)
is refused and "a refused build leaves the scene exactly as it was" - at every build site; and a tree whose bound IS 96 is
built, refitted and traversed.  The input is the nested comb of tests/ploc_sets.py, about a hundred triangles: with the PLOC
method its stack bound is its triangle count (one triangle per leaf), so 96 triangles sit on the limit and 97 are refused,
while the linear method and the host builder accept every one of these scenes.  Every test first asserts the fact it leans
on against the NumPy statement over the device's own triangles.  Every comparison is of bytes or bits."""
import copy

import numpy as np
import pytest

import ploc_sets
import test_gpu_hierarchy as linear
from conftest import default_pc, same_bits
from prosper_amd import capi, lbvh, ploc, structs as S
from prosper_amd.world import translate

pytestmark = pytest.mark.gpu

UPLOAD, MESH_UPDATES, DRIFT = S.GPU_BUILD_SITE_UPLOAD, S.GPU_BUILD_SITE_MESH_UPDATES, S.GPU_BUILD_SITE_DRIFT
PLOC, LINEAR = S.GPU_HIERARCHY_PLOC, S.GPU_HIERARCHY_LINEAR
LIMIT = lbvh.MAX_STACK_BOUND
UNSUPPORTED, NO_SCENE = -6, -4
W, H = 64, 48
HUGE = 1 << 20
# a second view so narrow that every camera ray stays within 2^-40 of the comb's axis: it enters every box of the comb
NARROW_FOV = 2.0 ** -36


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
    capi.debug(ldsStackEntries=None)


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


@pytest.fixture(scope="module")
def combs():
    made = {}

    def get(n, **kw):
        key = (n,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = ploc_sets.comb_world(n, **kw)
        return made[key]
    return get


def _camera(oracle, world, fov=None):
    c = world.camera
    return oracle.camera_uniforms(c["eye"], c["target"], c["up"], fov or c["fov"], c["zN"], c["zF"], W, H)


def _image(ctx, oracle, world, draw="Default", fov=None):
    cam, fl = _camera(oracle, world, fov)
    ctx.render(default_pc(S, fl, max_bounces=2, draw_type=S.DrawType[draw]), cam, W, H, frames=2)
    return ctx.read_hdr()


def _images(ctx, oracle, world):
    """Two frames of two bounces and where the camera rays hit (the plane z = s / 16 tells the triangle: every instance
    has primitive 0), in the scene's view and in the narrow one."""
    return np.stack([_image(ctx, oracle, world, draw, fov) for fov in (None, NARROW_FOV) for draw in ("Default", "Position")])


def _oracle_images(oracle, world):
    """The oracle's two-bounce images of both views (what _images holds at 0 and 2)."""
    osc = oracle.OracleScene(world)
    out = []
    for fov in (None, NARROW_FOV):
        cam, fl = _camera(oracle, world, fov)
        want = None
        for f in (1, 2):
            want, _ = osc.render(default_pc(S, fl, frame_index=f, skip_history=(f == 1), max_bounces=2), cam, W, H, history=want)
        out.append(want)
    return out


def _snapshot(ctx, oracle, world):
    """What "the scene is as it was" compares: the node bytes, the flat triangles and the permutation, every field of the
    build info (stage times and totalMs included) and of the method info, the hierarchy state without `rebuilds` (asserted
    where it matters), the scene's node count, stack bound and device bytes, and a two-frame render."""
    flat, perm = ctx.read_hierarchy_arrays()
    state, stats = ctx.hierarchy_state(), ctx.scene_stats()
    return dict(
        nodes=ctx.read_nodes().tobytes(), flat=flat.tobytes(), perm=perm.tobytes(),
        info=bytes(ctx.hierarchy_build_info()), method=bytes(ctx.gpu_hierarchy_method_info()),
        state=tuple((name, getattr(state, name)) for name, _ in S.HierarchyState._fields_ if name != "rebuilds"),
        stats=(int(stats.nodeCount), int(stats.maxDepth), int(stats.deviceBytes), int(stats.triangleCount)),
        image=_image(ctx, oracle, world))


def _assert_as_it_was(ctx, oracle, world, before):
    after = _snapshot(ctx, oracle, world)
    for key in before:
        if key == "image":
            assert same_bits(after[key], before[key]).all(), key
        else:
            assert after[key] == before[key], key


def _refused(call, *needles):
    with pytest.raises(capi.ProsperPtError) as e:
        call()
    assert e.value.code == UNSUPPORTED, e.value
    for needle in ("stack bound",) + needles:
        assert needle in str(e.value), e.value


def _statement_bound(ctx, n, leaf, radius=ploc.DEFAULT_RADIUS):
    """The PLOC statement's stack bound over the device's own triangles - which are the nested comb's, value for value."""
    flat, _ = ctx.read_hierarchy_arrays()
    assert np.array_equal(lbvh.vertices(flat)[-n:], ploc_sets.nested_comb(n))
    return ploc.build(flat, leaf_size=leaf, radius=radius, max_stack_bound=HUGE).stack_bound


def _check_against_the_ploc_statement(ctx, leaf, radius=ploc.DEFAULT_RADIUS):
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
    assert info.totalMs > 0.0
    linear._check_containment(flat, perm, nodes, want)
    return flat, perm, nodes, want


def _boxes_sticking_out(nodes):
    """linear._stored_boxes_sticking_out by comparison alone (the comb's largest boxes are infinite in binary16, and a
    difference of infinities is no number): (node, slot) pairs whose stored box does not contain the stored boxes of that
    child's own children."""
    lo, hi = lbvh.decode_boxes(nodes)
    child, reserved = linear._tree_words(nodes)
    out = 0
    for i in range(len(nodes)):
        for c in range(int(reserved[i])):
            ref = int(child[i, c])
            if ref >= 0:
                k = int(reserved[ref])
                out += bool((lo[ref, :k] < lo[i, c]).any() or (hi[ref, :k] > hi[i, c]).any())
    with np.errstate(invalid="ignore"):
        assert linear._stored_boxes_sticking_out(nodes)[0] <= out
    return out


def _moved(world, moves):
    """`world` with the given (instance, offset) moves."""
    w = copy.copy(world)
    w._frozen = None
    w.model_instances = list(world.model_instances)
    for instance, offset in moves:
        model, m = w.model_instances[instance]
        w.model_instances[instance] = (model, translate(offset) @ m)
    return w


# ---- 1. the synchronous build: refused over a host tree, and over a GPU tree in a scratch state a refusal has used ----
def test_synchronous_refusal_leaves_the_scene_and_the_scratch_state_usable(ctx, oracle, combs):
    world = combs(101)
    ctx.upload_scene(world)
    ctx.set_gpu_hierarchy_method(PLOC)
    assert _statement_bound(ctx, 101, ploc.DEFAULT_LEAF_SIZE) > LIMIT
    assert lbvh.build(ctx.read_hierarchy_arrays()[0]).stack_bound <= LIMIT and ctx.scene_stats().maxDepth <= LIMIT
    before = _snapshot(ctx, oracle, world)
    rebuilds = ctx.hierarchy_state().rebuilds
    _refused(ctx.build_hierarchy_gpu)
    _assert_as_it_was(ctx, oracle, world, before)
    assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST and ctx.hierarchy_state().rebuilds == rebuilds
    # the linear method in the scratch state the refused build has run its clustering, collapse, heights and sorts in
    ctx.set_gpu_hierarchy_method(LINEAR)
    ctx.build_hierarchy_gpu()
    flat, perm, nodes, want = linear._check_against_statement(ctx, lbvh.DEFAULT_LEAF_SIZE)
    linear._check_containment(flat, perm, nodes, want)
    assert _boxes_sticking_out(nodes) == 0 and ctx.hierarchy_state().rebuilds == rebuilds + 1
    assert same_bits(_image(ctx, oracle, world), before["image"]).all()
    # refused again, over a tree the GPU builder made: that tree's stage times stay too
    ctx.set_gpu_hierarchy_method(PLOC)
    standing = _snapshot(ctx, oracle, world)
    info = ctx.hierarchy_build_info()
    assert info.builder == S.BUILDER_GPU and info.totalMs > 0.0 and any(ms > 0.0 for ms in info.stageMs)
    _refused(ctx.build_hierarchy_gpu)
    _assert_as_it_was(ctx, oracle, world, standing)
    assert ctx.hierarchy_state().rebuilds == rebuilds + 1
    assert list(ctx.hierarchy_build_info().stageMs) == list(info.stageMs) and ctx.hierarchy_build_info().totalMs == info.totalMs


# ---- 2. one triangle apart ----
def test_one_triangle_between_the_limit_and_the_refusal(ctx, oracle, combs):
    world = combs(97)
    ctx.upload_scene(world)
    ctx.set_gpu_hierarchy_method(PLOC)
    ctx.set_debug(leafSize=1)  # (after the upload: the host's first tree is the default's)
    assert _statement_bound(ctx, 97, 1) == LIMIT + 1
    before = _snapshot(ctx, oracle, world)
    _refused(ctx.build_hierarchy_gpu)
    _assert_as_it_was(ctx, oracle, world, before)
    ctx.set_debug(leafSize=2)
    assert _statement_bound(ctx, 97, 2) == LIMIT
    ctx.build_hierarchy_gpu()
    _check_against_the_ploc_statement(ctx, 2)
    assert ctx.hierarchy_build_info().stackBound == LIMIT
    ctx.set_debug(leafSize=None)
    ctx.upload_scene(combs(96))
    ctx.set_debug(leafSize=1)
    assert _statement_bound(ctx, 96, 1) == LIMIT
    ctx.build_hierarchy_gpu()
    _check_against_the_ploc_statement(ctx, 1)
    assert ctx.hierarchy_build_info().stackBound == LIMIT


# ---- 3. traversal, refit and nest pass at the limit ----
@pytest.mark.parametrize("n,leaf", [(96, 1), (97, 2)])
def test_traversal_at_the_stack_limit(ctx, other, oracle, combs, n, leaf):
    """The deepest stack the traversal claims to hold: stackBound == 96, so the kernels run with 96 - ldsStackEntries
    overflow entries a lane (80 with the 16-entry variant), and the comb makes rays fill them - a ray along the axis
    enters every box, the nearer inner child is taken first and the node's leaves wait on the stack."""
    world = combs(n)
    ctx.set_gpu_hierarchy_method(PLOC)
    ctx.upload_scene(world)
    ctx.set_debug(leafSize=leaf)  # (after the upload: the host's first tree is the default's)
    assert _statement_bound(ctx, n, leaf) == LIMIT
    ctx.build_hierarchy_gpu()
    _, _, nodes, _ = _check_against_the_ploc_statement(ctx, leaf)
    assert ctx.scene_stats().maxDepth == LIMIT and _boxes_sticking_out(nodes) == 0
    got = _images(ctx, oracle, world)
    other.upload_scene(world)
    assert other.hierarchy_build_info().builder == S.BUILDER_HOST
    host = _images(other, oracle, world)
    assert np.isfinite(host).all()
    for view in (0, 1):  # the comb is in view: lit pixels differ, and so do the places the camera rays hit
        assert len(np.unique(host[view].reshape(-1, 4), axis=0)) > 2, view
    # ... and both views show many triangles of it, the narrow one those far below the scene view's pixel size
    assert len(np.unique(host[1][..., 2])) > 16 and len(np.unique(host[3][..., 2])) > 16
    assert host[3][..., 2].max() < 2.0 ** -30 < host[1][..., 2].max()
    assert same_bits(got, host).all()
    wide, narrow = _oracle_images(oracle, world)
    assert same_bits(host[0], wide).all() and same_bits(host[2], narrow).all()
    try:
        for forced in (16, 24, 32):  # 16: the deepest 80 entries of a lane's stack lie in the global overflow array
            capi.debug(ldsStackEntries=forced)
            assert same_bits(_images(ctx, oracle, world), host).all(), forced
    finally:
        capi.debug(ldsStackEntries=None)
    # the refit and the nest pass over the limit tree: every instance one exact step up
    pose = _moved(world, [(k, (0.0, 2.0 ** -7, 0.0)) for k in range(n)])
    ctx.update_transforms(pose)
    got = _images(ctx, oracle, pose)
    other.upload_scene(pose)
    fresh = _images(other, oracle, pose)
    assert same_bits(got, fresh).all() and not same_bits(fresh[0], host[0]).all()
    state = ctx.hierarchy_state()
    assert state.refits == 1 and ctx.scene_stats().maxDepth == LIMIT and ctx.hierarchy_build_info().builder == S.BUILDER_GPU
    moved_nodes = ctx.read_nodes()
    assert _boxes_sticking_out(moved_nodes) == 0
    assert np.array_equal(linear._tree_words(moved_nodes)[0], linear._tree_words(nodes)[0])


# ---- 4. rebuilds routed to the GPU builder ----
def test_routed_rebuilds_are_refused_and_the_staged_update_survives(ctx, other, oracle, combs):
    world = combs(101)
    ctx.upload_scene(world)
    ctx.set_hierarchy_builder(S.BUILDER_GPU)
    ctx.set_gpu_hierarchy_method(PLOC)
    assert _statement_bound(ctx, 101, ploc.DEFAULT_LEAF_SIZE) > LIMIT
    before = _snapshot(ctx, oracle, world)
    rebuilds = ctx.hierarchy_state().rebuilds
    _refused(ctx.rebuild_hierarchy)
    _assert_as_it_was(ctx, oracle, world, before)
    assert ctx.hierarchy_state().rebuilds == rebuilds
    pose = _moved(world, [(50, (0.0, 2.0 ** -7, 0.0))])
    ctx.set_debug(alwaysRebuild=1)
    _refused(lambda: ctx.update_transforms(pose))
    ctx.set_debug(alwaysRebuild=None)
    got = _image(ctx, oracle, pose)
    other.upload_scene(pose)
    assert same_bits(got, _image(other, oracle, pose)).all()
    assert not same_bits(got, before["image"]).all()
    state = ctx.hierarchy_state()
    assert state.rebuilds == rebuilds and state.refits >= 1 and ctx.hierarchy_build_info().builder == S.BUILDER_HOST
    assert ctx.read_nodes().shape[0] == len(before["nodes"]) // 80  # (refitted on the old tree)


# ---- 5. site UPLOAD ----
def _stats_or_code(ctx):
    try:
        return int(ctx.scene_stats().deviceBytes)
    except capi.ProsperPtError as e:
        return "error %d" % e.code


def test_a_refused_upload_leaves_no_scene_and_no_fall_back(ctx, other, oracle, combs, cornell_world):
    world = combs(101)
    ctx.upload_scene(cornell_world)
    ctx.set_gpu_hierarchy_sites(UPLOAD)
    ctx.set_gpu_hierarchy_method(PLOC, 4)
    assert ploc.build(ploc_sets.nested_comb(101), radius=4, max_stack_bound=HUGE).stack_bound > LIMIT
    _refused(lambda: ctx.upload_scene(world))
    cam, fl = _camera(oracle, world)
    with pytest.raises(capi.ProsperPtError) as e:
        ctx.render(default_pc(S, fl, max_bounces=2), cam, W, H)
    assert e.value.code == NO_SCENE
    bare = capi.Context(device=0)
    try:
        assert _stats_or_code(ctx) == _stats_or_code(bare)
    finally:
        bare.close()
    method = ctx.gpu_hierarchy_method_info()
    assert ctx.gpu_hierarchy_sites() == UPLOAD and method.selectedMethod == PLOC and method.selectedRadius == 4
    # clear the bit and upload again: a host upload like any other
    ctx.set_gpu_hierarchy_sites(0)
    ctx.upload_scene(world)
    other.upload_scene(world)
    assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST
    assert np.array_equal(ctx.read_nodes(), other.read_nodes())
    assert same_bits(_image(ctx, oracle, world), _image(other, oracle, world)).all()
    assert ctx.scene_stats().deviceBytes == other.scene_stats().deviceBytes
    # the bit again with the linear method, in the scratch state the refused upload has used
    ctx.set_gpu_hierarchy_sites(UPLOAD)
    ctx.set_gpu_hierarchy_method(LINEAR)
    ctx.upload_scene(world)
    flat, perm, nodes, want = linear._check_against_statement(ctx, lbvh.DEFAULT_LEAF_SIZE)
    assert np.array_equal(lbvh.vertices(flat), ploc_sets.nested_comb(101))
    linear._check_containment(flat, perm, nodes, want)
    assert same_bits(_image(ctx, oracle, world), _image(other, oracle, world)).all()


# ---- 6. site MESH_UPDATES ----
def test_a_refused_background_generation_leaves_the_scene_and_the_meshes_wait(ctx, other, oracle, combs):
    """What test_gpu_hierarchy_sites.test_a_failed_gpu_generation_leaves_the_scene_as_it_was asserts after failNextUpdate,
    after the device's own refusal.  The retry: "the meshes wait for the next build" (prosper_pt.h) - that build is
    started by the next prosper_pt_finish_mesh_updates with the selection of that moment."""
    full = combs(101, extra_quad=True)
    quad, comb = 0, 1
    ctx.set_gpu_hierarchy_method(PLOC)
    ctx.set_gpu_hierarchy_sites(UPLOAD | MESH_UPDATES)
    ctx.upload_scene(full.with_meshes_loaded([quad]))
    assert ctx.hierarchy_build_info().builder == S.BUILDER_GPU and ctx.scene_stats().triangleCount == 2
    before = _image(ctx, oracle, full)
    nodes_before, bytes_before = ctx.read_nodes(), ctx.scene_stats().deviceBytes
    info_before, installs = bytes(ctx.hierarchy_build_info()), ctx.hierarchy_state().geometryInstalls
    ctx.update_meshes(full, [comb], wait=False)
    _refused(ctx.finish_mesh_updates, "background build")
    assert same_bits(before, _image(ctx, oracle, full)).all() and np.array_equal(ctx.read_nodes(), nodes_before)
    assert ctx.scene_stats().deviceBytes == bytes_before and bytes(ctx.hierarchy_build_info()) == info_before
    state = ctx.hierarchy_state()
    assert state.geometryBuildRunning == 1 and state.geometryInstalls == installs  # the meshes still wait
    # the next build takes the selection of its own start: the linear method, in the worker's scratch state
    ctx.set_gpu_hierarchy_method(LINEAR)
    ctx.finish_mesh_updates()
    state = ctx.hierarchy_state()
    assert state.geometryInstalls == installs + 1 and state.geometryBuildRunning == 0
    flat, perm, nodes, want = linear._check_against_statement(ctx, lbvh.DEFAULT_LEAF_SIZE)
    assert len(flat) == 103 and np.array_equal(lbvh.vertices(flat)[2:], ploc_sets.nested_comb(101))
    assert ploc.build(flat, max_stack_bound=HUGE).stack_bound > LIMIT  # (what the refused generation was built over)
    linear._check_containment(flat, perm, nodes, want)
    other.upload_scene(full)
    assert same_bits(_image(ctx, oracle, full), _image(other, oracle, full)).all()
    assert not same_bits(_image(ctx, oracle, full), before).all()


# ---- 7. site DRIFT ----
def test_a_refused_drift_generation_is_reported_and_the_frames_go_on(oracle, other, combs):
    """The smallest triangle, which lies deepest, travels beyond the largest one's width and stretches every inner box
    above it (the refit's measure sums the inner children's boxes: moving a triangle that hangs off the root changes
    nothing); triangle 50 steps up into view.  The measure passes the trigger (rebuildCostRatio), the second update starts
    a background generation from the GPU builder, and that generation is refused."""
    world = combs(101)
    poses = [world] + [_moved(world, [(0, (far, 0.0, 0.0)), (50, (0.0, up, 0.0))]) for far, up in ((2.0 ** 51, 2.0 ** -7), (2.0 ** 52, 2.0 ** -6))]
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(poses[0])
        ctx.set_gpu_hierarchy_sites(DRIFT)
        ctx.set_gpu_hierarchy_method(PLOC)
        ctx.set_debug(rebuildCostRatio=1.0009765625)
        assert _statement_bound(ctx, 101, ploc.DEFAULT_LEAF_SIZE) > LIMIT
        assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST
        start = ctx.hierarchy_state()
        images = [_image(ctx, oracle, poses[0])]
        ctx.update_transforms(poses[1])
        images.append(_image(ctx, oracle, poses[1]))
        state = ctx.hierarchy_state()  # (waits for the refit's measure)
        assert state.refits == 1 and state.costRatio > 1.0009765625 and state.geometryBuildRunning == 0
        ctx.update_transforms(poses[2])  # past the trigger: the background generation starts
        assert ctx.hierarchy_state().geometryBuildRunning == 1
        _refused(ctx.finish_mesh_updates, "background build")  # the call that would have switched to it
        images.append(_image(ctx, oracle, poses[2]))
        # what the refused generation was built over: the moved pose's triangles, still a comb beyond the limit
        assert ploc.build(ctx.read_hierarchy_arrays()[0], max_stack_bound=HUGE).stack_bound > LIMIT
        after = ctx.hierarchy_state()
        assert after.geometryInstalls == start.geometryInstalls and after.rebuilds == start.rebuilds
        assert ctx.hierarchy_build_info().builder == S.BUILDER_HOST
        for k, (pose, got) in enumerate(zip(poses, images)):
            other.upload_scene(pose)
            assert same_bits(got, _image(other, oracle, pose)).all(), "pose %d" % k
        assert not same_bits(images[0], images[1]).all() and not same_bits(images[1], images[2]).all()
    finally:
        ctx.close()
    assert ctx._h is None
