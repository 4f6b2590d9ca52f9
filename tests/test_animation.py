"""Keyframe animation on the GPU: prosper_pt_set_animations / prosper_pt_animate over
tests/golden/animated_scene.gltf against the NumPy restatement tests/animation_reference.py - the samples bit for bit
(slerp within its libm tolerance), the hierarchy bit for bit over the GPU's own read-back TRS, and what the rest of the
library sees of an animated update: images equal to a fresh upload of the read-back scene, frames in flight, the host
mirrors, the previous table for the velocity target, the refusals.  Frames are 64 x 48, path tracing 1 spp."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import animation_reference as R
from conftest import default_pc
from prosper_amd import animation, capi, gltf, structs as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "animated_scene.gltf")
NONE = S.ANIMATION_NONE
W, H = 64, 48
IMAGE_TIMES = (0.0, 0.55, 1.0, 1.7)
FLIGHT_TIMES = (0.1, 0.55, 0.8, 1.0, 1.3, 1.7, 2.2, 3.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def words(struct):
    return np.frombuffer(struct, np.uint32).copy()


def table_array(transforms, count):
    return np.frombuffer(transforms, np.float32).reshape(-1, 2, 3, 4)[:count].copy()


def copy_tables(t):
    return animation.AnimationTables([S.AnimationNode.from_buffer_copy(n) for n in t.nodes],
                                     [S.AnimationChannel.from_buffer_copy(c) for c in t.channels], t.times.copy(), t.values.copy(),
                                     t.gltf_nodes)


@pytest.fixture(scope="module")
def world():
    return gltf.load_gltf(FIXTURE)


@pytest.fixture(scope="module")
def tables():
    return animation.load_animations(FIXTURE)


@pytest.fixture(scope="module")
def times(tables):
    return R.sample_times(tables)


def prepare(ctx, world, tables):
    ctx.upload_scene(world)
    ctx.set_animations(tables)


def expected_outputs(world, tables, world_matrices, base_table=None):
    """Kernel B's outputs over the uploaded scene's table and lights: (table, directional, points, spots) as uint32 words
    of the device's structs, and the camera record."""
    n = len(world.model_instances)
    base = table_array(world.freeze()["transforms"], n) if base_table is None else base_table
    d, p, s = words(world.directional), words(world.point_lights), words(world.spot_lights)
    df, pf, sf = d.view(np.float32), p.view(np.float32), s.view(np.float32)
    points, spots = pf[:1024 * 8].reshape(1024, 2, 4), sf[:1024 * 12].reshape(1024, 3, 4)
    table, direction, positions, spot_fields, camera = R.outputs(tables, world_matrices, base, df[4:8], points[:, 1], spots[:, 1:3])
    df[4:8] = direction
    points[:, 1] = positions
    spots[:, 1:3] = spot_fields
    return table, d, p, s, camera


@pytest.fixture(scope="module")
def sweep(gpu_ctx, world, tables, times):
    """Every sample time once: what the GPU reads back after prosper_pt_animate(t)."""
    prepare(gpu_ctx, world, tables)
    out = {}
    for k, t in enumerate(times):
        gpu_ctx.animate(t, now=(k % 2 == 1))  # staged, or enqueued by the call on the null stream
        trs, matrices = gpu_ctx.read_animation_nodes()
        d, p, s = gpu_ctx.read_lights()
        st = gpu_ctx.animation_state()
        out[t] = dict(trs=trs, world=matrices, table=table_array(gpu_ctx.read_animated_transforms(), len(world.model_instances)),
                      lights=(words(d), words(p), words(s)), camera=np.float32(list(st.eye) + list(st.target) + list(st.up)),
                      updates=st.updates, camera_valid=st.cameraValid)
    return out


def test_sampling_equals_the_restatement(sweep, tables, times):
    """Over all sample times every Step, CubicSpline and vec3-Linear target, and every rotation on slerp's mix branch, has
    the float32 restatement's bits; a rotation on the slerp branch lies within 4 * max(E_ref, 2^-22) per component of the
    float64 restatement (the 4 covers a second libm's acosf / sinf, each within a few ulp, not another formula)."""
    e_ref = R.slerp_error(tables, times)
    tolerance = 4.0 * max(e_ref, 2.0 ** -22)
    targets = R.resolve_targets(tables)
    flags, static = R.static_pose(tables)
    counted = {"exact": 0, "mix": 0, "slerp": 0}
    worst = 0.0
    for t in times:
        got = sweep[t]["trs"]
        untouched = np.ones(got.shape, bool)
        for (node, path), ch in targets.items():
            slot = R._SLOT[path]
            untouched[node, slot] = False
            kind = "exact"
            if path == S.ANIMATION_PATH_ROTATION and ch.interpolation == S.ANIMATION_LINEAR:
                a, _, first = R.key_frame(R.channel_times(tables, ch), ch.startTimeS, ch.endTimeS, t)
                if a != 0:
                    v = R.channel_values(tables, ch)
                    kind = R.slerp_branch(v[first], v[first + 1])
            counted[kind] += 1
            if kind == "slerp":
                # (the same sample E_ref is taken over: the float32 keys and the float32 interpolant, in float64)
                error = float(np.max(np.abs(got[node, slot].astype(np.float64) - R.slerp(v[first], v[first + 1], a, np.float64))))
                worst = max(worst, error)
                assert error <= tolerance, (t, node, error, tolerance)
            else:
                want = np.asarray(R.sample_channel(tables, ch, t, np.float32), np.float32)
                assert same(got[node, slot], want), (t, node, path, got[node, slot], want)
        assert same(got[untouched], static[untouched]), t  # what no channel targets stays the static pose
    print("slerp: worst distance from the float64 restatement %.3e, tolerance %.3e, E_ref %.3e" % (worst, tolerance, e_ref))
    assert counted["exact"] > 0 and counted["mix"] > 0 and counted["slerp"] > 0
    assert sum(counted.values()) == len(times) * len(targets) and len(targets) == 11


def test_hierarchy_equals_the_restatement_of_the_read_back_pose(sweep, world, tables, times):
    """The restatement fed the GPU's own TRS: world matrices, the ModelInstanceTransforms table, the three light buffers
    and the camera record are bit-exact for every node at every time."""
    for k, t in enumerate(times):
        got = sweep[t]
        matrices = R.hierarchy(tables, got["trs"])
        assert same(got["world"], matrices), t
        table, d, p, s, camera = expected_outputs(world, tables, matrices)
        assert same(got["table"], table), t
        for have, want in zip(got["lights"], (d, p, s)):
            assert np.array_equal(have, want), t
        assert got["camera_valid"] == 1 and same(got["camera"], camera), t
        assert got["updates"] == k + 1
    moving = [t for t in times if not same(sweep[t]["table"], sweep[times[0]]["table"])]
    assert len(moving) > len(times) // 2  # (the scene does move)


def test_an_unbound_instance_keeps_its_transform(gpu_ctx, world, tables):
    """A model instance no node binds keeps its bytes; a pending prosper_pt_update_transforms that moves it survives a
    prosper_pt_animate staged after it, and both are consumed by one flush."""
    from prosper_amd.world import translate
    loose = copy_tables(tables)
    floor_node = tables.gltf_nodes.index(4)
    floor = loose.nodes[floor_node].modelInstance
    loose.nodes[floor_node].modelInstance = NONE
    prepare(gpu_ctx, world, loose)
    n = len(world.model_instances)
    uploaded = table_array(world.freeze()["transforms"], n)
    gpu_ctx.animate(0.7)
    got = table_array(gpu_ctx.read_animated_transforms(), n)
    assert same(got[floor], uploaded[floor]) and not same(got, uploaded)
    moved = copy.copy(world)
    moved._frozen = None
    moved.model_instances = list(world.model_instances)
    model, m = moved.model_instances[floor]
    moved.model_instances[floor] = (model, translate((0.5, -0.25, 1.0)) @ m)
    refits = gpu_ctx.hierarchy_state().refits
    gpu_ctx.update_transforms(moved)
    gpu_ctx.animate(1.1)
    got = table_array(gpu_ctx.read_animated_transforms(), n)
    assert gpu_ctx.hierarchy_state().refits == refits + 1
    want_floor = table_array(moved.freeze()["transforms"], n)[floor]
    assert same(got[floor], want_floor) and not same(want_floor, uploaded[floor])
    trs, matrices = gpu_ctx.read_animation_nodes()
    table, *_ = expected_outputs(world, loose, R.hierarchy(loose, trs), base_table=table_array(moved.freeze()["transforms"], n))
    assert same(got, table)
    gpu_ctx.upload_scene(world)  # (the session's context goes back to the scene as loaded)


# ---- images ----

def read_back_world(world, transforms, lights):
    """`world` with the table and light buffers the device held: what a fresh upload of the animated scene takes."""
    w = copy.copy(world)
    w._frozen = None
    w.directional, w.point_lights, w.spot_lights = lights
    w._directional_found = True  # (the buffers are taken as they are)
    f = w.freeze()
    C.memmove(f["transforms"], transforms, C.sizeof(S.ModelInstanceTransforms) * len(world.model_instances))
    return w


def camera_of(oracle, world, state):
    c = world.camera
    return oracle.camera_uniforms(tuple(state.eye), tuple(state.target), tuple(state.up), c["fov"], c["zN"], c["zF"], W, H)


def render(ctx, cam, fl, frame_index=1):
    ctx.render(default_pc(S, fl, frame_index=frame_index, max_bounces=3, ibl=False), cam, W, H, frames=1)
    return ctx.read_hdr()


@pytest.fixture(scope="module")
def fresh_ctx():
    ctx = capi.Context(device=0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def fresh_frames(gpu_ctx, fresh_ctx, oracle, world, tables):
    """Per time, once: the scene the GPU holds after prosper_pt_animate(t) - table, lights, camera record - and the images
    a fresh prosper_pt_upload_scene of it gives."""
    cache = {}

    def frame(t):
        if t not in cache:
            prepare(gpu_ctx, world, tables)
            gpu_ctx.animate(t)
            transforms, lights, state = gpu_ctx.read_animated_transforms(), gpu_ctx.read_lights(), gpu_ctx.animation_state()
            cam, fl = camera_of(oracle, world, state)
            fresh_ctx.upload_scene(read_back_world(world, transforms, lights))
            cache[t] = dict(transforms=transforms, lights=lights, cam=cam, fl=fl, hdr=render(fresh_ctx, cam, fl),
                            gbuffer=fresh_ctx.trace_gbuffer(cam, W, H))
        return cache[t]
    return frame


def test_images_equal_a_fresh_upload_of_the_read_back_scene(gpu_ctx, fresh_frames, world, tables):
    images = []
    for t in IMAGE_TIMES:
        want = fresh_frames(t)
        prepare(gpu_ctx, world, tables)
        gpu_ctx.animate(t)
        got = render(gpu_ctx, want["cam"], want["fl"])
        assert same(got, want["hdr"]), t
        for a, b in zip(gpu_ctx.trace_gbuffer(want["cam"], W, H), want["gbuffer"]):
            assert same(a, b), t
        assert float(got[..., :3].max()) > 0.0
        images.append(got)
    assert not same(images[0], images[1]) and not same(images[1], images[3])  # (something in view moves)


def test_eight_frames_in_flight(gpu_ctx, fresh_frames, world, tables):
    """Eight pipelined frames, each preceded by prosper_pt_animate: more updates than scene versions.  Every frame equals
    its fresh-upload image and the hierarchy was refitted eight times."""
    hip = C.CDLL("libamdhip64.so")  # the runtime the library already uses
    want = [fresh_frames(t) for t in FLIGHT_TIMES]
    nbytes = W * H * 16
    buffers = []
    for _ in FLIGHT_TIMES:
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), C.c_size_t(nbytes)) == 0
        buffers.append(ptr)
    try:
        prepare(gpu_ctx, world, tables)
        refits = gpu_ctx.hierarchy_state().refits
        for t, frame, ptr in zip(FLIGHT_TIMES, want, buffers):
            gpu_ctx.animate(t)
            gpu_ctx.set_output_buffer(ptr.value, nbytes)
            gpu_ctx.render(default_pc(S, frame["fl"], max_bounces=3, ibl=False), frame["cam"], W, H, frames=1, flags=S.RENDER_PIPELINED)
        assert hip.hipDeviceSynchronize() == 0
        assert gpu_ctx.hierarchy_state().refits == refits + len(FLIGHT_TIMES)
        for t, frame, ptr in zip(FLIGHT_TIMES, want, buffers):
            got = np.empty((H, W, 4), np.float32)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), ptr, C.c_size_t(nbytes), 2) == 0  # device to host
            assert same(got, frame["hdr"]), t
    finally:
        gpu_ctx.set_output_buffer(None, 0)
        for ptr in buffers:
            hip.hipFree(ptr)


def test_the_host_mirrors_follow_an_animated_update(gpu_ctx, fresh_frames, world, tables):
    """After prosper_pt_animate the library's host copies are the animated scene: prosper_pt_update_transforms with the read-back
    table and prosper_pt_update_lights with the read-back lights are no-ops, and prosper_pt_rebuild_hierarchy re-splits
    the instances where they are now."""
    t = IMAGE_TIMES[1]
    frame = fresh_frames(t)
    prepare(gpu_ctx, world, tables)
    gpu_ctx.animate(t)
    transforms = gpu_ctx.read_animated_transforms()
    d, p, s = gpu_ctx.read_lights()
    before, light_updates = gpu_ctx.hierarchy_state(), gpu_ctx.animation_state().lightUpdates
    assert light_updates == 1
    capi._check(capi.lib().prosper_pt_update_transforms(gpu_ctx._h, C.cast(transforms, C.c_void_p), len(world.model_instances)))
    capi._check(capi.lib().prosper_pt_update_lights(gpu_ctx._h, C.byref(d), C.byref(p), C.byref(s)))
    image = render(gpu_ctx, frame["cam"], frame["fl"])
    assert gpu_ctx.hierarchy_state().refits == before.refits and gpu_ctx.animation_state().lightUpdates == light_updates
    assert same(image, frame["hdr"])
    # the table as uploaded is a change now (the mirror is not the upload's any more)
    capi._check(capi.lib().prosper_pt_update_transforms(
        gpu_ctx._h, C.cast(world.freeze()["transforms"], C.c_void_p), len(world.model_instances)))
    assert gpu_ctx.hierarchy_state().refits == before.refits + 1
    gpu_ctx.animate(t)
    assert same(render(gpu_ctx, frame["cam"], frame["fl"]), frame["hdr"])
    # (the instances have travelled: a background re-split may be under way, and counts as a rebuild of its own)
    gpu_ctx.finish_mesh_updates()
    rebuilds = gpu_ctx.hierarchy_state().rebuilds
    gpu_ctx.rebuild_hierarchy()
    assert gpu_ctx.hierarchy_state().rebuilds == rebuilds + 1
    assert same(render(gpu_ctx, frame["cam"], frame["fl"]), frame["hdr"])
    assert same(table_array(gpu_ctx.read_animated_transforms(), 3), table_array(transforms, 3))


def test_the_previous_table_feeds_the_velocity_target(gpu_ctx, fresh_frames, world, tables):
    t1, t2 = IMAGE_TIMES[1], IMAGE_TIMES[3]
    frame = fresh_frames(t2)
    n = len(world.model_instances)
    prepare(gpu_ctx, world, tables)
    uploaded = table_array(gpu_ctx.read_animated_transforms(previous=True), n)
    assert same(uploaded, table_array(world.freeze()["transforms"], n))  # before any update: the current table
    gpu_ctx.animate(t1)
    first = gpu_ctx.read_animated_transforms()
    assert same(table_array(gpu_ctx.read_animated_transforms(previous=True), n), uploaded)
    gpu_ctx.animate(t2)
    previous = gpu_ctx.read_animated_transforms(previous=True)
    assert same(table_array(previous, n), table_array(first, n))
    assert not same(table_array(gpu_ctx.read_animated_transforms(), n), table_array(first, n))
    a = gpu_ctx.trace_gbuffer_velocity(frame["cam"], W, H, previous_transforms=previous)
    b = gpu_ctx.trace_gbuffer_velocity(frame["cam"], W, H, previous_transforms=first)
    for x, y in zip(a, b):
        assert same(x, y)
    assert np.any(a[3] != 0.0)  # (instances in view moved between the two updates)


def test_the_host_layer_mirror(gpu_ctx, world, tables):
    """scene::Animations through its C shims: create = prosper_pt_set_animations, update = World::updateAnimations(timeS)."""
    lib = capi.lib()
    gpu_ctx.upload_scene(world)
    desc = tables.desc()
    handle = C.c_void_p()
    capi._check(lib.prosper_host_animations_create(gpu_ctx._h, C.byref(desc), C.byref(handle)))
    try:
        assert lib.prosper_host_animations_end_time(handle) == 2.5
        capi._check(lib.prosper_host_animations_update(handle, 0.8))
        gpu_ctx._animation_nodes = len(tables.nodes)
        trs, _ = gpu_ctx.read_animation_nodes()
        lamp = tables.gltf_nodes.index(6)
        want = R.sample_channel(tables, R.resolve_targets(tables)[(lamp, S.ANIMATION_PATH_TRANSLATION)], 0.8)
        assert same(trs[lamp, :3], np.asarray(want, np.float32)) and gpu_ctx.animation_state().updates == 1
    finally:
        lib.prosper_host_animations_destroy(handle)
    broken = copy_tables(tables)
    broken.channels[0].keyCount = 0
    desc = broken.desc()
    assert lib.prosper_host_animations_create(gpu_ctx._h, C.byref(desc), C.byref(handle)) == -1 and not handle.value
    assert b"keyCount" in lib.prosper_host_last_error()


# ---- refusals ----

def refused(ctx, t, code=-1):
    with pytest.raises(capi.ProsperPtError) as e:
        ctx.set_animations(t)
    assert e.value.code == code, e.value
    return str(e.value)


def test_refusals(gpu_ctx, fresh_ctx, world, tables):
    lib = capi.lib()
    empty = capi.Context(device=0)
    try:
        refused(empty, tables, code=-4)  # PROSPER_PT_ERR_NO_SCENE
        assert lib.prosper_pt_animate(empty._h, 0.0, 0, None) == -4
    finally:
        empty.close()
    ctx = fresh_ctx
    ctx.upload_scene(world)
    with pytest.raises(capi.ProsperPtError) as e:
        ctx.animate(0.5)  # before prosper_pt_set_animations
    assert e.value.code == -1 and "prosper_pt_set_animations" in str(e.value)

    def broken(change):
        t = copy_tables(tables)
        change(t)
        return t

    def node_field(index, name, value):
        return lambda t: setattr(t.nodes[index], name, value)

    def channel_field(index, name, value):
        return lambda t: setattr(t.channels[index], name, value)
    blade, bob = tables.gltf_nodes.index(3), tables.gltf_nodes.index(8)
    lamp, spot, camera = tables.gltf_nodes.index(6), tables.gltf_nodes.index(7), tables.gltf_nodes.index(10)
    rotation = next(i for i, c in enumerate(tables.channels) if c.path == S.ANIMATION_PATH_ROTATION)
    translation = next(i for i, c in enumerate(tables.channels) if c.path == S.ANIMATION_PATH_TRANSLATION)
    for change in (
            node_field(blade, "modelInstance", 3),                                  # indices out of range
            node_field(lamp, "pointLight", 1), node_field(spot, "spotLight", 1),
            node_field(blade, "parent", 12), channel_field(0, "node", 12),
            channel_field(0, "path", 3), channel_field(0, "interpolation", 3),
            node_field(blade, "parent", blade), node_field(1, "parent", 5),         # a parent at or after its child
            node_field(blade, "modelInstance", tables.nodes[bob].modelInstance),    # bound twice
            node_field(camera, "pointLight", 0), node_field(camera, "spotLight", 0),
            node_field(blade, "flags", S.NODE_CAMERA),                              # a second camera
            channel_field(0, "keyCount", 0),
            channel_field(rotation, "valueWidth", 3), channel_field(translation, "valueWidth", 4),
            channel_field(0, "timeOffset", tables.times.size), channel_field(0, "keyCount", tables.times.size + 1),
            channel_field(len(tables.channels) - 1, "valueOffset", tables.values.size - 1)):  # offsets past the arrays
        refused(ctx, broken(change))

    def decreasing(t):
        ch = t.channels[1]
        assert ch.keyCount >= 3
        t.times[ch.timeOffset + 2] = t.times[ch.timeOffset + 1] - np.float32(0.125)
    assert "decrease" in refused(ctx, broken(decreasing))
    desc = tables.desc()
    desc.struct_size -= 4
    assert lib.prosper_pt_set_animations(ctx._h, C.byref(desc)) == -1 and b"struct_size" in lib.prosper_pt_last_error()
    assert ctx.animation_state().nodeCount == 0  # nothing of the refused tables was kept

    ctx.set_animations(tables)
    st = ctx.animation_state()
    assert (st.nodeCount, st.animatedNodeCount, st.updates, st.cameraValid) == (12, 11, 0, 0) and st.endTimeS == 2.5
    assert lib.prosper_pt_animate(ctx._h, 0.5, 2, None) == -1 and b"unknown flag" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_animate(ctx._h, float("nan"), 0, None) == -1
    ctx.animate(0.5)
    assert ctx.animation_state().updates == 1
    ctx.upload_scene(world)  # a new scene forgets the animations
    assert ctx.animation_state().nodeCount == 0
    with pytest.raises(capi.ProsperPtError):
        ctx.animate(0.5)
