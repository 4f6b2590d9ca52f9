"""The traced G-buffer with a velocity target (prosper_pt_trace_gbuffer_velocity), on the small
synthetic scenes the traced-G-buffer tests use.

Exact: with zero jitter the three targets are prosper_pt_trace_gbuffer's without jitter, and a static camera, unmoved
instances and equal jitters give velocity (0, 0) on hits and on the sky.  The float64 comparisons restate
(posNDC - currentJitter) - (prevPosNDC - previousJitter), y negated, clamped, from the Position view of the same call,
which is the kernel's own float32 positionWS.  Their allowance is n * 2^-24 * S:
  S   the sum of absolute terms of the value: for each of the two projections, with |C| |M| |p| the product of the
      absolute matrices and the absolute point, (|C| |M| |p|).x / |w| + |x / w| (|C| |M| |p|).w / |w| (the numerator's
      products over |w|, and the denominator's scaled as they enter the quotient), plus |currentJitter| + |previousJitter|
  n   the float32 roundings of the chain as implemented (project_ndc and ndc_velocity, pt_gbuffer_kernels.hip), counted:
      worldToCamera row: 3 fma; cameraToClip row: 1 mul + 3 fma; numerator 7, denominator 7, division 1 = 15; the two
      jitter subtractions and the difference: 3.  n = 18 on hits whose previous position is the position itself.
      A moved instance: the test takes prevM curM^-1 positionWS from the float32 positionWS, which carries the 3 fma of
      the current transform, and the kernel's previous transform has 3 more; through a rigid map a vector's error spreads
      over its components (a factor below 2 on the largest), so 12 more, taken of |p| = the sum of the position's
      absolute terms on every axis: n = 30.  The sky: the test forms the ray's direction in float64, the kernel in
      float32 (uv 2 + jitter shift 2, ndc 1, the two scaled axes 3 + 2 in parallel, sum 2, normalise 6: 16): n = 34."""
import ctypes as C

import numpy as np
import pytest

from conftest import same_bits
from prosper_amd import capi, flight_helmet, structs as S
from test_traced_gbuffer import camera, make_world, mat, uint_to_color

W, H = 128, 96
EPS = 2.0 ** -24
N_HIT, N_MOVED, N_SKY = 18, 30, 34
NEW_SYMBOLS = ("prosper_pt_trace_gbuffer_velocity", "prosper_pt_get_velocity_device_ptr", "prosper_pt_read_velocity",
               "prosper_host_gbuffer_tracer_record_velocity")


def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    assert C.sizeof(S.VelocityGBufferDesc) == 48


def test_bad_arguments_are_rejected_before_touching_the_gpu():
    lib = capi.lib()
    cam = S.CameraUniforms()

    def refused(words, flags=0, camera=cam, w=4, h=4, desc=S.VelocityGBufferDesc(), draw_type=0):
        rc = lib.prosper_pt_trace_gbuffer_velocity(None, draw_type, 1, flags, None if camera is None else C.byref(camera), w, h,
                                                   None if desc is None else C.byref(desc), None)
        return rc == -1 and words in lib.prosper_pt_last_error().decode()

    assert refused("null argument")  # only the context is missing
    assert refused("null argument", camera=None) and refused("null argument", desc=None)
    assert refused("unknown flags", flags=1) and refused("unknown flags", flags=2)
    assert refused("empty extent", w=0) and refused("empty extent", h=0)
    assert refused("drawType out of range", draw_type=len(S.DRAW_TYPES))
    for given in ((64, 0, 0), (64, 128, 0), (0, 128, 256), (64, 0, 256)):  # a partly given target set
        assert refused("together or not at all", desc=S.VelocityGBufferDesc(S.GBufferTargets(*[g or None for g in given]), None, None, 0))
    assert refused("16-byte aligned", desc=S.VelocityGBufferDesc(S.GBufferTargets(64, 128, 260), None, None, 0))
    assert refused("8-byte aligned", desc=S.VelocityGBufferDesc(S.GBufferTargets(), 68, None, 0))
    assert refused("without previousTransforms", desc=S.VelocityGBufferDesc(S.GBufferTargets(), None, None, 5))
    p, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
    assert lib.prosper_pt_get_velocity_device_ptr(None, C.byref(p), C.byref(w), C.byref(h)) == -1
    assert lib.prosper_pt_read_velocity(None, None, 16, None) == -1


# ---- the float64 restatement ----

def still(cam):
    """`cam` with the previous matrices and jitter equal to the current ones."""
    out = S.CameraUniforms.from_buffer_copy(bytes(cam))
    out.previousWorldToCamera = cam.worldToCamera
    out.previousCameraToClip = cam.cameraToClip
    out.previousJitter[0], out.previousJitter[1] = cam.currentJitter[0], cam.currentJitter[1]
    return out


def project(c2c, w2c, p, direction=False):
    """(ndc xy, S) of the points p [n, 3]: the projection in float64 and its sum of absolute terms per axis."""
    c, m = mat(c2c), mat(w2c)
    if direction:
        m = m.copy()
        m[:3, 3] = 0.0
        m[3] = (0.0, 0.0, 0.0, 1.0)
    p4 = np.concatenate([p, np.ones((len(p), 1))], axis=-1)
    clip = p4 @ (c @ m).T
    absolute = np.abs(p4) @ (np.abs(c) @ np.abs(m)).T
    with np.errstate(all="ignore"):
        ndc = clip[:, :2] / clip[:, 3:4]
        s = absolute[:, :2] / np.abs(clip[:, 3:4]) + np.abs(ndc) * absolute[:, 3:4] / np.abs(clip[:, 3:4])
    return ndc, s


def velocity_of(cam, p, prev_p, direction=False):
    """(the unclamped velocity [n, 2], S [n, 2]) of gbuffer.frag:74-82 / skybox.frag:20-29 in float64."""
    cj, pj = np.array(cam.currentJitter[:], np.float64), np.array(cam.previousJitter[:], np.float64)
    pos, s0 = project(cam.cameraToClip, cam.worldToCamera, p, direction)
    prev, s1 = project(cam.previousCameraToClip, cam.previousWorldToCamera, prev_p, direction)
    v = (pos - cj) - (prev - pj)
    v[:, 1] = -v[:, 1]
    return v, s0 + s1 + np.abs(cj) + np.abs(pj)


def ray_directions(cam, w, h):
    """The primary rays of the velocity pass in float64: through uv = (px + .5) / res - currentJitter / 2."""
    w2c, c2c = mat(cam.worldToCamera), mat(cam.cameraToClip)
    right, up, fwd = w2c[0, :3], w2c[1, :3], -w2c[2, :3]
    tan_half, aspect = 1.0 / c2c[1, 1], c2c[1, 1] / c2c[0, 0]
    py, px = np.mgrid[0:h, 0:w]
    u = (px + 0.5) / w - cam.currentJitter[0] * 0.5
    v = (py + 0.5) / h - cam.currentJitter[1] * 0.5
    d = (u * 2.0 - 1.0)[..., None] * (right * tan_half * aspect) + (v * 2.0 - 1.0)[..., None] * (up * tan_half) + fwd
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def check_velocity(label, got, want, s, n):
    """Every texel: the clamped restatement within n * 2^-24 * S (a value the clamp holds at -1 or 1 exactly there)."""
    a = n * EPS * s
    lo, hi = np.clip(want - a, -1.0, 1.0), np.clip(want + a, -1.0, 1.0)
    g = got.astype(np.float64)
    err = np.maximum(lo - g, g - hi)
    with np.errstate(all="ignore"):
        share = np.abs(g - np.clip(want, -1.0, 1.0)) / a
    print("%s: worst error %.3f of the allowance over %d values, %d outside" % (label, float(np.nanmax(share)), g.size, (err > 0).sum()))
    assert np.isfinite(g).all() and (err <= 0).all(), label


def jittered_camera(world, w, h, frames):
    """The host camera of `world` with the jitter on, after `frames` frames: (host camera, uniforms)."""
    from prosper_amd.rt_reference import Camera
    hcam = Camera.from_world(world, w, h)
    hcam.set_jitter(True)
    for _ in range(frames):
        hcam.update_buffer()
        hcam.end_frame()
    return hcam, S.CameraUniforms.from_buffer_copy(bytes(hcam.update_buffer()[0]))


# ---- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "sponza", "flight_helmet"])
def test_gpu_zero_jitter_gives_the_plain_targets_and_no_velocity(gpu_ctx, oracle, scene):
    world = make_world(scene)
    cam = still(camera(oracle, world)[0])
    assert list(cam.currentJitter) == [0.0, 0.0]
    gpu_ctx.upload_scene(world)
    for draw_type in (0, S.DrawType["Position"]):
        want = gpu_ctx.trace_gbuffer(cam, W, H, draw_type=draw_type, frame_index=3, jitter=False)
        ar, nm, depth, velocity = gpu_ctx.trace_gbuffer_velocity(cam, W, H, draw_type=draw_type, frame_index=3)
        for a, b in zip((ar, nm, depth), want):
            assert a.tobytes() == b.tobytes()
        assert (depth != 0).any() and (scene != "flight_helmet" or (depth == 0).any())  # (the helmet stands before the sky)
        assert velocity.shape == (H, W, 2) and not velocity.any()  # hits and sky alike
    # the same jitter in both frames, and the current transforms given as the previous ones: still exactly zero
    jit = still(camera(oracle, world)[0])
    jit.currentJitter[0], jit.currentJitter[1] = capi.taa_jitter(1, W, H)
    jit = still(jit)
    velocity = gpu_ctx.trace_gbuffer_velocity(jit, W, H, frame_index=3, previous_transforms=world.freeze()["transforms"])[3]
    assert not velocity.any()
    # caller-owned buffers take the same bytes
    from test_depth_of_field import DeviceCopy
    want = gpu_ctx.trace_gbuffer(cam, W, H, frame_index=3, jitter=False)
    with DeviceCopy(np.zeros((H, W, 4), np.float32)) as a, DeviceCopy(np.zeros((H, W, 4), np.float32)) as n:
        with DeviceCopy(np.ones((H, W), np.float32)) as d, DeviceCopy(np.ones((H, W, 2), np.float32)) as v:
            assert gpu_ctx.trace_gbuffer_velocity(cam, W, H, frame_index=3, targets=(a, n, d), velocity_ptr=v) == (None,) * 4
            assert gpu_ctx.velocity_device_ptr() == (v, W, H)
            assert not gpu_ctx.read_velocity().any()
            for got, b in zip(gpu_ctx.read_gbuffer(), want):
                assert got.tobytes() == b.tobytes()
    # (the context's own buffers again, for whoever reads the last G-buffer next)
    gpu_ctx.trace_gbuffer_velocity(cam, W, H, frame_index=3)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "sponza"])
def test_gpu_the_jittered_projection_puts_every_hit_on_its_pixel_centre(gpu_ctx, scene):
    world = make_world(scene)
    gpu_ctx.upload_scene(world)
    for frames in (1, 2, 5):
        hcam, cam = jittered_camera(world, W, H, frames)
        jitter = np.array(cam.currentJitter[:], np.float64)
        assert jitter.all()
        pos, _, depth, _ = gpu_ctx.trace_gbuffer_velocity(cam, W, H, draw_type=S.DrawType["Position"], frame_index=3)
        hit = depth != 0
        ndc, _ = project(cam.cameraToClip, cam.worldToCamera, pos[..., :3][hit].astype(np.float64))
        py, px = np.mgrid[0:H, 0:W]
        centre = np.stack([(px[hit] + 0.5) / W * 2.0 - 1.0, (py[hit] + 0.5) / H * 2.0 - 1.0], axis=-1)
        # the bound of tests/test_traced_gbuffer.py's pixel-centre test, 1e-5 on the unit direction, in NDC: d ndc =
        # (tf + ndc^2 / tf) d angle, with tf the projection's scale on that axis
        c2c = mat(cam.cameraToClip)
        tf = np.array([abs(c2c[0, 0]), abs(c2c[1, 1])])
        bound = 1e-5 * (tf + centre * centre / tf)
        err = np.abs(ndc - centre)
        print("%s frame %d: worst offset %.3f of the bound, %.2e of the jitter" % (scene, frames, (err / bound).max(), (err / np.abs(jitter)).max()))
        assert (err <= bound).all()
        assert (bound < 0.05 * np.abs(jitter)).all()  # the other sign, or no shift, would miss by one or two jitters
        hcam.close()


@pytest.mark.gpu
def test_gpu_a_moved_and_turned_previous_camera(gpu_ctx, oracle):
    world = make_world("flight_helmet")  # hits and sky
    gpu_ctx.upload_scene(world)
    c = world.camera
    cam = S.CameraUniforms.from_buffer_copy(bytes(camera(oracle, world)[0]))
    eye, target = np.array(c["eye"], np.float64), np.array(c["target"], np.float64)
    for label, shift, turn, clamps in (("small", (0.05, -0.02, 0.03), (0.04, 0.01, 0.0), False), ("large", (0.3, 0.1, -0.2), (2.5, 0.8, 0.5), True)):
        before = oracle.camera_uniforms(tuple(eye + shift), tuple(target + turn), c["up"], c["fov"] * 1.02, c["zN"], c["zF"], W, H)[0]
        cam.previousWorldToCamera = before.worldToCamera
        cam.previousCameraToClip = before.cameraToClip
        cam.currentJitter[0], cam.currentJitter[1] = capi.taa_jitter(3, W, H)
        cam.previousJitter[0], cam.previousJitter[1] = capi.taa_jitter(2, W, H)
        pos, _, depth, velocity = gpu_ctx.trace_gbuffer_velocity(cam, W, H, draw_type=S.DrawType["Position"], frame_index=3)
        hit = depth != 0
        assert hit.any() and (~hit).any()
        p = pos[..., :3][hit].astype(np.float64)
        want, s = velocity_of(cam, p, p)
        check_velocity("moved camera (%s), hits" % label, velocity[hit], want, s, N_HIT)
        d = ray_directions(cam, W, H)[~hit]
        want_sky, s_sky = velocity_of(cam, d, d, direction=True)
        check_velocity("moved camera (%s), sky" % label, velocity[~hit], want_sky, s_sky, N_SKY)
        assert np.abs(velocity).max() > 1e-3
        beyond = (np.abs(want) > 1.0 + N_HIT * EPS * s)
        beyond_sky = (np.abs(want_sky) > 1.0 + N_SKY * EPS * s_sky)
        if clamps:  # values that leave [-1, 1] are held at the bound exactly, on hits and on the sky
            assert beyond.any() and beyond_sky.any()
            assert (np.abs(velocity[hit][beyond]) == 1.0).all() and (np.abs(velocity[~hit][beyond_sky]) == 1.0).all()
            assert (np.sign(velocity[hit][beyond]) == np.sign(want[beyond])).all()
        else:
            assert not beyond.any()
        assert np.abs(velocity).max() <= 1.0


@pytest.mark.gpu
def test_gpu_one_instance_with_another_previous_transform(gpu_ctx, oracle):
    world = make_world("cornell")
    gpu_ctx.upload_scene(world)
    frozen = world.freeze()
    count = len(world.model_instances)
    moved = count - 1
    previous = (S.ModelInstanceTransforms * count).from_buffer_copy(bytes(frozen["transforms"]))
    current = np.frombuffer(bytes(frozen["transforms"][moved].modelToWorld), np.float32).reshape(3, 4).astype(np.float64)
    angle = 0.2
    turn = np.array([[np.cos(angle), 0.0, np.sin(angle)], [0.0, 1.0, 0.0], [-np.sin(angle), 0.0, np.cos(angle)]])
    before = np.concatenate([turn @ current[:, :3], (turn @ current[:, 3] + np.array([0.07, 0.02, -0.05]))[:, None]], axis=1).astype(np.float32)
    C.memmove(C.byref(previous[moved].modelToWorld), before.ctypes.data, 48)
    cam = still(camera(oracle, world)[0])
    pos, _, depth, velocity = gpu_ctx.trace_gbuffer_velocity(cam, W, H, draw_type=S.DrawType["Position"], frame_index=3,
                                                             previous_transforms=previous)
    mesh_id = gpu_ctx.trace_gbuffer_velocity(cam, W, H, draw_type=S.DrawType["MeshID"], frame_index=3, previous_transforms=previous)
    assert mesh_id[3].tobytes() == velocity.tobytes()  # the velocity does not depend on the draw type
    meshes = [d.meshIndex for d in frozen["draw_instances"][:frozen["draw_instance_count"]] if d.modelInstanceIndex == moved]
    others = [d.meshIndex for d in frozen["draw_instances"][:frozen["draw_instance_count"]] if d.modelInstanceIndex != moved]
    assert meshes and not set(meshes) & set(others)
    hit = depth != 0
    on = np.zeros((H, W), bool)
    for m in meshes:
        on |= same_bits(mesh_id[0][..., :3], np.broadcast_to(uint_to_color(np.array([m]))[0], (H, W, 3))).all(axis=-1)
    on &= hit
    assert on.sum() > 50 and (hit & ~on).sum() > 50
    assert not velocity[hit & ~on].any()  # the unmoved instances go through their own transform again: exactly zero
    p = pos[..., :3][on].astype(np.float64)
    cur4 = np.concatenate([current, [[0.0, 0.0, 0.0, 1.0]]])
    prev4 = np.concatenate([before.astype(np.float64), [[0.0, 0.0, 0.0, 1.0]]])
    p4 = np.concatenate([p, np.ones((len(p), 1))], axis=-1)
    prev_p = (p4 @ (prev4 @ np.linalg.inv(cur4)).T)[:, :3]
    want, _ = velocity_of(cam, p, prev_p)
    # S with the sum of the position's absolute terms on every axis (see the module's docstring)
    size = np.abs(np.concatenate([p, prev_p], axis=-1)).max(axis=-1, keepdims=True) * 3.0 + np.abs(current[:, 3]).sum() + np.abs(before[:, 3]).sum()
    _, s = velocity_of(cam, np.broadcast_to(size, p.shape), np.broadcast_to(size, p.shape))
    check_velocity("moved instance", velocity[on], want, s, N_MOVED)
    assert np.abs(velocity[on]).max() > 1e-2


@pytest.mark.gpu
def test_gpu_refusals_and_the_resolve_over_the_traced_targets(oracle):
    import taa_reference as R
    world = make_world("cornell")
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        cam = still(camera(oracle, world)[0])
        lib = capi.lib()
        illum = R.design(W, H, 0)[0]

        def refused(words, fn, code=-1):
            with pytest.raises(capi.ProsperPtError) as e:
                fn()
            assert e.value.code == code and words in str(e.value), str(e.value)

        # no velocity target yet: a resolve without a velocity has nothing to read
        with pytest.raises(capi.ProsperPtError) as e:
            ctx.taa_resolve(S.TaaPC.default(), W, H, None, None, illum)
        assert "no velocity target has been traced" in str(e.value)
        count = len(world.model_instances)
        short = (S.ModelInstanceTransforms * (count - 1))()
        refused("differs from the scene's modelInstanceCount", lambda: ctx.trace_gbuffer_velocity(cam, W, H, previous_transforms=short))
        desc = S.VelocityGBufferDesc()
        assert lib.prosper_pt_trace_gbuffer_velocity(ctx._h, 0, 1, 1, C.byref(cam), W, H, C.byref(desc), None) == -1
        assert "unknown flags" in lib.prosper_pt_last_error().decode()
        desc.targets.albedoRoughness = 4096
        assert lib.prosper_pt_trace_gbuffer_velocity(ctx._h, 0, 1, 0, C.byref(cam), W, H, C.byref(desc), None) == -1
        assert "together or not at all" in lib.prosper_pt_last_error().decode()
        with pytest.raises(capi.ProsperPtError):
            ctx.read_velocity()
        # traced targets feed the resolve: NULL velocity and NULL depth read what the trace left
        _, _, depth, velocity = ctx.trace_gbuffer_velocity(cam, W, H, frame_index=1)
        frames = [R.design(W, H, f)[0] for f in range(2)]
        for f in range(2):
            ctx.taa_resolve(S.TaaPC.default(), W, H, None, None, frames[f])
        got = ctx.read_taa_history(), ctx.read_hdr()
        ctx.taa_release_history()
        for f in range(2):
            ctx.taa_resolve(S.TaaPC.default(), W, H, velocity, depth, frames[f])
        assert got[0].tobytes() == ctx.read_taa_history().tobytes() and got[1].tobytes() == ctx.read_hdr().tobytes()
        refused("velocity target has another extent", lambda: ctx.taa_resolve(S.TaaPC.default(), 64, 48, None, None, np.zeros((48, 64, 4), np.float32)))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_flight_helmet_eight_jittered_frames():
    from prosper_amd.rt_reference import Camera, GBufferTracer, TemporalAntiAliasing
    w, h = 160, 96
    world = flight_helmet.load_fixture(sky_size=16)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)

        def shade(cam):
            g, _, _ = ctx.gbuffer_device_ptrs()
            ctx.deferred_shading_device(cam, w, h, g.albedoRoughness, g.normalMetallic, g.nonLinearDepth)
            ctx.skybox_fill(cam, w, h)

        plain = Camera.from_world(world, w, h)
        cam = plain.update_buffer()[0]
        ctx.trace_gbuffer_velocity(cam, w, h)
        shade(cam)
        single = ctx.read_hdr()
        depth = ctx.read_gbuffer()[2]
        plain.close()

        hcam = Camera.from_world(world, w, h)
        hcam.set_jitter(True)
        taa, tracer = TemporalAntiAliasing(ctx), GBufferTracer(ctx)
        transforms = world.freeze()["transforms"]
        jitters = []
        for frame in range(8):
            cam = hcam.update_buffer()[0]
            jitters.append(tuple(cam.currentJitter))
            cam = S.CameraUniforms.from_buffer_copy(bytes(cam))
            if frame in (1, 5):
                # nothing moved: the two projections differ by the jitters alone, which the velocity takes out again
                pos, _, d, velocity = ctx.trace_gbuffer_velocity(cam, w, h, draw_type=S.DrawType["Position"], frame_index=frame)
                on = d != 0
                p = pos[..., :3][on].astype(np.float64)
                want, s = velocity_of(cam, p, p)
                assert np.abs(want).max() < 1e-6
                check_velocity("flight helmet frame %d, hits" % frame, velocity[on], want, s, N_HIT)
                rays = ray_directions(cam, w, h)[~on]
                want, s = velocity_of(cam, rays, rays, direction=True)
                check_velocity("flight helmet frame %d, sky" % frame, velocity[~on], want, s, N_SKY)
            gbuffer, velocity_ptr = tracer.record_velocity(hcam, w, h, frame_index=frame, transforms=transforms)
            assert velocity_ptr == ctx.velocity_device_ptr()[0] and gbuffer.nonLinearDepth == ctx.gbuffer_device_ptrs()[0].nonLinearDepth
            if frame in (1, 5):  # the unmoved instances' own transforms as the previous frame's change nothing
                assert ctx.read_velocity().tobytes() == velocity.tobytes()
            shade(cam)
            taa.record(w, h)  # in place, over the traced velocity and depth
            assert ctx.taa_info().ignoredHistory == (1 if frame == 0 else 0)
            hcam.end_frame()
        assert len(set(jitters)) == 8
        result = ctx.read_hdr()
        taa.close()
        tracer.close()
        hcam.close()
        assert np.isfinite(result).all() and (result[..., 3] == 1).all()
        # the accumulated image differs from the single unjittered frame along silhouettes, and less elsewhere
        hit = depth != 0
        edge = np.zeros_like(hit)
        edge[:, 1:] |= hit[:, 1:] != hit[:, :-1]
        edge[:, :-1] |= hit[:, 1:] != hit[:, :-1]
        edge[1:] |= hit[1:] != hit[:-1]
        edge[:-1] |= hit[1:] != hit[:-1]
        diff = np.abs(result[..., :3].astype(np.float64) - single[..., :3]).sum(axis=-1) / (np.abs(single[..., :3]).sum(axis=-1) + 1e-3)
        inner = ~edge & ~np.roll(edge, 1, 0) & ~np.roll(edge, -1, 0) & ~np.roll(edge, 1, 1) & ~np.roll(edge, -1, 1)
        print("flight helmet: %d silhouette texels, mean relative change %.4f there, %.4f elsewhere" % (edge.sum(), diff[edge].mean(), diff[inner].mean()))
        assert edge.sum() > 100 and (diff[edge] > 0.01).mean() > 0.25 and diff[edge].mean() > 2.0 * diff[inner].mean()
    finally:
        ctx.close()
