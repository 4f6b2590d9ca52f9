"""The ray-traced G-buffer (prosper_pt_trace_gbuffer, gbuffer_trace_kernel) and the ReSTIR-DI record that traces it
first (PROSPER_PT_RESTIR_TRACE_GBUFFER): the C-ABI surface on the CPU, and with -m gpu the G-buffer against the path
tracer's own primary hits, the debug draw types end to end, the record against host inputs and the oracle's trace,
pixel-centre mode against the oracle's traversal, queued scene updates, and the host mirror."""
import ctypes as C

import numpy as np
import pytest

import restir_resampling_reference as R
from conftest import default_pc, same_bits
from prosper_amd import capi, flight_helmet, scenes, structs as S

FLAG_SKIP_HISTORY, FLAG_ACCUMULATE = 1, 2
W, H = 128, 96
NEW_SYMBOLS = ("prosper_pt_trace_gbuffer", "prosper_pt_get_gbuffer_device_ptrs", "prosper_pt_read_gbuffer",
               "prosper_host_gbuffer_tracer_create", "prosper_host_gbuffer_tracer_destroy",
               "prosper_host_gbuffer_tracer_record")
DEBUG_VIEWS = ("PrimitiveID", "MeshID", "MaterialID", "ShadingNormal", "TexCoord0", "Albedo", "Roughness", "Metallic")


def make_world(scene):
    if scene == "cornell":
        return scenes.cornell()
    if scene == "sponza":
        return scenes.sponza_class(lights=True, foliage=True, texture_size=64, sky_size=32, detail=0.25)
    return flight_helmet.load_fixture(sky_size=0)


def camera(oracle, world, w=W, h=H):
    c = world.camera
    return oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)


def mat(m):
    """A CameraUniforms mat4 as a float64 row-major matrix."""
    return np.frombuffer(bytes(m), np.float32).reshape(4, 4).T.astype(np.float64)


def signed_oct_decode(nm):
    """scene/material.glsl:20-32 in float64 over the (x, y, w) of normalMetallic."""
    x, y, z = (nm[..., k].astype(np.float64) for k in (0, 1, 3))
    o = np.stack([x - y, (x + y) - 1.0, (z * 2.0 - 1.0)], axis=-1)
    o[..., 2] *= (1.0 - np.abs(o[..., 0])) - np.abs(o[..., 1])
    return o / np.linalg.norm(o, axis=-1, keepdims=True)


def project(cam, pos):
    """clip.z / clip.w of cameraToClip * worldToCamera * (pos, 1) in float64."""
    clip = np.concatenate([pos, np.ones(pos.shape[:-1] + (1,))], axis=-1) @ (mat(cam.cameraToClip) @ mat(cam.worldToCamera)).T
    with np.errstate(all="ignore"):
        return clip[..., 2] / clip[..., 3]


def linearize(cam, depth):
    c2c = mat(cam.cameraToClip)
    with np.errstate(all="ignore"):
        return -c2c[2, 3] / (depth.astype(np.float64) + c2c[2, 2])


def pcg(v):
    """random.glsl:7-12 on uint32 arrays."""
    v = np.asarray(v, np.uint32)
    state = v * np.uint32(747796405) + np.uint32(2891336453)
    word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
    return (word >> np.uint32(22)) ^ word


def uint_to_color(v):
    """debug.glsl uintToColor on uint32 arrays."""
    x = pcg(v)
    k = np.float32(1.0 / 1023.0)
    return np.stack([((x >> np.uint32(s)) & np.uint32(0x3FF)).astype(np.float32) * k for s in (20, 10, 0)], axis=-1)


def check_against_views(gb, cam, views, what):
    """The G-buffer (ar, nm, depth) against the debug views of the same frame (name -> [h, w, 4])."""
    ar, nm, depth = gb
    hit = views["ShadingNormal"][..., :3].sum(axis=-1) > 0.0
    assert 0.1 < hit.mean(), what
    assert (depth != 0.0).sum() == hit.sum() and (depth[hit] != 0.0).all(), what
    assert (ar[~hit] == 0).all() and (nm[~hit] == 0).all() and (depth[~hit] == 0).all(), what
    assert same_bits(ar[..., :3], views["Albedo"][..., :3]).all(), what
    assert same_bits(ar[..., 3][hit], views["Roughness"][..., 0][hit]).all(), what
    assert same_bits(nm[..., 2][hit], views["Metallic"][..., 0][hit]).all(), what
    n = signed_oct_decode(nm[hit])
    want_n = views["ShadingNormal"][..., :3][hit].astype(np.float64) * 2.0 - 1.0
    err = np.abs(n - want_n).max()
    assert err <= 2e-6, "%s: normal off by %.3g" % (what, err)
    # Depth: the kernel evaluates clip.z and clip.w of the fp32 hit position in fp32 (four fmas each, worldToClip rounded
    # once from the float64 product) and divides once: a few ulp of each, i.e. ~1e-7 relative to clip.w, which bounds
    # the absolute error of z / w (|z| <= |w| on visible points) well under 1e-6.  Linearised, the error is that of
    # depth over (depth + cameraToClip22) = cameraToClip32 / distance, again a few ulp relative: 1e-4 leaves room.
    pos = views["Position"][..., :3][hit].astype(np.float64)
    want_d = project(cam, pos)
    derr = np.abs(depth[hit].astype(np.float64) - want_d).max()
    assert derr <= 1e-6, "%s: depth off by %.3g" % (what, derr)
    lin, want_lin = linearize(cam, depth[hit]), linearize(cam, want_d)
    rel = (np.abs(lin - want_lin) / np.abs(want_lin)).max()
    assert rel <= 1e-4, "%s: linear depth off by %.3g relative" % (what, rel)
    return hit


def check_reservoirs(got, want_i, want_w, margin, mask):
    """Per-pixel decision margins (tests/restir_resampling_reference.py) on `mask`."""
    idx = np.ascontiguousarray(got[..., 0]).view(np.int32)
    decided = (margin >= 1e-4) & mask
    assert decided.sum() >= 0.99 * mask.sum()
    bad = decided & (idx != want_i)
    assert bad.sum() <= 0.001 * mask.sum(), "%d decided pixels pick another light" % bad.sum()
    same = decided & (idx == want_i)
    with np.errstate(all="ignore"):
        rel = np.abs(got[..., 1].astype(np.float64) - want_w) / np.maximum(np.abs(want_w), 1e-30)
    wrong = same & (rel > 1e-4)
    assert not wrong.any(), "%d pixels: W off by up to %.3g" % (wrong.sum(), rel[wrong].max())


# ---- CPU ----

def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    assert (S.GBUFFER_JITTER, S.RESTIR_TRACE_GBUFFER, S.RESTIR_JITTER_GBUFFER) == (1, 2, 4)
    assert S.RESTIR_SPATIAL_REUSE == 1 and C.sizeof(S.GBufferTargets) == 24


def test_bad_arguments_are_rejected_before_touching_the_gpu():
    lib = capi.lib()
    cam = S.CameraUniforms()

    def refused(rc, words):
        msg = lib.prosper_pt_last_error().decode()
        return rc == -1 and words in msg

    assert refused(lib.prosper_pt_trace_gbuffer(None, 0, 1, 1, C.byref(cam), 4, 4, None, None), "null argument")
    assert refused(lib.prosper_pt_trace_gbuffer(None, 0, 1, 1, None, 4, 4, None, None), "null argument")
    assert refused(lib.prosper_pt_trace_gbuffer(None, 0, 1, 1, C.byref(cam), 0, 4, None, None), "empty extent")
    assert refused(lib.prosper_pt_trace_gbuffer(None, 0, 1, 1, C.byref(cam), 4, 0, None, None), "empty extent")
    assert refused(lib.prosper_pt_trace_gbuffer(None, 0, 1, 2, C.byref(cam), 4, 4, None, None), "unknown flags")
    assert refused(lib.prosper_pt_trace_gbuffer(None, len(S.DRAW_TYPES), 1, 1,
                                                C.byref(cam), 4, 4, None, None), "drawType out of range")
    pc = S.RestirTracePC(0, 1, 1)
    assert refused(lib.prosper_pt_restir_di_record(None, C.byref(pc), S.RESTIR_JITTER_GBUFFER, C.byref(cam), 4, 4, None,
                                                   None), "without TRACE_GBUFFER")
    assert refused(lib.prosper_pt_restir_di_record(None, C.byref(pc), S.RESTIR_TRACE_GBUFFER | 8, C.byref(cam), 4, 4,
                                                   None, None), "")
    assert refused(lib.prosper_pt_restir_di_record(None, C.byref(pc), S.RESTIR_TRACE_GBUFFER, C.byref(cam), 4, 4, None,
                                                   None), "null argument")
    inp, w, h = S.RestirInputs(), C.c_uint32(), C.c_uint32()
    assert refused(lib.prosper_pt_get_gbuffer_device_ptrs(None, C.byref(inp), C.byref(w), C.byref(h)), "null argument")
    assert refused(lib.prosper_pt_read_gbuffer(None, None, None, None, 16, None), "null argument")
    t = C.c_void_p()
    assert lib.prosper_host_gbuffer_tracer_create(None, C.byref(t)) == -1 and not t.value


# ---- GPU ----

def _views(render, names):
    return {name: render(name) for name in names}


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "sponza", "flight_helmet"])
def test_gpu_jittered_gbuffer_is_the_path_tracers_primary_hit(gpu_ctx, oracle, scene):
    world = make_world(scene)
    cam, fl = camera(oracle, world)
    gpu_ctx.upload_scene(world)
    osc = oracle.OracleScene(world, brute_force=scene == "cornell")
    try:
        for frame in (1, 2, 3):
            views = _views(lambda name: osc.render(default_pc(S, fl, frame_index=frame, draw_type=S.DrawType[name],
                                                              max_bounces=1), cam, W, H)[0],
                           ("Position", "ShadingNormal", "Albedo", "Roughness", "Metallic"))
            gb = gpu_ctx.trace_gbuffer(cam, W, H, frame_index=frame, jitter=True)
            check_against_views(gb, cam, views, "%s frame %d" % (scene, frame))
    finally:
        osc.close()


@pytest.mark.gpu
def test_gpu_jittered_gbuffer_full_size_flight_helmet(gpu_ctx, oracle):
    """1920x1080 (the bench's size) against the GPU's own debug views of the same frame."""
    world = make_world("flight_helmet")
    w, h = 1920, 1080
    cam, fl = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)

    def render(name):
        gpu_ctx.render(default_pc(S, fl, frame_index=7, draw_type=S.DrawType[name], max_bounces=1), cam, w, h)
        return gpu_ctx.read_hdr()
    views = _views(render, ("Position", "ShadingNormal", "Albedo", "Roughness", "Metallic"))
    gb = gpu_ctx.trace_gbuffer(cam, w, h, frame_index=7, jitter=True)
    check_against_views(gb, cam, views, "flight_helmet 1920x1080")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "sponza", "flight_helmet"])
def test_gpu_debug_draw_types_end_to_end(gpu_ctx, oracle, scene):
    """record(TRACE | JITTER, drawType X) writes what prosper_pt_render(drawType X) writes at the same frame."""
    world = make_world(scene)
    cam, fl = camera(oracle, world)
    gpu_ctx.upload_scene(world)
    for name in DEBUG_VIEWS:
        gpu_ctx.render(default_pc(S, fl, frame_index=5, draw_type=S.DrawType[name], max_bounces=1), cam, W, H)
        want = gpu_ctx.read_hdr()
        gpu_ctx.restir_di_record_traced(S.RestirTracePC(S.DrawType[name], 5, FLAG_SKIP_HISTORY), cam, W, H)
        got = gpu_ctx.read_hdr()
        ok = same_bits(got, want).all(axis=2)
        assert ok.all(), "%s %s: %d pixels differ" % (scene, name, (~ok).sum())
        assert (got[..., 3] == 1.0).all()
        if name in ("PrimitiveID", "MaterialID", "ShadingNormal"):  # (the others may be black on a whole scene)
            assert (got[..., :3].sum(axis=2) > 0).mean() > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "sponza"])
def test_gpu_record_from_the_traced_gbuffer(gpu_ctx, oracle, scene):
    """Three accumulating frames of record(TRACE | JITTER): the HDR bit for bit what a record over the read-back
    G-buffers as host inputs makes, and what the oracle's trace makes of them and the reservoirs the record traced with;
    the reservoirs within the resampling reference's decision margins."""
    world = make_world(scene)
    cam, fl = camera(oracle, world)
    gpu_ctx.upload_scene(world)
    osc = oracle.OracleScene(world, brute_force=scene == "cornell")
    lights = R.Lights(world).count
    frames = ((1, FLAG_SKIP_HISTORY | FLAG_ACCUMULATE), (2, FLAG_ACCUMULATE), (3, FLAG_ACCUMULATE))
    try:
        for spatial in (True, False):
            gbs, recorded, want = [], [], None
            for frame, flags in frames:
                pc = S.RestirTracePC(0, frame, flags)
                gpu_ctx.restir_di_record_traced(pc, cam, W, H, spatial_reuse=spatial)
                gb = gpu_ctx.read_gbuffer()
                res = gpu_ctx.read_restir_reservoirs()
                gbs.append(gb)
                recorded.append(res)
                want = osc.restir_di_trace((0, frame, flags), cam, *gb, res, history=want)
            got = gpu_ctx.read_hdr()
            ok = same_bits(got, want).all(axis=2)
            assert ok.all(), "spatial=%s: %d pixels differ from the oracle's trace" % (spatial, (~ok).sum())
            assert (got[..., :3].sum(axis=2) > 0).mean() > 0.01
            assert not np.array_equal(gbs[0][2], gbs[1][2])  # the jitter moves with the frame index
            for (frame, flags), gb in zip(frames, gbs):
                gpu_ctx.restir_di_record(S.RestirTracePC(0, frame, flags), cam, *gb, spatial_reuse=spatial)
            assert same_bits(gpu_ctx.read_hdr(), got).all()
            for (frame, _), gb, res in zip(frames, gbs, recorded):
                ar, nm, depth = gb
                hit = depth != 0
                idx = np.ascontiguousarray(res[..., 0]).view(np.int32)
                assert ((idx >= -1) & (idx < lights)).all()
                ref_i, ref_w, ref_m = R.initial(world, cam, ar, nm, depth, frame)
                if not spatial:
                    check_reservoirs(res, ref_i, ref_w, ref_m, hit)
                else:  # fed the reference's initial reservoirs: a neighbour's undecided pick may differ
                    init = gpu_ctx.restir_di_resample(S.RESTIR_INITIAL, frame, cam, ar, nm, depth)
                    check_reservoirs(init, ref_i, ref_w, ref_m, hit)
                    ref_res = np.stack([ref_i.view(np.float32), ref_w.astype(np.float32)], axis=-1)
                    sp_i, sp_w, sp_m, _ = R.spatial(world, cam, ar, nm, depth, ref_res, frame, oracle)
                    decided = (sp_m >= 1e-4) & hit
                    assert decided.sum() >= 0.99 * hit.sum() and (idx[decided] == sp_i[decided]).mean() >= 0.99
    finally:
        osc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "sponza"])
def test_gpu_pixel_centre_mode(gpu_ctx, oracle, scene):
    """Without jitter the rays go through the pixel centres: the oracle's traversal of float64 centre rays agrees on
    the hit and the material wherever they are uniform over the 3x3 neighbourhood, the Position view lies on the centre
    ray, and the stored depth reconstructs that point at uv = (px + 0.5) / size."""
    world = make_world(scene)
    cam, fl = camera(oracle, world)
    gpu_ctx.upload_scene(world)
    w2c, c2c = mat(cam.worldToCamera), mat(cam.cameraToClip)
    eye = np.array([cam.eye.x, cam.eye.y, cam.eye.z], np.float64)
    right, up, fwd = w2c[0, :3], w2c[1, :3], -w2c[2, :3]
    tan_half, aspect = 1.0 / c2c[1, 1], c2c[1, 1] / c2c[0, 0]
    py, px = np.mgrid[0:H, 0:W]
    ndx, ndy = (px + 0.5) / W * 2.0 - 1.0, (py + 0.5) / H * 2.0 - 1.0
    d = ndx[..., None] * (right * tan_half * aspect) + ndy[..., None] * (up * tan_half) + fwd
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    # the any-hit seed of the kernel: pcg(x ^ z) of the rng after the jitter draw (made in both modes)
    rng = R.Rng(px.ravel(), py.ravel(), 3)
    rng.rnd2d01()
    seed = pcg(rng.s[0] ^ rng.s[2]).reshape(H, W)
    osc = oracle.OracleScene(world, brute_force=scene == "cornell")
    draw_material = np.array([di.materialIndex for di in world.freeze()["draw_instances"]], np.int64)
    try:
        instance = np.full((H, W), -1, np.int64)
        for y in range(H):
            for x in range(W):
                hit, di, _, _ = osc.trace_closest(eye, d[y, x], seed=int(seed[y, x]))
                if hit:
                    instance[y, x] = di
    finally:
        osc.close()
    material = np.where(instance >= 0, draw_material[np.maximum(instance, 0)], -1)
    uniform = np.ones((H, W), bool)
    for a in (instance, material):
        pad = np.pad(a, 1, mode="edge")
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                uniform &= pad[dy:dy + H, dx:dx + W] == a
    assert uniform.mean() > 0.25  # (the atrium at 128x96: many small instances)
    ar, nm, depth = gpu_ctx.trace_gbuffer(cam, W, H, frame_index=3, jitter=False)
    hit = depth != 0
    assert (hit[uniform] == (material[uniform] >= 0)).all()
    mid, _, _ = gpu_ctx.trace_gbuffer(cam, W, H, draw_type=S.DrawType["MaterialID"], frame_index=3, jitter=False)
    on = uniform & (material >= 0)
    agree = same_bits(mid[..., :3][on], uint_to_color(material[on])).all(axis=-1)
    assert agree.all(), "%d of %d uniform pixels hit another material" % ((~agree).sum(), agree.size)
    pos, _, pdepth = gpu_ctx.trace_gbuffer(cam, W, H, draw_type=S.DrawType["Position"], frame_index=3, jitter=False)
    assert same_bits(pdepth, depth).all()  # the depth does not depend on the draw type
    # the Position view lies on the float64 centre ray ...
    v = pos[..., :3][on].astype(np.float64) - eye
    dist = np.linalg.norm(v, axis=-1)
    assert np.abs(v / dist[:, None] - d[on]).max() <= 1e-5
    # ... and the depth reconstructs it there (clipToWorld at the pixel centre, camera.glsl:27-33 in float64)
    ndc = np.stack([ndx[on], ndy[on], depth[on].astype(np.float64), np.ones(on.sum())], axis=-1)
    p = ndc @ mat(cam.clipToWorld).T
    p = p[:, :3] / p[:, 3:4]
    q = p - eye
    assert np.abs(q / np.linalg.norm(q, axis=-1, keepdims=True) - d[on]).max() <= 1e-5
    assert (np.abs(np.linalg.norm(q, axis=-1) - dist) / dist).max() <= 1e-4
    # a jittered G-buffer of the same frame puts its depth elsewhere on most pixels
    _, _, jdepth = gpu_ctx.trace_gbuffer(cam, W, H, frame_index=3, jitter=True)
    assert (jdepth[on] != depth[on]).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("change", ["transforms", "lights"])
def test_gpu_queued_updates_reach_the_traced_gbuffer(gpu_ctx, oracle, change):
    """An update staged with no sync before record(TRACE): the G-buffer it leaves equals trace_gbuffer on a fresh upload
    of the changed scene, the HDR that upload's record."""
    from prosper_amd.world import translate
    world = make_world("cornell") if change == "transforms" else make_world("sponza")
    changed = make_world("cornell") if change == "transforms" else make_world("sponza")
    if change == "transforms":
        model, m = changed.model_instances[-1]
        changed.model_instances[-1] = (model, translate((0.08, 0.0, -0.05)) @ m)
    else:
        changed.point_lights.count = 8
    cam, fl = camera(oracle, world)
    pc = S.RestirTracePC(0, 2, FLAG_SKIP_HISTORY)
    gpu_ctx.upload_scene(world)
    gpu_ctx.restir_di_record_traced(pc, cam, W, H)
    before = gpu_ctx.read_gbuffer()
    if change == "transforms":
        gpu_ctx.update_transforms(changed)  # staged: the refit runs at the head of the next call
    else:
        gpu_ctx.update_lights(changed)
    gpu_ctx.restir_di_record_traced(pc, cam, W, H)
    got_gb, got = gpu_ctx.read_gbuffer(), gpu_ctx.read_hdr()
    fresh = capi.Context(0)
    try:
        fresh.upload_scene(changed)
        want_gb = fresh.trace_gbuffer(cam, W, H, frame_index=2, jitter=True)
        fresh.restir_di_record_traced(pc, cam, W, H)
        want = fresh.read_hdr()
    finally:
        fresh.close()
    for a, b in zip(got_gb, want_gb):
        assert same_bits(a, b).all()
    assert same_bits(got, want).all()
    if change == "transforms":
        assert not np.array_equal(before[2], got_gb[2])


@pytest.mark.gpu
def test_gpu_host_mirror_equals_the_traced_record(oracle):
    """render::GBufferTracer + render::rtdi::RtDirectIllumination through the C shims against
    prosper_pt_restir_di_record(TRACE | JITTER) with the TracePC they pushed: the same image and G-buffer bit for bit."""
    from prosper_amd.rt_reference import Camera, GBufferTracer, RtDirectIllumination
    world = make_world("cornell")
    host_ctx, abi_ctx = capi.Context(0), capi.Context(0)
    try:
        host_ctx.upload_scene(world)
        abi_ctx.upload_scene(world)
        cam_h = Camera.from_world(world, W, H)
        cam, _ = cam_h.update_buffer()
        tracer, pass_ = GBufferTracer(host_ctx), RtDirectIllumination(host_ctx)
        for frame in (1, 2, 3, 4):
            if frame == 3:
                pass_.draw_ui(spatial_reuse=False)
            gb = tracer.record(cam_h, W, H, frame_index=frame, jitter=True)
            assert gb.onDevice == 1
            pc = pass_.record_device(cam_h, gb, W, H)
            assert pc.frameIndex == frame
            abi_ctx.restir_di_record_traced(pc, cam, W, H, spatial_reuse=frame < 3)
            assert same_bits(host_ctx.read_hdr(), abi_ctx.read_hdr()).all()
            for a, b in zip(host_ctx.read_gbuffer(), abi_ctx.read_gbuffer()):
                assert same_bits(a, b).all()
        tracer.close()
        pass_.close()
    finally:
        host_ctx.close()
        abi_ctx.close()
