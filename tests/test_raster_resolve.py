"""The resolve of the rasteriser's visibility image on the GPU (prosper_pt_raster_resolve, prosper_pt_raster_gbuffer;
raster_resolve_kernel): against the traced G-buffer at the pixels where both name the same triangle, the
mesh shader's draw types, the four targets after both culling phases against the unculled draw, and the plumbing."""
import ctypes as C

import numpy as np
import pytest

import culling_reference as CR
import culling_scenes as CS
import raster_reference as R
import raster_scenes as RS
from prosper_amd import capi, flight_helmet, structs as S
from prosper_amd import world as W

pytestmark = pytest.mark.gpu

F = np.float32
W_, H_ = CS.WIDTH, CS.HEIGHT


def jittered_camera(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), width=W_, height=H_, frames=3, step=(0.05, 0.02, 0.0)):
    """a host camera with TAA jitter on, a few frames in: non-zero currentJitter, previous matrices of another view"""
    from prosper_amd import rt_reference
    cam = rt_reference.Camera()
    cam.set_parameters(CS.FOV, CS.NEAR, CS.FAR)
    cam.update_resolution(width, height)
    cam.set_jitter(True)
    u = None
    for k in range(frames):
        e = tuple(a + k * s for a, s in zip(eye, step))
        t = tuple(a + k * s for a, s in zip(target, step))
        cam.look_at(e, t, (0.0, 1.0, 0.0))
        u = S.CameraUniforms.from_buffer_copy(bytes(cam.update_buffer()[0]))
        cam.end_frame()
    cam.close()
    assert any(u.currentJitter[:]) and bytes(u.previousWorldToCamera) != bytes(u.worldToCamera)
    return u


def uint_to_color(v):
    v = np.asarray(v, np.uint64)
    state = (v * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    xr = (word >> np.uint64(22)) ^ word
    k = F(1.0) / F(1023.0)
    return np.stack([((xr >> np.uint64(20)) & np.uint64(0x3FF)).astype(F) * k, ((xr >> np.uint64(10)) & np.uint64(0x3FF)).astype(F) * k,
                     (xr & np.uint64(0x3FF)).astype(F) * k], axis=-1)


def previous_of(world):
    """the scene's transforms with every instance moved a little: a ctypes array for previousTransforms"""
    moved = world.freeze()["transforms"]
    n = len(world.model_instances)
    out = (S.ModelInstanceTransforms * n)()
    for i in range(n):
        C.memmove(C.byref(out[i]), C.byref(moved[i]), C.sizeof(S.ModelInstanceTransforms))
        out[i].modelToWorld.col[0].w += 0.03 * (i + 1)
    return out


def agreeing(ctx, world, cam, ids):
    """pixels where the raster id, mapped to its geometry triangle, is the traced PrimitiveID view's triangle of the same
    mesh instance"""
    got = R.geometry_ids(world, ids)
    prim_view = ctx.trace_gbuffer_velocity(cam, W_, H_, draw_type=S.DrawType["PrimitiveID"], opaque_only=True)[0]
    mesh_view = ctx.trace_gbuffer_velocity(cam, W_, H_, draw_type=S.DrawType["MeshID"], opaque_only=True)
    hit = mesh_view[2] != 0
    dis = CR.draw_instances_of(world)
    mesh_of = np.array([d[1] for d in dis] + [0], np.int64)
    covered = got[..., 0] >= 0
    want_prim = uint_to_color(np.maximum(got[..., 1], 0))
    want_mesh = uint_to_color(mesh_of[got[..., 0]])
    same = covered & hit & (prim_view[..., :3].view(np.uint32) == want_prim.view(np.uint32)).all(axis=2) & \
        (mesh_view[0][..., :3].view(np.uint32) == want_mesh.view(np.uint32)).all(axis=2)
    return same, covered, hit


def check_against_traced(ctx, world, cam, previous, cap):
    ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
    ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True)
    ids, depth = ctx.read_raster_visibility(W_, H_)
    same, covered, hit = agreeing(ctx, world, cam, ids)
    differ = (covered != hit) | (covered & ~same)
    print("agreeing %d of %d covered, %d differ" % (same.sum(), covered.sum(), differ.sum()))
    assert same.sum() > 0.8 * covered.sum() and covered.mean() > 0.1
    if cap is not None:
        assert differ.mean() <= cap
    for draw_type in (S.DrawType["Default"], S.DrawType["Position"], S.DrawType["ShadingNormal"], S.DrawType["TexCoord0"], S.DrawType["Albedo"],
                      S.DrawType["MaterialID"], S.DrawType["MeshID"], S.DrawType["Roughness"], S.DrawType["Metallic"]):
        t_ar, t_nm, t_depth, t_vel = ctx.trace_gbuffer_velocity(cam, W_, H_, draw_type=draw_type, previous_transforms=previous, opaque_only=True)
        r_ar, r_nm, r_depth, r_vel = ctx.raster_resolve(cam, draw_type=draw_type, previous_transforms=previous)
        for name, a, b in (("albedoRoughness", r_ar, t_ar), ("normalMetallic", r_nm, t_nm), ("velocity", r_vel, t_vel)):
            assert np.array_equal(a[same].view(np.uint32), b[same].view(np.uint32)), (draw_type, name)
        # the depth is the rasteriser's, the sky is the clear value with the traced sky's velocity
        assert np.array_equal(r_depth.view(np.uint32), depth.view(np.uint32))
        sky = ~covered & ~hit
        assert not r_ar[~covered].any() and not r_nm[~covered].any()
        assert np.array_equal(r_vel[sky].view(np.uint32), t_vel[sky].view(np.uint32))
    return ids, depth, same


def test_the_closed_scene_against_the_traced_gbuffer(gpu_ctx):
    world = RS.closed_world()
    gpu_ctx.upload_scene(world)
    cam = jittered_camera()
    ids, depth, same = check_against_traced(gpu_ctx, world, cam, previous_of(world), cap=0.02)
    # the draw types of the mesh shader
    ar, nm, _, _ = gpu_ctx.raster_resolve(cam, draw_type=S.DrawType["MeshletID"])
    covered = ids[..., 0] != R.NO_ID
    assert np.array_equal(ar[covered][:, :3].view(np.uint32), uint_to_color(ids[covered][:, 1]).view(np.uint32))
    assert (ar[covered][:, 3] == 1).all() and not nm.any() and not ar[~covered].any()
    ar, nm, _, _ = gpu_ctx.raster_resolve(cam, draw_type=S.DrawType["PrimitiveID"])
    assert np.array_equal(ar[covered][:, :3].view(np.uint32), uint_to_color(ids[covered][:, 2]).view(np.uint32))  # meshlet-local
    assert len(set(ids[covered][:, 1].tolist())) > 2 and not nm.any()
    assert_depth_bound(world, cam, ids, depth)


def assert_depth_bound(world, cam, ids, depth):
    """the raster depth against float64 over the unsnapped vertices: 4 x the restatement's own largest deviation on this scene"""
    covered = ids[..., 0] != R.NO_ID
    view = R.View(cam)
    f = world.freeze()
    from prosper_amd import meshlets as M
    m2w = CR.transforms_of(world)
    dis = CR.draw_instances_of(world)
    want_keys = R.rasterise(world, cam, CR.generate(world, CR.MODE_OPAQUE))["keys"]
    rest_depth = R.decode(world, want_keys)[1]
    exact = np.zeros((H_, W_))
    for py, px in zip(*np.nonzero(covered)):
        di, mi, t = (int(v) for v in ids[py, px])
        inst, mesh, _ = dis[di]
        md, info = world.metadatas[mesh], world.mesh_infos[mesh]
        built = M.read_meshlets(f["geometry_buffers"][md.bufferIndex], md, info)
        vo, to, vc, tc = (int(v) for v in built["meshlets"][mi])
        v = built["vertices"][vo:vo + vc][built["triangles"][to + 3 * t:to + 3 * t + 3]]
        clip = R.to_clip(view, m2w[inst], world.mesh_geometry(mesh)[0][v]).astype(np.float64)
        A = np.stack([(clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * W_, (clip[:, 1] / clip[:, 3] * 0.5 + 0.5) * H_, np.ones(3)], axis=1)
        exact[py, px] = np.linalg.solve(A, clip[:, 2] / clip[:, 3]) @ np.array([px + 0.5, py + 0.5, 1.0])
    own = np.abs(rest_depth.astype(np.float64) - exact)[covered].max()
    got = np.abs(depth.astype(np.float64) - exact)[covered].max()
    print("depth: the restatement's largest deviation %.3e, the library's %.3e" % (own, got))
    assert got <= 4.0 * own


def test_flight_helmet_with_texture_lod_against_the_traced_gbuffer():
    world = flight_helmet.load_fixture(sky_size=0)
    world.add_meshlets()
    ctx = capi.Context(device=0, flags=S.CREATE_TEXTURE_MIPS)
    try:
        ctx.upload_scene(world)
        ctx.set_texture_lod(True, -1.0)
        c = world.camera
        cam = jittered_camera(tuple(c["eye"]), tuple(c["target"]), step=(0.01, 0.005, 0.0))
        # the helmet is an open mesh seen from outside: a pixel whose nearest surface is a back face would disagree by
        # construction, and the cap still holds because the fixture's view shows none but at silhouettes (3 of 6 144 here)
        ids, depth, same = check_against_traced(ctx, world, cam, previous_of(world), cap=0.02)
        assert_depth_bound(world, cam, ids, depth)
    finally:
        ctx.close()


def test_two_phases_give_the_unculled_targets_and_the_last_gbuffer_is_the_raster_s(gpu_ctx):
    world, inst = CS.property_world()
    gpu_ctx.upload_scene(world)
    fresh = capi.Context(device=0)
    try:
        fresh.upload_scene(world)
        for frame, eye_x in enumerate((0.0, 0.3)):
            cam = CS.camera_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0))
            got = gpu_ctx.raster_gbuffer(cam)
            fresh.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
            fresh.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True)
            want = fresh.raster_resolve(cam)
            for a, b in zip(got, want):
                assert a.tobytes() == b.tobytes(), frame
            assert got[2].any() and got[0].any()
        # plumbing: the passes that take "NULL: the last traced G-buffer" run over the raster G-buffer
        ar, nm, depth, vel = got
        inp, w, h = gpu_ctx.gbuffer_device_ptrs()
        assert (w, h) == (W_, H_)
        gpu_ctx.hiz_downsample(W_, H_, slot=0)
        for x, y in zip(gpu_ctx.read_hiz(0), CR.hiz_pyramid(depth)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        gpu_ctx.deferred_shading_device(cam, W_, H_, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
        over_device = gpu_ctx.read_hdr().copy()
        gpu_ctx.deferred_shading(cam, ar, nm, depth)
        assert gpu_ctx.read_hdr().tobytes() == over_device.tobytes()
        # the skybox fill with a NULL depth reads the raster G-buffer's
        gpu_ctx.skybox_fill(cam, W_, H_)
        filled = gpu_ctx.read_hdr().copy()
        gpu_ctx.deferred_shading(cam, ar, nm, depth)
        gpu_ctx.skybox_fill(cam, W_, H_, depth=depth)
        assert gpu_ctx.read_hdr().tobytes() == filled.tobytes() and (depth == 0).any()
        # the read-backs and pointers of "the last G-buffer" are the raster's
        assert all(a.tobytes() == b.tobytes() for a, b in zip(gpu_ctx.read_gbuffer(), (ar, nm, depth)))
        assert gpu_ctx.read_velocity().tobytes() == vel.tobytes() and gpu_ctx.velocity_device_ptr()[1:] == (W_, H_)
        # caller-owned targets: the same bits, and the context's last G-buffer stays what it was
        import torch
        t_ar, t_nm = torch.zeros(H_ * W_ * 4, device="cuda"), torch.zeros(H_ * W_ * 4, device="cuda")
        t_d, t_v = torch.zeros(H_ * W_, device="cuda"), torch.zeros(H_ * W_ * 2, device="cuda")
        none = gpu_ctx.raster_resolve(cam, targets=(t_ar.data_ptr(), t_nm.data_ptr(), t_d.data_ptr()), velocity_ptr=t_v.data_ptr())
        assert none == (None, None, None, None)
        torch.cuda.synchronize()
        assert t_ar.cpu().numpy().tobytes() == ar.tobytes() and t_nm.cpu().numpy().tobytes() == nm.tobytes()
        assert t_d.cpu().numpy().tobytes() == depth.tobytes() and t_v.cpu().numpy().tobytes() == vel.tobytes()
        # a traced G-buffer afterwards is what it is without any raster call
        a = gpu_ctx.trace_gbuffer_velocity(cam, W_, H_, opaque_only=True)
        b = fresh_traced = capi.Context(device=0)
        try:
            b.upload_scene(world)
            want = b.trace_gbuffer_velocity(cam, W_, H_, opaque_only=True)
        finally:
            fresh_traced.close()
        for x, y in zip(a, want):
            assert x.tobytes() == y.tobytes()
    finally:
        fresh.close()


def test_refusals_of_the_resolve(gpu_ctx):
    lib = capi.lib()
    world = RS.closed_world()
    gpu_ctx.upload_scene(world)
    cam = CS.camera_at()
    desc = S.VelocityGBufferDesc()
    with pytest.raises(capi.ProsperPtError, match="nothing has been drawn") as e:
        gpu_ctx.raster_resolve(cam)  # a resolve before any draw
    assert e.value.code == -4
    gpu_ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
    gpu_ctx.raster_meshlets(cam)
    with pytest.raises(capi.ProsperPtError, match="visibility image's extent"):
        gpu_ctx.raster_resolve(CS.camera_at(width=40, height=30))
    assert lib.prosper_pt_raster_resolve(gpu_ctx._h, 11, C.byref(cam), C.byref(desc), None) == -1  # drawType
    assert lib.prosper_pt_raster_resolve(gpu_ctx._h, 0, None, C.byref(desc), None) == -1
    assert lib.prosper_pt_raster_resolve(gpu_ctx._h, 0, C.byref(cam), None, None) == -1
    assert lib.prosper_pt_raster_gbuffer(None, 0, C.byref(cam), C.byref(desc), None) == -1
    partly = S.VelocityGBufferDesc()
    partly.targets.albedoRoughness = 256
    for entry in (lib.prosper_pt_raster_resolve, lib.prosper_pt_raster_gbuffer):
        assert entry(gpu_ctx._h, 0, C.byref(cam), C.byref(partly), None) == -1  # a partly given target set
        odd = S.VelocityGBufferDesc()
        odd.velocity = 4
        assert entry(gpu_ctx._h, 0, C.byref(cam), C.byref(odd), None) == -1  # a misaligned velocity target
        count = S.VelocityGBufferDesc()
        count.previousTransformCount = 3
        assert entry(gpu_ctx._h, 0, C.byref(cam), C.byref(count), None) == -1
    # a meshlet triangle that is no triangle of the index buffer
    bad = RS.closed_world()
    mesh = 1
    md = bad.metadatas[mesh]
    words = bad._buffer_words_of(md.bufferIndex)
    tri = words.view(np.uint8)[md.meshletTrianglesByteOffset:md.meshletTrianglesByteOffset + 3]
    tri[:] = tri[::-1].copy()  # mirrored: another triangle
    bad._frozen = None
    fresh = capi.Context(device=0)
    try:
        fresh.upload_scene(bad)
        fresh.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
        with pytest.raises(capi.ProsperPtError, match="not a triangle of the mesh's index buffer") as e:
            fresh.raster_meshlets(cam)
        assert e.value.code == -5
    finally:
        fresh.close()


def test_two_streams_into_one_context_with_the_resolve(gpu_ctx):
    world = RS.closed_world()
    gpu_ctx.upload_scene(world)
    hip = C.CDLL("libamdhip64.so")
    s1, s2 = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s1), 1) == 0 and hip.hipStreamCreateWithFlags(C.byref(s2), 1) == 0
    try:
        small, big = CS.camera_at(width=40, height=30), CS.camera_at()
        want = None
        for _ in range(2):  # the second call grows and clears what the first still resolves; nothing waits on the host between
            lib = capi.lib()
            desc = S.VelocityGBufferDesc()
            assert lib.prosper_pt_raster_gbuffer(gpu_ctx._h, 0, C.byref(small), C.byref(desc), s1) == 0
            assert lib.prosper_pt_raster_gbuffer(gpu_ctx._h, 0, C.byref(big), C.byref(desc), s2) == 0
            got = gpu_ctx.read_gbuffer(stream=s2.value) + (gpu_ctx.read_velocity(stream=s2.value),)
            if want is None:
                assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
                want = gpu_ctx.raster_gbuffer(big)
                gpu_ctx.raster_release_preserved()
            assert all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))
    finally:
        assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
        hip.hipStreamDestroy(s1)
        hip.hipStreamDestroy(s2)


def test_the_cpp_gbuffer_renderer_records_what_the_direct_call_records(gpu_ctx):
    from prosper_amd import rt_reference
    world, inst = CS.property_world()
    gpu_ctx.upload_scene(world)
    fresh = capi.Context(device=0)
    hcam = rt_reference.Camera()
    hcam.set_parameters(CS.FOV, CS.NEAR, CS.FAR)
    renderer = rt_reference.GBufferRenderer(gpu_ctx)
    try:
        fresh.upload_scene(world)
        transforms = world.freeze()["transforms"]
        for frame, eye_x in enumerate((0.0, 0.3, 0.3)):
            if frame == 2:
                renderer.release_preserved()  # the third frame starts over: one phase, no previous transforms
                fresh.raster_release_preserved()
            hcam.look_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0), (0.0, 1.0, 0.0))
            out = renderer.record(hcam, W_, H_, transforms=transforms)
            stats, _ = renderer.read_draw_stats()
            inp, w, h = gpu_ctx.gbuffer_device_ptrs()
            assert (out.albedoRoughness, out.normalMetalness, out.depth) == (inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
            assert out.velocity == gpu_ctx.velocity_device_ptr()[0] and (w, h) == (W_, H_)
            got = gpu_ctx.read_gbuffer() + (gpu_ctx.read_velocity(),)
            cam = CS.camera_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0))
            want = fresh.raster_gbuffer(cam, previous_transforms=transforms if frame == 1 else None)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), frame
            assert bytes(stats) == bytes(fresh.draw_stats())
            second_valid = fresh.raster_info().draw[1].valid
            assert second_valid == (1 if frame == 1 else 0)
        with pytest.raises(capi.ProsperPtError, match="drawType") as e:
            renderer.record(hcam, W_, H_, draw_type=11)
        assert e.value.code == -1
    finally:
        renderer.close()
        hcam.close()
        fresh.close()


def test_the_mask_quad_is_sample_material_s_decision_and_the_resolve_s(gpu_ctx):
    """S1's MASK quad over a farther quad: the ids are the restatement's (raw alpha * factor against the cutoff, texel by
    texel); on the row of alpha 160 the rasteriser keeps the quad where the traced G-buffer's any-hit (sampleAlpha, sRGB ->
    linear) lets the ray through to the farther quad; and the resolve shades exactly the pixels the draw kept - the
    two call one device function for the pixel, so it never meets alpha == 0 (a kept pixel's albedo is the texel's)."""
    world, names = RS.s1_world()
    gpu_ctx.upload_scene(world)
    cam = RS.s1_camera()
    w, h = RS.S1_EXTENT
    dis = CR.draw_instances_of(world)
    di = [k for k, d in enumerate(dis) if d[0] == names["mask"]][0]
    db = [k for k, d in enumerate(dis) if d[0] == names["behind_mask"]][0]
    for lod in (False,):
        gpu_ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
        gpu_ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True)
        ids, depth = gpu_ctx.read_raster_visibility(w, h)
        want = R.decode(world, R.rasterise(world, cam, CR.generate(world, CR.MODE_OPAQUE))["keys"])
        assert np.array_equal(ids, want[0]) and np.array_equal(depth.view(np.uint32), want[1].view(np.uint32))
        quad = ids[2:14, 30:46, 0]
        keep = np.repeat(np.repeat(RS.MASK_ALPHA >= 128, 3, axis=0), 4, axis=1)  # 0 / 255 / 160 / 100 against 0.5 * 255
        assert np.array_equal(quad == di, keep) and (quad[~keep] == db).all()
        # the traced G-buffer: the 160 row goes to the farther quad (sampleAlpha), the 255 texels to the MASK quad
        mesh_view = gpu_ctx.trace_gbuffer_velocity(cam, w, h, draw_type=S.DrawType["MeshID"], opaque_only=True)[0]
        mesh_of = lambda k: uint_to_color(np.array([dis[k][1]]))[0]
        traced_behind = (mesh_view[2:14, 30:46, :3].view(np.uint32) == mesh_of(db).view(np.uint32)).all(axis=2)
        print("traced: the farther quad shows through\n%s" % traced_behind.astype(int))
        texel_rows = np.repeat(np.arange(4), 3)
        # on the row of 160 the rasteriser keeps every pixel and the any-hit lets rays through: the decisions differ there
        # (the any-hit's sampleAlpha has its own footprint as well, so nothing is asserted of it texel by texel)
        assert traced_behind[texel_rows == 2].any() and keep[texel_rows == 2].all()
        assert traced_behind[texel_rows == 3].all() and not keep[texel_rows == 3].any()  # 100: below the cutoff either way
        # the resolve: the kept pixels carry the texture's colour (200 / 255 through sRGB -> linear, whatever that is: one
        # value over the whole quad, and not the farther quad's), the discarded ones the farther quad's
        ar = gpu_ctx.raster_resolve(cam, draw_type=S.DrawType["Albedo"])[0][2:14, 30:46, :3]
        assert len(np.unique(ar[keep].view(np.uint32), axis=0)) == 1 and len(np.unique(ar[~keep].view(np.uint32), axis=0)) == 1
        assert not np.array_equal(ar[keep][0], ar[~keep][0])
