"""The forward opaque pass on the GPU (prosper_pt_raster_forward, prosper_pt_raster_forward_shade; forward_opaque_kernel;
DESIGN.md f19): its surfaces, depth and velocity against the rasteriser's resolve bit for bit, its colour against
tests/forward_reference.py over the read-back surfaces, against the transparent pass on a BLEND twin of the scene, the
draw types against the resolve's albedoRoughness, the two-phase sequence against the unculled draw, and the plumbing."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import culling_reference as CR
import culling_scenes as CS
import deferred_shading_reference as D
import forward_reference as FR
import raster_reference as R
import raster_scenes as RS
from prosper_amd import capi, flight_helmet, scenes, structs as S
from test_raster_resolve import jittered_camera, previous_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# the project's shading tolerance (test_deferred_shading.py, test_transparent.py), relative to the pixel's sum of absolute terms
REL = 2e-4
ABS = 1e-6
EXTENTS = ((48, 32), (33, 17), (1, 1), (96, 64))


def lit(world):
    """the point light and the spot light of test_transparent.designed_scene (and its sky, for the IBL maps) on top of the
    scene's own light; the sun is the world's"""
    world.add_point_light((1.0, 0.9, 0.8), 60.0, (0.75, 1.0, 3.0))
    world.add_spot_light((0.8, 0.9, 1.0), 80.0, (-1.0, 0.5, 3.5), (0.3, -0.1, -1.0), math.radians(25.0), math.radians(40.0))
    world.skybox = scenes.sky_cube(32)
    world._frozen = None
    return world


def make_world(scene):
    if scene == "s1":
        return lit(RS.s1_world()[0])
    if scene == "closed":
        return lit(RS.closed_world())
    return lit(CS.property_world()[0])


def draw_generated(ctx, cam):
    """CLEAR + the generated list: the unculled image"""
    ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
    ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True)


def outputs(ctx):
    return ctx.read_hdr().copy(), ctx.read_forward_depth(), ctx.read_velocity()


def shade_over_generated(ctx, cam, **kw):
    draw_generated(ctx, cam)
    ctx.raster_forward_shade(cam, **kw)
    return outputs(ctx)


def first_frame(ctx, cam, **kw):
    """prosper_pt_raster_forward without a kept pyramid: one culling phase, one draw, the shade.  (Not the unculled image on
    S1: the first phase's cone test drops the quad that a mirroring instance transform turns to the front, for
    prosper_pt_raster_gbuffer just the same.)  A 1 x 1 image has no pyramid: the generated list there."""
    if cam.resolution[0] > 1:
        ctx.raster_release_preserved()
        ctx.raster_forward(cam, **kw)
        return outputs(ctx)
    return shade_over_generated(ctx, cam, **kw)


def lists_of(ctx, world):
    return D.membership(ctx.read_light_clusters(), world.point_lights.count, world.spot_lights.count)


def signed_oct_encode(n):
    """gbuffer.frag:41-58 in float32, operation for operation as signed_oct_encode of the kernels"""
    n = n.astype(F)
    s = (np.abs(n[..., 0]) + np.abs(n[..., 1])) + np.abs(n[..., 2])
    x, y, z = n[..., 0] / s, n[..., 1] / s, n[..., 2] / s
    oy = y * F(0.5) + F(0.5)
    ox = x * F(0.5) + oy
    oy = x * F(-0.5) + oy
    with np.errstate(over="ignore"):
        oz = np.clip(z * F(3.40282e+38), F(0.0), F(1.0))
    return np.stack([ox, oy, oz], axis=-1)


def check_surfaces(surf, resolved, ids, world):
    """the records against the resolve's four targets and the visibility read-back, bit for bit"""
    ar, nm, depth, vel = resolved
    covered = ids[..., 0] != R.NO_ID
    assert np.array_equal(FR.covered_of(surf), covered)
    s = surf[covered]
    assert np.array_equal(s["albedo"].view(np.uint32), ar[covered][:, :3].view(np.uint32))
    assert np.array_equal(s["roughness"].view(np.uint32), ar[covered][:, 3].view(np.uint32))
    assert np.array_equal(s["metallic"].view(np.uint32), nm[covered][:, 2].view(np.uint32))
    enc = signed_oct_encode(s["normal"])
    assert np.array_equal(enc.view(np.uint32), nm[covered][:, [0, 1, 3]].view(np.uint32))
    off = surf["nonLinearDepth"].view(np.uint32) != depth.view(np.uint32)
    if off.any():
        y, x = np.argwhere(off)[0]
        print("depth: %d records differ from the target, first at (%d, %d): %r against %r, ids %s" % (
            off.sum(), x, y, surf["nonLinearDepth"][y, x], depth[y, x], ids[y, x]))
    assert not off.any()
    want = R.geometry_ids(world, ids)
    assert np.array_equal(s["drawInstance"].astype(np.int64), want[covered][:, 0]) and np.array_equal(s["primitive"].astype(np.int64), want[covered][:, 1])
    un = surf[~covered]
    assert (un["drawInstance"] == FR.NO_SURFACE).all() and not un["albedo"].any() and not un["positionWS"].any()


# ---- 1. surfaces, depth and velocity ----

@pytest.mark.parametrize("scene,extent", [("s1", EXTENTS[0]), ("s1", EXTENTS[1]), ("s1", EXTENTS[2]), ("closed", EXTENTS[3]), ("closed", EXTENTS[1])],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_surfaces_depth_and_velocity_are_the_resolve_s(gpu_ctx, scene, extent):
    """under jitter, previous transforms and a moved previous camera, as test_raster_resolve.py sets them up"""
    w, h = extent
    world = make_world(scene)
    cam = jittered_camera(width=w, height=h)
    previous = previous_of(world)
    gpu_ctx.upload_scene(world)
    gpu_ctx.set_forward_debug_surfaces(True)
    try:
        hdr, depth, vel = first_frame(gpu_ctx, cam, previous_transforms=previous)
        surf = gpu_ctx.read_forward_surfaces()
        info = gpu_ctx.forward_opaque_info()
    finally:
        gpu_ctx.set_forward_debug_surfaces(False)
    ids, vdepth = gpu_ctx.read_raster_visibility(w, h)
    fresh = capi.Context(device=0)
    try:
        fresh.upload_scene(world)
        if w > 1:
            resolved = fresh.raster_gbuffer(cam, previous_transforms=previous)
        else:
            draw_generated(fresh, cam)
            resolved = fresh.raster_resolve(cam, previous_transforms=previous)
    finally:
        fresh.close()
    covered = ids[..., 0] != R.NO_ID
    print("%s %dx%d: %d of %d covered" % (scene, w, h, covered.sum(), covered.size))
    assert covered.any() and (covered.all() or (~covered).any())
    for name, a, b in (("depth", depth, resolved[2]), ("velocity", vel, resolved[3])):
        off = (a.view(np.uint32) != b.view(np.uint32)).reshape(h, w, -1).any(axis=2)
        if off.any():
            y, x = np.argwhere(off)[0]
            print("%s: %d pixels differ from the fresh context's G-buffer, first at (%d, %d): %r against %r, ids %s" % (
                name, off.sum(), x, y, a[y, x], b[y, x], ids[y, x]))
    check_surfaces(surf, resolved, ids, world)
    assert depth.tobytes() == resolved[2].tobytes() == vdepth.tobytes() and vel.tobytes() == resolved[3].tobytes()
    assert vel.any()
    assert info is not None and info.shadedPixels == covered.sum() and info.ms >= info.shadeMs > 0.0
    # alpha: 1 on covered pixels (no BLEND surface is drawn, the MASK quad's kept texels have alpha 1), 0 elsewhere, exactly
    assert (hdr[covered][:, 3] == 1.0).all() and not hdr[~covered].any()
    # the debug mode does not change the images, and its read-back is refused after a call without it
    again = first_frame(gpu_ctx, cam, previous_transforms=previous)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (hdr, depth, vel)))
    with pytest.raises(capi.ProsperPtError, match="debug mode") as e:
        gpu_ctx.read_forward_surfaces()
    assert e.value.code == -4


# ---- 2. colour against the restatement ----

def check_colour(world, cam, hdr, surf, lists, what, maps=None, margin_cap=0.99):
    covered = FR.covered_of(surf)
    want, total, margin = FR.shade(world, cam, surf, lists, maps)
    assert np.array_equal(hdr[..., 3].astype(np.float64), want[..., 3]), "%s: alpha" % what
    assert not hdr[~covered].any()
    ok = covered & (margin > 1e-4)  # the slice pick was not a coin flip between fp32 and float64 (test_deferred_shading.py)
    assert ok.sum() >= margin_cap * covered.sum(), what
    err = np.abs(hdr[..., :3].astype(np.float64) - want[..., :3]).max(-1)
    worst = np.argmax(np.where(ok, err / (REL * total + ABS), 0.0))
    print("%s: %d covered pixels, worst error %.3g of scale %.3g (%.2f of the tolerance)" % (
        what, covered.sum(), err.ravel()[worst], total.ravel()[worst], err.ravel()[worst] / (REL * total.ravel()[worst] + ABS)))
    bad = ok & ~(err <= REL * total + ABS)
    assert not bad.any(), "%s: %d pixels off, worst %.3g of %.3g" % (what, bad.sum(), err[bad].max(), total[bad][np.argmax(err[bad])])
    assert (hdr[covered][:, :3] > 0).any()


@pytest.mark.parametrize("scene,extent", [("s1", EXTENTS[0]), ("closed", EXTENTS[3])], ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_colour_against_the_restatement(scene, extent):
    w, h = extent
    world = make_world(scene)
    cam = RS.s1_camera(w, h) if scene == "s1" else CS.camera_at(width=w, height=h)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        ctx.set_forward_debug_surfaces(True)
        draw_generated(ctx, cam)
        with pytest.raises(capi.ProsperPtError, match="prosper_pt_generate_ibl") as e:
            ctx.raster_forward_shade(cam, ibl=1)
        assert e.value.code == -6
        ctx.raster_forward_shade(cam)
        plain, surf = ctx.read_hdr().copy(), ctx.read_forward_surfaces()
        assert ctx.forward_opaque_info().reclustered == 1
        lists = lists_of(ctx, world)
        ctx.generate_ibl()
        maps = ctx.read_ibl()
        ctx.raster_forward_shade(cam, ibl=1)
        with_ibl, surf_ibl = ctx.read_hdr().copy(), ctx.read_forward_surfaces()
        assert ctx.forward_opaque_info().reclustered == 0  # same camera terms, extent and lights: the lists served
    finally:
        ctx.close()
    assert surf.tobytes() == surf_ibl.tobytes()
    check_colour(world, cam, plain, surf, lists, "%s ibl 0" % scene)
    check_colour(world, cam, with_ibl, surf, lists, "%s ibl 1" % scene, maps=maps)
    covered = FR.covered_of(surf)
    assert (with_ibl[covered][:, :3] != plain[covered][:, :3]).any()


def test_three_hundred_point_lights_on_a_grid(gpu_ctx):
    """20 x 15 point lights of radius 0.6 on a plane in front of the closed scene: neighbouring clusters list different
    lights, in x, in y and from one depth slice to the next - which is where the lists differ inside a wave: its 8 x 8 block
    lies in one 32 x 32 cluster and, on the sphere, in two slices -, and 160 more of a large radius at one spot make the
    clusters there overflow their 128 kept entries."""
    w, h = EXTENTS[3]
    world = lit(RS.closed_world())
    for j in range(15):
        for i in range(20):
            world.add_point_light((1.0, 0.8 + 0.01 * i, 0.6 + 0.02 * j), 3.0, (-3.8 + 0.4 * i, -2.1 + 0.3 * j, -2.0), light_range=0.6)
    for k in range(160):
        world.add_point_light((0.5, 0.7, 1.0), 0.5, (-0.9 + 0.002 * k, 0.1, -1.9), light_range=3.0)
    world._frozen = None
    cam = CS.camera_at(width=w, height=h)
    gpu_ctx.upload_scene(world)
    gpu_ctx.set_forward_debug_surfaces(True)
    try:
        hdr, _, _ = shade_over_generated(gpu_ctx, cam)
        surf = gpu_ctx.read_forward_surfaces()
    finally:
        gpu_ctx.set_forward_debug_surfaces(False)
    clusters = gpu_ctx.read_light_clusters()
    assert clusters["overflowing"] > 0 and clusters["dropped"] > 0
    counts = clusters["pointers"][..., 1] >> 16
    assert counts.max() == S.CLUSTER_MAX_POINTS and len(np.unique(counts)) > 3
    lists = lists_of(gpu_ctx, world)
    # clusters of one slice that are neighbours in x or y and hold different lists, with covered pixels in both
    covered = FR.covered_of(surf)
    slices = np.full((h, w), -1, np.int64)
    slices[covered] = D.slices(cam, FR.T.LayerSurfaces(cam, surf[covered], 0, 0).z_cam)[0]
    used = sorted(set(slices[covered].tolist()))
    assert any((lists[0][s, :, 0] != lists[0][s, :, 1]).any() for s in used)
    # a wave's block with covered pixels of two slices whose lists differ in that cluster
    mixed = 0
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            in_block = sorted(set(slices[by:by + 8, bx:bx + 8].ravel().tolist()) - {-1})
            mixed += len(in_block) > 1 and (lists[0][in_block[0], by // 32, bx // 32] != lists[0][in_block[1], by // 32, bx // 32]).any()
    print("%d waves shade over two different lists" % mixed)
    assert mixed > 0
    check_colour(world, cam, hdr, surf, lists, "300 + 160 point lights")


# ---- 3. the bit-exact twin ----

def test_the_transparent_pass_on_a_blend_twin_gives_the_same_colour(gpu_ctx):
    """closed_world as it is through the forward opaque pass, and with every material BLEND with alpha factor 1 through
    prosper_pt_forward_transparent (CAMERA_JITTER: the same pixel ray) over a zeroed HDR image and a zero depth: wherever
    layer 0 names the forward surface's (drawInstance, primitive) the rgb values are equal as float32 values (not bits: the
    blend's + dst * 0 may turn a -0 into +0).  At least 98 % of the covered pixels qualify (tests/test_raster_cpu.py's cap
    for raster against traced; tests/test_forward_opaque_cpu.py checks the restatement alone stays within it)."""
    from test_forward_opaque_cpu import blend_twin
    w, h = EXTENTS[3]
    world, twin = lit(RS.closed_world()), blend_twin(lit(RS.closed_world()))
    cam = jittered_camera(width=w, height=h)
    gpu_ctx.upload_scene(world)
    gpu_ctx.set_forward_debug_surfaces(True)
    try:
        hdr, _, _ = shade_over_generated(gpu_ctx, cam)
        surf = gpu_ctx.read_forward_surfaces()
    finally:
        gpu_ctx.set_forward_debug_surfaces(False)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(twin)
        ctx.deferred_shading_traced(cam, w, h)  # sizes the HDR image, which is then zeroed
        ptr, nbytes = ctx.hdr_device_ptr()
        assert nbytes >= h * w * 16
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemset(ptr, 0, h * w * 16) == 0 and hip.hipDeviceSynchronize() == 0
        assert not ctx.read_hdr().any()
        ctx.set_transparent_debug_layers(2)
        ctx.forward_transparent(cam, w, h, flags=S.TRANSPARENT_CAMERA_JITTER, depth=np.zeros((h, w), F))
        blended = ctx.read_hdr().copy()
        counts, layers = ctx.read_transparent_layers()
    finally:
        ctx.close()
    covered = FR.covered_of(surf)
    first = layers[..., 0]
    same = covered & (counts > 0) & (first["drawInstance"] == surf["drawInstance"]) & (first["primitive"] == surf["primitive"])
    print("twin: %d of %d covered pixels name the same triangle" % (same.sum(), covered.sum()))
    assert covered.sum() > 500 and same.sum() >= 0.98 * covered.sum()
    assert (counts[same] == 1).all()  # alpha 1: T == 0 after the first layer
    assert np.array_equal(hdr[same][:, :3], blended[same][:, :3])
    assert (hdr[same][:, :3] != 0).any()


# ---- 4. draw types ----

@pytest.mark.parametrize("scene,extent", [("s1", EXTENTS[0]), ("closed", EXTENTS[3])], ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_draw_types_write_the_resolve_s_albedo_roughness(gpu_ctx, scene, extent):
    w, h = extent
    world = make_world(scene)
    cam = jittered_camera(width=w, height=h)
    gpu_ctx.upload_scene(world)
    draw_generated(gpu_ctx, cam)
    ids, _ = gpu_ctx.read_raster_visibility(w, h)
    covered = ids[..., 0] != R.NO_ID
    default = None
    for dt in range(len(S.DRAW_TYPES)):
        gpu_ctx.raster_forward_shade(cam, draw_type=dt)
        hdr = gpu_ctx.read_hdr().copy()
        if dt == S.DrawType["Default"]:
            default = hdr
            continue
        ar = gpu_ctx.raster_resolve(cam, draw_type=dt)[0]
        assert np.array_equal(hdr[covered][:, :3].view(np.uint32), ar[covered][:, :3].view(np.uint32)), S.DRAW_TYPES[dt]
        assert (hdr[covered][:, 3] == 1.0).all() and not hdr[~covered].any(), S.DRAW_TYPES[dt]
        assert hdr.tobytes() != default.tobytes(), S.DRAW_TYPES[dt]
        if dt == S.DrawType["MeshletID"]:
            assert np.array_equal(hdr[covered][:, :3].view(np.uint32), FR.uint_to_color(ids[covered][:, 1]).view(np.uint32))
        if dt == S.DrawType["PrimitiveID"]:
            assert np.array_equal(hdr[covered][:, :3].view(np.uint32), FR.uint_to_color(ids[covered][:, 2]).view(np.uint32))


# ---- 5. the sequence ----

def test_the_two_phase_sequence_gives_the_unculled_frame(gpu_ctx):
    w, h = EXTENTS[3]
    world = make_world("property")
    gpu_ctx.upload_scene(world)
    gpu_ctx.raster_release_preserved()
    fresh = capi.Context(device=0)
    second_phase = 0
    try:
        fresh.upload_scene(world)
        for frame, eye_x in enumerate((0.0, 0.3, 0.6)):
            cam = CS.camera_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0))
            gpu_ctx.raster_forward(cam)
            got = outputs(gpu_ctx)
            second_phase += len(gpu_ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE)[0]) if frame else 0
            assert gpu_ctx.raster_info().draw[1].valid == (1 if frame else 0)
            want = shade_over_generated(fresh, cam)
            for name, a, b in zip(("illumination", "depth", "velocity"), got, want):
                assert a.tobytes() == b.tobytes(), (frame, name)
            assert got[0].any() and got[1].any()
            # the kept pyramid is the pyramid of the depth: the slots alternate, starting at 0 after releasePreserved
            slot = frame % 2
            assert gpu_ctx.hiz_info(slot).valid == 1
            for x, y in zip(gpu_ctx.read_hiz(slot), CR.hiz_pyramid(got[1])):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), frame
        assert second_phase > 0, "the second-phase lists are all empty"
        # releasePreserved: the next sequence runs one phase
        gpu_ctx.raster_release_preserved()
        gpu_ctx.raster_forward(cam)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outputs(gpu_ctx), want))
        assert gpu_ctx.raster_info().draw[1].valid == 0
    finally:
        fresh.close()


# ---- 6. MASK and texture LOD ----

def test_the_mask_quad_shades_its_kept_texels_and_the_farther_quad_elsewhere(gpu_ctx):
    world, names = RS.s1_world()
    lit(world)
    gpu_ctx.upload_scene(world)
    cam = RS.s1_camera()
    w, h = RS.S1_EXTENT
    gpu_ctx.set_forward_debug_surfaces(True)
    try:
        hdr, _, _ = shade_over_generated(gpu_ctx, cam)
        surf = gpu_ctx.read_forward_surfaces()
    finally:
        gpu_ctx.set_forward_debug_surfaces(False)
    dis = CR.draw_instances_of(world)
    di = [k for k, d in enumerate(dis) if d[0] == names["mask"]][0]
    db = [k for k, d in enumerate(dis) if d[0] == names["behind_mask"]][0]
    quad = surf[2:14, 30:46]
    keep = np.repeat(np.repeat(RS.MASK_ALPHA >= 128, 3, axis=0), 4, axis=1)
    assert np.array_equal(quad["drawInstance"] == di, keep) and (quad["drawInstance"][~keep] == db).all()
    # the kept texels: the quad's colour (one albedo, the texture's), alpha 1 (the 160 row too: alpha = 1 past the cutoff);
    # the discarded ones: the farther quad's.  The kernel never meets alpha == 0.
    assert (hdr[2:14, 30:46, 3] == 1.0).all() and (surf["alpha"][FR.covered_of(surf)] != 0.0).all()
    assert len(np.unique(quad["albedo"][keep].view(np.uint32), axis=0)) == 1 and len(np.unique(quad["albedo"][~keep].view(np.uint32), axis=0)) == 1
    assert not np.array_equal(quad["albedo"][keep][0], quad["albedo"][~keep][0])
    ar = gpu_ctx.raster_resolve(cam, draw_type=S.DrawType["Albedo"])[0][2:14, 30:46, :3]
    assert np.array_equal(ar.view(np.uint32), quad["albedo"].view(np.uint32))
    check_colour(world, cam, hdr, surf, lists_of(gpu_ctx, world), "s1 with the MASK quad")


def test_flight_helmet_with_texture_lod():
    world = flight_helmet.load_fixture(sky_size=0)
    world.add_meshlets()
    ctx = capi.Context(device=0, flags=S.CREATE_TEXTURE_MIPS)
    try:
        ctx.upload_scene(world)
        ctx.set_texture_lod(True, -1.0)
        c = world.camera
        cam = jittered_camera(tuple(c["eye"]), tuple(c["target"]), step=(0.01, 0.005, 0.0))
        previous = previous_of(world)
        ctx.set_forward_debug_surfaces(True)
        hdr, depth, vel = shade_over_generated(ctx, cam, previous_transforms=previous)
        surf = ctx.read_forward_surfaces()
        ids, _ = ctx.read_raster_visibility(CS.WIDTH, CS.HEIGHT)
        resolved = ctx.raster_resolve(cam, previous_transforms=previous)
        check_surfaces(surf, resolved, ids, world)
        assert depth.tobytes() == resolved[2].tobytes() and vel.tobytes() == resolved[3].tobytes()
        ctx.set_texture_lod(False)
        shade_over_generated(ctx, cam, previous_transforms=previous)
        assert ctx.read_forward_surfaces()["albedo"].tobytes() != surf["albedo"].tobytes()  # the LOD state applies
    finally:
        ctx.close()


# ---- 7. chaining and ownership ----

def test_the_passes_that_read_the_last_depth_and_velocity_run_over_the_forward_frame(gpu_ctx):
    w, h = EXTENTS[3]
    world = make_world("closed")
    gpu_ctx.upload_scene(world)
    gpu_ctx.raster_release_preserved()
    cam = jittered_camera(width=w, height=h)
    gpu_ctx.raster_forward(cam)
    hdr, depth, vel = outputs(gpu_ctx)
    assert gpu_ctx.velocity_device_ptr()[1:] == (w, h) and gpu_ctx.forward_depth_device_ptr()[1:] == (w, h)
    assert (depth == 0).any() and (depth != 0).any()
    # no albedo or normal target: the consumers that need them refuse, and the process goes on
    for call in (gpu_ctx.gbuffer_device_ptrs, gpu_ctx.read_gbuffer):
        with pytest.raises(capi.ProsperPtError, match="no G-buffer has been traced yet") as e:
            call()
        assert e.value.code == -4
    pc = S.DeferredShadingPC(0, 0)
    null = S.RestirInputs()
    null.onDevice = 1
    assert capi.lib().prosper_pt_deferred_shading(gpu_ctx._h, C.byref(pc), 0, 0, C.byref(cam), w, h, C.byref(null), None) == -1
    assert capi.lib().prosper_pt_deferred_shading(gpu_ctx._h, C.byref(pc), 0, 0, C.byref(cam), w, h, None, None) == -1
    # the registry: depth valid, the attribute targets not yet run
    by_name = {r.name.decode(): r for r in gpu_ctx.debug_resources()}
    assert len(by_name) == 23
    assert by_name["depth"].valid == 1 and by_name["velocity"].valid == 1
    assert by_name["albedoRoughness"].valid == 0 and by_name["normalMetalness"].valid == 0

    def restore():
        gpu_ctx.raster_forward_shade(cam)
        assert gpu_ctx.read_hdr().tobytes() == hdr.tobytes()

    # skybox_fill(NULL) against the same over a host copy of the depth
    gpu_ctx.skybox_fill(cam, w, h)
    filled = gpu_ctx.read_hdr().copy()
    restore()
    gpu_ctx.skybox_fill(cam, w, h, depth=depth)
    assert gpu_ctx.read_hdr().tobytes() == filled.tobytes() and filled.tobytes() != hdr.tobytes()
    # forward_transparent(NULL)
    restore()
    gpu_ctx.forward_transparent(cam, w, h, flags=S.TRANSPARENT_CAMERA_JITTER)
    over_null = gpu_ctx.read_hdr().copy()
    restore()
    gpu_ctx.forward_transparent(cam, w, h, flags=S.TRANSPARENT_CAMERA_JITTER, depth=depth)
    assert gpu_ctx.read_hdr().tobytes() == over_null.tobytes()
    # hiz_downsample(NULL)
    gpu_ctx.hiz_downsample(w, h, slot=0)
    for x, y in zip(gpu_ctx.read_hiz(0), CR.hiz_pyramid(depth)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # taa_resolve: velocity and depth NULL against host copies
    restore()
    gpu_ctx.taa_resolve(S.TaaPC.default(reset_history=1), w, h)
    resolved = gpu_ctx.read_hdr().copy()
    gpu_ctx.taa_resolve(S.TaaPC.default(reset_history=1), w, h, velocity=vel, depth=depth, illumination=hdr)
    assert gpu_ctx.read_hdr().tobytes() == resolved.tobytes()
    # debug_lines: depth-tested against the forward depth, which it writes: the restatement over host copies, bit for bit
    lines = np.array([[-3.0, -2.0, -3.0, 3.0, 2.0, -3.0, 1.0, 0.0, 0.0], [-3.0, 1.0, -6.0, 3.0, -1.0, -1.5, 0.0, 1.0, 0.0]], F)
    restore()
    gpu_ctx.debug_lines(lines, cam, w, h)
    lined, lined_depth = gpu_ctx.read_hdr().copy(), gpu_ctx.read_forward_depth()
    assert lined.tobytes() != hdr.tobytes() and lined_depth.tobytes() != depth.tobytes()
    import debug_view_reference as DV
    want_hdr, want_depth, _ = DV.debug_lines(lines, cam, w, h, hdr, depth)
    assert lined_depth.tobytes() == want_depth.tobytes() and lined.tobytes() == want_hdr.tobytes()
    # a traced G-buffer afterwards is what it is in a context that never ran forward
    a = gpu_ctx.trace_gbuffer_velocity(cam, w, h, opaque_only=True)
    other = capi.Context(device=0)
    try:
        other.upload_scene(world)
        b = other.trace_gbuffer_velocity(cam, w, h, opaque_only=True)
    finally:
        other.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    with pytest.raises(capi.ProsperPtError, match="not a forward frame's"):
        gpu_ctx.read_forward_depth()
    assert {r.name.decode(): r.valid for r in gpu_ctx.debug_resources()}["albedoRoughness"] == 1


def test_caller_owned_targets(gpu_ctx):
    w, h = EXTENTS[1]
    world = make_world("closed")
    gpu_ctx.upload_scene(world)
    cam = jittered_camera(width=w, height=h)
    previous = previous_of(world)
    hdr, depth, vel = shade_over_generated(gpu_ctx, cam, previous_transforms=previous)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    t_d, t_v = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(t_d), h * w * 4) == 0 and hip.hipMalloc(C.byref(t_v), h * w * 8) == 0
    try:
        gpu_ctx.raster_forward_shade(cam, previous_transforms=previous, depth_ptr=t_d.value, velocity_ptr=t_v.value)
        assert gpu_ctx.read_hdr().tobytes() == hdr.tobytes()  # (synchronises)
        own_d, own_v = np.empty((h, w), F), np.empty((h, w, 2), F)
        assert hip.hipMemcpy(own_d.ctypes.data, t_d, own_d.nbytes, 2) == 0 and hip.hipMemcpy(own_v.ctypes.data, t_v, own_v.nbytes, 2) == 0
        assert own_d.tobytes() == depth.tobytes() and own_v.tobytes() == vel.tobytes()
        # the caller's buffers are the last depth and velocity now, as after a resolve into caller-owned targets
        assert gpu_ctx.forward_depth_device_ptr()[0] == t_d.value and gpu_ctx.velocity_device_ptr()[0] == t_v.value
        gpu_ctx.raster_forward_shade(cam, previous_transforms=previous)  # back to the context's own before the buffers go
        assert gpu_ctx.forward_depth_device_ptr()[0] != t_d.value
        gpu_ctx.read_hdr()  # (synchronises)
    finally:
        hip.hipFree(t_d)
        hip.hipFree(t_v)


def test_two_streams_into_one_context(gpu_ctx):
    world = make_world("closed")
    gpu_ctx.upload_scene(world)
    gpu_ctx.raster_release_preserved()
    hip = C.CDLL("libamdhip64.so")
    s1, s2 = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s1), 1) == 0 and hip.hipStreamCreateWithFlags(C.byref(s2), 1) == 0
    try:
        small, big = CS.camera_at(width=40, height=30), CS.camera_at()
        want = None
        lib = capi.lib()
        for _ in range(2):  # the second call grows and overwrites what the first still shades; nothing waits on the host between
            pc, desc = S.ForwardPC(0, 0, 0), S.ForwardOpaqueDesc()
            assert lib.prosper_pt_raster_forward(gpu_ctx._h, C.byref(pc), C.byref(small), C.byref(desc), s1) == 0
            assert lib.prosper_pt_raster_forward(gpu_ctx._h, C.byref(pc), C.byref(big), C.byref(desc), s2) == 0
            gpu_ctx._forward_extent = (CS.WIDTH, CS.HEIGHT)
            got = (gpu_ctx.read_hdr(stream=s2.value).copy(), gpu_ctx.read_forward_depth(stream=s2.value), gpu_ctx.read_velocity(stream=s2.value))
            if want is None:
                assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
                gpu_ctx.raster_release_preserved()
                gpu_ctx.raster_forward(big)
                want = outputs(gpu_ctx)
                gpu_ctx.raster_release_preserved()
            assert all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))
    finally:
        assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
        hip.hipStreamDestroy(s1)
        hip.hipStreamDestroy(s2)


def test_refusals_leave_the_three_images_as_they_were():
    lib = capi.lib()
    world = make_world("closed")
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        cam = CS.camera_at()
        w, h = CS.WIDTH, CS.HEIGHT
        with pytest.raises(capi.ProsperPtError, match="nothing has been drawn") as e:
            ctx.raster_forward_shade(cam)  # a shade before any draw
        assert e.value.code == -4
        with pytest.raises(capi.ProsperPtError, match="not a forward frame's"):
            ctx.read_forward_depth()  # and no last depth came of it
        before = shade_over_generated(ctx, cam)

        def unchanged():
            assert all(a.tobytes() == b.tobytes() for a, b in zip(outputs(ctx), before))

        with pytest.raises(capi.ProsperPtError, match="visibility image's extent"):
            ctx.raster_forward_shade(CS.camera_at(width=40, height=30))
        unchanged()
        pc, desc = S.ForwardPC(0, 0, 0), S.ForwardOpaqueDesc()
        bad_camera = S.CameraUniforms.from_buffer_copy(bytes(cam))
        bad_camera.far_ = bad_camera.near_
        odd_depth, odd_velocity, count, wrong_count = S.ForwardOpaqueDesc(), S.ForwardOpaqueDesc(), S.ForwardOpaqueDesc(), S.ForwardOpaqueDesc()
        odd_depth.nonLinearDepth = 258
        odd_velocity.velocity = 260
        count.previousTransformCount = 3
        previous = previous_of(world)
        wrong_count.previousTransforms = C.cast(previous, C.c_void_p)
        wrong_count.previousTransformCount = len(previous) + 1
        for entry in (lib.prosper_pt_raster_forward_shade, lib.prosper_pt_raster_forward):
            for pc_, cam_, desc_, code in ((S.ForwardPC(len(S.DRAW_TYPES), 0, 0), cam, desc, -1), (S.ForwardPC(0, 2, 0), cam, desc, -1),
                                           (S.ForwardPC(0, 1, 0), cam, desc, -6), (pc, bad_camera, desc, -1), (pc, cam, odd_depth, -1),
                                           (pc, cam, odd_velocity, -1), (pc, cam, count, -1), (pc, cam, wrong_count, -1)):
                assert entry(ctx._h, C.byref(pc_), C.byref(cam_), C.byref(desc_), None) == code
            assert entry(ctx._h, None, C.byref(cam), C.byref(desc), None) == -1
            assert entry(ctx._h, C.byref(pc), None, C.byref(desc), None) == -1
            assert entry(ctx._h, C.byref(pc), C.byref(cam), None, None) == -1
            unchanged()
        # refused before the culling phases: the lists and the image are the generated draw's still
        assert ctx.raster_info().draw[1].valid == 0
        # geometry that changed since the image was drawn: a new upload forgets the image
        ctx.upload_scene(world)
        with pytest.raises(capi.ProsperPtError, match="nothing has been drawn"):
            ctx.raster_forward_shade(cam)
    finally:
        ctx.close()
    # a meshlet triangle that is no triangle of the index buffer
    bad = RS.closed_world()
    md = bad.metadatas[1]
    words = bad._buffer_words_of(md.bufferIndex)
    tri = words.view(np.uint8)[md.meshletTrianglesByteOffset:md.meshletTrianglesByteOffset + 3]
    tri[:] = tri[::-1].copy()
    bad._frozen = None
    fresh = capi.Context(device=0)
    try:
        fresh.upload_scene(bad)
        with pytest.raises(capi.ProsperPtError, match="not a triangle of the mesh's index buffer") as e:
            fresh.raster_forward(CS.camera_at())
        assert e.value.code == -5
    finally:
        fresh.close()


def test_the_cpp_forward_renderer_records_what_the_direct_call_records(gpu_ctx):
    from prosper_amd import rt_reference
    world = make_world("property")
    gpu_ctx.upload_scene(world)
    fresh = capi.Context(device=0)
    hcam = rt_reference.Camera()
    hcam.set_parameters(CS.FOV, CS.NEAR, CS.FAR)
    renderer = rt_reference.ForwardRenderer(gpu_ctx)
    w, h = CS.WIDTH, CS.HEIGHT
    try:
        fresh.upload_scene(world)
        renderer.release_preserved()
        transforms = world.freeze()["transforms"]
        for frame, eye_x in enumerate((0.0, 0.3, 0.3)):
            if frame == 2:
                renderer.release_preserved()  # the third frame starts over: one phase, no previous transforms
                fresh.raster_release_preserved()
            hcam.look_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0), (0.0, 1.0, 0.0))
            out = renderer.record_opaque(hcam, w, h, transforms=transforms)
            assert out.illumination == gpu_ctx.hdr_device_ptr()[0] and out.velocity == gpu_ctx.velocity_device_ptr()[0]
            assert (out.depth, w, h) == gpu_ctx.forward_depth_device_ptr()
            got = outputs(gpu_ctx)
            cam = CS.camera_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0))
            fresh.raster_forward(cam, previous_transforms=transforms if frame == 1 else None)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, outputs(fresh))), frame
            assert fresh.raster_info().draw[1].valid == gpu_ctx.raster_info().draw[1].valid == (1 if frame == 1 else 0)
        with pytest.raises(capi.ProsperPtError, match="drawType") as e:
            renderer.record_opaque(hcam, w, h, draw_type=11)
        assert e.value.code == -1
    finally:
        renderer.close()
        hcam.close()
        fresh.close()


def test_render_gltf_forward(tmp_path):
    out = tmp_path / "forward.png"
    script = os.path.join(ROOT, "scripts", "render_gltf.py")
    gltf = os.path.join(ROOT, "tests", "golden", "tiny_scene.gltf")
    done = subprocess.run([sys.executable, script, gltf, "--forward", "--sky", "--size", "96x64", "--out", str(out)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert out.exists() and out.stat().st_size > 100
    for extra in ("--deferred", "--restir-di"):
        refused = subprocess.run([sys.executable, script, gltf, "--forward", extra, "--out", str(out)], capture_output=True, text=True)
        assert refused.returncode == 2 and "--forward" in refused.stderr
