"""The forward transparent pass (prosper_pt_forward_transparent; forward_transparent_kernel) and the opaque-only traced
G-buffer (PROSPER_PT_GBUFFER_OPAQUE_ONLY) on the GPU: the G-buffer against a copy of the world whose BLEND materials have
alpha 0, the pass's nearest layer against the G-buffer of a copy whose BLEND materials are OPAQUE, a designed stack of
quads whose layer lists are known from projecting its corners, and the composited image against
tests/transparent_reference.py over clustered lights, IBL, the debug draw types and the host mirror.

The designed scene and its expected layers are defined here; tests/test_transparent_cpu.py checks the design itself."""
import math

import numpy as np
import pytest

import deferred_shading_reference as D
import transparent_reference as T
from conftest import same_bits
from prosper_amd import capi, scenes, structs as S
from test_traced_gbuffer import signed_oct_decode

EXTENTS = ((96, 64), (33, 17), (1, 1))
# test_deferred_shading.py's shading tolerance, relative to the pixel's sum of absolute terms
REL = 2e-4
ABS = 1e-6
LAYERS = 8  # layers per pixel the debug read-back keeps in these tests (the designed stack is 6 deep)
DEEP = 48   # the same for the small sponza's foliage
MODES = ("centre", "jitter", "camera_jitter")
FRAME = 3


# ---- the designed stack ----
#
# The camera looks down -z from (0, 0, 4).  Every quad is perpendicular to the view axis and taller than the view, so
# only vertical edges show, and every vertical edge lies on one of three lines through the eye, x = t * distance with
# t = -0.25, 0, 0.25: the edge pixels (left out of the layer-sequence check) are three pairs of columns.  All corner
# coordinates are multiples of 1/16 below 8: exact in the binary16 the geometry is stored in.
EYE_Z = 4.0
# (name, z, (t0, t1), kind, rgba)   kind: "opaque", "blend", "away" (BLEND, wound clockwise), "texture" (BLEND, alpha 0
# in the texture's left half)
DESIGN = (
    ("wall", -1.0, (-0.75, 0.25), "opaque", (0.7, 0.7, 0.7, 1.0)),
    ("L3", 0.5, (-0.75, 0.75), "blend", (0.1, 0.8, 0.2, 0.7)),       # the four parallel layers, in shuffled order
    ("L1", 1.5, (-0.75, 0.0), "blend", (0.9, 0.1, 0.1, 0.3)),
    ("L4", 0.0, (0.0, 0.75), "blend", (0.9, 0.8, 0.1, 0.4)),
    ("L2", 1.0, (-0.25, 0.75), "blend", (0.1, 0.2, 0.9, 0.5)),
    ("zero", 2.0, (-0.75, 0.75), "blend", (1.0, 1.0, 1.0, 0.0)),     # alpha 0: never a layer
    ("texture", 1.75, (-0.75, 0.75), "texture", (0.8, 0.3, 0.8, 1.0)),
    ("away", 1.25, (-0.75, 0.75), "away", (0.2, 0.9, 0.9, 0.5)),     # faces away: culled
    ("behind", -2.0, (0.0, 0.75), "blend", (0.5, 0.5, 0.1, 0.6)),    # behind the wall where the wall is, over the sky past it
    ("D1", 0.75, (-0.25, 0.25), "blend", (0.9, 0.5, 0.1, 0.25)),     # two coplanar duplicates
    ("D2", 0.75, (-0.25, 0.25), "blend", (0.1, 0.5, 0.9, 0.6)),
)
TEXTURE_ALPHA = 204  # of the texture's right half


def designed_scene():
    """The world; draw instance k is DESIGN[k]."""
    w = scenes.World()
    tex = np.zeros((4, 4, 4), np.uint8)
    tex[..., :3] = 255
    tex[:, 2:, 3] = TEXTURE_ALPHA
    texture = w.add_texture(tex)
    nearest = w.add_sampler(S.FILTER_NEAREST, S.FILTER_NEAREST, S.WRAP_CLAMP_TO_EDGE, S.WRAP_CLAMP_TO_EDGE)
    for name, z, (t0, t1), kind, rgba in DESIGN:
        dist = EYE_Z - z
        x0, x1, y0, y1 = t0 * dist, t1 * dist, -0.5 * dist, 0.5 * dist
        for v in (x0, x1, y0, y1, z):
            assert float(np.float16(v)) == v, (name, v)
        mode = S.ALPHA_MODE_OPAQUE if kind == "opaque" else S.ALPHA_MODE_BLEND
        extra = {"base_tex": (texture, nearest)} if kind == "texture" else {}
        mat = w.add_material(base_color=rgba, metallic=0.1 if name != "L2" else 0.8, roughness=0.3 + 0.05 * len(w.materials),
                             alpha_mode=mode, **extra)
        corners = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]  # counter-clockwise seen from +z, the camera's side
        if kind == "away":
            corners.reverse()
        mesh = scenes._add(w, scenes.quad(*corners), mat)
        w.add_instance(w.add_model([(mesh, mat)]))
    w.add_point_light((1.0, 0.9, 0.8), 60.0, (0.75, 1.0, 3.0))
    w.add_spot_light((0.8, 0.9, 1.0), 80.0, (-1.0, 0.5, 3.5), (0.3, -0.1, -1.0), math.radians(25.0), math.radians(40.0))
    w.camera = dict(eye=(0.0, 0.0, EYE_Z), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=math.radians(40.0), zN=0.1, zF=50.0)
    w.skybox = scenes.sky_cube(32)
    return w


def camera(oracle, world, w, h):
    c = world.camera
    return oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)[0]


def pixel_coordinates(cam, points, w, h):
    """World points [n, 3] in pixel units, float64 [n, 2]: (ndc * 0.5 + 0.5) * extent of cameraToClip * worldToCamera,
    the inverse of the primary ray's uv -> direction (pinhole_camera_ray)."""
    clip = np.concatenate([points, np.ones((len(points), 1))], axis=-1) @ (D.mat(cam.cameraToClip) @ D.mat(cam.worldToCamera)).T
    return (clip[:, :2] / clip[:, 3:4] * 0.5 + 0.5) * np.array([w, h], np.float64)


def expected_layers(cam, w, h, offset=(0.5, 0.5)):
    """(sequences, undecided): per pixel the tuple of DESIGN indices of its layers front to back, and the pixels whose
    sample lies within one pixel of a projected quad edge (or of the texture's alpha boundary).  `offset`: the sample's
    position in the pixel, [h, w, 2] or one pair."""
    py, px = np.mgrid[0:h, 0:w]
    off = np.broadcast_to(np.asarray(offset, np.float64), (h, w, 2))
    sx, sy = px + off[..., 0], py + off[..., 1]
    undecided = np.zeros((h, w), bool)
    covers = []
    for name, z, (t0, t1), kind, rgba in DESIGN:
        dist = EYE_Z - z
        lo_t = 0.0 if kind == "texture" else t0  # left of the boundary the texture's alpha is 0
        corners = np.array([[lo_t * dist, -0.5 * dist, z], [t1 * dist, 0.5 * dist, z], [t0 * dist, 0.0, z]])
        p = pixel_coordinates(cam, corners, w, h)
        x0, x1 = sorted((p[0, 0], p[1, 0]))
        y0, y1 = sorted((p[0, 1], p[1, 1]))
        inside = (sx > x0) & (sx < x1) & (sy > y0) & (sy < y1)
        for edge in (x0, x1, p[2, 0]):
            undecided |= (np.abs(sx - edge) <= 1.0) & (sy > y0 - 1.0) & (sy < y1 + 1.0)
        for edge in (y0, y1):
            undecided |= (np.abs(sy - edge) <= 1.0) & (sx > x0 - 1.0) & (sx < x1 + 1.0)
        covers.append(inside)
    wall = covers[0]
    wall_z = DESIGN[0][1]
    # nearest first: larger z; coplanar: the lower draw instance
    order = sorted(range(1, len(DESIGN)), key=lambda k: (-DESIGN[k][1], k))
    seq = np.empty((h, w), object)
    for y in range(h):
        for x in range(w):
            s = []
            for k in order:
                name, z, _, kind, rgba = DESIGN[k]
                if kind == "away" or rgba[3] == 0.0 or not covers[k][y, x]:
                    continue
                if wall[y, x] and not z > wall_z:
                    continue
                s.append(k)
            seq[y, x] = tuple(s)
    return seq, undecided


def layer_alpha(k):
    return TEXTURE_ALPHA / 255.0 if DESIGN[k][3] == "texture" else DESIGN[k][4][3]


# ---- GPU helpers ----

def make_world(scene):
    if scene == "c2":
        return scenes.cornell(with_skybox=True)
    if scene == "c4":
        return scenes.sponza_class(lights=(64, 32), foliage=True, texture_size=64, sky_size=32, detail=0.25)
    return designed_scene()


def blend_materials(world):
    return [m for m in world.materials if m.alphaMode == S.ALPHA_MODE_BLEND]


def opaque_copy(scene):
    """A copy of the world with every BLEND material switched to OPAQUE.  In the designed scene the two quads that can
    never be a layer (alpha 0, facing away) would then hide the whole stack: they get alpha 0 instead, which the
    stochastic any-hit always rejects."""
    copy = make_world(scene)
    for k, m in enumerate(copy.materials):
        if m.alphaMode != S.ALPHA_MODE_BLEND:
            continue
        if scene == "designed" and DESIGN[k - 1][0] in ("zero", "away"):  # (material 0 is the world's default material)
            m.baseColorFactor.w = 0.0
        else:
            m.alphaMode = S.ALPHA_MODE_OPAQUE
    return copy


def mode_camera(oracle, world, w, h, mode):
    cam = camera(oracle, world, w, h)
    if mode == "camera_jitter":
        cam.currentJitter[0], cam.currentJitter[1] = 0.6 / w, -0.4 / h  # NDC: 0.3 and 0.2 of a pixel
    return cam


def trace(ctx, cam, w, h, mode, opaque_only, draw_type=0):
    """The G-buffer (ar, nm, depth) in one of the three ray modes."""
    if mode == "camera_jitter":
        return ctx.trace_gbuffer_velocity(cam, w, h, draw_type=draw_type, frame_index=FRAME, opaque_only=opaque_only)[:3]
    return ctx.trace_gbuffer(cam, w, h, draw_type=draw_type, frame_index=FRAME, jitter=mode == "jitter", opaque_only=opaque_only)


def mode_flags(mode):
    return {"centre": 0, "jitter": S.TRANSPARENT_JITTER, "camera_jitter": S.TRANSPARENT_CAMERA_JITTER}[mode]


def run_pass(ctx, cam, w, h, mode="centre", draw_type=0, ibl=0, keep=LAYERS):
    """The deferred frame up to the pass, then the pass in debug mode: (input image, output image, counts, layers, depth)."""
    ctx.set_transparent_debug_layers(keep)
    ar, nm, depth = trace(ctx, cam, w, h, mode, True)
    inp, _, _ = ctx.gbuffer_device_ptrs()
    ctx.deferred_shading_device(cam, w, h, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth, ibl=ibl)
    ctx.skybox_fill(cam, w, h)
    before = ctx.read_hdr()
    ctx.forward_transparent(cam, w, h, draw_type=draw_type, ibl=ibl, flags=mode_flags(mode), frame_index=FRAME)
    after = ctx.read_hdr()
    counts, layers = ctx.read_transparent_layers()
    ctx.set_transparent_debug_layers(0)
    return before, after, counts, layers, depth


def check_image(world, cam, before, after, counts, layers, lists, what, maps=None, margin_cap=0.99):
    """The composited image against the restatement; pixels without layers bit for bit the input."""
    none = counts == 0
    assert same_bits(after[none], before[none]).all(), "%s: a pixel without layers changed" % what
    want, alpha, scale, margin = T.composite(world, cam, counts, layers, before, lists=lists, maps=maps)
    has = ~none
    if not has.any():
        return
    ok = has & (margin > 1e-4)  # the slice pick was not a coin flip between fp32 and float64 (test_deferred_shading.py)
    assert ok.sum() >= margin_cap * has.sum(), what
    err = np.abs(after[..., :3].astype(np.float64) - want).max(-1)
    print("%s: %d pixels with layers (deepest %d), worst error %.3g of scale %.3g" % (
        what, has.sum(), counts.max(), err[ok].max(), scale[ok][np.argmax(err[ok])]))
    bad = ok & ~(err <= REL * scale + ABS)
    assert not bad.any(), "%s: %d pixels off, worst %.3g of %.3g" % (what, bad.sum(), err[bad].max(), scale[bad][np.argmax(err[bad])])
    aerr = np.abs(after[..., 3][has].astype(np.float64) - alpha[has]).max()
    assert aerr <= 1e-6, "%s: alpha off by %.3g" % (what, aerr)


# ---- 1. the opaque-only G-buffer ----

@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["c2", "c4"])
def test_gpu_opaque_only_gbuffer_is_the_gbuffer_without_blend_surfaces(gpu_ctx, oracle, scene):
    """All targets byte-identical to the plain G-buffer of a copy of the world whose BLEND materials have
    baseColorFactor.a = 0 (same geometry, same hierarchy: the stochastic any-hit always rejects alpha 0)."""
    world, copy = make_world(scene), make_world(scene)
    assert blend_materials(world)
    for m in blend_materials(copy):
        m.baseColorFactor.w = 0.0
    w, h = EXTENTS[0]
    cam = mode_camera(oracle, world, w, h, "camera_jitter")
    got = {}
    gpu_ctx.upload_scene(world)
    for jitter in (False, True):
        got[jitter] = gpu_ctx.trace_gbuffer(cam, w, h, frame_index=FRAME, jitter=jitter, opaque_only=True)
        plain = gpu_ctx.trace_gbuffer(cam, w, h, frame_index=FRAME, jitter=jitter)
        assert any(a.tobytes() != b.tobytes() for a, b in zip(got[jitter], plain)), "the flag changes nothing: no BLEND surface in view"
    got["velocity"] = gpu_ctx.trace_gbuffer_velocity(cam, w, h, frame_index=FRAME, opaque_only=True)
    gpu_ctx.upload_scene(copy)
    for jitter in (False, True):
        want = gpu_ctx.trace_gbuffer(cam, w, h, frame_index=FRAME, jitter=jitter)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[jitter], want)), (scene, jitter)
    want = gpu_ctx.trace_gbuffer_velocity(cam, w, h, frame_index=FRAME)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["velocity"], want)), scene
    assert got["velocity"][3].any()  # a jittered camera: the velocity target is not all zero


# ---- 2. the nearest layer against the G-buffer of an OPAQUE copy ----

@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["c2", "c4", "designed"])
def test_gpu_nearest_layer_is_the_opaque_copys_gbuffer_texel(gpu_ctx, oracle, scene):
    """The copy's G-buffer shows a pixel's nearest layer wherever nothing the pass does not count lies in front of it
    in the copy: a BLEND surface seen from behind (the ray tracer does not cull) or one whose alpha texture is 0 there
    (the copy ignores alpha).  Those pixels are told apart by the depth - the copy's surface must then be nearer -, the
    others compared with test_traced_gbuffer.py's tolerances."""
    world, copy = make_world(scene), opaque_copy(scene)
    w, h = EXTENTS[0]
    keep = DEEP if scene == "c4" else LAYERS
    results = {}
    gpu_ctx.upload_scene(world)
    for mode in MODES:
        cam = mode_camera(oracle, world, w, h, mode)
        results[mode] = (cam,) + run_pass(gpu_ctx, cam, w, h, mode, keep=keep)
    gpu_ctx.upload_scene(copy)
    total = 0
    for mode in MODES:
        cam, _, _, counts, layers, depth = results[mode]
        ar, nm, cdepth = trace(gpu_ctx, cam, w, h, mode, False)
        first = layers[..., 0]
        # where the copy's nearest surface is the layer itself (not an opaque or MASK surface in front, and not a layer
        # the original's alpha texture makes transparent)
        has = (counts > 0) & (np.abs(cdepth - first["nonLinearDepth"]) <= 1e-6)
        hidden = (counts > 0) & ~has
        assert (cdepth[hidden] > first["nonLinearDepth"][hidden]).all(), "%s %s: a layer in front of the copy's surface" % (scene, mode)
        print("%s %s: %d pixels with layers, %d of them the copy's surface" % (scene, mode, (counts > 0).sum(), has.sum()))
        assert has.sum() > 0, (scene, mode)
        total += has.sum()
        f = first[has]
        assert same_bits(f["albedo"], ar[has][:, :3]).all(), (scene, mode)
        assert same_bits(f["roughness"], ar[has][:, 3]).all() and same_bits(f["metallic"], nm[has][:, 2]).all(), (scene, mode)
        nerr = np.abs(signed_oct_decode(nm[has]) - f["normal"].astype(np.float64)).max()
        assert nerr <= 2e-6, "%s %s: normal off by %.3g" % (scene, mode, nerr)
        # every layer lies in front of the stored depth, nearest first
        k = np.arange(keep)
        live = k[None, None, :] < np.minimum(counts, keep)[..., None]
        d = layers["nonLinearDepth"]
        assert (d[live] > np.broadcast_to(depth[..., None], d.shape)[live]).all(), (scene, mode)
        both = live[..., 1:] & live[..., :-1]
        assert (d[..., :-1][both] >= d[..., 1:][both]).all(), (scene, mode)
    assert total > 100


# ---- 3. the designed stack ----

def _sample_offsets(w, h, mode, cam):
    if mode == "jitter":
        import restir_resampling_reference as R
        py, px = np.mgrid[0:h, 0:w]
        jx, jy = R.Rng(px.astype(np.uint32), py.astype(np.uint32), FRAME).rnd2d01()
        return np.stack([jx, jy], axis=-1).astype(np.float64)
    if mode == "camera_jitter":
        return (0.5 - cam.currentJitter[0] * 0.5 * w, 0.5 - cam.currentJitter[1] * 0.5 * h)
    return (0.5, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%d" % e)
def test_gpu_designed_stack(gpu_ctx, oracle, extent):
    w, h = extent
    world = designed_scene()
    gpu_ctx.upload_scene(world)
    for mode in MODES:
        what = "designed %dx%d %s" % (w, h, mode)
        cam = mode_camera(oracle, world, w, h, mode)
        before, after, counts, layers, depth = run_pass(gpu_ctx, cam, w, h, mode)
        seq, undecided = expected_layers(cam, w, h, _sample_offsets(w, h, mode, cam))
        if (w, h) == EXTENTS[0]:
            assert undecided.mean() <= 0.10, what
        checked = 0
        for y, x in zip(*np.nonzero(~undecided)):
            got = tuple(int(v) for v in layers["drawInstance"][y, x, :counts[y, x]])
            assert got == seq[y, x], "%s: pixel (%d, %d) has layers %s, expected %s" % (what, x, y, got, seq[y, x])
            assert np.allclose(layers["alpha"][y, x, :counts[y, x]], [layer_alpha(k) for k in got], rtol=0, atol=1e-6), what
            checked += 1
        if (w, h) == EXTENTS[0]:
            deepest = max(len(s) for s in seq[~undecided])
            assert deepest == 6 and counts[~undecided].max() == 6 and (counts[~undecided] == 0).sum() == 0, what
        gpu_ctx.cluster_lights(cam, w, h)
        lists = D.membership(gpu_ctx.read_light_clusters(), world.point_lights.count, world.spot_lights.count)
        check_image(world, cam, before, after, counts, layers, lists, what)
        info = gpu_ctx.transparent_info()
        assert (info.coveredPixels, info.totalLayers, info.maxLayers) == ((counts > 0).sum(), counts.sum(), counts.max()), what
        # two calls on the same input
        again = run_pass(gpu_ctx, cam, w, h, mode)
        assert again[0].tobytes() == before.tobytes() and again[1].tobytes() == after.tobytes(), what
        assert again[2].tobytes() == counts.tobytes(), what
        # the debug mode does not change the image
        trace(gpu_ctx, cam, w, h, mode, True)
        inp, _, _ = gpu_ctx.gbuffer_device_ptrs()
        gpu_ctx.deferred_shading_device(cam, w, h, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
        gpu_ctx.skybox_fill(cam, w, h)
        gpu_ctx.forward_transparent(cam, w, h, flags=mode_flags(mode), frame_index=FRAME)
        assert gpu_ctx.read_hdr().tobytes() == after.tobytes(), what
        with pytest.raises(capi.ProsperPtError):
            gpu_ctx.read_transparent_layers()


@pytest.mark.gpu
def test_gpu_pixels_without_layers_keep_their_bits_and_depth_inputs_agree(gpu_ctx, oracle):
    """A scene without BLEND surfaces leaves the image alone; a caller-owned host or device depth gives the image the
    traced depth gives; a depth of 1 everywhere (everything at the near plane) hides every layer."""
    w, h = EXTENTS[1]
    world = designed_scene()
    cam = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    before, after, counts, layers, depth = run_pass(gpu_ctx, cam, w, h)
    assert (counts > 0).any()
    for kind in ("host", "device", "near"):
        trace(gpu_ctx, cam, w, h, "centre", True)
        inp, _, _ = gpu_ctx.gbuffer_device_ptrs()
        gpu_ctx.deferred_shading_device(cam, w, h, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
        gpu_ctx.skybox_fill(cam, w, h)
        if kind == "host":
            gpu_ctx.forward_transparent(cam, w, h, depth=depth)
        elif kind == "device":
            gpu_ctx.forward_transparent(cam, w, h, depth_ptr=inp.nonLinearDepth)  # the traced depth, as the caller's
        else:
            gpu_ctx.forward_transparent(cam, w, h, depth=np.ones((h, w), np.float32))
        got = gpu_ctx.read_hdr()
        assert got.tobytes() == (before if kind == "near" else after).tobytes(), kind
    assert gpu_ctx.transparent_info().coveredPixels == 0
    masked = designed_scene()
    for m in blend_materials(masked):
        m.alphaMode = S.ALPHA_MODE_MASK
    gpu_ctx.upload_scene(masked)
    b2, a2, c2, _, _ = run_pass(gpu_ctx, cam, w, h)
    assert not c2.any() and a2.tobytes() == b2.tobytes()


# ---- 4. clustered lights ----

@pytest.mark.gpu
def test_gpu_clustered_lights_and_queued_light_update(oracle):
    world = make_world("c4")
    w, h = EXTENTS[0]
    cam = camera(oracle, world, w, h)
    n_point, n_spot = world.point_lights.count, world.spot_lights.count
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        before, after, counts, layers, _ = run_pass(ctx, cam, w, h, keep=DEEP)
        assert (counts > 0).mean() > 0.01
        # run_pass's deferred shading clustered for this camera: the pass reused it
        assert ctx.transparent_info().reclustered == 0
        lists = D.membership(ctx.read_light_clusters(), n_point, n_spot)
        check_image(world, cam, before, after, counts, layers, lists, "c4")
        # a queued light update: the next call clusters again and matches the new lights; the one after reuses
        for i in range(n_point):
            world.point_lights.lights[i].radianceAndRadius.x *= 3.0
            world.point_lights.lights[i].position.y += 0.25
        ctx.update_lights(world)
        ctx.set_transparent_debug_layers(DEEP)
        ctx.forward_transparent(cam, w, h)  # over `after`: the input of this call
        assert ctx.transparent_info().reclustered == 1
        twice = ctx.read_hdr()
        counts2, layers2 = ctx.read_transparent_layers()
        assert counts2.tobytes() == counts.tobytes()
        lists2 = D.membership(ctx.read_light_clusters(), n_point, n_spot)
        check_image(world, cam, after, twice, counts2, layers2, lists2, "c4 after update_lights")
        ctx.forward_transparent(cam, w, h)
        assert ctx.transparent_info().reclustered == 0
        thrice = ctx.read_hdr()
        counts3, layers3 = ctx.read_transparent_layers()
        check_image(world, cam, twice, thrice, counts3, layers3, lists2, "c4, the clustering reused")
        # another extent: clustered again
        cam2 = camera(oracle, world, *EXTENTS[1])
        run_pass(ctx, cam2, *EXTENTS[1])
        ctx.cluster_lights(cam, w, h)
        ctx.forward_transparent(cam2, *EXTENTS[1])
        assert ctx.transparent_info().reclustered == 1
    finally:
        ctx.close()


# ---- 5. ibl = 1 ----

@pytest.mark.gpu
def test_gpu_ibl(oracle):
    world = designed_scene()
    w, h = EXTENTS[0]
    cam = camera(oracle, world, w, h)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        run_pass(ctx, cam, w, h)
        with pytest.raises(capi.ProsperPtError) as e:
            ctx.forward_transparent(cam, w, h, ibl=1)
        assert e.value.code == -6 and "prosper_pt_generate_ibl" in str(e.value)
        ctx.generate_ibl()
        maps = ctx.read_ibl()
        before, after, counts, layers, _ = run_pass(ctx, cam, w, h, ibl=1)
        lists = D.membership(ctx.read_light_clusters(), world.point_lights.count, world.spot_lights.count)
        plain = run_pass(ctx, cam, w, h, ibl=0)
    finally:
        ctx.close()
    # the quads face the camera: no layer is near the LUT's grazing column, where test_image_based_lighting.py widens
    sf = T.LayerSurfaces(cam, layers[..., 0][counts > 0], 0, 0)
    assert (sf.NoV > 1.5 / 512).all()
    check_image(world, cam, before, after, counts, layers, lists, "designed ibl", maps=maps)
    assert (after[..., :3][counts > 0] != plain[1][..., :3][counts > 0]).any()


# ---- 6. debug draw types ----

@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["c2", "designed"])
def test_gpu_debug_draw_types_show_the_nearest_layer(gpu_ctx, oracle, scene):
    world, copy = make_world(scene), opaque_copy(scene)
    w, h = EXTENTS[0]
    cam = camera(oracle, world, w, h)
    got = {}
    gpu_ctx.upload_scene(world)
    for dt in range(len(S.DRAW_TYPES)):
        got[dt] = run_pass(gpu_ctx, cam, w, h, draw_type=dt)
    gpu_ctx.upload_scene(copy)
    _, _, cdepth = gpu_ctx.trace_gbuffer(cam, w, h, frame_index=FRAME, jitter=False)
    for dt in range(len(S.DRAW_TYPES)):
        before, after, counts, layers, depth = got[dt]
        has = (counts > 0) & (np.abs(cdepth - layers[..., 0]["nonLinearDepth"]) <= 1e-6)
        assert has.sum() > 100
        if dt in (S.DrawType["Default"], S.DrawType["MeshletID"]):
            assert after.tobytes() == got[0][1].tobytes(), dt
            continue
        view, _, _ = gpu_ctx.trace_gbuffer(cam, w, h, draw_type=dt, frame_index=FRAME, jitter=False)
        assert same_bits(after[has][:, :3], view[has][:, :3]).all(), S.DRAW_TYPES[dt]
        assert (after[has][:, 3] == 0.0).all(), "alpha 1: a (1 - a) = 0"
        none = counts == 0
        assert same_bits(after[none], before[none]).all(), dt


# ---- 7. the host mirror ----

@pytest.mark.gpu
def test_gpu_host_mirror_equals_the_c_entry(oracle):
    from prosper_amd.rt_reference import Camera, DeferredShading, ForwardRenderer, GBufferTracer, SkyboxRenderer
    world = designed_scene()
    w, h = EXTENTS[0]
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        hcam = Camera.from_world(world, w, h)
        cam, _ = hcam.update_buffer()
        _, direct, counts, _, _ = run_pass(ctx, cam, w, h)
        assert (counts > 0).any()
        tracer, shading, sky, forward = GBufferTracer(ctx), DeferredShading(ctx), SkyboxRenderer(ctx), ForwardRenderer(ctx)
        gb = tracer.record(hcam, w, h, jitter=False, opaque_only=True)
        shading.record_device(hcam, gb, w, h)
        sky.record(hcam, w, h)
        pc = forward.record_transparent(hcam, w, h)
        assert (pc.drawType, pc.ibl) == (0, 0)
        assert ctx.read_hdr().tobytes() == direct.tobytes()
        with pytest.raises(capi.ProsperPtError):
            forward.record_transparent(hcam, w, h, apply_ibl=True)
        for closable in (tracer, shading, sky, forward):
            closable.close()
    finally:
        ctx.close()
