"""The rasterised transparent pass on the GPU (prosper_pt_raster_forward_transparent, prosper_pt_raster_transparent_draw;
DESIGN.md f20): its per-pixel fragment lists against tests/raster_transparent_reference.py, deep pixels, the colour against
tests/transparent_reference.py over the pass's own layer read-back, the traced pass over the same depth and image, the
forward and the deferred chain around it, and the plumbing."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import culling_reference as CR
import deferred_shading_reference as D
import raster_reference as R
import raster_transparent_reference as RT
from conftest import same_bits
from prosper_amd import capi, scenes, structs as S
from test_transparent import camera, check_image, designed_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EXTENTS = ((48, 32), (33, 17), (1, 1), (96, 64), (257, 5))  # 257 x 5: pixel counts across the scan's blocks of 1024
LAYERS = 8  # the designed stack is 6 deep


def designed():
    world = designed_scene()
    assert world.add_meshlets() > 0
    return world


def opaque_frame(ctx, cam):
    """the forward opaque image of the unculled list (any extent, 1 x 1 included): HDR image, depth and velocity"""
    ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
    ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True)
    ctx.raster_forward_shade(cam)
    return ctx.read_hdr().copy(), ctx.read_forward_depth(), ctx.read_velocity()


def keys_of(world, fragments):
    base = np.array(R.meshlet_base(world), np.int64)
    low = (base[fragments["drawInstance"].astype(np.int64)] + fragments["meshlet"]) * 128 + fragments["triangle"]
    return (fragments["depth"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (~low.astype(np.uint64) & np.uint64(0xFFFFFFFF))


def per_pixel(counts, keys):
    h, w = counts.shape
    starts = np.concatenate([[0], np.cumsum(counts.ravel().astype(np.int64))]).astype(np.int64)
    return [[keys[starts[y * w + x]:starts[y * w + x + 1]].tolist() for x in range(w)] for y in range(h)]


def check_lists(world, cam, stored, counts, fragments, what, pairs=None):
    """counts and sorted fragments against the restatement, exactly; a fragment whose uv lies on a texel border of the
    alpha texture (raster_transparent_reference.UNDECIDED) may be in the list or not"""
    assert counts.sum() == len(fragments), what
    got = per_pixel(counts, keys_of(world, fragments))
    pairs = CR.generate(world, CR.MODE_TRANSPARENT) if pairs is None else pairs
    sure, maybe = RT.lists(world, cam, pairs, stored)
    undecided = 0
    for y in range(counts.shape[0]):
        for x in range(counts.shape[1]):
            g = got[y][x]
            assert all(a > b for a, b in zip(g, g[1:])), "%s: pixel (%d, %d): keys not unique or not sorted front to back" % (what, x, y)
            if maybe[y][x]:
                undecided += 1
                assert set(sure[y][x]) <= set(g) <= set(sure[y][x]) | maybe[y][x], "%s: pixel (%d, %d)" % (what, x, y)
            else:
                assert g == sure[y][x], "%s: pixel (%d, %d): %s, expected %s" % (
                    what, x, y, [RT.decode_key(world, k) for k in g], [RT.decode_key(world, k) for k in sure[y][x]])
    print("%s: %d fragments, deepest pixel %d, %d pixels on a texel border" % (what, len(fragments), counts.max(initial=0), undecided))
    assert undecided <= max(counts.shape[0], 0.02 * counts.size), what  # one column of pixel centres at the most
    return got


# ---- 1. the lists ----

@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%d" % e)
def test_lists_equal_the_restatement(gpu_ctx, oracle, extent):
    w, h = extent
    world = designed()
    cam = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    before, stored, _ = opaque_frame(gpu_ctx, cam)
    gpu_ctx.raster_forward_transparent(cam)
    counts, fragments = gpu_ctx.read_raster_fragments()
    what = "designed %dx%d" % extent
    check_lists(world, cam, stored, counts, fragments, what)
    assert counts.sum() > 0 and (w % 2 or counts.max() == 6)  # (an odd width puts a column of pixel centres on the stack's edges)
    info = gpu_ctx.raster_transparent_info()
    assert info is not None and (info.fragments, info.coveredPixels, info.maxLayers) == (counts.sum(), (counts > 0).sum(), counts.max())
    first_phase = (counts.copy(), fragments.copy(), gpu_ctx.read_hdr().copy())
    stats = gpu_ctx.draw_stats()
    want = CR.totals(world, CR.MODE_TRANSPARENT)
    assert all(getattr(stats, k) == v for k, v in want.items()), "DrawStats are the TRANSPARENT first phase's"
    # the same lists from GENERATED (the cull drops nothing visible here) ...
    pairs, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_GENERATED)
    assert sorted(map(tuple, pairs.tolist())) == sorted(map(tuple, CR.generate(world, CR.MODE_TRANSPARENT).tolist()))
    opaque_frame(gpu_ctx, cam)
    gpu_ctx.cull_first_phase(cam, S.CULL_MODE_TRANSPARENT)
    gpu_ctx.raster_transparent_draw(cam, S.DRAW_LIST_GENERATED)
    counts2, fragments2 = gpu_ctx.read_raster_fragments()
    assert counts2.tobytes() == first_phase[0].tobytes() and fragments2.tobytes() == first_phase[1].tobytes(), what
    assert gpu_ctx.read_hdr().tobytes() == first_phase[2].tobytes(), what
    # ... and from a shuffled list
    list_ptr, _, capacity = gpu_ctx.draw_list_device_ptr(S.DRAW_LIST_GENERATED)
    shuffled = np.ascontiguousarray(pairs[np.random.default_rng(5).permutation(len(pairs))])
    assert len(pairs) <= capacity and not np.array_equal(shuffled, pairs)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    opaque_frame(gpu_ctx, cam)
    gpu_ctx.cull_first_phase(cam, S.CULL_MODE_TRANSPARENT)
    gpu_ctx.read_draw_list(S.DRAW_LIST_GENERATED)  # (synchronises: the generator has written the list)
    list_ptr, _, capacity = gpu_ctx.draw_list_device_ptr(S.DRAW_LIST_GENERATED)
    assert hip.hipMemcpy(list_ptr + 4, shuffled.ctypes.data, shuffled.nbytes, 1) == 0
    gpu_ctx.raster_transparent_draw(cam, S.DRAW_LIST_GENERATED)
    counts3, fragments3 = gpu_ctx.read_raster_fragments()
    assert counts3.tobytes() == first_phase[0].tobytes() and fragments3.tobytes() == first_phase[1].tobytes(), what
    assert gpu_ctx.read_hdr().tobytes() == first_phase[2].tobytes(), what


# ---- 2. deep pixels ----

def stack_world(n, opaque_at=None):
    """n BLEND quads that fill the view, parallel to the image, their depth order a permutation of their draw order;
    `opaque_at`: the quad at that position of the depth order has alpha 1"""
    world = scenes.World()
    order = np.random.default_rng(n).permutation(n) if n else np.zeros(0, np.int64)
    for k in range(n):
        z = 2.0 - order[k] / 32.0  # exact in binary16
        alpha = 1.0 if opaque_at is not None and order[k] == opaque_at else 0.2 + 0.6 * ((k * 7) % 11) / 11.0
        mat = world.add_material(base_color=(0.2 + 0.1 * (k % 7), 0.9 - 0.1 * (k % 5), 0.3, alpha), metallic=0.1, roughness=0.5, alpha_mode=S.ALPHA_MODE_BLEND)
        mesh = scenes._add(world, scenes.quad((-4.0, -4.0, z), (4.0, -4.0, z), (4.0, 4.0, z), (-4.0, 4.0, z)), mat)
        world.add_instance(world.add_model([(mesh, mat)]))
    # one opaque quad far behind, so that the scene has an opaque list too
    mat = world.add_material(base_color=(0.5, 0.5, 0.5, 1.0), metallic=0.0, roughness=0.8)
    mesh = scenes._add(world, scenes.quad((-8.0, -8.0, -4.0), (8.0, -8.0, -4.0), (8.0, 8.0, -4.0), (-8.0, 8.0, -4.0)), mat)
    world.add_instance(world.add_model([(mesh, mat)]))
    world.add_point_light((1.0, 0.9, 0.8), 60.0, (0.75, 1.0, 3.0))
    world.camera = dict(eye=(0.0, 0.0, 4.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=math.radians(40.0), zN=0.1, zF=50.0)
    world.add_meshlets()
    return world, order


@pytest.mark.parametrize("n", [0, 1, 2, 17, 65])
def test_deep_pixels(gpu_ctx, oracle, n):
    for opaque_at in (None, n // 2) if n > 1 else (None,):
        world, order = stack_world(n, opaque_at)
        gpu_ctx.upload_scene(world)
        front_to_back = np.argsort(order).tolist()  # draw instances, nearest first
        for w, h in ((1, 1), (8, 8)):
            cam = camera(oracle, world, w, h)
            before, stored, velocity = opaque_frame(gpu_ctx, cam)
            gpu_ctx.set_raster_transparent_debug_layers(128)
            try:
                gpu_ctx.raster_forward_transparent(cam)
                counts, fragments = gpu_ctx.read_raster_fragments()
                shaded, layers = gpu_ctx.read_raster_transparent_layers()
            finally:
                gpu_ctx.set_raster_transparent_debug_layers(0)
            after = gpu_ctx.read_hdr()
            what = "%d quads, %s, %dx%d" % (n, opaque_at, w, h)
            assert (counts == n).all(), what
            for y, x in np.ndindex(h, w):
                i = (y * w + x) * n
                assert fragments["drawInstance"][i:i + n].tolist() == front_to_back, what
            ends = n if opaque_at is None else opaque_at + 1
            assert (shaded == ends).all(), what
            assert all(layers["drawInstance"][y, x, :ends].tolist() == front_to_back[:ends] for y, x in np.ndindex(h, w)), what
            info = gpu_ctx.raster_transparent_info()
            assert (info.fragments, info.coveredPixels, info.shadedLayers, info.maxLayers) == (n * w * h, (w * h if n else 0), ends * w * h, n), what
            assert gpu_ctx.read_forward_depth().tobytes() == stored.tobytes() and gpu_ctx.read_velocity().tobytes() == velocity.tobytes()
            if n == 0:
                assert after.tobytes() == before.tobytes(), what
                continue
            gpu_ctx.cluster_lights(cam, w, h)
            lists = D.membership(gpu_ctx.read_light_clusters(), world.point_lights.count, world.spot_lights.count)
            check_image(world, cam, before, after, shaded, layers, lists, what, margin_cap=0.0)


# ---- 3. colour ----

def transparent_frame(ctx, cam, ibl=0, draw_type=0, keep=LAYERS):
    """the forward opaque frame, then the pass in debug mode: (input image, output image, shaded counts, layers)"""
    ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
    ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True)
    ctx.raster_forward_shade(cam, ibl=ibl)
    before = ctx.read_hdr().copy()
    ctx.set_raster_transparent_debug_layers(keep)
    try:
        ctx.raster_forward_transparent(cam, ibl=ibl, draw_type=draw_type)
        after = ctx.read_hdr().copy()
        counts, layers = ctx.read_raster_transparent_layers()
    finally:
        ctx.set_raster_transparent_debug_layers(0)
    return before, after, counts, layers


def lists_of(ctx, world):
    return D.membership(ctx.read_light_clusters(), world.point_lights.count, world.spot_lights.count)


def test_colour_against_the_restatement(oracle):
    """sun, point light and spot light of the designed scene, ibl 0 and 1; pixels without a layer keep their bits (check_image);
    debug layers on and off give identical bytes"""
    w, h = 96, 64
    world = designed()
    cam = camera(oracle, world, w, h)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        before, after, counts, layers = transparent_frame(ctx, cam)
        assert ctx.raster_transparent_info().reclustered == 0  # the forward shade clustered for this camera
        lists = lists_of(ctx, world)
        check_image(world, cam, before, after, counts, layers, lists, "designed ibl 0")
        opaque_frame(ctx, cam)
        ctx.raster_forward_transparent(cam)
        assert ctx.read_hdr().tobytes() == after.tobytes(), "debug layers off"
        with pytest.raises(capi.ProsperPtError, match="debug mode"):
            ctx.read_raster_transparent_layers()
        with pytest.raises(capi.ProsperPtError, match="prosper_pt_generate_ibl") as e:
            ctx.raster_forward_transparent(cam, ibl=1)
        assert e.value.code == -6
        ctx.generate_ibl()
        maps = ctx.read_ibl()
        b1, a1, c1, l1 = transparent_frame(ctx, cam, ibl=1)
        assert c1.tobytes() == counts.tobytes()
        check_image(world, cam, b1, a1, c1, l1, lists, "designed ibl 1", maps=maps)
        assert (a1[..., :3][counts > 0] != after[..., :3][counts > 0]).any()
    finally:
        ctx.close()


def test_three_hundred_point_lights_on_a_grid(gpu_ctx, oracle):
    w, h = 96, 64
    world = designed()
    for j in range(15):
        for i in range(20):
            world.add_point_light((1.0, 0.8 + 0.01 * i, 0.6 + 0.02 * j), 3.0, (-1.9 + 0.2 * i, -1.4 + 0.2 * j, 2.25), light_range=0.6)
    world._frozen = None
    cam = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    before, after, counts, layers = transparent_frame(gpu_ctx, cam)
    lists = lists_of(gpu_ctx, world)
    assert len(np.unique(gpu_ctx.read_light_clusters()["pointers"][..., 1] >> 16)) > 3
    check_image(world, cam, before, after, counts, layers, lists, "300 point lights")


# ---- 4. against the traced pass ----

@pytest.mark.parametrize("extent", [(96, 64), (48, 32)], ids=lambda e: "%dx%d" % e)
def test_against_the_traced_pass(gpu_ctx, oracle, extent):
    w, h = extent
    world = designed()
    cam = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    before, raster, counts, layers = transparent_frame(gpu_ctx, cam)
    opaque_frame(gpu_ctx, cam)  # the same depth and image again
    gpu_ctx.set_transparent_debug_layers(LAYERS)
    try:
        gpu_ctx.forward_transparent(cam, w, h)
        traced = gpu_ctx.read_hdr().copy()
        tcounts, tlayers = gpu_ctx.read_transparent_layers()
    finally:
        gpu_ctx.set_transparent_debug_layers(0)
    k = np.arange(LAYERS)
    live = (k[None, None, :] < counts[..., None]) | (k[None, None, :] < tcounts[..., None])
    same = counts == tcounts
    for field in ("drawInstance", "primitive"):
        same &= ~((layers[field] != tlayers[field]) & live).any(axis=2)
    differ = ~same
    print("%dx%d: %d of %d pixels name other layers than the traced pass" % (w, h, differ.sum(), differ.size))
    assert differ.mean() <= 0.02
    assert (counts[same] > 0).sum() > 0.5 * counts.size
    assert (raster[same] == traced[same]).all(), "the same layers: the same four floats"


# ---- 5. the chain ----

def test_forward_chain_and_kept_pyramid(oracle):
    w, h = 96, 64
    world = designed()
    cam = camera(oracle, world, w, h)
    ctx, fresh = capi.Context(device=0), capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        fresh.upload_scene(world)
        ctx.raster_forward(cam)
        before, stored, velocity = ctx.read_hdr().copy(), ctx.read_forward_depth(), ctx.read_velocity()
        ctx.set_raster_transparent_debug_layers(LAYERS)
        ctx.raster_forward_transparent(cam)
        after = ctx.read_hdr().copy()
        counts, fragments = ctx.read_raster_fragments()
        shaded, layers = ctx.read_raster_transparent_layers()
        ctx.set_raster_transparent_debug_layers(0)
        check_lists(world, cam, stored, counts, fragments, "forward chain")
        check_image(world, cam, before, after, shaded, layers, lists_of(ctx, world), "forward chain")
        assert ctx.read_forward_depth().tobytes() == stored.tobytes() and ctx.read_velocity().tobytes() == velocity.tobytes()
        # the kept pyramid survives: the next frame is a two-phase frame, equal to one in a context that never ran the pass
        ctx.raster_forward(cam)
        fresh.raster_forward(cam)
        fresh.raster_forward(cam)
        for a, b in zip((ctx.read_hdr(), ctx.read_forward_depth(), ctx.read_velocity()), (fresh.read_hdr(), fresh.read_forward_depth(), fresh.read_velocity())):
            assert a.tobytes() == b.tobytes()
        assert ctx.raster_info().draw[1].valid == fresh.raster_info().draw[1].valid == 1  # (the reads above waited for the counts)
    finally:
        ctx.close()
        fresh.close()


def test_deferred_chain(gpu_ctx, oracle):
    w, h = 96, 64
    world = designed()
    cam = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    gpu_ctx.raster_release_preserved()
    _, _, stored, velocity = gpu_ctx.raster_gbuffer(cam)
    inp, _, _ = gpu_ctx.gbuffer_device_ptrs()
    gpu_ctx.deferred_shading_device(cam, w, h, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
    gpu_ctx.skybox_fill(cam, w, h)
    before = gpu_ctx.read_hdr().copy()
    gpu_ctx.set_raster_transparent_debug_layers(LAYERS)
    try:
        gpu_ctx.raster_forward_transparent(cam)
        after = gpu_ctx.read_hdr().copy()
        counts, fragments = gpu_ctx.read_raster_fragments()
        shaded, layers = gpu_ctx.read_raster_transparent_layers()
    finally:
        gpu_ctx.set_raster_transparent_debug_layers(0)
    check_lists(world, cam, stored, counts, fragments, "deferred chain")
    check_image(world, cam, before, after, shaded, layers, lists_of(gpu_ctx, world), "deferred chain")
    _, _, depth2 = gpu_ctx.read_gbuffer()
    assert depth2.tobytes() == stored.tobytes() and gpu_ctx.read_velocity().tobytes() == velocity.tobytes()


def test_a_scene_without_blend_keeps_the_image_and_has_empty_lists(gpu_ctx, oracle):
    w, h = 33, 17
    world = designed()
    for m in world.materials:
        if m.alphaMode == S.ALPHA_MODE_BLEND:
            m.alphaMode = S.ALPHA_MODE_MASK
    cam = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    before, stored, velocity = opaque_frame(gpu_ctx, cam)
    gpu_ctx.raster_forward_transparent(cam)
    assert gpu_ctx.read_hdr().tobytes() == before.tobytes()
    counts, fragments = gpu_ctx.read_raster_fragments()
    assert not counts.any() and len(fragments) == 0
    info = gpu_ctx.raster_transparent_info()
    assert (info.fragments, info.coveredPixels, info.shadedLayers, info.maxLayers) == (0, 0, 0, 0)
    assert gpu_ctx.draw_stats().totalMeshletCount == 0


# ---- 6. other states ----

def test_texture_lod_on_a_minified_blend_quad_is_the_traced_pass_s_layer(oracle):
    import test_texture_lod_gbuffer as TL
    rng = np.random.default_rng(37)
    world, _ = TL.flat_world(rng, 8.0, alpha_mode=S.ALPHA_MODE_BLEND, smooth=True)
    world.add_meshlets()
    cam = TL.camera(oracle)
    w, h = TL.W, TL.H
    ctx = TL.mips_context(world)
    try:
        off = None
        for lod in (False, True):
            ctx.set_texture_lod(lod, 0.0)
            _, _, tcounts, tlayers, _ = TL.transparent_frame(ctx, cam)  # the traced frame: depth 0 everywhere
            ctx.set_raster_transparent_debug_layers(2)
            ctx.raster_forward_transparent(cam)  # over the traced depth, the context's last
            counts, layers = ctx.read_raster_transparent_layers()
            ctx.set_raster_transparent_debug_layers(0)
            assert (counts == 1).all() and (tcounts == 1).all()
            for k in ("albedo", "roughness", "metallic", "alpha", "normal"):
                err = np.abs(layers[..., 0][k].astype(np.float64) - tlayers[..., 0][k]).max()
                print("lod %s, layer %s: max difference from the traced pass %.3g" % (lod, k, err))
                assert err <= 2e-4, k  # (f14)'s tolerance of a layer
            if lod:
                assert off.tobytes() != layers.tobytes(), "the pass follows prosper_pt_set_texture_lod"
            off = layers.copy()
    finally:
        ctx.close()


def test_debug_draw_types(gpu_ctx, oracle):
    w, h = 48, 32
    world = designed()
    cam = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    default = transparent_frame(gpu_ctx, cam)
    for dt in range(1, len(S.DRAW_TYPES)):
        before, after, counts, layers = transparent_frame(gpu_ctx, cam, draw_type=dt)
        has = default[2] > 0
        assert ((counts == 1) == has).all() and ((counts == 0) == ~has).all(), S.DRAW_TYPES[dt]
        assert same_bits(after[~has], before[~has]).all()
        assert (after[has][:, 3] == 0.0).all(), "alpha 1: a (1 - a) = 0"
        first, dfirst = layers[..., 0], default[3][..., 0]
        assert np.array_equal(first["drawInstance"][has], dfirst["drawInstance"][has]), "the nearest layer"
        if S.DRAW_TYPES[dt] == "Albedo":
            assert same_bits(after[has][:, :3], first["albedo"][has]).all()
        if S.DRAW_TYPES[dt] == "Position":
            assert same_bits(after[has][:, :3], first["positionWS"][has]).all()
        if S.DRAW_TYPES[dt] in ("MeshletID", "PrimitiveID"):
            # every quad is one meshlet of two triangles: one colour for MeshletID, two for PrimitiveID
            assert len(np.unique(after[has][:, :3], axis=0)) == (1 if S.DRAW_TYPES[dt] == "MeshletID" else 2)


def test_caller_owned_depth(gpu_ctx, oracle):
    w, h = 33, 17
    world = designed()
    cam = camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    before, stored, _ = opaque_frame(gpu_ctx, cam)
    gpu_ctx.raster_forward_transparent(cam)
    want = gpu_ctx.read_hdr().copy()
    assert want.tobytes() != before.tobytes()
    depth_ptr = gpu_ctx.forward_depth_device_ptr()[0]
    for kw in (dict(depth=stored), dict(depth_ptr=depth_ptr)):
        opaque_frame(gpu_ctx, cam)
        gpu_ctx.raster_forward_transparent(cam, **kw)
        assert gpu_ctx.read_hdr().tobytes() == want.tobytes(), list(kw)
    opaque_frame(gpu_ctx, cam)
    gpu_ctx.raster_forward_transparent(cam, depth=np.ones((h, w), F))  # everything at the near plane: no layer passes
    assert gpu_ctx.read_hdr().tobytes() == before.tobytes()
    assert gpu_ctx.raster_transparent_info().fragments == 0


def test_two_streams_into_one_context(gpu_ctx, oracle):
    world = designed()
    gpu_ctx.upload_scene(world)
    small, big = camera(oracle, world, 40, 30), camera(oracle, world, 96, 64)
    opaque_frame(gpu_ctx, big)
    gpu_ctx.raster_forward_transparent(big)
    want = gpu_ctx.read_hdr().copy()
    hip = C.CDLL("libamdhip64.so")
    s1, s2 = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s1), 1) == 0 and hip.hipStreamCreateWithFlags(C.byref(s2), 1) == 0
    try:
        for _ in range(2):
            opaque_frame(gpu_ctx, small)
            gpu_ctx.raster_forward_transparent(small, stream=s1.value)
            gpu_ctx.read_hdr(stream=s1.value)
            opaque_frame(gpu_ctx, big)
            # the lists of the small frame may still be resolved on s1 when s2 rebuilds them
            gpu_ctx.raster_forward_transparent(big, stream=s2.value)
            assert gpu_ctx.read_hdr(stream=s2.value).tobytes() == want.tobytes()
    finally:
        assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
        hip.hipStreamDestroy(s1)
        hip.hipStreamDestroy(s2)


def test_refusals_leave_the_image_as_it_was(oracle):
    lib = capi.lib()
    world = designed()
    w, h = 48, 32
    cam = camera(oracle, world, w, h)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        with pytest.raises(capi.ProsperPtError) as e:
            ctx.raster_transparent_info()
        assert e.value.code == -4
        with pytest.raises(capi.ProsperPtError) as e:
            ctx.read_raster_fragments()
        assert e.value.code == -4
        before, stored, velocity = opaque_frame(ctx, cam)
        # the opaque lists are the context's: FIRST_PHASE exists, SECOND_PHASE does not
        pc = S.ForwardPC(0, 0, 0)
        draw, forward = lib.prosper_pt_raster_transparent_draw, lib.prosper_pt_raster_forward_transparent
        bad_camera = S.CameraUniforms.from_buffer_copy(bytes(cam))
        bad_camera.far_ = bad_camera.near_
        other = camera(oracle, world, 40, 30)
        cases = ((S.ForwardPC(len(S.DRAW_TYPES), 0, 0), cam, None, -1), (S.ForwardPC(0, 2, 0), cam, None, -1), (S.ForwardPC(0, 1, 0), cam, None, -6),
                 (pc, bad_camera, None, -1), (pc, cam, 258, -1), (pc, other, None, -1))
        for pc_, cam_, depth, code in cases:
            assert draw(ctx._h, S.DRAW_LIST_FIRST_PHASE, C.byref(pc_), C.byref(cam_), depth, 1, None) == code
            assert forward(ctx._h, C.byref(pc_), C.byref(cam_), depth, 1, None) == code
        assert "extent is not camera->resolution" in lib.prosper_pt_last_error().decode()
        assert draw(ctx._h, S.DRAW_LIST_SECOND_PHASE, C.byref(pc), C.byref(cam), None, 1, None) == -4
        assert draw(ctx._h, S.DRAW_LIST_SECOND_PHASE_INPUT, C.byref(pc), C.byref(cam), None, 1, None) == -1
        assert draw(ctx._h, S.DRAW_LIST_FIRST_PHASE, None, C.byref(cam), None, 1, None) == -1
        assert forward(ctx._h, C.byref(pc), None, None, 1, None) == -1
        assert ctx.read_hdr().tobytes() == before.tobytes()
        assert ctx.read_forward_depth().tobytes() == stored.tobytes() and ctx.read_velocity().tobytes() == velocity.tobytes()
        # refused before the culling phase: the lists are the opaque ones still
        assert ctx.draw_stats().totalMeshletCount == CR.totals(world, CR.MODE_OPAQUE)["totalMeshletCount"]
        with pytest.raises(capi.ProsperPtError) as e:
            ctx.read_raster_fragments()
        assert e.value.code == -4
        # an image and a last depth of another extent: after a frame at 40 x 30
        opaque_frame(ctx, other)
        small = ctx.read_hdr().copy()
        assert forward(ctx._h, C.byref(pc), C.byref(cam), None, 1, None) == -1
        assert ctx.read_hdr().tobytes() == small.tobytes()
    finally:
        ctx.close()
    # no meshlets in the scene
    plain = capi.Context(device=0)
    try:
        plain.upload_scene(designed_scene())
        with pytest.raises(capi.ProsperPtError, match="no meshlets") as e:
            plain.raster_forward_transparent(cam)
        assert e.value.code == -4
    finally:
        plain.close()


def test_the_cpp_forward_renderer_records_what_the_direct_call_records(gpu_ctx):
    from prosper_amd.rt_reference import Camera, ForwardRenderer
    world = designed()
    w, h = 96, 64
    gpu_ctx.upload_scene(world)
    hcam = Camera.from_world(world, w, h)
    cam, _ = hcam.update_buffer()
    before, _, _ = opaque_frame(gpu_ctx, cam)
    gpu_ctx.raster_forward_transparent(cam)
    direct = gpu_ctx.read_hdr().copy()
    assert direct.tobytes() != before.tobytes()
    opaque_frame(gpu_ctx, cam)
    renderer = ForwardRenderer(gpu_ctx)
    try:
        pc = renderer.record_transparent_raster(hcam, w, h)
        assert (pc.drawType, pc.ibl) == (0, 0)
        assert gpu_ctx.read_hdr().tobytes() == direct.tobytes()
        assert gpu_ctx.draw_stats().totalMeshletCount == CR.totals(world, CR.MODE_TRANSPARENT)["totalMeshletCount"]
        with pytest.raises(capi.ProsperPtError, match="prosper_pt_generate_ibl"):
            renderer.record_transparent_raster(hcam, w, h, apply_ibl=True)
        with pytest.raises(capi.ProsperPtError, match="drawType"):
            renderer.record_transparent_raster(hcam, w, h, draw_type=11)
    finally:
        renderer.close()
        hcam.close()


def test_render_gltf_forward_transparents(tmp_path):
    out = tmp_path / "forward.png"
    script = os.path.join(ROOT, "scripts", "render_gltf.py")
    gltf = os.path.join(ROOT, "tests", "golden", "tiny_scene.gltf")
    for path in (["--forward"], ["--deferred", "--raster"]):
        done = subprocess.run([sys.executable, script, gltf] + path + ["--transparents", "--sky", "--size", "96x64", "--out", str(out)],
                              capture_output=True, text=True)
        assert done.returncode == 0, done.stdout + done.stderr
        assert "transparents (rasterised)" in done.stderr, done.stderr
        assert out.exists() and out.stat().st_size > 100
