"""The rasterised transparent pass without a GPU: the C-ABI surface and its refusals, and the restatement
tests/raster_transparent_reference.py itself - hand-computed lists, uniqueness across shared edges and clipped fans, the
strict depth test, the alpha-0 drop, the selection order, both arrangements of the blend - and the condition the GPU test
against the traced pass inherits: the restated rasteriser's layers against the oracle's peel along the pixels' rays."""
import ctypes as C
import math
import os
import re

import numpy as np

import culling_reference as CR
import raster_reference as R
import raster_transparent_reference as RT
import transparent_reference as T
from prosper_amd import capi, scenes, structs as S
from test_transparent import DESIGN, EYE_Z, camera, designed_scene, pixel_coordinates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("prosper_pt_raster_transparent_draw", "prosper_pt_raster_forward_transparent", "prosper_pt_get_raster_transparent_info",
               "prosper_pt_read_raster_fragments", "prosper_pt_set_raster_transparent_debug_layers", "prosper_pt_read_raster_transparent_layers",
               "prosper_host_forward_renderer_record_transparent_raster")


def header_fields(struct):
    text = open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()
    body = text[text.index("typedef struct " + struct):text.index("} " + struct + ";")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"\b(?:uint32_t|uint64_t|float)\s+([^;]+);", body):
        names += [n.strip() for n in decl.split(",")]
    return names


def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    for name in ("raster_forward_transparent", "raster_transparent_draw", "raster_transparent_info", "read_raster_fragments",
                 "set_raster_transparent_debug_layers", "read_raster_transparent_layers"):
        assert hasattr(capi.Context, name), name
    from prosper_amd import rt_reference
    assert hasattr(rt_reference.ForwardRenderer, "record_transparent_raster")


def test_struct_sizes_equal_the_headers():
    assert C.sizeof(S.RasterTransparentInfo) == 40 and C.sizeof(S.RasterFragment) == 16 and np.dtype(S.RasterFragment).itemsize == 16
    assert header_fields("prosper_pt_raster_transparent_info") == [n for n, _ in S.RasterTransparentInfo._fields_]
    assert header_fields("prosper_pt_raster_fragment") == [n for n, _ in S.RasterFragment._fields_]


def test_bad_arguments_are_rejected_before_touching_the_gpu(oracle):
    lib = capi.lib()
    cam = camera(oracle, scenes.cornell(), 4, 4)
    pc = S.ForwardPC(0, 0, 0)

    def refused(rc, words, code=-1):
        return rc == code and words in lib.prosper_pt_last_error().decode()

    def draw(which=S.DRAW_LIST_FIRST_PHASE, pc_=C.byref(pc), cam_=C.byref(cam), depth=None):
        return lib.prosper_pt_raster_transparent_draw(None, which, pc_, cam_, depth, 1, None)

    def forward(pc_=C.byref(pc), cam_=C.byref(cam), depth=None):
        return lib.prosper_pt_raster_forward_transparent(None, pc_, cam_, depth, 1, None)

    assert refused(draw(which=S.DRAW_LIST_SECOND_PHASE_INPUT), "GENERATED, FIRST_PHASE or SECOND_PHASE")
    assert refused(draw(which=7), "GENERATED, FIRST_PHASE or SECOND_PHASE")
    bad = S.CameraUniforms.from_buffer_copy(bytes(cam))
    bad.far_ = bad.near_
    for run in (draw, forward):
        assert refused(run(), "null argument")  # only the context is missing
        assert refused(run(pc_=None), "null argument")
        assert refused(run(cam_=None), "null argument")
        assert refused(run(pc_=C.byref(S.ForwardPC(len(S.DRAW_TYPES), 0, 0))), "drawType out of range")
        assert refused(run(pc_=C.byref(S.ForwardPC(0, 2, 0))), "ibl is 0 or 1")
        assert refused(run(pc_=C.byref(S.ForwardPC(0, 1, 0))), "ImageBasedLighting", code=-6)  # UNSUPPORTED
        assert refused(run(cam_=C.byref(bad)), "near_ < far_")
        assert refused(run(depth=258), "4-byte aligned")
    info = S.RasterTransparentInfo()
    assert refused(lib.prosper_pt_get_raster_transparent_info(None, C.byref(info)), "null argument")
    assert refused(lib.prosper_pt_set_raster_transparent_debug_layers(None, 4), "null argument")
    assert refused(lib.prosper_pt_read_raster_transparent_layers(None, None, None, 16, 4, None), "null argument")
    assert refused(lib.prosper_pt_read_raster_fragments(None, None, 0, None, 0, None, None), "null argument")
    assert lib.prosper_host_forward_renderer_record_transparent_raster(None, None, 4, 4, None, 1, 0, 0, None, None) == -1


# ---- the restatement ----

def quad_world(quads, camera_=None):
    """`quads`: (corners, rgba) of BLEND quads -> the world, with meshlets"""
    world = scenes.World()
    for corners, rgba in quads:
        mat = world.add_material(base_color=rgba, metallic=0.1, roughness=0.5, alpha_mode=S.ALPHA_MODE_BLEND)
        mesh = scenes._add(world, scenes.quad(*corners), mat)
        world.add_instance(world.add_model([(mesh, mat)]))
    world.camera = camera_ or dict(eye=(0.0, 0.0, EYE_Z), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=math.radians(40.0), zN=0.1, zF=50.0)
    world.add_meshlets()
    return world


def rect(x0, x1, y0, y1, z):
    return [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]


def blend_pairs(world):
    return CR.generate(world, CR.MODE_TRANSPARENT)


def test_hand_computed_lists_of_two_overlapping_quads(oracle):
    """16 x 12: a pixel's list holds the quads whose projected rectangle (corners projected in float64, no rasteriser) holds
    its centre, the nearer first; one fragment per quad, although each quad is two triangles"""
    w, h = 16, 12
    a, b = rect(-1.0, 0.25, -0.5, 0.75, 1.0), rect(-0.25, 1.0, -0.75, 0.5, 2.0)  # b is nearer (the eye is at z = 4)
    world = quad_world([(a, (0.9, 0.1, 0.1, 0.5)), (b, (0.1, 0.9, 0.1, 0.25))])
    cam = camera(oracle, world, w, h)
    sure, maybe = RT.lists(world, cam, blend_pairs(world))
    py, px = np.mgrid[0:h, 0:w]
    inside = []
    for corners in (a, b):
        p = pixel_coordinates(cam, np.array(corners, np.float64), w, h)
        x0, x1, y0, y1 = p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max()
        assert min(np.abs(px + 0.5 - x0).min(), np.abs(px + 0.5 - x1).min(), np.abs(py + 0.5 - y0).min(), np.abs(py + 0.5 - y1).min()) > 1e-3
        inside.append((px + 0.5 > x0) & (px + 0.5 < x1) & (py + 0.5 > y0) & (py + 0.5 < y1))
    assert inside[0].sum() > 10 and inside[1].sum() > 10 and (inside[0] & inside[1]).sum() > 4 and (~inside[0] & ~inside[1]).sum() > 4
    for y in range(h):
        for x in range(w):
            assert not maybe[y][x]
            got = [RT.decode_key(world, k)[0] for k in sure[y][x]]
            assert got == [di for di in (1, 0) if inside[di][y, x]], (x, y, got)
    # the depth of a fragment is the plane's: (z / w) of any of its vertices, the same for the whole quad
    depths = {RT.decode_key(world, k)[0]: RT.decode_key(world, k)[3] for row in sure for keys in row for k in keys}
    assert depths[1] > depths[0] > 0


def test_shared_edges_and_clipped_fans_never_emit_a_pixel_twice(oracle):
    """every (pixel, triangle) pair at most once, and the two triangles of a quad never both: on the designed stack, and on a
    floor that passes under the eye and behind it, which the clipper turns into fans"""
    floor = quad_world([([(-6.0, -1.0, 7.0), (6.0, -1.0, 7.0), (6.0, -1.0, -20.0), (-6.0, -1.0, -20.0)], (0.5, 0.5, 0.9, 0.5)),
                        ([(-6.0, -0.5, 7.0), (6.0, -0.5, 7.0), (6.0, -0.5, -20.0), (-6.0, -0.5, -20.0)], (0.9, 0.5, 0.5, 0.5))])
    designed = designed_scene()
    designed.add_meshlets()
    for world, extents in ((floor, ((48, 32), (33, 17), (97, 5))), (designed, ((48, 32), (33, 17)))):
        for w, h in extents:
            cam = camera(oracle, world, w, h)
            frags = RT.fragments(world, cam, blend_pairs(world))
            assert len(frags) > w
            seen, quads = set(), set()
            for y, x, k, d in frags:
                assert (y, x, k & 0xFFFFFFFF) not in seen, "a (pixel, triangle) pair twice"
                seen.add((y, x, k & 0xFFFFFFFF))
                di = RT.decode_key(world, k)[0]
                assert (y, x, di) not in quads, "both triangles of a quad own pixel (%d, %d)" % (x, y)
                quads.add((y, x, di))
    # the floor is really clipped: its nearest fragments reach the image's bottom row across its whole width
    cam = camera(oracle, floor, 48, 32)
    counts = R.rasterise(floor, cam, blend_pairs(floor))["counts"]
    assert counts["clipped"] == 4 and counts["queued"] == 4
    bottom = {x for y, x, k, d in RT.fragments(floor, cam, blend_pairs(floor)) if y == 31}
    assert bottom == set(range(48))


def test_the_depth_test_is_strict(oracle):
    w, h = 16, 12
    world = quad_world([(rect(-1.0, 1.0, -1.0, 1.0, 1.0), (0.9, 0.1, 0.1, 0.5))])
    cam = camera(oracle, world, w, h)
    pairs = blend_pairs(world)
    own = R.rasterise(world, cam, pairs)["keys"]
    stored = (own >> np.uint64(32)).astype(np.uint32).view(F)
    covered = stored > 0
    assert covered.sum() > 20 and (~covered).sum() > 20
    everything = RT.fragments(world, cam, pairs)
    assert len(everything) == covered.sum()  # a stored 0 passes everything
    assert RT.fragments(world, cam, pairs, stored) == []  # coplanar with the stored depth: fails
    below = np.nextafter(stored, F(0.0)).astype(F)
    assert len(RT.fragments(world, cam, pairs, below)) == covered.sum()
    above = np.nextafter(stored, F(2.0)).astype(F)
    assert RT.fragments(world, cam, pairs, above) == []
    assert RT.fragments(world, cam, pairs, np.full((h, w), np.nan, F)) == []


def test_alpha_zero_is_no_layer(oracle):
    w, h = 48, 32
    world = designed_scene()
    world.add_meshlets()
    cam = camera(oracle, world, w, h)
    names = [d[0] for d in DESIGN]
    sure, maybe = RT.lists(world, cam, blend_pairs(world))
    texture = names.index("texture")
    columns = set()
    for y in range(h):
        for x in range(w):
            assert not maybe[y][x]  # an even width: no pixel centre on the texture's alpha border
            dis = [RT.decode_key(world, k)[0] for k in sure[y][x]]
            assert names.index("zero") not in dis and names.index("away") not in dis and 0 not in dis
            if texture in dis:
                columns.add(x)
    assert columns == set(range(w // 2, w))  # alpha 0 in the texture's left half
    # an odd width puts the centre column on the border: undecided there, and nowhere else
    cam = camera(oracle, world, 33, 17)
    sure, maybe = RT.lists(world, cam, blend_pairs(world))
    assert {x for y in range(17) for x in range(33) if maybe[y][x]} == {16}
    assert all(RT.decode_key(world, k)[0] == texture for y in range(17) for k in maybe[y][16])


def test_selection_order(oracle):
    """the greatest key first; on equal depths the lowest (drawInstance, meshlet, triangle): the visibility image's tie rule"""
    w, h = 48, 32
    world = designed_scene()
    world.add_meshlets()
    cam = camera(oracle, world, w, h)
    names = [d[0] for d in DESIGN]
    sure, _ = RT.lists(world, cam, blend_pairs(world))
    d1, d2 = names.index("D1"), names.index("D2")
    both = 0
    rng = np.random.default_rng(4)
    for y in range(h):
        for x in range(w):
            keys = sure[y][x]
            shuffled = [keys[i] for i in rng.permutation(len(keys))]
            assert RT.select_front_to_back(shuffled) == keys
            dis = [RT.decode_key(world, k)[0] for k in keys]
            if d1 in dis:
                i = dis.index(d1)
                assert dis[i + 1] == d2 and (keys[i] >> 32) == (keys[i + 1] >> 32) and keys[i] > keys[i + 1]
                both += 1
    assert both > 100
    # synthetic: equal depth bits, ordinals and triangles in every order
    depth = int(np.array([0.25], F).view(np.uint32)[0])
    keys = [(depth << 32) | (~(o * 128 + t) & 0xFFFFFFFF) for o in (5, 2, 9) for t in (3, 0)]
    order = [(RT_low >> 7, RT_low & 127) for RT_low in ((~k) & 0xFFFFFFFF for k in RT.select_front_to_back(keys))]
    assert order == sorted(order)
    assert RT.select_front_to_back([]) == []


def test_front_to_back_selection_equals_back_to_front_blending():
    """random stacks, alphas 0 and 1 among them, handed over as unsorted keys: selecting front to back and compositing as the
    resolve does equals prosper's blend state applied farthest first, in float64"""
    rng = np.random.default_rng(20)
    for trial in range(500):
        k = int(rng.integers(0, 13))
        depth = rng.uniform(0.01, 1.0, k).astype(F)
        keys = [(int(depth[i:i + 1].view(np.uint32)[0]) << 32) | (~(i * 128) & 0xFFFFFFFF) for i in range(k)]
        src = rng.uniform(0.0, 20.0, (k, 3))
        a = rng.uniform(0.0, 1.0, k)
        special = rng.uniform(0.0, 1.0, k)
        a = np.where(special < 0.15, 0.0, np.where(special > 0.85, 1.0, a))
        dst = rng.uniform(0.0, 20.0, 4)
        chosen = [(~key & 0xFFFFFFFF) >> 7 for key in RT.select_front_to_back(keys)]
        assert sorted(chosen) == list(range(k))
        assert all(depth[i] >= depth[j] for i, j in zip(chosen, chosen[1:]))
        f, fa = T.composite_front_to_back(src[chosen], a[chosen], dst)
        b, ba = T.composite_back_to_front(src[chosen], a[chosen], dst)
        assert np.allclose(f, b, rtol=1e-13, atol=1e-13) and fa == ba


# ---- the cross-check condition ----

def oracle_peel(oracle, cam, w, h):
    """Per pixel the (drawInstance, primitive) sequence of the designed stack along the ray through the pixel's centre, by
    the oracle's traversal: one copy of the world per BLEND quad in which only that quad can be hit, the hits filtered by
    the pass's rules (front face, alpha not 0, in front of the wall) and sorted by (t, drawInstance, primitive)."""
    def only(k):
        world = designed_scene()
        for j, m in enumerate(world.materials[1:]):  # (material 0 is the world's default material)
            if j == k:
                m.alphaMode = S.ALPHA_MODE_OPAQUE
            else:
                m.alphaMode = S.ALPHA_MODE_BLEND
                m.baseColorFactor.w = 0.0  # the any-hit always rejects alpha 0
        return world

    base = designed_scene()
    w2c, c2c = CR.mat4_of(cam.worldToCamera).astype(np.float64), CR.mat4_of(cam.cameraToClip).astype(np.float64)
    eye = np.array([cam.eye.x, cam.eye.y, cam.eye.z], np.float64)
    right, up, fwd = w2c[0, :3], w2c[1, :3], -w2c[2, :3]
    py, px = np.mgrid[0:h, 0:w]
    d = ((px + 0.5) / w * 2.0 - 1.0)[..., None] * (right / c2c[0, 0]) + ((py + 0.5) / h * 2.0 - 1.0)[..., None] * (up / c2c[1, 1]) + fwd
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    hits = [[[] for _ in range(w)] for _ in range(h)]
    wall_t = np.full((h, w), np.inf)
    dis = CR.draw_instances_of(base)
    for k, (name, z, _, kind, rgba) in enumerate(DESIGN):
        if kind != "opaque" and rgba[3] == 0.0:
            continue  # alpha 0 everywhere: never a layer
        positions, indices = base.mesh_geometry(dis[k][1])
        uvs = R.mesh_uvs(base, dis[k][1])
        osc = oracle.OracleScene(only(k), brute_force=True)
        try:
            for y in range(h):
                for x in range(w):
                    hit, di, prim, bary = osc.trace_closest(eye, d[y, x])
                    if not hit:
                        continue
                    assert di == k
                    v = indices[3 * prim:3 * prim + 3]
                    p0, p1, p2 = positions[v].astype(np.float64)
                    if np.dot(np.cross(p1 - p0, p2 - p0), d[y, x]) >= 0.0:
                        continue  # seen from behind: culled
                    t = (z - eye[2]) / d[y, x][2]
                    if kind == "opaque":
                        wall_t[y, x] = t
                        continue
                    if kind == "texture":
                        uv = uvs[v[0]] + bary[0] * (uvs[v[1]] - uvs[v[0]]) + bary[1] * (uvs[v[2]] - uvs[v[0]])
                        if uv[0] < 0.5:
                            continue  # the texture's left half has alpha 0
                    hits[y][x].append((t, k, prim))
        finally:
            osc.close()
    return [[[(k, prim) for t, k, prim in sorted(hits[y][x]) if t < wall_t[y, x]] for x in range(w)] for y in range(h)]


def test_the_designed_stack_stays_within_the_raster_against_traced_cap(oracle):
    """The condition the GPU test against the traced pass inherits, at its extents (not 33 x 17: there a pixel centre lies
    exactly on the quads' diagonal, where the two tie rules legitimately differ): the pixels where the restated rasteriser's
    layer list and the oracle's peel name different (drawInstance, primitive) sequences number at most 2 %."""
    world = designed_scene()
    world.add_meshlets()
    for w, h in ((96, 64), (48, 32)):
        cam = camera(oracle, world, w, h)
        opaque = R.rasterise(world, cam, CR.generate(world, CR.MODE_OPAQUE))["keys"]
        stored = (opaque >> np.uint64(32)).astype(np.uint32).view(F)
        sure, maybe = RT.lists(world, cam, blend_pairs(world), stored)
        peel = oracle_peel(oracle, cam, w, h)
        maps = {}
        differ = sum(bool(maybe[y][x]) or RT.geometry_sequence(world, sure[y][x], maps) != peel[y][x] for y in range(h) for x in range(w))
        deepest = max(len(sure[y][x]) for y in range(h) for x in range(w))
        print("%dx%d: %d of %d pixels differ from the oracle's peel (deepest pixel %d)" % (w, h, differ, w * h, deepest))
        assert deepest == 6 and differ <= 0.02 * w * h
