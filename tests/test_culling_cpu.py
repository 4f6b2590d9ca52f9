"""The visibility system without a GPU: the depth pyramid's definition in tests/culling_reference.py
against the literal level-by-level reduction of the shader, its extents against hand-computed ones, and the refusals
prosper_pt_hiz_downsample makes before it touches a device; the host camera's frustum planes; the meshlet builder
(prosper_amd/meshlets.py), the packed layout read back through GeometryMetadata, and the cache writer's sections."""
import ctypes as C

import numpy as np
import pytest

import culling_reference as R
from prosper_amd import capi, structs as S

F = np.float32
# width x height, as the issue lists them
SIZES = [(2, 2), (3, 5), (64, 64), (65, 33), (130, 70)]


def test_the_extents_are_the_reference_s():
    # bit_ceil / 2 per side, floor(log2(larger side)) + 1 levels, max(side >> l, 1)
    assert R.hiz_extents(2, 2) == [(1, 1)]
    assert R.hiz_extents(3, 5) == [(2, 4), (1, 2), (1, 1)]
    assert R.hiz_extents(64, 64) == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert R.hiz_extents(65, 33) == [(64, 32), (32, 16), (16, 8), (8, 4), (4, 2), (2, 1), (1, 1)]
    assert R.hiz_extents(130, 70) == [(128, 64), (64, 32), (32, 16), (16, 8), (8, 4), (4, 2), (2, 1), (1, 1)]
    e = R.hiz_extents(1920, 1080)
    assert e[0] == (1024, 1024) and len(e) == 11 and e[-1] == (1, 1)
    e = R.hiz_extents(3840, 2160)
    assert e[0] == (2048, 2048) and len(e) == 12
    with pytest.raises(AssertionError):
        R.hiz_extents(4097, 2)  # a thirteenth level: sMaxMips
    with pytest.raises(AssertionError):
        R.hiz_extents(1, 8)


@pytest.mark.parametrize("w,h", SIZES + [(5, 3), (33, 65), (9, 130)])
def test_the_footprint_definition_is_the_literal_reduction(w, h):
    depth = R.designed_depth(w, h, seed=w * 1000 + h)
    want = R.hiz_pyramid_literal(depth)
    got = R.hiz_pyramid(depth)
    assert [l.shape for l in got] == [(eh, ew) for ew, eh in R.hiz_extents(w, h)]
    assert len(got) == len(want)
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == F and np.array_equal(a.view(np.uint32), b.view(np.uint32)), "level %d" % l
    # the last level is the whole image's minimum, and that is a planted one
    assert got[-1].shape == (1, 1) and got[-1][0, 0] == depth.min() < F(0.25)


def test_a_hand_computed_pyramid():
    # 3 x 5: the clamp repeats the last column and the last row
    d = np.array([[9, 8, 7],
                  [6, 5, 4],
                  [3, 9, 9],
                  [9, 9, 2],
                  [8, 9, 1]], F)
    l0, l1, l2 = R.hiz_pyramid(d)
    assert np.array_equal(l0, np.array([[5, 4], [3, 2], [8, 1], [8, 1]], F))
    assert np.array_equal(l1, np.array([[2], [1]], F))
    assert np.array_equal(l2, np.array([[1]], F))


def test_texels_past_the_image_repeat_its_last_column_and_row():
    w, h = 130, 70
    depth = R.designed_depth(w, h, seed=7)
    l0 = R.hiz_pyramid(depth)[0]  # 128 x 64 over a 130 x 70 image: columns 65.. and rows 35.. lie wholly outside
    for y in range(35):
        assert (l0[y, 65:] == depth[2 * y:2 * y + 2, w - 1].min()).all()
    for x in range(65):
        assert (l0[35:, x] == depth[h - 1, 2 * x:2 * x + 2].min()).all()
    assert (l0[35:, 65:] == depth[h - 1, w - 1]).all()


def test_the_info_struct_matches_the_header():
    assert C.sizeof(S.HizInfo) == 32
    assert [n for n, _ in S.HizInfo._fields_] == [
        "valid", "width", "height", "levelCount", "sourceWidth", "sourceHeight", "launches", "reserved"]


def test_bad_arguments_are_refused_before_the_context_is_touched():
    lib = capi.lib()
    depth = np.zeros((4, 4), F)
    p = C.c_void_p(depth.ctypes.data)
    for slot, w, h, word in ((2, 4, 4, b"slot"), (0, 1, 4, b"above 1"), (0, 4, 1, b"above 1"), (0, 0, 0, b"above 1"),
                             (1, 4097, 4, b"4096"), (0, 4, 4, b"null")):
        assert lib.prosper_pt_hiz_downsample(None, slot, p, 0, w, h, None) == -1, (slot, w, h)
        assert word in lib.prosper_pt_last_error(), (lib.prosper_pt_last_error(), word)
    info = S.HizInfo()
    assert lib.prosper_pt_get_hiz_info(None, 0, C.byref(info)) == -1
    assert lib.prosper_pt_get_hiz_info(None, 2, C.byref(info)) == -1
    out = np.zeros(4, F)
    assert lib.prosper_pt_read_hiz_level(None, 0, 0, C.c_void_p(out.ctypes.data), 16, None) == -1
    ptr = C.c_void_p()
    assert lib.prosper_pt_get_hiz_device_ptr(None, 0, 0, C.byref(ptr), None, None) == -1
    assert lib.prosper_pt_get_hiz_device_ptr(None, 3, 0, C.byref(ptr), None, None) == -1


# ---- the camera's frustum planes (host/camera.cpp; Camera.cpp:39-45, 397-415) ----

PLANES = ("nearPlane", "farPlane", "leftPlane", "rightPlane", "topPlane", "bottomPlane")


def planes_of(eye, target, up, fov, zn, zf, w, h):
    from prosper_amd import rt_reference
    cam = rt_reference.Camera()
    try:
        cam.set_parameters(fov, zn, zf)
        cam.look_at(eye, target, up)
        cam.update_resolution(w, h)
        u, _ = cam.update_buffer()
        return u, {n: np.array([getattr(u, n).x, getattr(u, n).y, getattr(u, n).z, getattr(u, n).w], np.float64) for n in PLANES}
    finally:
        cam.close()


def test_the_planes_of_a_known_camera_are_the_hand_computed_ones():
    # at the origin, looking down -z, 90 degrees, square, near 1 and far 10: the side planes pass through the eye at 45 degrees
    import math
    _, p = planes_of((0, 0, 0), (0, 0, -1), (0, 1, 0), math.radians(90.0), 1.0, 10.0, 64, 64)
    r = math.sqrt(0.5)
    want = {"nearPlane": (0, 0, -1, -1), "farPlane": (0, 0, 1, 10), "leftPlane": (r, 0, -r, 0), "rightPlane": (-r, 0, -r, 0),
            "topPlane": (0, -r, -r, 0), "bottomPlane": (0, r, -r, 0)}
    for n in PLANES:
        assert np.abs(p[n] - np.array(want[n])).max() < 2e-6, (n, p[n])
    # 2 : 1, at (3, 2, 1) looking down +x: forward = +x, right = +z, up = +y
    _, q = planes_of((3, 2, 1), (4, 2, 1), (0, 1, 0), math.radians(90.0), 1.0, 10.0, 128, 64)
    s = 1 / math.sqrt(5.0)  # half width 2 at distance 1: the side normals are (1, 0, 2) / sqrt(5) in the camera's frame
    want = {"nearPlane": (1, 0, 0, -4), "farPlane": (-1, 0, 0, 13), "leftPlane": (2 * s, 0, s, -7 * s),
            "rightPlane": (2 * s, 0, -s, -5 * s), "topPlane": (r, -r, 0, -r), "bottomPlane": (r, r, 0, -5 * r)}
    for n in PLANES:
        assert np.abs(q[n] - np.array(want[n])).max() < 4e-6, (n, q[n])


def test_the_planes_hold_the_frustum_s_corners_and_face_inwards():
    import math
    from prosper_amd import debug_geometry
    u, p = planes_of((1.0, 0.5, 1.0), (0.2, 0.1, -0.3), (0, 1, 0), math.radians(59.0), 0.1, 100.0, 1920, 1080)
    corners = debug_geometry.frustum_corners(u)
    inside = np.mean([np.asarray(c, np.float64) for c in corners.values()], axis=0)
    on = {"nearPlane": "Near", "farPlane": "Far", "leftPlane": "Left", "rightPlane": "Right", "topPlane": "top", "bottomPlane": "bottom"}
    for n in PLANES:
        assert abs(np.linalg.norm(p[n][:3]) - 1.0) < 1e-6
        assert p[n][:3] @ inside + p[n][3] > 1.0  # the centre of the frustum lies well inside
        for name, c in corners.items():
            d = p[n][:3] @ np.asarray(c, np.float64) + p[n][3]
            scale = max(1.0, np.abs(c).max())
            if on[n] in name:
                assert abs(d) < 2e-4 * scale, (n, name, d)  # (the far corners lie 100 away: float32 of clipToWorld)
            else:
                assert d > -2e-4 * scale, (n, name, d)


# ---- the meshlet builder (prosper_amd/meshlets.py) and the packed layout ----

def grid_mesh(n=24):
    """a flat n x n grid of quads in the plane y = 0, normals up"""
    xs = np.linspace(-1.0, 1.0, n + 1)
    p = np.array([(x, 0.0, z) for z in xs for x in xs], F)
    idx = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            idx += [a, a + n + 1, a + 1, a + 1, a + n + 1, a + n + 2]
    return p, np.array(idx, np.uint32)


def sphere_mesh(rings=20, segments=28):
    """a closed UV sphere, outward normals"""
    import math
    p = [(0.0, 1.0, 0.0)]
    for r in range(1, rings):
        t = math.pi * r / rings
        for s in range(segments):
            a = 2 * math.pi * s / segments
            p.append((math.sin(t) * math.cos(a), math.cos(t), math.sin(t) * math.sin(a)))
    p.append((0.0, -1.0, 0.0))
    idx = []
    ring = lambda r, s: 1 + (r - 1) * segments + s % segments
    for s in range(segments):
        idx += [0, ring(1, s + 1), ring(1, s)]
        idx += [len(p) - 1, ring(rings - 1, s), ring(rings - 1, s + 1)]
    for r in range(1, rings - 1):
        for s in range(segments):
            idx += [ring(r, s), ring(r, s + 1), ring(r + 1, s), ring(r + 1, s), ring(r, s + 1), ring(r + 1, s + 1)]
    return np.array(p, F), np.array(idx, np.uint32)


def tiny_meshes():
    import os
    from prosper_amd import gltf
    w = gltf.load_gltf(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_scene.gltf"))
    return [w.mesh_geometry(i) for i in range(len(w.metadatas))]


def builder_cases():
    big = np.random.default_rng(3).random((70000, 3), dtype=F)  # more than 0xFFFF vertices: u32 meshlet vertices
    big_idx = np.arange(69999, dtype=np.uint32)[-300:].reshape(-1, 3)
    return [("grid",) + grid_mesh(), ("sphere",) + sphere_mesh(), ("u32", big, big_idx)] + [
        ("tiny%d" % i, p, ix) for i, (p, ix) in enumerate(tiny_meshes())]


@pytest.fixture(scope="module")
def built():
    from prosper_amd import meshlets as M
    return [(name, p, ix, M.build_meshlets(p, ix)) for name, p, ix in builder_cases()]


def test_every_triangle_is_in_exactly_one_meshlet_within_the_limits(built):
    from prosper_amd import meshlets as M
    assert (M.MAX_VERTICES, M.MAX_TRIANGLES) == (64, 124)
    for name, p, ix, b in built:
        m, v, t = b["meshlets"], b["vertices"], b["triangles"]
        assert (m[:, 2] <= 64).all() and (m[:, 3] <= 124).all() and (m[:, 2] > 0).all() and (m[:, 3] > 0).all(), name
        got = []
        for vo, to, vc, tc in m.tolist():
            assert to % 4 == 0  # every meshlet's triangles start on a 4-byte boundary
            local = t[to:to + 3 * tc].reshape(-1, 3)
            assert local.max() < vc
            assert len(np.unique(v[vo:vo + vc])) == vc  # a vertex once per meshlet
            got.append(v[vo:vo + vc][local])
        got = np.concatenate(got)
        assert np.array_equal(got, ix.reshape(-1, 3)), name  # the greedy scan keeps the index buffer's order, so: equal
        # the sections are tight and padded as generateMeshlets pads them
        assert len(v) == m[-1, 0] + m[-1, 2]
        assert t.size == ((int(m[-1, 1]) + int(m[-1, 3]) + 3) & ~3) * 3 and t.size % 4 == 0
        assert (m[1:, 0] == m[:-1, 0] + m[:-1, 2]).all()
        assert (m[1:, 1] == ((m[:-1, 1] + 3 * m[:-1, 3] + 3) & ~np.uint32(3))).all()
    assert len(built[0][3]["meshlets"]) > 8 and len(built[1][3]["meshlets"]) > 8  # more than a few


def test_every_vertex_lies_inside_its_sphere(built):
    for name, p, ix, b in built:
        for (vo, to, vc, tc), words in zip(b["meshlets"].tolist(), b["bounds"]):
            centre = words[:3].view(F).astype(np.float64)
            radius = float(words[3:4].view(F)[0])
            d = np.sqrt(((p[b["vertices"][vo:vo + vc]].astype(np.float64) - centre) ** 2).sum(axis=1))
            assert (d <= radius).all(), name


def cone_hidden(words, eye):
    """draw_list_culler.comp isConeCapHidden over the decoded bounds, in float64; the shader normalises the axis"""
    from prosper_amd import meshlets as M
    axis, cutoff = M.decode_cone(int(words[4]))
    if not axis.any():
        return False
    axis = axis / np.sqrt((axis * axis).sum())
    d = words[:3].view(F).astype(np.float64) - eye
    return d @ axis >= cutoff * np.sqrt((d * d).sum()) + float(words[3:4].view(F)[0])


def test_a_cone_that_reports_hidden_has_no_front_facing_triangle(built):
    rng = np.random.default_rng(17)
    eyes = rng.uniform(-3.0, 3.0, (1000, 3))
    hidden_seen = 0
    for name, p, ix, b in built:
        if name == "u32":
            continue  # (random triangles: every cone there is the never-hidden one, checked below)
        pd = p.astype(np.float64)
        for (vo, to, vc, tc), words in zip(b["meshlets"].tolist(), b["bounds"]):
            tri = pd[b["vertices"][vo:vo + vc][b["triangles"][to:to + 3 * tc].reshape(-1, 3)]]
            n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
            for eye in eyes:
                if cone_hidden(words, eye):
                    hidden_seen += 1
                    # front-facing: the eye lies on the side the normal points to
                    facing = ((eye - tri[:, 0]) * n).sum(axis=1)
                    assert (facing <= 0).all(), (name, eye)
    assert hidden_seen > 1000  # the test saw hidden cones: the grid from below, the sphere's far side


def test_normals_that_span_a_hemisphere_are_never_hidden():
    from prosper_amd import meshlets as M
    # two triangles facing opposite ways, and a fan that wraps more than a hemisphere
    p = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], F)
    for idx in ([0, 1, 2, 0, 2, 1], [0, 1, 2, 0, 2, 3, 0, 3, 1, 1, 3, 2]):
        b = M.build_meshlets(p, np.array(idx, np.uint32))
        assert len(b["meshlets"]) == 1
        axis, cutoff = M.decode_cone(int(b["bounds"][0, 4]))
        assert cutoff == 1.0 and not axis.any()
        assert int(b["bounds"][0, 4]) >> 24 == 127
        for eye in np.random.default_rng(1).uniform(-5, 5, (200, 3)):
            assert not cone_hidden(b["bounds"][0], eye)
    # one triangle: the tightest cone there is, and its axis is the normal
    b = M.build_meshlets(p, np.array([0, 1, 2], np.uint32))
    axis, cutoff = M.decode_cone(int(b["bounds"][0, 4]))
    assert np.allclose(axis, (0, 0, 1)) and 0 < cutoff <= 2 / 127
    assert cone_hidden(b["bounds"][0], np.array([0.3, 0.3, -5.0])) and not cone_hidden(b["bounds"][0], np.array([0.3, 0.3, 5.0]))


def test_the_packed_layout_reads_back_through_the_metadata():
    from prosper_amd import meshlets as M, scenes
    w = scenes.World()
    mat = w.add_material()
    p, ix = grid_mesh(12)
    sp, six = sphere_mesh(10, 12)
    a = w.add_mesh(p, ix, mat, normals=np.tile(np.array([[0, 1, 0]], F), (len(p), 1)))
    b = w.add_mesh(sp, six, mat, normals=sp, force_u32_indices=True)
    w.add_instance(w.add_model([(a, mat), (b, mat)]))
    before = [x.copy() for x in w.freeze()["geometry_buffers"]]
    md_before = [bytes(m) for m in w.metadatas]
    added = w.add_meshlets()
    f = w.freeze()
    # nothing that was there moved, and the metadata changed only in the four meshlet offsets
    assert np.array_equal(f["geometry_buffers"][0][:before[0].size], before[0])
    for m0, m1 in zip(md_before, w.metadatas):
        assert bytes(m1)[:24] == m0[:24] and bytes(m1)[40:] == m0[40:]
    assert added == sum(i.meshletCount for i in w.mesh_infos) > 4
    for i in (a, b):
        md, info = w.metadatas[i], w.mesh_infos[i]
        want = M.build_meshlets(*w.mesh_geometry(i))
        got = M.read_meshlets(f["geometry_buffers"][md.bufferIndex], md, info)
        assert info.meshletCount == len(want["meshlets"])
        assert np.array_equal(got["meshlets"], want["meshlets"]) and np.array_equal(got["bounds"], want["bounds"])
        assert np.array_equal(got["vertices"], want["vertices"])
        assert np.array_equal(got["triangles"], want["triangles"][:got["triangles"].size])
        # writeCache's order: meshlets, bounds, vertices, triangles, each where the one before ends
        assert md.meshletBoundsOffset == md.meshletsOffset + 4 * info.meshletCount
        unit = 2 if md.usesShortIndices == 1 else 1
        assert md.meshletVerticesOffset == (md.meshletBoundsOffset + 5 * info.meshletCount) * unit
        vwords = (len(want["vertices"]) + 1) // 2 if unit == 2 else len(want["vertices"])
        assert md.meshletTrianglesByteOffset == (md.meshletVerticesOffset // unit + vwords) * 4
    assert (w.metadatas[a].usesShortIndices, w.metadatas[b].usesShortIndices) == (1, 0)
    assert w.add_meshlets() == 0  # a second call finds nothing to do


def test_the_default_packing_is_unchanged_and_the_cache_writer_orders_the_sections(tmp_path):
    from prosper_amd import mesh_cache, meshlets as M
    p, ix = sphere_mesh(10, 12)
    plain_h, plain = mesh_cache.pack_cache(p, ix, p)
    h, blob = mesh_cache.pack_cache(p, ix, p, with_meshlets=True)
    assert plain_h["meshletCount"] == 0 and np.array_equal(blob[:plain.size], plain)  # the default blob is a prefix
    for k in ("indexCount", "vertexCount", "positionsOffset", "normalsOffset", "tangentsOffset", "texCoord0sOffset", "usesShortIndices"):
        assert h[k] == plain_h[k]
    n = h["meshletCount"]
    assert n > 1 and h["meshletsOffset"] == plain.size
    assert h["meshletBoundsOffset"] == h["meshletsOffset"] + 4 * n
    assert h["meshletVerticesOffset"] == 2 * (h["meshletBoundsOffset"] + 5 * n)  # u16 units: 122 vertices
    built = M.build_meshlets(p.astype(np.float16).astype(F), ix)
    assert h["meshletTrianglesByteOffset"] == 4 * (h["meshletVerticesOffset"] // 2 + (len(built["vertices"]) + 1) // 2)
    assert blob.size * 4 == h["meshletTrianglesByteOffset"] + built["triangles"].size
    # through a file and into a world
    path = tmp_path / "m.prosper_mesh"
    mesh_cache.write_mesh_cache(str(path), h, blob)
    h2, blob2 = mesh_cache.read_mesh_cache(str(path))
    from prosper_amd import scenes
    w = scenes.World()
    w.add_mesh(*grid_mesh(4), 0)  # something in front, so the blob does not land at 0
    i = mesh_cache.add_cached_mesh(w, h2, blob2, 0)
    got = M.read_meshlets(w.freeze()["geometry_buffers"][0], w.metadatas[i], w.mesh_infos[i])
    assert np.array_equal(got["meshlets"], built["meshlets"]) and np.array_equal(got["bounds"], built["bounds"])
    assert np.array_equal(got["vertices"], built["vertices"])


# ---- the restatement of the scales and the culler (tests/culling_reference.py) on hand-computed cases ----

def _m2w(sx, sy, sz, t=(0.0, 0.0, 0.0)):
    """modelToWorld's three vec4 columns (the rows of the affine matrix) of a scale and a translation"""
    return np.array([[sx, 0, 0, t[0]], [0, sy, 0, t[1]], [0, 0, sz, t[2]]], F)


def test_the_scale_rule_at_inside_and_outside_its_tolerance():
    # relativeEq: |a - b| < 1e-4 * max(|a|, |b|), strictly
    cases = [(_m2w(2, 2, 2), 2.0), (_m2w(-1.5, -1.5, -1.5), 1.5), (_m2w(1, 2, 1), 0.0),
             (_m2w(1, 1.00005, 1), 1.0),            # inside: 5e-5 < 1e-4 * 1.00005
             (_m2w(1, 1.0002, 1), 0.0),             # outside
             (_m2w(1, 1, 1.0002), 0.0),
             (_m2w(0, 0, 0), 0.0)]                  # 0 < 0 is false: a collapsed instance counts as non-uniform
    got = R.instance_scales(np.stack([c[0] for c in cases]))
    assert got.tolist() == [F(c[1]) for c in cases]
    # at the tolerance: b = a * (1 + 1e-4) rounded; the strict comparison decides on the rounded float32 values
    a = F(3.0)
    for k in range(-4, 5):
        b = a
        b = np.nextafter(F(a * (F(1.0) + F(0.0001))), F(np.inf) if k > 0 else F(-np.inf)) if k else F(a * (F(1.0) + F(0.0001)))
        for _ in range(abs(k) - 1):
            b = np.nextafter(b, F(np.inf) if k > 0 else F(-np.inf))
        want = a if abs(F(a - b)) < F(0.0001) * max(a, b) else F(0.0)
        assert R.instance_scales(_m2w(a, b, a)[None])[0] == want
    # a rotation keeps the rows' lengths
    import math
    c, s = math.cos(0.7), math.sin(0.7)
    rot = np.array([[2 * c, 0, 2 * s, 1], [0, 2, 0, 2], [-2 * s, 0, 2 * c, 3]], F)
    assert abs(R.instance_scales(rot[None])[0] - 2.0) < 1e-6


def _view():
    import culling_scenes as CS
    cam = CS.camera_at()
    return CS, cam, R.View(cam)


def test_the_culler_on_hand_computed_spheres():
    CS, cam, view = _view()
    ident = _m2w(1, 1, 1)

    def run(bounds, hiz=None, m=ident, scale=1.0):
        b = np.array(bounds, np.uint32).reshape(-1, 5)
        return R.cull(b, np.tile(m[None], (len(b), 1, 1)), np.full(len(b), scale, F), view, hiz)
    # the frustum of a 90 degree, 3 : 2 camera at the origin looking down -z, near 0.1, far 100: one sphere for each plane
    cases = [((0, 0, 0.5), 0.3, True), ((0, 0, 0.1), 0.3, False),        # near: -z - 0.1 < -r
             ((0, 0, -100.5), 0.3, True), ((0, 0, -100.2), 0.3, False),  # far
             ((-16, 0, -10), 0.5, True), ((-15.5, 0, -10), 0.5, False),  # left: the half width at 10 is 15
             ((16, 0, -10), 0.5, True), ((15.5, 0, -10), 0.5, False),    # right
             ((0, -11, -10), 0.5, True), ((0, -10.5, -10), 0.5, False),  # bottom: the half height is 10
             ((0, 11, -10), 0.5, True), ((0, 10.5, -10), 0.5, False)]    # top
    r = run([CS.bounds_word(c, rad) for c, rad, _ in cases])
    assert r["outside"].tolist() == [o for _, _, o in cases]
    assert (r["visible"] == ~r["outside"]).all()
    # the cone: hidden while dot(d, axis) >= cutoff * |d| + r; at distance 10 straight ahead, axis away from the eye
    r = run([CS.bounds_word((0, 0, -10), 0.5, (0, 0, -127), 120), CS.bounds_word((0, 0, -10), 0.5, (0, 0, -127), 121),
             CS.bounds_word((0, 0, -10), 0.5, (0, 0, 127), 0), CS.bounds_word((0, 0, -10), 0.5, (0, 0, 0), 127)])
    assert r["cone_hidden"].tolist() == [True, False, False, False]
    # a non-uniform instance (scale 0) skips every test
    r = run([CS.bounds_word((0, 0, 50), 1.0, (0, 0, -127), 0)], scale=0.0)
    assert r["visible"].tolist() == [True]
    # a wall at z = -5 over the whole image
    hiz = R.hiz_pyramid(CS.wall_depth(cam))
    b = [CS.bounds_word((0, 0, -12), 0.5),     # behind the wall
         CS.bounds_word((0, 0, -3), 0.5),      # in front of it
         CS.bounds_word((0, 0, -1), 5.0),      # the eye inside the sphere: projectSphereView gives up
         CS.bounds_word((0, 0, -0.05), 0.3),   # straddling the near plane: the same
         CS.bounds_word((0, 0, -30), 20.0),    # a footprint past the top level: the 1 x 1 level decides, and that is the wall
         CS.bounds_word((-16.5, 0, -10), 1.6)]  # its centre off the screen: the gather reads the border's 0, never culled
    r = run(b, hiz)
    assert r["occluded"].tolist() == [True, False, False, False, True, False]
    assert r["visible"].tolist() == [False, True, True, True, False, True]
    # the same spheres against the sky are all visible
    assert run(b, R.hiz_pyramid(np.zeros((CS.HEIGHT, CS.WIDTH), F)))["visible"].all()
    # under a uniform scale the radius scales and the centre goes through the whole matrix
    r = run([CS.bounds_word((0, 0, -6), 0.25)], hiz, m=_m2w(2, 2, 2), scale=2.0)
    assert r["center"][0].tolist() == [0, 0, -12] and r["radius"][0] == 0.5 and r["occluded"][0]
    r = run([CS.bounds_word((0, 0, 6), 0.25)], hiz, m=_m2w(-2, -2, -2), scale=2.0)
    assert r["center"][0].tolist() == [0, 0, -12] and r["radius"][0] == 0.5 and r["occluded"][0]


def test_the_restatement_is_conservative_on_the_designed_scene():
    """what the GPU property test relies on, here first: with the pyramids of the scene's own depth, the two phases' lists
    hold every meshlet that owns a pixel, in both frames; and the hidden, outside and away-facing instances drop out"""
    CS, _, _ = _view()
    world, inst = CS.property_world()
    di_of = {name: [k for k, d in enumerate(R.draw_instances_of(world)) if d[0] == i] for name, i in inst.items()}
    previous = None
    for eye_x in (0.0, 0.3):
        cam = CS.camera_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0))
        owning, depth = CS.owners(world, cam)
        hiz = R.hiz_pyramid(depth.astype(F))
        vis1, occ1, _ = R.cull_list(world, R.generate(world, R.MODE_OPAQUE), R.View(cam), None, previous)
        vis2 = R.cull_list(world, occ1, R.View(cam), None, hiz)[0] if previous is not None else vis1[:0]
        drawn = set(map(tuple, vis1.tolist())) | set(map(tuple, vis2.tolist()))
        assert owning <= drawn and len(owning) >= 10
        assert not any(d in di_of["outside"] + di_of["away"] for d, m in drawn)
        assert any(d in di_of["hidden"] for d, m in drawn) == (previous is None)
        previous = hiz
    assert 0 < sum(1 for d, m in drawn if d in di_of["plane"]) < 36
