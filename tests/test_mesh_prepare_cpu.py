"""The statements behind prosper_pt_prepare_mesh, without a GPU: prosper_amd.tangents (known answers, the
fallback, order independence), the ordered form of the meshlet cone against the default, and the cache round trip.
Also the meshes that test_mesh_prepare.py runs on the GPU."""
import functools
import math

import numpy as np
import pytest

from prosper_amd import mesh_cache, meshlets as M, structs as S, tangents as T
from prosper_amd import world as W

F = np.float32
QUAD = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], F)
QUAD_INDICES = np.array([0, 1, 2, 0, 2, 3], np.uint32)
UP = np.tile(np.array([[0, 0, 1]], F), (4, 1))


def decode_snorm(words):
    """glm::unpackSnorm3x10_1x2 -> float64 [n, 4]"""
    w = np.asarray(words, np.uint32)
    def field(shift, bits):
        v = ((w >> shift) & ((1 << bits) - 1)).astype(np.int64)
        return np.where(v >= 1 << (bits - 1), v - (1 << bits), v)
    return np.stack([np.clip(field(0, 10) / 511.0, -1, 1), np.clip(field(10, 10) / 511.0, -1, 1),
                     np.clip(field(20, 10) / 511.0, -1, 1), np.clip(field(30, 2) / 1.0, -1, 1)], axis=1)


# ---- meshes, shared with the GPU tests ----

def grid(nx, ny, triangles=None, vertices=None):
    """an nx x ny grid of vertices over the unit square, uv = (x, y), normals +z; cut to its first `triangles` triangles
    or to the triangles among its first `vertices` vertices"""
    xs, ys = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny))
    p = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(nx * ny)], axis=1).astype(F)
    a = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).reshape(-1)
    idx = np.stack([a, a + 1, a + nx + 1, a, a + nx + 1, a + nx], axis=1).reshape(-1, 3)
    if triangles is not None:
        idx = idx[:triangles]
        assert len(idx) == triangles
    if vertices is not None:
        p = p[:vertices]
        idx = idx[(idx < vertices).all(axis=1)]
    n = np.tile(np.array([[0, 0, 1]], F), (len(p), 1))
    return dict(positions=p, normals=n, uvs=p[:, :2].copy(), indices=idx.astype(np.uint32).reshape(-1))


def displaced_grid(nx=33, ny=17, seed=5):
    """a grid with a relief, its normals those of the relief, and a warped uv map"""
    g = grid(nx, ny)
    x, y = g["positions"][:, 0].astype(np.float64), g["positions"][:, 1].astype(np.float64)
    rng = np.random.default_rng(seed)
    z = 0.15 * np.sin(5 * x) * np.cos(4 * y) + 0.01 * rng.standard_normal(x.shape)
    dzdx, dzdy = 0.75 * np.cos(5 * x) * np.cos(4 * y), -0.6 * np.sin(5 * x) * np.sin(4 * y)
    n = np.stack([-dzdx, -dzdy, np.ones_like(x)], axis=1)
    n /= np.sqrt((n * n).sum(axis=1))[:, None]
    uv = np.stack([x + 0.1 * np.sin(3 * y), 1.3 * y + 0.07 * x * x], axis=1)
    return dict(positions=np.stack([3 * x, 2 * y, z], axis=1).astype(F), normals=n.astype(F), uvs=uv.astype(F), indices=g["indices"])


def fan(triangles=200, seed=0):
    """`triangles` triangles around vertex 0, a shallow cone with an uneven rim, in the order of `seed`'s shuffle"""
    a = np.linspace(0, 2 * math.pi, triangles, endpoint=False)
    r = 1.0 + 0.2 * np.sin(7 * a)
    p = np.concatenate([[(0, 0, 0.3)], np.stack([r * np.cos(a), r * np.sin(a), 0.05 * np.cos(3 * a)], axis=1)]).astype(F)
    i = np.arange(triangles)
    idx = np.stack([np.zeros_like(i), 1 + i, 1 + (i + 1) % triangles], axis=1)
    if seed:
        idx = idx[np.random.default_rng(seed).permutation(triangles)]
    n = p.astype(np.float64) * (0.3, 0.3, 0) + (0, 0, 1)
    n /= np.sqrt((n * n).sum(axis=1))[:, None]
    return dict(positions=p, normals=n.astype(F), uvs=(p[:, :2] * F(0.4) + F(0.5)).astype(F), indices=idx.astype(np.uint32).reshape(-1))


def quad(uvs, positions=QUAD, normals=UP):
    return dict(positions=np.asarray(positions, F), normals=np.asarray(normals, F), uvs=np.asarray(uvs, F), indices=QUAD_INDICES)


def rotated_quad():
    """the unit quad under a rotation, with a non-uniform affine uv map -> (mesh, the analytic dP/du, unit)"""
    c, s = math.cos(0.7), math.sin(0.7)
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    c, s = math.cos(-0.4), math.sin(-0.4)
    rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    r = rx @ rz
    a = np.array([[2.0, 0.5], [-0.3, 0.7]])  # uv = a @ (x, y) + b
    uv = QUAD[:, :2].astype(np.float64) @ a.T + (0.1, 0.2)
    dpdu = r[:, :2] @ np.linalg.inv(a)[:, 0]
    return quad(uv, positions=QUAD.astype(np.float64) @ r.T, normals=np.tile(r[:, 2], (4, 1))), dpdu / np.sqrt((dpdu * dpdu).sum())


def degenerate_uv_mesh():
    """every triangle has det == 0 (one uv for all vertices); normals of every kind, a zero one among them"""
    g = grid(5, 4)
    rng = np.random.default_rng(9)
    n = rng.standard_normal((20, 3))
    n /= np.sqrt((n * n).sum(axis=1))[:, None]
    n[0], n[1], n[2], n[3], n[4] = (0, 0, 1), (1, 0, 0), (0, -1, 0), (0.5, 0.5, math.sqrt(0.5)), (0, 0, 0)
    return dict(g, normals=n.astype(F), uvs=np.full((20, 2), 0.25, F))


def tangent_cases():
    """name -> mesh, for the bit-for-bit comparison on the GPU (the known answers among them)"""
    cases = {"quad": quad(QUAD[:, :2]), "quad_u_mirrored": quad(QUAD[:, :2] * (-1, 1)), "quad_uv_rotated": quad(np.stack([QUAD[:, 1], -QUAD[:, 0]], axis=1)),
             "quad_rotated_affine": rotated_quad()[0], "degenerate_uvs": degenerate_uv_mesh(), "displaced_33x17": displaced_grid(),
             "fan_200": fan(), "fan_200_shuffled": fan(seed=2), "grid_65537_vertices": grid(257, 256, vertices=65537)}
    for k in (1, 63, 64, 65, 257):
        cases["grid_%d_triangles" % k] = grid(20, 9, triangles=k)
    return cases


@functools.lru_cache(maxsize=None)
def scene_meshes():
    """(name, positions as the buffers hold them, indices) of every mesh of the designed scenes of raster_scenes.py and
    culling_scenes.py"""
    import culling_scenes as CS
    import raster_scenes as RS
    worlds = {"s1": RS.s1_world(), "list": RS.list_world(5), "queue": RS.queue_world(40, True), "zoo": RS.clip_zoo_world(),
              "soup": RS.soup_world(1), "floor": RS.graded_floor_world(), "scan": RS.scan_world(), "closed": RS.closed_world(),
              "property": CS.property_world(), "sweep": CS.sweep_world(CS.camera_at())}
    out = []
    for name, world in worlds.items():
        world = world[0] if isinstance(world, tuple) else world
        for i, info in enumerate(world.mesh_infos):
            if info.indexCount:
                out.append(("%s%d" % (name, i),) + world.mesh_geometry(i))
    return out


def generate(mesh):
    return T.generate_tangents(mesh["positions"], mesh["normals"], mesh["uvs"], mesh["indices"])


# ---- the tangent statement ----

@pytest.mark.parametrize("name, want", [("quad", (1, 0, 0, 1)), ("quad_u_mirrored", (-1, 0, 0, -1)), ("quad_uv_rotated", (0, 1, 0, 1))])
def test_the_unit_quad_has_the_known_tangent_exactly(name, want):
    got = generate(tangent_cases()[name])
    assert got.dtype == F and got.shape == (4, 4)
    assert np.array_equal(got, np.tile(np.array(want, F), (4, 1))), got


def test_the_packed_tangent_of_a_rotated_affine_quad_is_dp_du():
    mesh, want = rotated_quad()
    got = generate(mesh)
    assert (got[:, 3] == 1).all()
    t = decode_snorm(W.pack_snorm3x10_1x2(got))[:, :3]
    t /= np.sqrt((t * t).sum(axis=1))[:, None]
    angle = np.arccos(np.clip(t @ want, -1, 1))
    print("angle to dP/du (rad):", angle)
    # the half step 0.5 / 511 of the snorm in three components: sqrt(3) * 0.5 / 511 = 1.7e-3
    assert (angle < 2e-3).all()
    # and it lies in the plane
    assert np.abs(got[:, :3].astype(np.float64) @ mesh["normals"][0].astype(np.float64)).max() < 1e-6


def test_degenerate_uvs_get_the_fallback_everywhere():
    mesh = degenerate_uv_mesh()
    assert not T.corner_contributions(mesh["positions"], mesh["uvs"], mesh["indices"]).any()
    got = generate(mesh)
    assert np.isfinite(got).all() and (got[:, 3] == 1).all()
    t = decode_snorm(W.pack_snorm3x10_1x2(got))[:, :3]
    assert np.abs(np.sqrt((t * t).sum(axis=1)) - 1).max() < math.sqrt(3) * 0.5 / 511 + 1e-6
    n = mesh["normals"].astype(np.float64)
    assert np.abs((got[:, :3].astype(np.float64) * n).sum(axis=1)).max() < 1e-6  # at right angles to the normal
    # the axis of the smallest component, the lowest index on a tie
    assert np.array_equal(got[0], np.array((0, 1, 0, 1), F))    # n = +z: axis x, cross(n, x) = (0, nz, -ny)
    assert np.array_equal(got[1, :3], np.array((0, 0, 1), F))   # n = +x: axis y, cross(n, y) = (-nz, 0, nx)
    assert np.array_equal(got[2, :3], np.array((0, 0, 1), F))   # n = -y: axis x, (0, nz, -ny) = (0, 0, 1)
    assert np.array_equal(got[4], np.array((1, 0, 0, 1), F))    # a zero normal


def test_a_vertex_with_a_zero_normal_gets_the_unit_x():
    mesh = quad(QUAD[:, :2], normals=np.zeros((4, 3), F))
    assert np.array_equal(generate(mesh), np.tile(np.array((1, 0, 0, 1), F), (4, 1)))
    broken = quad(QUAD[:, :2], normals=np.full((4, 3), np.nan, F))
    assert np.array_equal(generate(broken), np.tile(np.array((1, 0, 0, 1), F), (4, 1)))


def test_the_order_of_the_triangles_does_not_change_a_bit():
    want = generate(fan())
    assert len(np.unique(want[:, :3], axis=0)) > 100  # (not one tangent for all)
    for seed in (1, 2, 3):
        shuffled = fan(seed=seed)
        assert not np.array_equal(shuffled["indices"], fan()["indices"])
        assert generate(shuffled).tobytes() == want.tobytes()


def test_every_result_is_finite_with_a_unit_hand():
    cases = tangent_cases()
    # and a mesh with everything that can go wrong in it: repeated vertices, zero edges, huge and tiny scales, inf and NaN
    bad = displaced_grid(9, 7)
    bad["positions"][3] = bad["positions"][4]
    bad["positions"][10] *= F(1e30)
    bad["positions"][20] = (np.inf, 0, 0)
    bad["positions"][30] *= F(1e-30)
    bad["uvs"][40] = (np.nan, 0)
    bad["uvs"][41] *= F(1e25)
    bad["indices"][:3] = (5, 5, 6)
    cases["bad"] = bad
    for name, mesh in cases.items():
        got = generate(mesh)
        assert got.shape == (len(mesh["positions"]), 4) and np.isfinite(got).all(), name
        assert (np.abs(got[:, 3]) == 1).all(), name
        length = np.sqrt((got[:, :3].astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(length - 1).max() < 1e-6, name


def test_the_weight_does_not_depend_on_the_scale():
    mesh = displaced_grid()
    want = T.corner_contributions(mesh["positions"], mesh["uvs"], mesh["indices"])
    assert want.any() and np.abs(want).max() <= 1 << 32
    for scale in (F(2.0 ** -20), F(2.0 ** 30)):  # (powers of two: every operation scales exactly)
        assert np.array_equal(T.corner_contributions(mesh["positions"] * scale, mesh["uvs"], mesh["indices"]), want)


def test_a_mirror_seam_vertex_takes_the_hand_of_the_larger_sum():
    # two quads that share the edge x = 1; u runs forwards over the large one and backwards over the small one
    p = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (1.25, 0, 0), (1.25, 1, 0)], F)
    uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1), (0.75, 0), (0.75, 1)], F)
    idx = np.array([0, 1, 2, 0, 2, 3, 1, 4, 5, 1, 5, 2], np.uint32)
    got = T.generate_tangents(p, np.tile(np.array([[0, 0, 1]], F), (6, 1)), uv, idx)
    assert (got[[0, 3], 3] == 1).all() and (got[[4, 5], 3] == -1).all()
    assert np.array_equal(got[4], np.array((-1, 0, 0, -1), F))
    assert np.isfinite(got).all() and (np.abs(got[[1, 2], 3]) == 1).all()


# ---- ordered=True against the default ----

def test_the_ordered_cone_agrees_with_the_default_and_both_are_conservative():
    from test_culling_cpu import cone_hidden
    eyes = np.random.default_rng(23).uniform(-4.0, 4.0, (60, 3))
    meshlets = hidden = stepped = 0
    for name, p, ix in scene_meshes():
        a, b = M.build_meshlets(p, ix), M.build_meshlets(p, ix, ordered=True)
        for key in ("meshlets", "vertices", "triangles"):
            assert np.array_equal(a[key], b[key]), name
        assert np.array_equal(a["bounds"][:, :4], b["bounds"][:, :4]), name                            # the sphere's words
        assert np.array_equal(a["bounds"][:, 4] & 0xFFFFFF, b["bounds"][:, 4] & 0xFFFFFF), name        # the axis' bytes
        ca, cb = (a["bounds"][:, 4] >> 24).astype(np.int64), (b["bounds"][:, 4] >> 24).astype(np.int64)
        assert np.abs(ca - cb).max() <= 1, name                                                        # one s8 step
        stepped += int((ca != cb).sum())
        pd = p.astype(np.float64)
        for built in (a, b):
            for (vo, to, vc, tc), words in zip(built["meshlets"].tolist(), built["bounds"]):
                meshlets += 1
                if not words[4] & 0xFFFFFF:
                    continue
                tri = pd[built["vertices"][vo:vo + vc][built["triangles"][to:to + 3 * tc].reshape(-1, 3)]]
                n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
                for eye in eyes:
                    if cone_hidden(words, eye):
                        hidden += 1
                        assert (((eye - tri[:, 0]) * n).sum(axis=1) <= 0).all(), (name, eye)  # no front-facing triangle
    print("meshlets", meshlets, "hidden", hidden, "cutoffs a step apart", stepped)
    assert meshlets > 200 and hidden > 100


def test_pack_cache_passes_ordered_through():
    mesh = displaced_grid()
    args = (mesh["positions"], mesh["indices"], mesh["normals"], generate(mesh), mesh["uvs"])
    (ha, ba), (hb, bb) = mesh_cache.pack_cache(*args, with_meshlets=True), mesh_cache.pack_cache(*args, with_meshlets=True, ordered=True)
    assert ha == hb and ba.shape == bb.shape
    n = ha["meshletCount"]
    differ = np.flatnonzero(ba != bb)
    cones = ha["meshletBoundsOffset"] + 5 * np.arange(n) + 4
    assert np.isin(differ, cones).all()  # nothing but a cone's word may differ
    half = mesh["positions"].astype(np.float16).astype(F)
    want = M.build_meshlets(half, mesh["indices"], ordered=True)["bounds"]
    assert np.array_equal(bb[hb["meshletBoundsOffset"]:hb["meshletBoundsOffset"] + 5 * n].reshape(n, 5), want)


# ---- the cache round trip ----

def test_generated_tangents_and_meshlets_survive_the_cache_file(tmp_path):
    mesh = displaced_grid()
    tangents = generate(mesh)
    header, blob = mesh_cache.pack_cache(mesh["positions"], mesh["indices"], mesh["normals"], tangents, mesh["uvs"], with_meshlets=True, ordered=True)
    path = str(tmp_path / "cache0.prosper_mesh")
    mesh_cache.write_mesh_cache(path, header, blob, source_write_time=-1234567)
    got_header, got_blob = mesh_cache.read_mesh_cache(path)
    assert got_header == dict(header, blobByteCount=blob.size * 4, sourceWriteTime=-1234567)
    assert np.array_equal(got_blob, blob)
    n = header["vertexCount"]
    assert np.array_equal(got_blob[header["tangentsOffset"]:header["tangentsOffset"] + n], W.pack_snorm3x10_1x2(tangents))

    cached, direct = W.World(), W.World()
    a = mesh_cache.add_cached_mesh(cached, got_header, got_blob, 0)
    b = direct.add_mesh(mesh["positions"], mesh["indices"], 0, normals=mesh["normals"], tangents=tangents, uvs=mesh["uvs"])
    direct.attach_meshlets(b, M.build_meshlets(*direct.mesh_geometry(b), ordered=True))
    for name, _ in S.GeometryMetadata._fields_:
        assert getattr(cached.metadatas[a], name) == getattr(direct.metadatas[b], name), name
    for name, _ in S.MeshInfo._fields_:
        assert getattr(cached.mesh_infos[a], name) == getattr(direct.mesh_infos[b], name), name
    assert np.array_equal(cached.freeze()["geometry_buffers"][0], direct.freeze()["geometry_buffers"][0])
    assert cached.mesh_infos[a].meshletCount > 8 and cached.metadatas[a].tangentsOffset != S.ABSENT


def test_build_for_gltf_writes_what_is_missing_or_stale_and_load_gltf_reads_it(tmp_path):
    """the writer and the reader without a GPU: a stand-in for the context that packs on the host"""
    import os
    import shutil
    from prosper_amd import gltf
    here = os.path.dirname(os.path.abspath(__file__))
    for name in os.listdir(os.path.join(here, "golden")):
        if name.startswith("tiny_scene") and not name.endswith(".npy"):
            shutil.copy(os.path.join(here, "golden", name), str(tmp_path / name))
    path = str(tmp_path / "tiny_scene.gltf")

    class HostContext:
        calls = 0

        def prepare_mesh(self, positions, indices, normals=None, tangents=None, uvs=None, generate_tangents=True, meshlets=True):
            self.calls += 1
            generated = None
            if tangents is None and uvs is not None and generate_tangents:
                tangents = generated = T.generate_tangents(positions, normals, uvs, indices)
            header, blob = mesh_cache.pack_cache(positions, indices, normals, tangents, uvs, with_meshlets=meshlets, ordered=True)
            return dict(header, blobByteCount=blob.size * 4), blob, generated

    ctx = HostContext()
    plain = gltf.load_gltf(path)
    written = mesh_cache.build_for_gltf(ctx, path)
    assert len(written) == ctx.calls == len(plain.metadatas) > 0
    assert [os.path.basename(f) for f in written] == ["cache%d.prosper_mesh" % i for i in range(len(written))]
    assert mesh_cache.build_for_gltf(ctx, path) == [] and ctx.calls == len(written)  # all valid: nothing to do
    assert not gltf.load_gltf(path).cached_meshes  # opt-in: the default does not look
    cached = gltf.load_gltf(path, use_mesh_cache=True)
    assert cached.cached_meshes == written
    uvs_without_tangents = 0
    for i, (md, info, pmd, pinfo) in enumerate(zip(cached.metadatas, cached.mesh_infos, plain.metadatas, plain.mesh_infos)):
        assert (info.vertexCount, info.indexCount, info.materialIndex) == (pinfo.vertexCount, pinfo.indexCount, pinfo.materialIndex)
        assert info.meshletCount > 0 and pinfo.meshletCount == 0
        for got, want in zip(cached.mesh_geometry(i), plain.mesh_geometry(i)):
            assert np.array_equal(got, want)
        if pmd.texCoord0sOffset != S.ABSENT and pmd.tangentsOffset == S.ABSENT:
            uvs_without_tangents += 1
            assert md.tangentsOffset != S.ABSENT  # generated
    print("primitives with uvs and no TANGENT:", uvs_without_tangents)
    # another write time: stale, written again; a file of another version likewise
    stat = os.stat(path)
    os.utime(path, ns=(stat.st_atime_ns, stat.st_mtime_ns + 2_000_000_000))
    assert not mesh_cache.cache_valid(written[0], path)
    assert not gltf.load_gltf(path, use_mesh_cache=True).cached_meshes
    assert mesh_cache.build_for_gltf(ctx, path) == written
    data = bytearray(open(written[0], "rb").read())
    data[8] = 3
    open(written[0], "wb").write(bytes(data))
    assert mesh_cache.build_for_gltf(ctx, path) == written[:1]
