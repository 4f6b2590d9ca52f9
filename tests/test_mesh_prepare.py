"""prosper_pt_prepare_mesh on the GPU against its statements in NumPy, bit for bit: prosper_amd.tangents,
world.pack_mesh_data, meshlets.build_meshlets(ordered=True) laid out by mesh_cache.pack_cache; then through the renderer,
the cache writer, the refusals, the timing and the C++ mirror."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import culling_scenes as CS
from prosper_amd import capi, gltf, mesh_cache, meshlets as M, scenes, structs as S, tangents as T
from test_meshlet_build_host import CASES as PARTITION_CASES, EXPECTED as PARTITION_EXPECTED
from test_mesh_prepare_cpu import displaced_grid, fan, quad, scene_meshes, tangent_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def want_header(header, blob):
    return dict(header, blobByteCount=int(blob.size) * 4)


def prepare(ctx, mesh, **kw):
    return ctx.prepare_mesh(mesh["positions"], mesh["indices"], normals=mesh.get("normals"), tangents=mesh.get("tangents"),
                            uvs=mesh.get("uvs"), **kw)


# ---- tangents ----

@pytest.fixture(scope="module")
def cases():
    return tangent_cases()


@pytest.mark.parametrize("name", sorted(tangent_cases()))
def test_generated_tangents_are_the_statement_s_bit_for_bit(gpu_ctx, cases, name):
    mesh = cases[name]
    want = T.generate_tangents(mesh["positions"], mesh["normals"], mesh["uvs"], mesh["indices"])
    header, blob, got = prepare(gpu_ctx, mesh, meshlets=False)
    differ = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert differ.size == 0, (name, differ[:5], got[differ[:5]], want[differ[:5]])
    wh, wb = mesh_cache.pack_cache(mesh["positions"], mesh["indices"], mesh["normals"], want, mesh["uvs"])
    assert header == want_header(wh, wb)
    assert np.array_equal(blob, wb)
    if name == "grid_65537_vertices":
        assert header["usesShortIndices"] == 0 and header["vertexCount"] == 65537


def test_the_order_of_the_triangles_does_not_change_a_byte(gpu_ctx):
    a, b = fan(), fan(seed=3)
    assert not np.array_equal(a["indices"], b["indices"])
    (_, _, ta), (_, _, tb) = prepare(gpu_ctx, a, meshlets=False), prepare(gpu_ctx, b, meshlets=False)
    assert ta.tobytes() == tb.tobytes()


# ---- the whole blob and header ----

@pytest.mark.parametrize("config", ["tangents_supplied", "tangents_generated", "no_uvs", "meshlets_off", "zero_indices", "positions_only"])
def test_blob_and_header_are_pack_cache_s_word_for_word(gpu_ctx, config):
    mesh = displaced_grid()
    generated = T.generate_tangents(mesh["positions"], mesh["normals"], mesh["uvs"], mesh["indices"])
    meshlets, tangents = config != "meshlets_off", generated
    if config == "tangents_supplied":
        rng = np.random.default_rng(4)
        tangents = rng.uniform(-1.2, 1.2, generated.shape).astype(F)  # (past the clamp too)
        tangents[:, 3] = rng.choice([-1.0, 1.0], len(tangents))
        mesh["tangents"] = tangents
    elif config == "no_uvs":
        mesh["uvs"], tangents = None, None
    elif config == "zero_indices":
        mesh["indices"] = np.zeros(0, np.uint32)
        tangents = T.generate_tangents(mesh["positions"], mesh["normals"], mesh["uvs"], mesh["indices"])  # the fallback everywhere
    elif config == "positions_only":
        mesh["uvs"], mesh["normals"], tangents = None, None, None
    header, blob, got = prepare(gpu_ctx, mesh, meshlets=meshlets)
    wh, wb = mesh_cache.pack_cache(mesh["positions"], mesh["indices"], mesh["normals"], tangents, mesh["uvs"], with_meshlets=meshlets, ordered=True)
    assert header == want_header(wh, wb), config
    differ = np.flatnonzero(blob != wb)
    assert differ.size == 0, (config, differ[:8])
    assert (got is None) == (config in ("tangents_supplied", "no_uvs", "positions_only"))
    if config in ("no_uvs", "positions_only"):
        assert header["tangentsOffset"] == mesh_cache.ABSENT
    if config == "zero_indices":
        assert header["meshletCount"] == 0 and header["meshletsOffset"] == header["meshletBoundsOffset"] == header["blobByteCount"] // 4
    elif meshlets:
        assert header["meshletCount"] > 8


# ---- meshlets ----

def sections(header, blob):
    """(partition bytes, bounds words [n, 5]) of a blob"""
    n = header["meshletCount"]
    bounds = blob[header["meshletBoundsOffset"]:header["meshletBoundsOffset"] + 5 * n].reshape(n, 5)
    return blob[header["meshletsOffset"]:header["meshletBoundsOffset"]].tobytes() + blob[header["meshletBoundsOffset"] + 5 * n:].tobytes(), bounds


@pytest.mark.parametrize("name", sorted(PARTITION_CASES))
def test_meshlets_of_the_partition_s_cases(gpu_ctx, name):
    vertex_count, tri = PARTITION_CASES[name]
    positions = np.random.default_rng(len(name)).uniform(-3.0, 3.0, (vertex_count, 3)).astype(F)
    header, blob, _ = gpu_ctx.prepare_mesh(positions, tri, generate_tangents=False)
    wh, wb = mesh_cache.pack_cache(positions, tri, None, with_meshlets=True, ordered=True)
    assert header == want_header(wh, wb) and header["meshletCount"] == PARTITION_EXPECTED[name]
    (got_partition, got_bounds), (want_partition, want_bounds) = sections(header, blob), sections(wh, wb)
    assert got_partition == want_partition
    differ = np.flatnonzero((got_bounds != want_bounds).any(axis=1))
    assert differ.size == 0, (name, differ[:5], got_bounds[differ[:5]], want_bounds[differ[:5]])
    assert np.array_equal(blob, wb)


def test_meshlets_of_the_designed_scenes(gpu_ctx):
    cones = 0
    for name, positions, indices in scene_meshes():
        header, blob, _ = gpu_ctx.prepare_mesh(positions, indices, generate_tangents=False)
        wh, wb = mesh_cache.pack_cache(positions, indices, None, with_meshlets=True, ordered=True)
        assert header == want_header(wh, wb), name
        (got_partition, got_bounds), (want_partition, want_bounds) = sections(header, blob), sections(wh, wb)
        assert got_partition == want_partition, name
        differ = np.flatnonzero((got_bounds != want_bounds).any(axis=1))
        assert differ.size == 0, (name, differ[:5], got_bounds[differ[:5]], want_bounds[differ[:5]])
        cones += int((want_bounds[:, 4] & 0xFFFFFF != 0).sum())
    assert cones > 50  # (not only the never-hidden cone)


# ---- through the renderer ----

def normal_mapped_quad(tangents=None, prepared=None):
    """a quad that fills a 48 x 32 view from the origin (raster_scenes' S1 camera), with a normal map and a turned uv map"""
    world = scenes.World()
    rng = np.random.default_rng(8)
    texel = np.concatenate([rng.integers(40, 216, (8, 8, 2)), np.full((8, 8, 1), 230), np.full((8, 8, 1), 255)], axis=2).astype(np.uint8)
    material = world.add_material(base_color=(0.8, 0.8, 0.8, 1.0), metallic=0.0, roughness=0.7, normal_tex=(world.add_texture(texel), 0))
    p = np.array([(-1.5, -1, -1), (1.5, -1, -1), (1.5, 1, -1), (-1.5, 1, -1)], F)
    c, s = np.cos(0.6), np.sin(0.6)
    uv = (p[:, :2].astype(np.float64) @ np.array([[c, -s], [s, c]]) * 0.4 + 0.5).astype(F)
    mesh = quad(uv, positions=p)
    if prepared is not None:
        index = mesh_cache.add_cached_mesh(world, *prepared(mesh), material)
    else:
        index = world.add_mesh(mesh["positions"], mesh["indices"], material, normals=mesh["normals"], uvs=mesh["uvs"],
                               tangents=None if tangents is None else tangents(mesh))
    world.add_instance(world.add_model([(index, material)]))
    world.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 3.0, 0.0))
    return world


def test_a_normal_mapped_quad_prepared_on_the_gpu_renders_like_one_with_the_statement_s_tangents(gpu_ctx):
    cam = CS.camera_at(width=48, height=32)

    def normal_metalness(world):
        gpu_ctx.upload_scene(world)
        return gpu_ctx.trace_gbuffer(cam, 48, 32, jitter=False)[1]

    def statement(mesh):
        return T.generate_tangents(mesh["positions"], mesh["normals"], mesh["uvs"], mesh["indices"])

    def on_the_gpu(mesh):
        header, blob, _ = prepare(gpu_ctx, mesh, meshlets=False)
        return header, blob

    without = normal_metalness(normal_mapped_quad())
    supplied = normal_metalness(normal_mapped_quad(tangents=statement))
    prepared = normal_metalness(normal_mapped_quad(prepared=on_the_gpu))
    assert prepared.tobytes() == supplied.tobytes()
    assert np.isfinite(supplied).all() and supplied.any()
    changed = (without != supplied).any(axis=2).mean()
    print("pixels whose normal the map changes: %.0f %%" % (100 * changed))
    assert changed > 0.5


def copy_tiny_scene(folder):
    golden = os.path.join(ROOT, "tests", "golden")
    for name in os.listdir(golden):
        if name.startswith("tiny_scene") and not name.endswith(".npy"):
            shutil.copy(os.path.join(golden, name), os.path.join(folder, name))
    return os.path.join(folder, "tiny_scene.gltf")


def test_a_gltf_loads_from_the_mesh_caches_build_for_gltf_wrote(gpu_ctx, tmp_path):
    from prosper_amd.rt_reference import Camera
    path = copy_tiny_scene(str(tmp_path))
    written = mesh_cache.build_for_gltf(gpu_ctx, path)
    built = gltf.load_gltf(path)
    assert len(written) == len(built.metadatas) > 0 and all(os.path.exists(f) for f in written)
    assert built.add_meshlets() > 0
    cached = gltf.load_gltf(path, use_mesh_cache=True)
    assert cached.cached_meshes == written and all(i.meshletCount > 0 for i in cached.mesh_infos)
    assert [i.meshletCount for i in cached.mesh_infos] == [i.meshletCount for i in built.mesh_infos]
    w, h = 96, 64
    camera = Camera.from_world(cached, w, h)
    cam, _ = camera.update_buffer()
    camera.close()
    got = {}
    for name, world in (("cached", cached), ("built", built)):
        gpu_ctx.upload_scene(world)
        gpu_ctx.raster_release_preserved()
        raster_depth = gpu_ctx.raster_gbuffer(cam)[2]  # (no add_meshlets() for the cached one)
        got[name] = (raster_depth.copy(), gpu_ctx.trace_gbuffer(cam, w, h, jitter=False)[2].copy())
    assert (got["cached"][0] > 0).any() and (got["cached"][1] > 0).any()
    assert got["cached"][1].tobytes() == got["built"][1].tobytes()  # the traced depth, bit for bit
    assert got["cached"][0].tobytes() == got["built"][0].tobytes()  # and the rasterised one: the same partition
    # every cache is valid: nothing to write; a new write time: all of them again
    assert mesh_cache.build_for_gltf(gpu_ctx, path) == []
    stat = os.stat(path)
    os.utime(path, ns=(stat.st_atime_ns, stat.st_mtime_ns + 3_000_000_000))
    assert mesh_cache.build_for_gltf(gpu_ctx, path) == written
    assert mesh_cache.build_for_gltf(gpu_ctx, path) == []


# ---- refusals ----

def test_refusals_leave_the_last_result_readable():
    lib = capi.lib()
    ctx = capi.Context(device=0)
    try:
        mesh = displaced_grid(9, 7)
        n = len(mesh["positions"])
        out, blob = S.PreparedMesh(), np.zeros(1 << 16, np.uint32)
        tangents = np.zeros((n, 4), F)
        read_blob = lambda nbytes, dst=blob, handle=ctx._h: lib.prosper_pt_read_prepared_mesh(handle, dst.ctypes.data if dst is not None else None, nbytes)
        read_tangents = lambda nbytes, dst=tangents, handle=ctx._h: lib.prosper_pt_read_prepared_tangents(
            handle, dst.ctypes.data if dst is not None else None, nbytes)
        ms = [C.c_float() for _ in range(5)]
        timing = lambda handle=ctx._h, skip=None: lib.prosper_pt_get_prepare_mesh_timing(
            handle, *[None if k == skip else C.byref(m) for k, m in enumerate(ms)])

        def source(positions=mesh["positions"], normals=mesh["normals"], tangents=None, uvs=mesh["uvs"], indices=mesh["indices"], vertices=n, count=None):
            src = S.MeshSource(vertexCount=vertices, indexCount=indices.size if count is None else count)
            keep = [a for a in (positions, normals, tangents, uvs, indices)]
            for name, a in zip(("positions", "normals", "tangents", "texCoord0s", "indices"), keep):
                setattr(src, name, None if a is None else a.ctypes.data)
            return src, keep

        def call(src, flags=S.PREPARE_GENERATE_TANGENTS | S.PREPARE_MESHLETS, handle=ctx._h, result=out):
            return lib.prosper_pt_prepare_mesh(handle, C.byref(src[0]) if src is not None else None, flags, C.byref(result) if result is not None else None, None)

        before = ((lambda: read_blob(16), "no prosper_pt_prepare_mesh has completed"),
                  (lambda: read_tangents(16 * n), "no prosper_pt_prepare_mesh has generated tangents"),
                  (lambda: timing(), "no prosper_pt_prepare_mesh has completed"))
        for refused, text in before:
            assert refused() == -1
            assert text in lib.prosper_pt_last_error().decode(), text

        assert call(source()) == 0
        size = out.blobByteCount
        assert read_blob(size) == 0 and read_tangents(16 * n) == 0
        kept_blob, kept_tangents, kept_header = blob[:size // 4].copy(), tangents.copy(), bytes(out)
        assert kept_blob.any() and kept_tangents.any()

        bad_index = mesh["indices"].copy()
        bad_index[7] = n
        refusals = ((lambda: call(source(), handle=None), "null"), (lambda: call(None), "null"), (lambda: call(source(), result=None), "null"),
                    (lambda: call(source(positions=None)), "null"), (lambda: call(source(indices=None, count=3)), "null"),
                    (lambda: call(source(vertices=0)), "zero vertices"),
                    (lambda: call(source(count=mesh["indices"].size - 1)), "not a multiple of 3"),
                    (lambda: call(source(indices=bad_index)), "index 7 is %d, at or past the %d vertices" % (n, n)),
                    (lambda: call(source(normals=None)), "needs normals"),
                    (lambda: call(source(), flags=4), "unknown flags"), (lambda: call(source(), flags=0x80000001), "unknown flags"),
                    (lambda: read_blob(size - 4), "the blob holds %d bytes" % size), (lambda: read_blob(size + 4), "the blob holds"),
                    (lambda: read_blob(size, dst=None), "null"), (lambda: read_blob(size, handle=None), "null"),
                    (lambda: read_tangents(16 * n - 4), "the tangents hold %d bytes" % (16 * n)),
                    (lambda: read_tangents(16 * n, dst=None), "null"), (lambda: read_tangents(16 * n, handle=None), "null"),
                    (lambda: timing(handle=None), "null"), (lambda: timing(skip=2), "null"))
        for refused, text in refusals:
            result_before = bytes(out)
            assert refused() == -1
            assert text in lib.prosper_pt_last_error().decode(), text
            assert bytes(out) == result_before == kept_header
            blob[:] = 0
            tangents[:] = 0
            assert read_blob(size) == 0 and read_tangents(16 * n) == 0
            assert np.array_equal(blob[:size // 4], kept_blob) and np.array_equal(tangents, kept_tangents)
        # GENERATE_TANGENTS is prosper's condition: without uvs, or with tangents, it is not read - and needs no normals
        assert call(source(normals=None, uvs=None)) == 0 and out.tangentsOffset == mesh_cache.ABSENT
        assert call(source(normals=None, tangents=kept_tangents)) == 0 and out.tangentsOffset != mesh_cache.ABSENT
        # ... and the tangents of the last call that generated any stay readable
        assert read_tangents(16 * n) == 0 and np.array_equal(tangents, kept_tangents)
        # zero indices need no index pointer
        assert call(source(indices=None, count=0)) == 0 and out.meshletCount == 0 and out.indexCount == 0
    finally:
        ctx.close()


# ---- timing and the mirror ----

def test_the_stage_times_are_finite_and_not_negative(gpu_ctx):
    prepare(gpu_ctx, displaced_grid())
    ms = gpu_ctx.prepare_mesh_timing()
    print("tangents %.3f ms, pack %.3f ms, partition (host) %.3f ms, bounds %.3f ms, read back %.3f ms" % ms)
    assert len(ms) == 5 and all(np.isfinite(m) and m >= 0 for m in ms)


def test_cpp_mesh_preparer_through_a_compiled_consumer(gpu_ctx, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "the host C++ compiler (g++) is needed"
    exe = str(tmp_path / "mesh_preparer_main")
    lib_dir = os.path.join(ROOT, "prosper_amd")
    subprocess.check_call([gxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "mesh_preparer_main.cpp"), "-o", exe,
                           "-L" + lib_dir, "-lprosper_pt", "-Wl,-rpath," + lib_dir])
    supplied = displaced_grid()
    supplied["tangents"] = np.tile(np.array([[0, 1, 0, -1]], F), (len(supplied["positions"]), 1))
    for mesh, meshlets in ((displaced_grid(), 1), (supplied, 0), (dict(displaced_grid(9, 7), uvs=None), 1)):
        src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        streams = [mesh.get(k) for k in ("normals", "tangents", "uvs")]
        with open(src, "wb") as f:
            f.write(np.array([len(mesh["positions"]), mesh["indices"].size] + [int(a is not None) for a in streams] + [meshlets], np.uint32).tobytes())
            for a in [mesh["positions"]] + [a for a in streams if a is not None]:
                f.write(np.ascontiguousarray(a, F).tobytes())
            f.write(mesh["indices"].astype(np.uint32).tobytes())
        run = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        data = open(out, "rb").read()
        header, blob, tangents = prepare(gpu_ctx, mesh, meshlets=bool(meshlets))
        assert np.frombuffer(data, "<u4", 13).tolist() == [header[name] for name, _ in S.PreparedMesh._fields_]
        count = int(np.frombuffer(data, "<u4", 1, 52)[0])
        assert count == (0 if tangents is None else tangents.size)
        assert data[56:56 + blob.nbytes] == blob.tobytes()
        assert data[56 + blob.nbytes:] == (b"" if tangents is None else tangents.tobytes())
