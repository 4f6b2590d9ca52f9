import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture
def _experiments_only():
    """Tests of the measured-slower variants: they exist only in libprosper_pt_experiments.so (make EXPERIMENTS=1; run the
    suite with PROSPER_PT_LIB=prosper_amd/libprosper_pt_experiments.so).  Decided when the test runs, not at import: the
    library must not be loaded before the test modules are collected (one of them imports torch, which brings its own
    copy of the HIP runtime; whichever loads first is the one the process uses)."""
    from prosper_amd import capi
    if not capi.has_experiments():
        pytest.skip("library built without -DPPT_EXPERIMENTS")


needs_experiments = pytest.mark.usefixtures("_experiments_only")


@pytest.fixture(autouse=True)
def _no_debug_options_leak():
    """Process-wide debug options (capi.debug) never outlive the test that set them."""
    yield
    from prosper_amd import capi
    capi.debug()


@pytest.fixture(scope="session", autouse=True)
def _extra_streams():
    """PROSPER_TEST_EXTRA_STREAMS=n: n more HIP streams alive (and used once) for the whole session.  Which streams share a
    hardware queue - and with it the order in which the frames' streams get to run - depends on the streams alive in the
    process: a dependency that is missing between two of the library's streams can hide behind one sharing and show behind
    another (it did: tests/test_adoption.py "fifth_stream").  Run the GPU suite with 1 and 2 now and then."""
    n = int(os.environ.get("PROSPER_TEST_EXTRA_STREAMS", "0"))
    streams = []
    if n:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        for _ in range(n):
            st, ev = ctypes.c_void_p(), ctypes.c_void_p()
            assert hip.hipStreamCreateWithFlags(ctypes.byref(st), 1) == 0 and hip.hipEventCreate(ctypes.byref(ev)) == 0
            assert hip.hipEventRecord(ev, st) == 0 and hip.hipStreamSynchronize(st) == 0
            hip.hipEventDestroy(ev)
            streams.append(st)
    yield
    # (left alive: contexts of the session fixture are closed after this one)


@pytest.fixture(scope="session")
def oracle():
    from oracle import binding
    binding.lib()
    return binding


@pytest.fixture(scope="session")
def gpu_ctx():
    """One prosper_pt context on cuda:0 for the whole session (loads libprosper_pt.so; no fallback)."""
    from prosper_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build()  # the test harness may build the product; the product itself never falls back
    ctx = capi.Context(device=0)
    yield ctx
    ctx.close()


def flight_helmet_bin(doc, world):
    """FlightHelmet.bin rebuilt from the packed fixture (tests/golden/flight_helmet.npz): every accessor of the glTF `doc`
    filled with what the fixture's streams hold (fp16 positions and uvs, snorm10 normals and tangents, u16 indices) as
    float32 / u16.  The packing is exact on these values, so ingesting the rebuilt buffer gives the fixture's bytes
    wherever ingesting the shipped one does (tests/golden/make_reference_assets.py checks both on the shipped asset)."""
    words = np.concatenate(world._buffers[0]).astype(np.uint32)
    out = bytearray(doc["buffers"][0]["byteLength"])

    def put(accessor, values):
        a = doc["accessors"][accessor]
        view = doc["bufferViews"][a["bufferView"]]
        data = np.ascontiguousarray(values).tobytes()
        assert view.get("byteStride", len(data) // a["count"]) * a["count"] == len(data) <= view["byteLength"]
        off = view.get("byteOffset", 0) + a.get("byteOffset", 0)
        out[off:off + len(data)] = data

    def snorm(w):  # glm::unpackSnorm3x10_1x2: sign-extended 10/10/10/2-bit fields / (511, 511, 511, 1), clamped to -1
        fields = [(w << np.uint32(22 - s)).view(np.int32) >> 22 for s in (0, 10, 20)] + [w.view(np.int32) >> 30]
        return np.maximum(np.stack(fields, axis=1).astype(np.float32) / np.array([511, 511, 511, 1], np.float32), np.float32(-1))

    for mesh, md, info in zip(doc["meshes"], world.metadatas, world.mesh_infos):
        (prim,) = mesh["primitives"]
        attrs, n = prim["attributes"], info.vertexCount
        assert md.usesShortIndices == 1 and doc["accessors"][prim["indices"]]["componentType"] == 5123
        put(prim["indices"], words.view(np.uint16)[md.indicesOffset:md.indicesOffset + info.indexCount])
        put(attrs["POSITION"], words[md.positionsOffset:md.positionsOffset + 2 * n].view(np.float16).reshape(n, 4)[:, :3].astype(np.float32))
        put(attrs["NORMAL"], snorm(words[md.normalsOffset:md.normalsOffset + n])[:, :3])
        put(attrs["TANGENT"], snorm(words[md.tangentsOffset:md.tangentsOffset + n]))
        put(attrs["TEXCOORD_0"], words[md.texCoord0sOffset:md.texCoord0sOffset + n].view(np.float16).reshape(n, 2).astype(np.float32))
    return bytes(out)


@pytest.fixture(scope="session")
def flight_helmet_gltf(tmp_path_factory):
    """The reference's FlightHelmet glTF asset in a temporary directory; the path of its .gltf.  From
    tests/golden/flight_helmet_gltf.tar.xz: the .gltf as shipped and its images reduced to 64 x 64
    (tests/golden/make_reference_assets.py); the .bin (3.4 MB) rebuilt from tests/golden/flight_helmet.npz."""
    import json
    import lzma
    import tarfile
    from prosper_amd import flight_helmet
    d = tmp_path_factory.mktemp("flight_helmet_gltf")
    with lzma.open(os.path.join(ROOT, "tests", "golden", "flight_helmet_gltf.tar.xz")) as f, tarfile.open(fileobj=f) as tar:
        tar.extractall(d, filter="data")
    doc = json.loads((d / "FlightHelmet.gltf").read_text())
    (d / doc["buffers"][0]["uri"]).write_bytes(flight_helmet_bin(doc, flight_helmet.load_fixture(sky_size=0)))
    return str(d / "FlightHelmet.gltf")


@pytest.fixture(scope="session")
def cornell_world():
    from prosper_amd import scenes
    return scenes.cornell(with_skybox=True)


def default_pc(structs, focal_length, frame_index=1, max_bounces=4, draw_type=0, ibl=False, dof=False,
               skip_history=True, accumulate=True, clamp=True, roulette=3):
    flags = 0
    flags |= structs.PC_FLAG_SKIP_HISTORY if skip_history else 0
    flags |= structs.PC_FLAG_ACCUMULATE if accumulate else 0
    flags |= structs.PC_FLAG_IBL if ibl else 0
    flags |= structs.PC_FLAG_DEPTH_OF_FIELD if dof else 0
    flags |= structs.PC_FLAG_CLAMP_INDIRECT if clamp else 0
    return structs.ReferencePC(draw_type, flags, frame_index, 1e-5, 1.0, focal_length, roulette, max_bounces)


def same_bits(a, b):
    """Bitwise equality of float32 arrays, with NaN == NaN regardless of payload."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    eq = a.view(np.uint32) == b.view(np.uint32)
    return eq | (np.isnan(a) & np.isnan(b))
