"""glTF -> World ingest (prosper_amd/gltf.py) against a hand-made fixture whose expected tables
are derived here from the reference's conventions (file:line in the assertions), plus the reference's own
FlightHelmet asset (tests/golden/flight_helmet_gltf.tar.xz)."""
import math
import os

import numpy as np
import pytest

from prosper_amd import gltf, structs as S

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "tiny_scene.gltf")


@pytest.fixture(scope="module")
def tiny():
    return gltf.load_gltf(TINY)


def _v(v4):
    return np.array([v4.x, v4.y, v4.z, v4.w], np.float64)


def test_index_conventions(tiny):
    w = tiny
    assert w.missing_images == []
    # sampler i -> i + 1, NEAREST_MIPMAP_LINEAR -> nearest, mirrored / clamp (WorldData.cpp:183-217,699-719)
    assert w.samplers == [(S.FILTER_LINEAR, S.FILTER_LINEAR, S.WRAP_REPEAT, S.WRAP_REPEAT),
                          (S.FILTER_NEAREST, S.FILTER_NEAREST, S.WRAP_MIRRORED_REPEAT, S.WRAP_CLAMP_TO_EDGE)]
    # image i -> texture i + 1; slot 0 is the 1x1 "empty" texture (WorldData.cpp:724-737)
    assert len(w.textures) == 2 and w.textures[0].shape == (1, 1, 4)
    assert np.array_equal(w.textures[1], np.load(os.path.join(HERE, "golden", "tiny_scene_texture.npy")))
    # material m -> m + 1; Texture2DSampler packs (sampler << 24) | texture of the glTF *texture* (not image):
    # texture 0 = (image 0 + 1, sampler 0 + 1), texture 1 = (image 0 + 1, default sampler 0)
    m = w.materials
    assert len(m) == 4 and m[0].alphaMode == S.ALPHA_MODE_OPAQUE
    assert (m[1].baseColorTextureSampler, m[1].metallicRoughnessTextureSampler, m[1].normalTextureSampler) == (0x01000001, 0, 0)
    assert (m[1].alphaMode, m[2].alphaMode, m[3].alphaMode) == (S.ALPHA_MODE_MASK, S.ALPHA_MODE_BLEND, S.ALPHA_MODE_OPAQUE)
    assert m[1].alphaCutoff == pytest.approx(0.4) and m[2].alphaCutoff == pytest.approx(0.5)
    assert (m[2].baseColorTextureSampler, m[2].metallicRoughnessTextureSampler, m[2].normalTextureSampler) == (0, 0x00000001, 0x00000001)
    assert m[3].metallicFactor == 0.0 and m[3].roughnessFactor == 1.0  # glTF defaults copied (WorldData.cpp:800-805)
    np.testing.assert_allclose(_v(m[2].baseColorFactor), (0.2, 0.4, 0.9, 0.5), rtol=1e-7)


def test_meshes_models_and_draw_instances(tiny):
    w = tiny
    # one mesh per primitive, running index; a glTF mesh is a Model of sub-models (WorldData.cpp:830-915)
    assert w.models == [[(0, 1), (1, 2)], [(2, 3)]]
    infos = [(i.vertexCount, i.indexCount, i.materialIndex) for i in w.mesh_infos]
    assert infos == [(4, 6, 1), (3, 3, 2), (4, 6, 3)]
    md = w.metadatas
    assert all(x.usesShortIndices == 1 for x in md)  # vertexCount <= 0xFFFF whatever the source index type
    assert md[0].tangentsOffset != S.ABSENT and md[0].texCoord0sOffset != S.ABSENT
    assert md[1].tangentsOffset == S.ABSENT and md[1].texCoord0sOffset == S.ABSENT
    # scene nodes are popped from a LIFO stack: root, its children last-to-first, each subtree before the next
    # sibling (WorldData.cpp:1364-1456) -> model instances: floor, second quads (child of floor), quads
    assert [mi for mi, _ in w.model_instances] == [1, 0, 0]
    f = w.freeze()
    di = [(d.modelInstanceIndex, d.meshIndex, d.materialIndex) for d in f["draw_instances"][: f["draw_instance_count"]]]
    assert di == [(0, 2, 3), (1, 0, 1), (1, 1, 2), (2, 0, 1), (2, 1, 2)]  # World.cpp:478-513
    assert w.triangle_count() == 2 + 3 + 3


def test_node_transforms(tiny):
    w = tiny
    f = w.freeze()
    t = f["transforms"]
    # instance 2 ("quads"): translation kept, scale (1.0005, 0.9996, 1) is inside the 1e-3 threshold and
    # dropped, as is the root's 4e-4 translation (WorldData.cpp:1197-1211)
    rows = np.array([_v(t[2].modelToWorld.col[r]) for r in range(3)])
    np.testing.assert_array_equal(rows, [[1, 0, 0, 0.5], [0, 1, 0, 0.25], [0, 0, 1, 0]])
    # instance 1: the matrix node (decomposed to T*R*S and recomposed); modelToWorld = transpose(M4) i.e. its
    # three columns are the rows of the affine (World.cpp:405-414)
    rows = np.array([_v(t[1].modelToWorld.col[r]) for r in range(3)])
    np.testing.assert_allclose(rows, [[0, 0, 2, -2], [0, 2, 0, 0], [-2, 0, 0, -1]], atol=1e-6)
    # normalToWorld = mat3x4(inverse(M4)): its columns are the columns of the inverse
    inv = np.linalg.inv(np.array([[0, 0, 2, -2], [0, 2, 0, 0], [-2, 0, 0, -1], [0, 0, 0, 1.0]]))
    cols = np.array([_v(t[1].normalToWorld.col[c]) for c in range(3)])
    np.testing.assert_allclose(cols, inv[:, :3].T, atol=1e-6)
    # uv accessor was normalised u16: 65535 -> 1.0 -> half 0x3C00
    uv_words = f["geometry_buffers"][w.metadatas[0].bufferIndex][w.metadatas[0].texCoord0sOffset: w.metadatas[0].texCoord0sOffset + 4]
    assert [hex(int(x)) for x in uv_words] == ["0x0", "0x3c00", "0x3c003c00", "0x3c000000"]


def test_lights_and_camera(tiny):
    w = tiny
    w.freeze()
    # point: W -> radiance / (4 pi); no range -> radius = sqrt(luminance / 0.01) (WorldData.cpp:1482-1500)
    assert w.point_lights.count == 1 and w.spot_lights.count == 1
    rad = np.array([1.0, 0.5, 0.25]) * 50.0 / (4.0 * math.pi)
    lum = float(rad @ [0.2126, 0.7152, 0.0722])
    np.testing.assert_allclose(_v(w.point_lights.lights[0].radianceAndRadius), [*rad, math.sqrt(lum / 0.01)], rtol=1e-6)
    np.testing.assert_allclose(_v(w.point_lights.lights[0].position)[:3], (0.0, 2.5, 0.5), atol=1e-6)
    # spot: angle scale/offset from the cone angles, axis = -Z of the node (rotated -60 deg about x)
    scale = 1.0 / max(0.001, math.cos(0.3) - math.cos(0.6))
    s = w.spot_lights.lights[0]
    np.testing.assert_allclose(_v(s.radianceAndAngleScale), [*(np.ones(3) * 80.0 / (4 * math.pi)), scale], rtol=1e-6)
    np.testing.assert_allclose(_v(s.positionAndAngleOffset), [1.0, 2.0, 2.0, -math.cos(0.6) * scale], rtol=1e-6)
    np.testing.assert_allclose(_v(s.direction)[:3], (0.0, -math.sin(math.radians(60)), -math.cos(math.radians(60))), atol=1e-6)
    # sun: W/m^2 kept, direction = -Z rotated -45 deg about x (WorldData.cpp:1469-1480, World.cpp:428-433)
    np.testing.assert_allclose(_v(w.directional.irradiance)[:3], np.array([1.0, 0.9, 0.8]) * 3.0, rtol=1e-6)
    np.testing.assert_allclose(_v(w.directional.direction)[:3], (0.0, -math.sqrt(0.5), -math.sqrt(0.5)), atol=1e-6)
    # camera 0: eye = node origin, target = eye + (-Z), up = +Y (World.cpp:414-426)
    assert w.camera["eye"] == (0.0, 0.5, 4.0) and w.camera["target"] == (0.0, 0.5, 3.0) and w.camera["up"] == (0.0, 1.0, 0.0)
    assert (w.camera["fov"], w.camera["zN"], w.camera["zF"]) == (0.8, 0.05, 50.0)


def test_png_fallback_decoder_matches_pillow():
    import base64
    import json
    uri = json.load(open(TINY))["images"][0]["uri"]
    blob = base64.b64decode(uri.split(",", 1)[1])
    want = np.load(os.path.join(HERE, "golden", "tiny_scene_texture.npy"))
    assert np.array_equal(gltf._decode_png(blob), want)
    assert np.array_equal(gltf.decode_image(blob), want)


def test_rejects_what_the_reference_asserts_on(tmp_path):
    import json
    doc = json.load(open(TINY))
    del doc["meshes"][0]["primitives"][1]["indices"]
    p = tmp_path / "noindex.gltf"
    p.write_text(json.dumps(doc))
    with pytest.raises(gltf.GltfError):
        gltf.load_gltf(str(p))
    doc = json.load(open(TINY))
    del doc["materials"][1]["pbrMetallicRoughness"]
    p = tmp_path / "nopbr.gltf"
    p.write_text(json.dumps(doc))
    with pytest.raises(gltf.GltfError):
        gltf.load_gltf(str(p))


def test_tiny_scene_renders_on_the_oracle(oracle, tiny):
    from conftest import default_pc
    c = tiny.camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], 64, 48)
    osc = oracle.OracleScene(tiny, brute_force=True)
    img, _ = osc.render(default_pc(S, fl, draw_type=S.DrawType["MaterialID"], max_bounces=1), cam, 64, 48)
    assert len(np.unique(img[..., :3].reshape(-1, 3), axis=0)) >= 3  # floor + two materials + background
    rad, _ = osc.render(default_pc(S, fl, max_bounces=3), cam, 64, 48)
    assert np.isfinite(rad).all() and rad[..., :3].max() > 0.0


def test_flight_helmet_tables(oracle, flight_helmet_gltf):
    from conftest import default_pc
    w = gltf.load_gltf(flight_helmet_gltf)
    assert w.triangle_count() == 94722
    assert len(w.materials) == 6 and len(w.textures) == 16 and len(w.samplers) == 1
    assert len(w.missing_images) == 5  # the checkout carries 10 of the 15 images
    f = w.freeze()
    assert f["draw_instance_count"] == 5
    # nodes 0..4 hang off node 5 and are popped last-to-first: mesh 4 first (WorldData.cpp:1364-1456)
    order = [(d.modelInstanceIndex, d.meshIndex, d.materialIndex) for d in f["draw_instances"][:5]]
    assert order == [(0, 4, 5), (1, 3, 4), (2, 2, 3), (3, 1, 2), (4, 0, 1)]
    assert all(m.usesShortIndices == 1 for m in w.metadatas)
    # LeatherParts_low carries a 0.03 translation (kept: above the 1e-3 threshold)
    row = f["transforms"][3].modelToWorld.col[1]
    assert abs(row.w - 0.032592997) < 1e-7
    # a quick look through the default camera pulled back to see the helmet: the oracle traces it
    w.camera = dict(eye=(0.0, 0.0, 1.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=math.radians(45.0), zN=0.05, zF=50.0)
    c = w.camera
    cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], 96, 96)
    osc = oracle.OracleScene(w, brute_force=False)
    img, cnt = osc.render(default_pc(S, fl, draw_type=S.DrawType["MeshID"], max_bounces=1), cam, 96, 96)
    covered = (img[..., :3].sum(axis=2) > 0).mean()
    assert 0.15 < covered < 0.9
