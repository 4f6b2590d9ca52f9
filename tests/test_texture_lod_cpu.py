"""Texture mip chains and sample_texture_lod without a GPU: the entry points exist and refuse bad arguments
before they touch the device, TextureDesc.mipLevelCount mirrors the header, and tests/texture_lod_reference.py gives the
answers worked by hand for the box reduction, lambda, the clamp at the last level and prosper's level counts."""
import ctypes as C
import os
import re

import numpy as np

import texture_lod_reference as R
from prosper_amd import capi, structs as S, world as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_the_symbols_exist_and_the_abi_is_4():
    lib = capi.lib()
    for name in ("prosper_pt_get_texture_mips_info", "prosper_pt_read_texture_level", "prosper_pt_debug_sample_texture_lod",
                 "prosper_pt_texture_mip_level_count", "prosper_pt_check_texture_desc", "prosper_pt_set_texture_lod",
                 "prosper_pt_set_texture_lod_debug", "prosper_pt_read_texture_lod_derivatives"):
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    assert S.CREATE_TEXTURE_MIPS == 1 << 3
    text = open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()
    assert re.search(r"PROSPER_PT_CREATE_TEXTURE_MIPS\s*=\s*1u\s*<<\s*3", text)


def test_bad_arguments_are_refused_before_the_gpu_is_touched():
    lib = capi.lib()
    texels = np.zeros((64, 64, 4), np.uint8)
    rec = np.zeros((1, 6), F)
    out = np.zeros((1, 5), F)
    # the null context
    assert lib.prosper_pt_get_texture_mips_info(None, 1, C.byref(S.TextureMipsInfo())) == -1
    assert lib.prosper_pt_read_texture_level(None, 1, 0, texels.ctypes.data, texels.nbytes, None) == -1
    assert lib.prosper_pt_debug_sample_texture_lod(None, 1, 0, rec.ctypes.data, 1, 0.0, out.ctypes.data) == -1
    assert b"null argument" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_set_texture_lod(None, 1, 0.0) == -1 and b"null context" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_set_texture_lod_debug(None, 1) == -1
    assert lib.prosper_pt_read_texture_lod_derivatives(None, out.ctypes.data, 16, None) == -1
    # a bias that is not finite
    for bias in (float("nan"), float("inf"), -float("inf")):
        assert lib.prosper_pt_set_texture_lod(None, 1, bias) == -1
        assert b"lodBias is not finite" in lib.prosper_pt_last_error()
        assert lib.prosper_pt_debug_sample_texture_lod(None, 1, 0, rec.ctypes.data, 1, bias, out.ctypes.data) == -1
        assert b"not finite" in lib.prosper_pt_last_error()
    # a level count above prosper's (64 x 64 has five levels): refused with the flag, not read without it
    desc = S.TextureDesc(texels.ctypes.data, 64, 64, S.FORMAT_RGBA8_UNORM, 6)
    assert lib.prosper_pt_check_texture_desc(C.byref(desc), S.CREATE_TEXTURE_MIPS) == -5
    assert b"mipLevelCount 6 exceeds the 5 levels" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_check_texture_desc(C.byref(desc), 0) == 0
    for count in (0, 1, 2, 5):
        desc.mipLevelCount = count
        assert lib.prosper_pt_check_texture_desc(C.byref(desc), S.CREATE_TEXTURE_MIPS) == 0
    # a supplied BC7 level that is no whole number of blocks: 24 x 24 -> 12 x 12 -> 6 x 6
    bc7 = S.TextureDesc(texels.ctypes.data, 24, 24, S.FORMAT_BC7_UNORM, 3)
    assert lib.prosper_pt_check_texture_desc(C.byref(bc7), S.CREATE_TEXTURE_MIPS) == -5
    assert b"mip level 2" in lib.prosper_pt_last_error()
    bc7.mipLevelCount = 2
    assert lib.prosper_pt_check_texture_desc(C.byref(bc7), S.CREATE_TEXTURE_MIPS) == 0
    assert lib.prosper_pt_check_texture_desc(None, 0) == -1


def test_the_texture_desc_keeps_its_layout_with_the_new_field():
    assert C.sizeof(S.TextureDesc) == 24
    assert [(n, getattr(S.TextureDesc, n).offset) for n, _ in S.TextureDesc._fields_] == [
        ("texels", 0), ("width", 8), ("height", 12), ("format", 16), ("mipLevelCount", 20)]
    text = open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()
    body = text[text.index("typedef struct prosper_pt_texture_desc"):text.index("} prosper_pt_texture_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(?:const void \*|uint32_t )([A-Za-z]+);", body) == [n for n, _ in S.TextureDesc._fields_]
    body = text[text.index("typedef struct prosper_pt_texture_mips_info"):text.index("} prosper_pt_texture_mips_info;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for line in re.findall(r"\b(?:uint32_t|uint64_t)\s+([A-Za-z_, ]+);", body) for n in line.replace(" ", "").split(",")]
    assert fields == [n for n, _ in S.TextureMipsInfo._fields_]
    assert C.sizeof(S.TextureMipsInfo) == 24
    # the descriptors world.py fills: a chain says how many levels it holds, a plain array says none
    chain = W.TextureChain(R.generate_chain(np.zeros((16, 4, 4), np.uint8), False))
    d = S.TextureDesc()
    W.fill_texture_desc(d, chain)
    assert (d.width, d.height, d.mipLevelCount) == (4, 16, 3) and chain.texels.size == (64 + 16 + 4) * 4
    W.fill_texture_desc(d, np.zeros((8, 8, 4), np.uint8))
    assert (d.width, d.height, d.mipLevelCount) == (8, 8, 0)


def test_prospers_level_counts():
    lib = capi.lib()
    for (w, h), count in {(64, 64): 5, (16, 4): 3, (36, 20): 4, (5, 3): 1, (1, 1): 1, (4, 4): 1, (8, 8): 2, (1024, 512): 9}.items():
        assert R.mip_level_count(w, h) == count
        assert W.mip_level_count(w, h) == count
        assert lib.prosper_pt_texture_mip_level_count(w, h) == count
        assert lib.prosper_pt_texture_mip_level_count(h, w) == count
    assert [R.level_extent(36, 20, l) for l in range(4)] == [(36, 20), (18, 10), (9, 5), (4, 2)]
    assert [R.level_extent(16, 4, l) for l in range(3)] == [(16, 4), (8, 2), (4, 1)]
    assert [a.shape[:2] for a in R.generate_chain(np.zeros((20, 36, 4), np.uint8), False)] == [(20, 36), (10, 18), (5, 9), (2, 4)]


def test_a_4x4_linear_reduction_worked_by_hand():
    p = np.zeros((4, 4, 4), np.uint8)
    p[..., 0] = [[0, 1, 10, 20], [2, 4, 30, 40], [255, 255, 0, 0], [255, 254, 0, 1]]
    p[..., 1] = 7
    p[..., 3] = p[..., 0]
    c = R.generate_level(p, False)
    assert c.shape == (2, 2, 4)
    # (0 + 1 + 2 + 4 + 2) >> 2 = 2, (100 + 2) >> 2 = 25, (1019 + 2) >> 2 = 255, (1 + 2) >> 2 = 0
    assert c[..., 0].tolist() == [[2, 25], [255, 0]]
    assert (c[..., 1] == 7).all() and (c[..., 3] == c[..., 0]).all()
    # an odd parent repeats its last column and row: 5 x 3 -> 2 x 1
    q = np.zeros((3, 5, 4), np.uint8)
    q[..., 0] = [[0, 4, 8, 12, 100], [0, 4, 8, 12, 100], [50, 50, 50, 50, 50]]
    assert R.generate_level(q, False)[..., 0].tolist() == [[2, 10]]
    # 1 x 4 -> 1 x 2: both rows of the box are row 0
    r = np.zeros((1, 4, 4), np.uint8)
    r[..., 0] = [[10, 20, 30, 33]]
    assert R.generate_level(r, False)[..., 0].tolist() == [[15, 32]]  # (10+20+10+20+2)>>2, (30+33+30+33+2)>>2 = 128>>2


def test_a_4x4_srgb_reduction_worked_by_hand(oracle):
    lut = R.srgb_lut()
    # the restated curve is the device's (the oracle's is the same bits: tests/test_gpu_parity.py)
    want = oracle.eval_fn(2, (np.arange(256, dtype=F) * R.K255).astype(F).reshape(-1, 1))
    assert (np.asarray(want, F).reshape(-1)[:256].view(np.uint32) == lut.view(np.uint32)).all()
    assert (np.diff(lut) > 0).all()
    p = np.zeros((4, 4, 4), np.uint8)
    # two black and two white codes: linear mean 0.5, between code 187 (0.4969) and 188 (0.5029): 188, not the 128 of
    # an average of codes.  One white in four: 0.25 -> 137 (0.2502; 136 is 0.2462).  Equal codes stay.
    p[..., 0] = [[0, 255, 0, 0], [255, 0, 0, 255], [90, 90, 255, 255], [90, 90, 255, 255]]
    p[..., 1] = p[..., 0]
    p[..., 2] = 33
    p[..., 3] = [[0, 255, 0, 0], [255, 0, 0, 255], [1, 2, 3, 4], [5, 6, 7, 8]]
    c = R.generate_level(p, True)
    assert c[..., 0].tolist() == [[188, 137], [90, 255]]
    assert (c[..., 1] == c[..., 0]).all() and (c[..., 2] == 33).all()
    assert c[..., 3].tolist() == [[128, 64], [4, 6]]  # alpha is linear: (510 + 2) >> 2, (255 + 2) >> 2, (14 + 2) >> 2, (22 + 2) >> 2
    assert abs(float(lut[188]) - 0.5) < abs(float(lut[187]) - 0.5) and abs(float(lut[137]) - 0.25) < abs(float(lut[136]) - 0.25)


def test_lambda_for_rho_1_2_3_0_and_inf_with_bias():
    w, h = 64, 32

    def lam(rho_x, rho_y, bias):
        # du/dx = rho_x / w along u only, dv/dy = rho_y / h along v only
        d = np.array([[rho_x / w, 0.0, 0.0, rho_y / h]], F)
        return float(R.texture_lambda(w, h, d, bias)[0])

    assert lam(1, 0, 0.0) == 0.0 and lam(1, 1, 1.0) == 1.0 and lam(1, 0.5, -1.0) == -1.0
    assert lam(2, 1, 0.0) == 1.0 and lam(1, 2, -1.0) == 0.0 and lam(2, 2, 1.0) == 2.0
    assert abs(lam(3, 1, 0.0) - 1.584962500721156) <= 2.0 ** -22
    assert abs(lam(0, 3, 1.0) - 2.584962500721156) <= 2.0 ** -21
    assert lam(0, 0, 0.0) == -np.inf and lam(0, 0, 1.0) == -np.inf
    for bad in (np.inf, -np.inf, np.nan):
        for k in range(4):
            d = np.array([[1.0 / w, 0.0, 0.0, 1.0 / h]], F)
            d[0, k] = bad
            assert R.texture_lambda(w, h, d, -1.0)[0] == np.inf
    assert R.texture_lambda(w, h, np.array([[3e38, 0, 0, 0]], F), 0.0)[0] == np.inf  # rho overflows
    # both components of one axis: |(3, 4)| = 5
    d = np.array([[3.0 / w, 4.0 / h, 0.0, 0.0]], F)
    assert abs(float(R.texture_lambda(w, h, d, 0.0)[0]) - np.log2(5.0)) <= 2.0 ** -21
    # the restated log2_ against float64 over the range a lambda can take
    x = np.exp2(np.random.default_rng(5).uniform(-20, 20, 4096)).astype(F)
    assert np.abs(R.log2_(x).astype(np.float64) - np.log2(x.astype(np.float64))).max() <= 2.0 ** -18


def test_the_clamp_at_the_last_level_and_the_blend():
    lo, hi, f = R.lod_levels(np.array([0.25, 1.0, 2.25, 2.999, 3.0, 5.3, np.inf], F), 4)
    assert lo.tolist() == [0, 1, 2, 2, 3, 3, 3] and hi.tolist() == [1, 2, 3, 3, 3, 3, 3]
    assert f.tolist() == [0.25, 0.0, 0.25, float(F(2.999) - F(2.0)), 0.0, 0.0, 0.0]
    lo, hi, f = R.lod_levels(np.array([0.5, 7.0], F), 1)  # a chain of one level: level 0 through minFilter
    assert lo.tolist() == [0, 0] and hi.tolist() == [0, 0] and f.tolist() == [0.0, 0.0]
    # flat levels 10, 50, 90, 130: the sample reads lambda off the blend
    chain = [np.full((32 >> l, 32 >> l, 4), 10 + 40 * l, np.uint8) for l in range(4)]
    uv = np.full((5, 2), 0.3, F)
    d = np.zeros((5, 4), F)
    d[:, 0] = np.array([0.5, 1.0, 2.0, 2.0 ** 1.5, 64.0], F) / F(32)
    rgba, lam = R.sample_texture_lod(chain, (R.LINEAR, R.LINEAR, R.REPEAT, R.REPEAT), uv, d, 0.0)
    assert lam[:3].tolist() == [-1.0, 0.0, 1.0] and abs(float(lam[3]) - 1.5) < 1e-6 and lam[4] == 6.0
    assert np.allclose(rgba[:, 0] * 255.0, [10, 10, 50, 70, 130], atol=1e-3)
    # bias -1 moves the ones above a level down by one level, +1 up
    assert np.allclose(R.sample_texture_lod(chain, (1, 1, 0, 0), uv, d, -1.0)[0][:, 0] * 255.0, [10, 10, 10, 30, 130], atol=1e-3)
    assert np.allclose(R.sample_texture_lod(chain, (1, 1, 0, 0), uv, d, 1.0)[0][:, 0] * 255.0, [10, 50, 90, 110, 130], atol=1e-3)


def test_lambda_at_most_zero_is_the_lod_0_sample_through_the_mag_filter():
    rng = np.random.default_rng(11)
    chain = R.generate_chain(rng.integers(0, 256, (20, 36, 4), dtype=np.uint8), False)
    uv = rng.uniform(-2, 3, (200, 2)).astype(F)
    d = np.zeros((200, 4), F)
    d[:, 0] = rng.uniform(0, 1.0 / 36, 200)
    d[:, 3] = rng.uniform(0, 1.0 / 20, 200)
    for mag in (R.NEAREST, R.LINEAR):
        for wrap in (R.REPEAT, R.MIRRORED_REPEAT, R.CLAMP_TO_EDGE):
            rgba, lam = R.sample_texture_lod(chain, (mag, 1 - mag, wrap, wrap), uv, d, 0.0)
            assert (lam <= 0).all()
            assert (rgba.view(np.uint32) == R.sample_level(chain[0], mag, wrap, wrap, uv).view(np.uint32)).all()


def test_the_gltf_loader_passes_a_caches_levels_through(tmp_path):
    import base64
    import json
    from prosper_amd import bc7, dds, gltf
    rng = np.random.default_rng(3)
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    blob = pos.tobytes() + np.array([0, 1, 2], np.uint16).tobytes() + b"\0\0" + np.tile(np.array([0, 0, 1], np.float32), (3, 1)).tobytes()
    doc = {
        "asset": {"version": "2.0"},
        "buffers": [{"byteLength": len(blob), "uri": "data:application/octet-stream;base64," + base64.b64encode(blob).decode()}],
        "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 36}, {"buffer": 0, "byteOffset": 36, "byteLength": 6},
                        {"buffer": 0, "byteOffset": 44, "byteLength": 36}],
        "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3", "min": [0, 0, 0], "max": [1, 1, 0]},
                      {"bufferView": 1, "componentType": 5123, "count": 3, "type": "SCALAR"},
                      {"bufferView": 2, "componentType": 5126, "count": 3, "type": "VEC3"}],
        "images": [{"uri": "a.png"}, {"uri": "b.png"}],
        "textures": [{"source": 0}, {"source": 1}],
        "materials": [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicRoughnessTexture": {"index": 1}}}],
        "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 2}, "indices": 1, "material": 0}]}],
        "nodes": [{"mesh": 0}], "scenes": [{"nodes": [0]}], "scene": 0,
    }
    path = str(tmp_path / "scene.gltf")
    with open(path, "w") as f:
        json.dump(doc, f)
    os.makedirs(tmp_path / "prosper_cache")
    # a BC7 cache of 16 x 16 (prosper's three levels: 16, 8, 4) and an RGBA8 one of 8 x 8 that holds one level too many
    blocks = rng.integers(0, 256, (21, 16), dtype=np.uint8)
    payloads = [blocks[:16].tobytes(), blocks[16:20].tobytes(), blocks[20:].tobytes()]
    dds.write_texture(dds.cache_path(str(tmp_path / "a.png")), dds.DXGI_FORMAT_BC7_UNORM, 16, 16, payloads)
    rgba = [rng.integers(0, 256, (8 >> l, 8 >> l, 4), dtype=np.uint8) for l in range(3)]
    dds.write_texture(dds.cache_path(str(tmp_path / "b.png")), dds.DXGI_FORMAT_R8G8B8A8_UNORM, 8, 8, [a.tobytes() for a in rgba])
    assert dds.level_count(dds.cache_path(str(tmp_path / "a.png"))) == 3
    plain = gltf.load_gltf(path, use_texture_cache="always", bc7_on_gpu=True)
    assert plain.textures[1].levels == 1 and plain.textures[1].blocks.shape == (16, 16) and (plain.textures[2] == rgba[0]).all()
    w = gltf.load_gltf(path, use_texture_cache="always", bc7_on_gpu=True, mip_chains=True)
    a, b = w.textures[1], w.textures[2]
    assert isinstance(a, W.Bc7Texture) and a.levels == 3 and (a.blocks == blocks).all()
    assert isinstance(b, W.TextureChain) and len(b.levels) == 2 and all((x == y).all() for x, y in zip(b.levels, rgba))
    descs = w.freeze()["textures"]
    assert (descs[1].mipLevelCount, descs[2].mipLevelCount) == (3, 2)
    assert all(capi.lib().prosper_pt_check_texture_desc(C.byref(descs[i]), S.CREATE_TEXTURE_MIPS) == 0 for i in (0, 1, 2))
    # decoded on the host instead: the same texels as a chain
    w = gltf.load_gltf(path, use_texture_cache="always", mip_chains=True)
    assert [x.shape[:2] for x in w.textures[1].levels] == [(16, 16), (8, 8), (4, 4)]
    assert (w.textures[1].levels[1] == bc7.decode_image(payloads[1], 8, 8)).all()


def test_the_host_mirrors_bias_is_minus_one_with_taa_and_zero_without():
    from prosper_amd.rt_reference import renderer_lod_bias
    lib = capi.lib()
    assert hasattr(lib, "prosper_host_gbuffer_tracer_set_texture_lod")
    assert renderer_lod_bias(True) == -1.0 and renderer_lod_bias(False) == 0.0
    assert lib.prosper_host_gbuffer_tracer_set_texture_lod(None, 1, -1.0) == -1


def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    import subprocess
    import sys
    objects = [os.path.join(ROOT, "prosper_amd", "csrc", n) for n in ("pt_texture_mips.o", "pt_gbuffer_kernels.o")]
    assert all(os.path.exists(o) for o in objects)  # (the build leaves them in the tree)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py")] + objects, text=True)
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(.*?)\s+vgpr\s+(\d+) spill\s+(\d+) sgpr\s+(\d+) lds\s+(\d+) scratch\s+(\d+)", line)
        rows[m.group(1).strip()] = tuple(int(v) for v in m.groups()[1:])
    new = [k for k in rows if "generate_mip_kernel" in k or "untile_level_kernel" in k or "sample_texture_lod_kernel" in k
           or re.match(r"(gbuffer_trace|forward_transparent)_kernel<\w+, \w+, true>", k)]
    assert len(new) == 12, sorted(rows)
    for k in new:
        vgpr, spill, _, _, scratch = rows[k]
        assert spill == 0 and scratch == 0 and vgpr <= 256, (k, rows[k])
