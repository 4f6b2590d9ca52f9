"""The HIP BC7 encoder and prosper_pt_compress_texture against prosper_amd.bc7.encode_blocks, the numpy
statement of the encoder rule: every block byte for byte, every squared error as it is."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from prosper_amd import bc7, capi, scenes, structs as S
from prosper_amd.world import World
from test_bc7_encode_cpu import MASKS, sample_blocks, write_gltf, write_png

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIP_SIZES = ((8, 8), (32, 32), (64, 64))


def rand_image(w, h, seed):
    """random texels with smooth and opaque regions, so that every candidate gets chosen somewhere"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.stack([x * 7 + y, 255 - y * 5, (x * y) % 256, 128 + x - y], axis=2) % 256
    img[:, : w // 2] = (smooth[:, : w // 2] + rng.integers(0, 4, (h, w // 2, 4))).clip(0, 255)
    img[: h // 2, :, 3] = 255
    return img


@pytest.fixture(scope="module")
def ctx():
    """a context of its own: no scene, no CREATE_TEXTURE_MIPS"""
    c = capi.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference_blocks():
    """the mixed blocks and what the rule makes of them under every mask, computed once"""
    texels = sample_blocks(11, 160)
    texels = texels[np.random.default_rng(1).permutation(len(texels))[:257 + 65 + 64 + 63 + 1]]
    return texels, {mask: bc7.encode_blocks(texels, mask) for mask in MASKS}


@pytest.mark.parametrize("mask", MASKS)
def test_loose_blocks_equal_the_rule(ctx, reference_blocks, mask):
    texels, want = reference_blocks
    rng = np.random.default_rng(2)
    order = rng.permutation(len(texels))
    start = 0
    for n in (0, 1, 63, 64, 65, 257):
        pick = order[start:start + n]
        start += n
        blocks, sse = ctx.debug_bc7_encode_blocks(texels[pick], mask)
        assert blocks.shape == (n, 16) and sse.shape == (n,)
        bad = (blocks != want[mask][0][pick]).any(axis=1)
        assert not bad.any(), "n = %d: %d blocks differ, first at %d" % (n, bad.sum(), np.nonzero(bad)[0][0])
        assert np.array_equal(sse.astype(np.int64), want[mask][1][pick])
    assert start == len(texels)
    assert len(set(want[0][2].tolist())) == 3      # all three modes are chosen somewhere in the mix


@pytest.mark.parametrize("size", [(4, 4), (8, 4), (12, 4), (4, 8), (260, 12)])
def test_images_without_mips(ctx, size):
    """one block, one full tile, a half-filled last tile, two tile rows, a 65-block row that crosses a wave"""
    img = rand_image(size[0], size[1], 20 + size[0])
    fmt, levels = ctx.compress_texture(img, mips=False)
    assert fmt == S.FORMAT_BC7_UNORM and len(levels) == 1
    assert levels[0] == bc7.encode_image(img)


@pytest.fixture(scope="module")
def generated_chains():
    """Levels as the library itself generates them: the same textures in a CREATE_TEXTURE_MIPS context, once as a base
    colour (averaged in linear light) and once as metallic-roughness (integer box)."""
    w = World()
    index = {}
    for size in MIP_SIZES:
        img = rand_image(size[0], size[1], 40 + size[0])
        index[size] = (img, w.add_texture(img), w.add_texture(img.copy()))
        material = w.add_material(base_tex=(index[size][1], 0), mr_tex=(index[size][2], 0))
        q = scenes._add(w, scenes.quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)), material)
        w.add_instance(w.add_model([(q, material)]))
    mip_ctx = capi.Context(device=0, flags=S.CREATE_TEXTURE_MIPS)
    try:
        mip_ctx.upload_scene(w)
        out = {}
        for size, (img, base, linear) in index.items():
            for srgb, texture in ((True, base), (False, linear)):
                info = mip_ctx.texture_mips_info(texture)
                assert info.srgbAveraged == int(srgb)
                out[size, srgb] = (img, [mip_ctx.read_texture_level(texture, l, size[0], size[1]) for l in range(info.levelCount)])
    finally:
        mip_ctx.close()
    return out


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("size", MIP_SIZES)
def test_images_with_mips(ctx, generated_chains, size, srgb):
    img, chain = generated_chains[size, srgb]
    fmt, levels = ctx.compress_texture(img, srgb=srgb, mips=True)
    assert fmt == S.FORMAT_BC7_UNORM
    assert len(levels) == len(chain) == capi.compressed_texture_layout(size[0], size[1], True)[1]
    assert np.array_equal(chain[0], img)
    for l, (payload, texels) in enumerate(zip(levels, chain)):
        assert payload == bc7.encode_image(texels), "level %d" % l
    if size == (64, 64):
        assert generated_chains[size, True][1][2].tobytes() != generated_chains[size, False][1][2].tobytes()


def test_a_supplied_chain_is_encoded_as_given(ctx):
    chain = [rand_image(32 >> l, 32 >> l, 60 + l) for l in range(3)]   # nothing like a reduction; shorter than prosper's 4
    fmt, levels = ctx.compress_texture(chain, srgb=True)
    assert fmt == S.FORMAT_BC7_UNORM and len(levels) == 3
    for payload, texels in zip(levels, chain):
        assert payload == bc7.encode_image(texels)


@pytest.mark.parametrize("size", [(24, 12), (10, 6)])
def test_rgba8_fallback_returns_the_raw_chain(ctx, size):
    img = rand_image(size[0], size[1], 70 + size[0])
    fmt, levels = ctx.compress_texture(img, srgb=False, mips=True)
    count = capi.compressed_texture_layout(size[0], size[1], True)[1]
    assert fmt == S.FORMAT_RGBA8_UNORM and len(levels) == count == (3 if size == (24, 12) else 2)
    assert levels[0] == img.tobytes()
    p = img.astype(np.int64)
    for payload in levels[1:]:
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2      # (even extents here)
        assert payload == p.astype(np.uint8).tobytes()
    if size == (10, 6):                 # (24 x 12 alone is whole blocks)
        assert ctx.compress_texture(img, mips=False) == (S.FORMAT_RGBA8_UNORM, [img.tobytes()])


def test_two_streams_give_the_same_bytes(ctx):
    hip = C.CDLL("libamdhip64.so")
    s1, s2 = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s1), 1) == 0 and hip.hipStreamCreateWithFlags(C.byref(s2), 1) == 0
    try:
        a, b = rand_image(64, 64, 80), rand_image(128, 32, 81)       # (the second call grows the staging)
        want = [ctx.compress_texture(a, srgb=True), ctx.compress_texture(b)]
        for _ in range(2):
            got = [ctx.compress_texture(a, srgb=True, stream=s1.value), ctx.compress_texture(b, stream=s2.value)]
            assert got == want
            s1, s2 = s2, s1
    finally:
        assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
        hip.hipStreamDestroy(s1)
        hip.hipStreamDestroy(s2)


def test_refusals(ctx):
    lib = capi.lib()
    img = rand_image(16, 16, 90)
    out = np.zeros(4096, np.uint8)

    def desc(texels=img, width=16, height=16, fmt=S.FORMAT_RGBA8_UNORM, levels=0):
        d = S.TextureDesc()
        d.texels, d.width, d.height, d.format, d.mipLevelCount = (texels.ctypes.data if texels is not None else None), width, height, fmt, levels
        return d

    def call(d, flags=S.COMPRESS_GENERATE_MIPS, dst=out, nbytes=256 + 64 + 16, handle=ctx._h):
        return lib.prosper_pt_compress_texture(handle, C.byref(d) if d is not None else None, flags, dst.ctypes.data if dst is not None else None, nbytes, None)

    assert call(desc()) == 0                                   # 16 x 16 with mips: 16 + 4 + 1 blocks
    refusals = ((lambda: call(desc(), handle=None), "null"), (lambda: call(None), "null"), (lambda: call(desc(), dst=None), "null"),
                (lambda: call(desc(texels=None)), "null"),
                (lambda: call(desc(width=0)), "empty extent"), (lambda: call(desc(height=0)), "empty extent"),
                (lambda: call(desc(fmt=S.FORMAT_BC7_UNORM)), "RGBA8"),
                (lambda: call(desc(), nbytes=256), "336 bytes"), (lambda: call(desc(), flags=0), "256 bytes"),
                (lambda: call(desc(levels=4), nbytes=256 + 64 + 16 + 16), "exceeds the 3 levels"),
                (lambda: call(desc(), flags=4), "unknown flags"))
    for refused, text in refusals:
        assert refused() == -1
        assert text in lib.prosper_pt_last_error().decode(), text
    # the hook: null pointers, bits outside the three modes; n = 0 does nothing and succeeds
    words = np.zeros(16, np.uint32)
    blocks, sse = np.zeros(4, np.uint32), np.zeros(1, np.uint32)
    hook = lib.prosper_pt_debug_bc7_encode_blocks
    assert hook(ctx._h, None, 0, 0, None, None, None) == 0
    assert hook(ctx._h, None, 1, 0, blocks.ctypes.data, sse.ctypes.data, None) == -1
    assert hook(ctx._h, words.ctypes.data, 1, 0, None, sse.ctypes.data, None) == -1
    assert hook(None, words.ctypes.data, 1, 0, blocks.ctypes.data, sse.ctypes.data, None) == -1
    assert hook(ctx._h, words.ctypes.data, 1, 1 << 3, blocks.ctypes.data, sse.ctypes.data, None) == -1
    assert "modeMask" in lib.prosper_pt_last_error().decode()
    assert hook(ctx._h, words.ctypes.data, 1, 1 << 6, blocks.ctypes.data, sse.ctypes.data, None) == 0


# ---- through the renderer ----

def compressed_wall(ctx, decoded):
    """test_bc7.py's wall of quads, its textures compressed here from random RGBA8 (level 0 of compress_texture);
    `decoded` swaps each for its RGBA8 twin decoded by prosper_amd.bc7."""
    w = World()
    textures = []
    for k, (tw, th) in enumerate([(16, 8), (32, 32), (4, 4), (24, 12)]):
        fmt, levels = ctx.compress_texture(rand_image(tw, th, 100 + k), mips=False)
        assert fmt == S.FORMAT_BC7_UNORM
        if decoded:
            textures.append(w.add_texture(bc7.decode_image(levels[0], tw, th)))
        else:
            textures.append(w.add_texture_bc7(levels[0], tw, th))
    wraps = [S.WRAP_REPEAT, S.WRAP_MIRRORED_REPEAT, S.WRAP_CLAMP_TO_EDGE]
    for k, (flt, wrap) in enumerate([(f, x) for f in (S.FILTER_LINEAR, S.FILTER_NEAREST) for x in wraps]):
        smp = w.add_sampler(flt, flt, wrap, wraps[(k + 1) % 3])
        mat = w.add_material(base_color=(1.0, 1.0, 1.0, 1.0), metallic=0.5, roughness=0.8,
                             base_tex=(textures[k % 4], smp), mr_tex=(textures[(k + 1) % 4], smp),
                             normal_tex=(textures[(k + 2) % 4], smp), alpha_mode=S.ALPHA_MODE_BLEND if k == 2 else S.ALPHA_MODE_OPAQUE)
        cx, cy = (k % 3) - 1.5, (k // 3) - 1.0
        p, n_, t, uv, idx = scenes.quad((cx, cy, 0.0), (cx + 0.95, cy, 0.0), (cx + 0.95, cy + 0.95, 0.0), (cx, cy + 0.95, 0.0))
        uv = uv * (2.3 + 0.4 * k) - (0.7 + 0.3 * k)
        q = scenes._add(w, (p, n_, t, uv, idx), mat)
        w.add_instance(w.add_model([(q, mat)]))
    w.add_point_light((1.0, 1.0, 1.0), 40.0, (0.0, 0.0, 3.0))
    w.camera = dict(eye=(0.0, 0.0, 4.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=math.radians(50.0), zN=0.1, zF=100.0)
    return w


def test_compressed_textures_render_like_their_decoded_twins(ctx, oracle):
    from conftest import default_pc, same_bits
    w, h = 160, 112
    images = []
    for decoded in (False, True):
        world = compressed_wall(ctx, decoded)
        c = world.camera
        cam, fl = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)
        pc = default_pc(S, fl, draw_type=S.DrawType["Albedo"], max_bounces=2)
        render_ctx = capi.Context(0)
        try:
            render_ctx.upload_scene(world)
            render_ctx.render(pc, cam, w, h)
            images.append(render_ctx.read_hdr())
        finally:
            render_ctx.close()
    assert same_bits(images[0], images[1]).all()
    assert len(np.unique(images[0][..., :3].reshape(-1, 3), axis=0)) > 200


# ---- the cache writer over the real context ----

def test_texture_cache_for_a_gltf(ctx, tmp_path):
    from prosper_amd import dds, gltf, texture_cache
    albedo, rough = rand_image(32, 32, 130), rand_image(16, 16, 131)
    write_png(str(tmp_path / "albedo.png"), albedo)
    write_png(str(tmp_path / "rough.png"), rough)
    materials = [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicRoughnessTexture": {"index": 1}}}]
    path = write_gltf(str(tmp_path), ["albedo.png", "rough.png"], materials)
    written = texture_cache.build_for_gltf(path, ctx)
    assert written == [dds.cache_path(str(tmp_path / name)) for name in ("albedo.png", "rough.png")]
    assert all(dds.cache_valid(c, str(tmp_path / name)) for c, name in zip(written, ("albedo.png", "rough.png")))
    # the base colour went through the linear-light chain, the other image through the integer box
    for cached, img, srgb in ((written[0], albedo, True), (written[1], rough, False)):
        fmt, levels = ctx.compress_texture(img, srgb=srgb, mips=True)
        assert dds.read_texture_raw(cached, levels=None) == (dds.DXGI_FORMAT_BC7_UNORM, img.shape[1], img.shape[0], b"".join(levels))
    world = gltf.load_gltf(path)
    assert world.cached_images == written
    assert np.array_equal(world.textures[1], bc7.decode_image(bc7.encode_image(albedo), 32, 32))
    assert texture_cache.build_for_gltf(path, ctx) == []


# ---- the C++ mirror ----

def test_cpp_texture_compressor_through_a_compiled_consumer(ctx, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "the host C++ compiler (g++) is needed"
    exe = str(tmp_path / "texture_compressor_main")
    lib_dir = os.path.join(ROOT, "prosper_amd")
    subprocess.check_call([gxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "texture_compressor_main.cpp"), "-o", exe,
                           "-L" + lib_dir, "-lprosper_pt", "-Wl,-rpath," + lib_dir])
    for (w, h), mips, srgb in (((32, 32), 1, 1), ((24, 12), 1, 0), ((12, 4), 0, 0)):
        img = rand_image(w, h, 120 + w)
        src, out = str(tmp_path / "in.rgba"), str(tmp_path / "out.bin")
        img.tofile(src)
        run = subprocess.run([exe, src, str(w), str(h), str(mips), str(srgb), out], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        blob = open(out, "rb").read()
        fmt, count = np.frombuffer(blob, "<u4", 2)
        offsets = np.frombuffer(blob, "<u4", count, 8).tolist()
        payload = blob[8 + 4 * count:]
        want_fmt, want_levels = ctx.compress_texture(img, srgb=bool(srgb), mips=bool(mips))
        assert (fmt, count) == (want_fmt, len(want_levels))
        assert offsets == np.concatenate([[0], np.cumsum([len(l) for l in want_levels])])[:-1].tolist()
        assert payload == b"".join(want_levels)
