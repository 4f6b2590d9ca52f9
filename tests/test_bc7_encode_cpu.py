"""The BC7 encoder rule as prosper_amd.bc7.encode_blocks states it, held to the format and to a quality
floor by conditions that do not come from the encoder itself: every block decodes through bc7.decode_blocks (pinned
against Pillow in test_bc7.py), exact inputs round-trip exactly, and no block is worse than a baseline written here."""
import base64
import json
import os
import struct
import zlib

import numpy as np
import pytest

from prosper_amd import bc7, capi, dds, gltf, structs as S, texture_cache
from prosper_amd.flight_helmet import load_fixture

MASKS = (0, 1 << 6, 1 << 5, 1 << 4)


def sample_blocks(seed=1, count=192):
    """uint8 [n, 16, 4]: random, solid, two-colour, opaque, ramp and near-constant blocks."""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 256, (count, 16, 4), dtype=np.uint8)]
    out.append(np.repeat(rng.integers(0, 256, (count // 4, 1, 4), dtype=np.uint8), 16, axis=1))
    pair = rng.integers(0, 256, (count // 4, 2, 4), dtype=np.uint8)
    pick = rng.integers(0, 2, (count // 4, 16))
    out.append(np.take_along_axis(pair, pick[:, :, None].repeat(4, axis=2), axis=1))
    opaque = rng.integers(0, 256, (count // 2, 16, 4), dtype=np.uint8)
    opaque[..., 3] = 255
    out.append(opaque)
    a, b = rng.integers(0, 256, (count, 1, 4)), rng.integers(0, 256, (count, 1, 4))
    t = rng.permuted(np.tile(np.arange(16), (count, 1)), axis=1)[:, :, None]
    ramp = (a * (15 - t) + b * t + 7) // 15
    ramp[::3, :, 3] = 255
    out.append(ramp.astype(np.uint8))
    near = rng.integers(0, 256, (count // 4, 1, 4)) + rng.integers(-2, 3, (count // 4, 16, 4))
    out.append(np.clip(near, 0, 255).astype(np.uint8))
    extremes = rng.choice(np.array([0, 1, 254, 255], np.uint8), (count // 4, 16, 4))
    out.append(extremes)
    return np.concatenate(out)


def decoded_sse(blocks, texels):
    return ((bc7.decode_blocks(blocks).astype(np.int64) - texels.astype(np.int64)) ** 2).sum(axis=(1, 2))


def block_mode(blocks):
    first = blocks[:, 0].astype(np.int64)
    assert (first != 0).all()
    return np.log2(first & -first).astype(np.int64)


def pack_bits(fields):
    value, pos = 0, 0
    for v, n in fields:
        assert 0 <= v < (1 << n)
        value |= v << pos
        pos += n
    assert pos == 128
    return np.frombuffer(value.to_bytes(16, "little"), np.uint8)


def helmet_blocks():
    world = load_fixture(sky_size=0)
    images = [np.asarray(t) for t in world.textures[1:] if np.asarray(t).shape[0] >= 4]
    assert len(images) >= 5
    return np.concatenate([bc7.image_blocks(t) for t in images])


# ---- legality ----

@pytest.mark.parametrize("mask", MASKS)
def test_blocks_are_legal_and_the_error_is_the_decoders(mask):
    texels = sample_blocks()
    blocks, sse, mode = bc7.encode_blocks(texels, mask)
    assert blocks.shape == (len(texels), 16) and blocks.dtype == np.uint8
    assert np.array_equal(block_mode(blocks), mode)
    assert np.isin(mode, [4, 5, 6]).all()
    if mask:
        assert (mode == int(np.log2(mask))).all()
    # rotation (bits 5-6 of mode 4, 6-7 of mode 5) is always 0
    assert ((blocks[mode == 4, 0] >> 5) & 3 == 0).all() and ((blocks[mode == 5, 0] >> 6) & 3 == 0).all()
    assert np.array_equal(sse, decoded_sse(blocks, texels))


def test_mask_zero_means_all_three_modes():
    texels = sample_blocks(3, 32)
    assert np.array_equal(bc7.encode_blocks(texels, 0)[0], bc7.encode_blocks(texels, 0x70)[0])


# ---- exact round trips ----

def test_solid_blocks_of_one_parity_round_trip_exactly():
    rng = np.random.default_rng(4)
    colour = rng.integers(0, 128, (200, 1, 4)) * 2 + rng.integers(0, 2, (200, 1, 1))
    texels = np.repeat(colour, 16, axis=1).astype(np.uint8)
    blocks, sse, mode = bc7.encode_blocks(texels)
    assert (sse == 0).all() and (mode == 6).all()
    assert np.array_equal(bc7.decode_blocks(blocks), texels)


def test_two_colour_blocks_of_uniform_parity_round_trip_exactly():
    rng = np.random.default_rng(5)
    pair = rng.integers(0, 128, (300, 2, 4)) * 2 + rng.integers(0, 2, (300, 2, 1))
    pick = rng.integers(0, 2, (300, 16))
    texels = np.take_along_axis(pair, pick[:, :, None].repeat(4, axis=2), axis=1).astype(np.uint8)
    blocks, sse, mode = bc7.encode_blocks(texels)
    assert (sse == 0).all() and (mode == 6).all()
    assert np.array_equal(bc7.decode_blocks(blocks), texels)


def test_hand_packed_blocks():
    # solid (201, 201, 201, 201): 7-bit 100 with p = 1 on both endpoints, every index 0
    solid = np.full((16, 4), 201, np.uint8)
    want_solid = pack_bits([(1 << 6, 7)] + [(100, 7)] * 8 + [(1, 1), (1, 1), (0, 3)] + [(0, 4)] * 15)
    # two colours, even c1 and odd c2, every channel rising from c1 to c2: e0 = c1 (p = 0), e1 = c2 (p = 1)
    c1, c2 = np.array([10, 20, 30, 40]), np.array([201, 101, 51, 255])
    pick = np.array([0, 1, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 0, 1])
    two = np.where(pick[:, None] == 1, c2, c1).astype(np.uint8)
    ends = [(5, 7), (100, 7), (10, 7), (50, 7), (15, 7), (25, 7), (20, 7), (127, 7)]
    want_two = pack_bits([(1 << 6, 7)] + ends + [(0, 1), (1, 1), (0, 3)] + [(15 * int(p), 4) for p in pick[1:]])
    # the same block with the colours exchanged: texel 0 sits on e1, so the endpoints swap and the indices complement
    flipped = np.where(pick[:, None] == 1, c1, c2).astype(np.uint8)
    swapped = [ends[1], ends[0], ends[3], ends[2], ends[5], ends[4], ends[7], ends[6]]
    want_flipped = pack_bits([(1 << 6, 7)] + swapped + [(1, 1), (0, 1), (0, 3)] + [(15 * int(p), 4) for p in pick[1:]])
    blocks, sse, mode = bc7.encode_blocks(np.stack([solid, two, flipped]))
    assert (sse == 0).all() and (mode == 6).all()
    assert np.array_equal(blocks[0], want_solid)
    assert np.array_equal(blocks[1], want_two)
    assert np.array_equal(blocks[2], want_flipped)
    assert np.array_equal(bc7.decode_blocks(blocks), np.stack([solid, two, flipped]))


# ---- opaque blocks ----

@pytest.mark.parametrize("mask", MASKS)
def test_opaque_blocks_stay_opaque(mask):
    rng = np.random.default_rng(6)
    texels = rng.integers(0, 256, (400, 16, 4), dtype=np.uint8)
    texels[200:, :, :3] = (texels[200:, :1, :3].astype(np.int64) + rng.integers(-3, 4, (200, 16, 3))).clip(0, 255)
    texels[..., 3] = 255
    blocks = bc7.encode_blocks(texels, mask)[0]
    assert (bc7.decode_blocks(blocks)[..., 3] == 255).all()


# ---- quality floor ----

_W4 = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], np.int64)


def baseline_sse(texels):
    """Mode 6 with the bounding box's diagonal as endpoints, no refinement: written here on its own, block by block.
    The encoder always tries this candidate and keeps a refinement only where strictly better, so it is never worse."""
    out = np.zeros(len(texels), np.int64)
    for n, block in enumerate(texels.astype(np.int64)):
        lo, hi = block.min(axis=0), block.max(axis=0)
        ref = int(np.argmax(hi - lo))
        e0, e1 = lo.copy(), hi.copy()
        for c in range(4):
            if 16 * int((block[:, ref] * block[:, c]).sum()) - int(block[:, ref].sum()) * int(block[:, c].sum()) < 0:
                e0[c], e1[c] = hi[c], lo[c]
        opaque = bool((block[:, 3] == 255).all())
        ends = []
        for e in (e0, e1):
            choices = []
            for p in (0, 1):
                q = np.array([v if v % 2 == p else (v - 1 if v >= 1 else v + 1) for v in e])
                choices.append((int(((q - e) ** 2).sum()), q))
            ends.append(choices[1][1] if opaque or choices[1][0] < choices[0][0] else choices[0][1])
        palette = ((64 - _W4)[:, None] * ends[0][None, :] + _W4[:, None] * ends[1][None, :] + 32) >> 6       # [16, 4]
        out[n] = int(((block[:, None, :] - palette[None, :, :]) ** 2).sum(axis=2).min(axis=1).sum())
    return out


@pytest.fixture(scope="module")
def gradients():
    y, x = np.mgrid[0:64, 0:64]
    image = np.stack([x * 4, y * 4, (x + y) * 2, 255 - x * 3], axis=2).clip(0, 255).astype(np.uint8)
    return bc7.image_blocks(image)


def test_no_block_is_worse_than_the_baseline(gradients):
    for texels in (sample_blocks(7), gradients, helmet_blocks()[::5]):
        sse = bc7.encode_blocks(texels)[1]
        floor = baseline_sse(texels)
        assert (sse <= floor).all(), np.nonzero(sse > floor)[0][:4]
        assert (sse < floor).any()          # (the refinement and the other modes do buy something)
        assert (bc7.encode_blocks(texels, 1 << 6)[1] <= floor).all()


# ---- mode choice ----

def test_mode_choice():
    x, y = np.meshgrid(np.arange(4), np.arange(4))
    block = np.stack([40 + 50 * x, 200 - 45 * x, 10 + 30 * x, 20 + 70 * y], axis=2).reshape(1, 16, 4).astype(np.uint8)
    blocks, sse, mode = bc7.encode_blocks(block)
    assert mode[0] in (4, 5)
    assert sse[0] < bc7.encode_blocks(block, 1 << 6)[1][0]
    for m in (4, 5, 6):
        assert bc7.encode_blocks(block, 1 << m)[2][0] == m
        assert block_mode(bc7.encode_blocks(block, 1 << m)[0])[0] == m


def test_mode_4_uses_both_index_selections():
    t = np.arange(16)
    fine_colour = np.stack([16 * t, 255 - 16 * t, 8 * t, np.where(t < 8, 0, 255)], axis=1)
    fine_alpha = np.stack([np.where(t < 8, 30, 220), np.where(t < 8, 200, 10), np.where(t < 8, 90, 140), 17 * t], axis=1)
    texels = np.stack([fine_colour, fine_alpha]).astype(np.uint8)
    blocks, sse, mode = bc7.encode_blocks(texels, 1 << 4)
    assert (mode == 4).all()
    selection = (blocks[:, 0] >> 7) & 1
    assert selection[0] == 1 and selection[1] == 0      # the 3-bit indices go where the detail is
    assert np.array_equal(sse, decoded_sse(blocks, texels))


# ---- anchor rule ----

@pytest.mark.parametrize("mask", MASKS)
def test_anchor_swap_decodes_like_the_mirrored_block(mask):
    """A block and the same texels in reverse order have the same endpoints and mirrored indices; when texel 0 of one
    sits near e1 its endpoints are swapped and its indices complemented, and the texels must not move."""
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, 256, (64, 1, 4)), rng.integers(0, 256, (64, 1, 4))
    t = np.arange(16)[None, :, None]
    texels = ((a * (15 - t) + b * t) // 15).astype(np.uint8)       # texel 0 on one end, texel 15 on the other
    forward, sse_f, _ = bc7.encode_blocks(texels, mask)
    backward, sse_b, _ = bc7.encode_blocks(texels[:, ::-1], mask)
    assert np.array_equal(sse_f, sse_b)
    assert np.array_equal(bc7.decode_blocks(forward), bc7.decode_blocks(backward)[:, ::-1])
    assert (forward != backward).any(axis=1).all()                 # (different blocks: one of each pair carries the swap)


# ---- layout ----

def test_compressed_layout():
    lib = capi.lib()
    bc7_cases = {(4, 4): 1, (8, 8): 2, (32, 32): 4, (64, 64): 5}
    for (w, h), levels in bc7_cases.items():
        fmt, count, nbytes = capi.compressed_texture_layout(w, h, True)
        assert (fmt, count) == (S.FORMAT_BC7_UNORM, levels)
        assert nbytes == sum((max(w >> l, 1) // 4) * (max(h >> l, 1) // 4) * 16 for l in range(levels))
        assert count == lib.prosper_pt_texture_mip_level_count(w, h)
    for (w, h), mips in (((64, 16), True), ((48, 48), True), ((24, 12), True), ((10, 6), True), ((10, 6), False)):
        fmt, count, nbytes = capi.compressed_texture_layout(w, h, mips)
        assert fmt == S.FORMAT_RGBA8_UNORM
        assert count == (lib.prosper_pt_texture_mip_level_count(w, h) if mips else 1)
        assert nbytes == sum(max(w >> l, 1) * max(h >> l, 1) * 4 for l in range(count))
    for w, h in ((12, 4), (260, 12)):
        assert capi.compressed_texture_layout(w, h, False) == (S.FORMAT_BC7_UNORM, 1, (w // 4) * (h // 4) * 16)
    # the payload sizes are the DDS writer's
    assert capi.compressed_texture_layout(64, 64, True)[2] == sum(s[2] for s in dds._level_sizes(64, 64, dds.DXGI_FORMAT_BC7_UNORM, 5))
    fmt, count, nbytes = C_args()
    assert lib.prosper_pt_compressed_texture_layout(0, 4, 1, fmt, count, nbytes) == -1
    assert lib.prosper_pt_compressed_texture_layout(4, 4, 1, None, count, nbytes) == -1
    assert lib.prosper_pt_last_error()
    # nothing of the other entries runs without a context
    assert lib.prosper_pt_compress_texture(None, None, 0, None, 0, None) == -1
    assert lib.prosper_pt_debug_bc7_encode_blocks(None, None, 0, 0, None, None, None) == -1


def C_args():
    import ctypes as C
    return C.byref(C.c_uint32()), C.byref(C.c_uint32()), C.byref(C.c_uint64())


# ---- the cache writer ----

class HostCompressor:
    """Stands in for capi.Context.compress_texture: the 2 x 2 integer box and bc7.encode_image on the host."""

    def __init__(self):
        self.calls = []

    def compress_texture(self, rgba, srgb=False, mips=True):
        self.calls.append((rgba.shape, srgb, mips))
        h, w = rgba.shape[:2]
        levels = [rgba]
        for _ in range(1, max(max(w, h).bit_length() - 2, 1) if mips else 1):
            p = levels[-1].astype(np.int64)
            levels.append(((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8))
        if all(l.shape[0] % 4 == 0 and l.shape[1] % 4 == 0 for l in levels):
            return S.FORMAT_BC7_UNORM, [bc7.encode_image(l) for l in levels]
        return S.FORMAT_RGBA8_UNORM, [l.tobytes() for l in levels]


def write_png(path, rgba):
    h, w, _ = rgba.shape
    raw = b"".join(b"\0" + rgba[y].tobytes() for y in range(h))

    def chunk(kind, data):
        body = kind + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def write_gltf(folder, images, materials):
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (3, 1))
    idx = np.array([0, 1, 2], np.uint16)
    blob = pos.tobytes() + idx.tobytes() + b"\0\0" + nrm.tobytes()
    doc = {
        "asset": {"version": "2.0"},
        "buffers": [{"byteLength": len(blob), "uri": "data:application/octet-stream;base64," + base64.b64encode(blob).decode()}],
        "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 36}, {"buffer": 0, "byteOffset": 36, "byteLength": 6},
                        {"buffer": 0, "byteOffset": 44, "byteLength": 36}],
        "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3", "min": [0, 0, 0], "max": [1, 1, 0]},
                      {"bufferView": 1, "componentType": 5123, "count": 3, "type": "SCALAR"},
                      {"bufferView": 2, "componentType": 5126, "count": 3, "type": "VEC3"}],
        "images": [{"uri": name} for name in images],
        "textures": [{"source": i} for i in range(len(images))],
        "materials": materials,
        "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 2}, "indices": 1, "material": 0}]}],
        "nodes": [{"mesh": 0}],
        "scenes": [{"nodes": [0]}],
        "scene": 0,
    }
    path = os.path.join(folder, "scene.gltf")
    with open(path, "w") as f:
        json.dump(doc, f)
    return path


def test_texture_cache_build_writes_what_load_gltf_reads(tmp_path):
    rng = np.random.default_rng(9)
    albedo = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    normal = rng.integers(0, 256, (6, 10, 4), dtype=np.uint8)         # not whole blocks: the RGBA8 fallback
    write_png(str(tmp_path / "albedo.png"), albedo)
    write_png(str(tmp_path / "normal.png"), normal)
    materials = [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}}, "normalTexture": {"index": 1}}]
    path = write_gltf(str(tmp_path), ["albedo.png", "normal.png"], materials)
    assert not gltf.load_gltf(path).cached_images

    host = HostCompressor()
    cached = texture_cache.build(str(tmp_path / "albedo.png"), host, srgb=True)
    assert cached == dds.cache_path(str(tmp_path / "albedo.png")) and os.path.exists(cached)
    assert dds.cache_valid(cached, str(tmp_path / "albedo.png"))
    fmt, w, h, payload = dds.read_texture_raw(cached, levels=None)
    assert (fmt, w, h, dds.level_count(cached)) == (dds.DXGI_FORMAT_BC7_UNORM, 16, 16, 3)
    assert payload[:256] == bc7.encode_image(albedo)

    # the rest through the glTF: only what is missing or stale, base colour as sRGB and the normal map as linear
    host.calls.clear()
    written = texture_cache.build_for_gltf(path, host)
    assert written == [dds.cache_path(str(tmp_path / "normal.png"))]
    assert host.calls == [((6, 10, 4), False, True)]
    assert dds.read_texture_raw(written[0])[0] == dds.DXGI_FORMAT_R8G8B8A8_UNORM
    assert texture_cache.build_for_gltf(path, host) == []
    world = gltf.load_gltf(path)
    assert world.cached_images == [cached, written[0]] and not world.stale_cached_images
    assert np.array_equal(world.textures[1], bc7.decode_image(bc7.encode_image(albedo), 16, 16))
    assert np.array_equal(world.textures[2], normal)
    # a touched source is stale and gets compressed again, this time as what the materials say it is
    st = os.stat(tmp_path / "albedo.png")
    os.utime(tmp_path / "albedo.png", ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))
    host.calls.clear()
    assert texture_cache.build_for_gltf(path, host) == [cached]
    assert host.calls == [((16, 16, 4), True, True)] and dds.cache_valid(cached, str(tmp_path / "albedo.png"))
