"""The registry of the context's images and the one-texel readback on the GPU (prosper_pt_get_debug_resource,
prosper_pt_texture_readback): after one frame of the quad-and-sky scene of test_debug_lines.py at 48 x 32
through the traced velocity G-buffer, deferred shading, sky, bloom, TAA and depth of field, every entry agrees with the
existing read-back call for its image, and a read-back texel equals that image's texel bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import debug_view_reference as R
from debug_view_scene import H, NAMES, QUAD_DISTANCE, W, by_name, camera, frame, quad_world, read_back
from conftest import same_bits
from prosper_amd import capi, debug_geometry as G, structs as S

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def setup(gpu_ctx, oracle):
    gpu_ctx.upload_scene(quad_world())
    gpu_ctx.generate_ibl()
    cam = camera(oracle)
    frame(gpu_ctx, cam)
    return gpu_ctx, cam


def test_a_fresh_context_lists_every_image_and_none_is_valid():
    ctx = capi.Context(device=0)
    try:
        res = ctx.debug_resources()
        assert [r.name.decode() for r in res] == NAMES
        assert all(r.valid == 0 and r.width == 0 and r.height == 0 and r.levelCount == 0 for r in res)
        lib = capi.lib()
        assert lib.prosper_pt_texture_readback(ctx._h, 3, 1.0, 1.0, None) == -4  # NO_SCENE: its pass has not run
        assert b"not valid" in lib.prosper_pt_last_error()
        assert lib.prosper_pt_texture_readback(ctx._h, len(NAMES), 1.0, 1.0, None) == -1
        assert lib.prosper_pt_get_debug_resource(ctx._h, len(NAMES), C.byref(S.DebugResource())) == -1
        assert ctx.try_texture_readback() is None
    finally:
        ctx.close()


def test_every_entry_agrees_with_the_read_back_call_for_its_image(setup):
    ctx, _ = setup
    res = by_name(ctx)
    assert list(res) == NAMES
    fft = set(NAMES[17:21])
    formats = {"BloomKernelImageCentered": S.DEBUG_FORMAT_RGBA32F, "BloomKernelDft": S.DEBUG_FORMAT_RGBA32F,
               "BloomFftConvolved": S.DEBUG_FORMAT_RGBA32F, "illumination": S.DEBUG_FORMAT_RGBA32F, "albedoRoughness": S.DEBUG_FORMAT_RGBA32F, "normalMetalness": S.DEBUG_FORMAT_RGBA32F,
               "depth": S.DEBUG_FORMAT_R32F, "velocity": S.DEBUG_FORMAT_RG32F, "SpecularBrdfLut": S.DEBUG_FORMAT_RG16_UNORM,
               "HalfResCircleOfConfusion": S.DEBUG_FORMAT_R16F, "tileMinMaxCircleOfConfusion": S.DEBUG_FORMAT_RG16F,
               "dilatedTileMinMaxCoC": S.DEBUG_FORMAT_RG16F}
    for name, (_, r) in res.items():
        if name == "toneMapped":
            continue  # (its own test below)
        if name in fft:
            # the FFT technique is not part of this frame: its entries are valid if and only if it has run on this context
            assert r.valid == ctx.bloom_fft_info().valid, name
            if not r.valid:
                continue
        assert r.valid == 1, name
        assert r.format == formats.get(name, S.DEBUG_FORMAT_RGBA16F), name
        for level in range(r.levelCount):
            image = read_back(ctx, name, level)
            w, h = max(r.width >> level, 1), max(r.height >> level, 1)
            assert image.shape[:2] == (h, w), (name, level)
            assert image.nbytes == w * h * R.FORMAT_BYTES[r.format], (name, level)
    assert (res["illumination"][1].width, res["illumination"][1].height) == (W, H)
    dof, bloom = ctx.dof_info(), ctx.bloom_info()
    assert res["HalfResIllumination"][1].levelCount == dof.mips > 1
    assert (res["tileMinMaxCircleOfConfusion"][1].width, res["tileMinMaxCircleOfConfusion"][1].height) == (dof.tileWidth, dof.tileHeight)
    assert res["BloomWorkingImage"][1].levelCount == 4 and res["BloomBlurPong"][1].levelCount == 3 == res["BloomBlurred"][1].levelCount
    assert (res["BloomWorkingImage"][1].width, res["BloomWorkingImage"][1].height) == (bloom.workingWidth, bloom.workingHeight)
    assert res["SpecularBrdfLut"][1].width == S.IBL_LUT_SIZE


PIXELS = ((0.0, 0.0), (17.0, 9.0), (17.75, 9.25), (W - 1.0, H - 1.0), (float(W), float(H)), (W + 100.0, 3.0), (-0.25, 5.0),
          (-7.0, -3.5), (1e30, -1e30))


def read_texel(ctx, resource, px, py):
    ctx.texture_readback(resource, px, py)
    ctx.read_hdr()  # (synchronises the stream)
    got = ctx.try_texture_readback()
    assert got is not None and got.dtype == F and got.shape == (4,)
    assert ctx.try_texture_readback() is None  # handed out once
    return got


def test_the_depth_texel_is_the_read_back_depth_at_the_clamped_texel(setup):
    ctx, _ = setup
    depth = ctx.read_gbuffer()[2]
    assert (depth > 0).any() and (depth == 0).any()
    for px, py in PIXELS:
        got = read_texel(ctx, "depth", px, py)
        x, y = min(max(math.floor(px), 0), W - 1), min(max(math.floor(py), 0), H - 1)
        assert (R.nearest_texel(px, W), R.nearest_texel(py, H)) == (x, y), (px, py)
        assert same_bits(got, np.array([depth[y, x], 0.0, 0.0, 1.0], F)).all(), (px, py)


@pytest.mark.parametrize("name", ("illumination", "velocity", "SpecularBrdfLut", "HalfResIllumination",
                                  "HalfResCircleOfConfusion", "dilatedTileMinMaxCoC", "previousResolvedIllumination"))
def test_a_texel_of_every_format_equals_the_restatement_over_the_read_back_image(setup, name):
    ctx, _ = setup
    index, r = by_name(ctx)[name]
    image = read_back(ctx, name)
    for fx, fy in ((0.0, 0.0), (0.37, 0.61), (0.999, 0.999), (1.0, 1.0), (-0.1, 0.5)):
        px, py = fx * r.width, fy * r.height
        got = read_texel(ctx, index, px, py)
        assert same_bits(got, R.texture_readback(image, F(px), F(py))).all(), (name, px, py)


def test_try_never_blocks_and_a_second_record_is_refused(setup):
    ctx, _ = setup
    assert ctx.try_texture_readback() is None  # nothing queued
    ctx.texture_readback("depth", 3.0, 4.0)
    with pytest.raises(Exception, match="queued and unread"):
        ctx.texture_readback("depth", 5.0, 6.0)
    ctx.read_hdr()
    got = ctx.try_texture_readback()
    assert got is not None and same_bits(got[0], ctx.read_gbuffer()[2][4, 3]).all()
    assert ctx.try_texture_readback() is None
    with pytest.raises(Exception, match="non-finite"):
        ctx.texture_readback("depth", float("nan"), 0.0)
    ctx.texture_readback("depth", 5.0, 6.0)  # the slot is free again
    ctx.read_hdr()
    assert ctx.try_texture_readback() is not None


def test_an_entry_goes_stale_when_what_it_described_is_gone(setup):
    ctx, cam = setup
    index, r = by_name(ctx)["previousResolvedIllumination"]
    assert r.valid == 1
    ctx.taa_release_history()
    assert by_name(ctx)["previousResolvedIllumination"][1].valid == 0
    with pytest.raises(Exception, match="not valid"):
        ctx.texture_readback(index, 1.0, 1.0)
    ctx.taa_resolve(S.TaaPC.default(reset_history=1), W, H)
    assert by_name(ctx)["previousResolvedIllumination"][1].valid == 1
    # a new scene: the LUT describes the old sky until it is generated again
    ctx.upload_scene(quad_world())
    assert by_name(ctx)["SpecularBrdfLut"][1].valid == 0 and by_name(ctx)["previousResolvedIllumination"][1].valid == 0
    ctx.generate_ibl()
    frame(ctx, cam)
    assert by_name(ctx)["SpecularBrdfLut"][1].valid == 1


def test_the_cpp_texture_readback_counts_frames_as_the_reference_does(setup):
    ctx, _ = setup
    lib = capi.lib()
    h = C.c_void_p()
    assert lib.prosper_host_texture_readback_create(ctx._h, C.byref(h)) == 0
    try:
        out, ready = (C.c_float * 4)(), C.c_uint32()
        frames = lambda: lib.prosper_host_texture_readback_frames_until_ready(h)
        depth_index = ctx.debug_resource_index("depth")
        assert frames() == -1
        assert lib.prosper_host_texture_readback_readback(h, C.byref(out), C.byref(ready)) == -1  # "No readback in flight"
        assert b"No readback in flight" in lib.prosper_host_last_error()
        assert lib.prosper_host_texture_readback_start_frame(h) == 0  # nothing queued: nothing to count
        assert lib.prosper_host_texture_readback_record(h, depth_index, 7.0, 8.0, None) == 0 and frames() == 2
        assert lib.prosper_host_texture_readback_record(h, depth_index, 7.0, 8.0, None) == -1
        assert b"already queued and unread" in lib.prosper_host_last_error()
        ctx.read_hdr()  # the copy has finished - the frames have not
        for left in (1, 0):
            assert lib.prosper_host_texture_readback_readback(h, C.byref(out), C.byref(ready)) == 0 and ready.value == 0
            assert lib.prosper_host_texture_readback_start_frame(h) == 0 and frames() == left
        assert lib.prosper_host_texture_readback_start_frame(h) == -1  # at 0 and nobody asked
        assert b"Forgot to call readback" in lib.prosper_host_last_error()
        assert lib.prosper_host_texture_readback_readback(h, C.byref(out), C.byref(ready)) == 0 and ready.value == 1
        assert frames() == -1
        assert same_bits(np.array(out[:], F), np.array([ctx.read_gbuffer()[2][8, 7], 0.0, 0.0, 1.0], F)).all()
        assert lib.prosper_host_texture_readback_record(h, depth_index, 1.0, 1.0, None) == 0  # free again
        ctx.read_hdr()
        for _ in range(2):
            assert lib.prosper_host_texture_readback_start_frame(h) == 0
        assert lib.prosper_host_texture_readback_readback(h, C.byref(out), C.byref(ready)) == 0 and ready.value == 1
    finally:
        lib.prosper_host_texture_readback_destroy(h)


def test_click_to_focus_on_the_quad_gives_its_distance(setup):
    """--focus-at: the read-back depth texel through focus_distance_from_depth; 1e-5 relative against the float64
    restatement over the same texel (about ten float32 operations at 6e-8 each, tenfold margin)."""
    ctx, cam = setup
    for px, py in ((3.0, 4.0), (20.5, 16.25), (34.0, 31.0)):
        texel = read_texel(ctx, "depth", px, py)
        assert texel[0] > 0 and tuple(texel[1:]) == (0.0, 0.0, 1.0)
        d32 = G.focus_distance_from_depth(cam, (px, py), (W, H), texel[0])
        d64 = G.focus_distance_from_depth(cam, (px, py), (W, H), texel[0], dtype=np.float64)
        assert abs(float(d32) - d64) <= 1e-5 * d64
        assert abs(float(d32) - QUAD_DISTANCE) <= 1e-5 * QUAD_DISTANCE


def test_targets_in_a_callers_buffers_are_not_vouched_for(setup):
    """a G-buffer and a velocity traced into the caller's buffers: the context cannot say how long they live"""
    ctx, cam = setup
    hip = C.CDLL("libamdhip64.so")
    ptrs = []
    try:
        for nbytes in (W * H * 16, W * H * 16, W * H * 4, W * H * 8):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
            ptrs.append(p)
        ctx.trace_gbuffer_velocity(cam, W, H, targets=tuple(p.value for p in ptrs[:3]), velocity_ptr=ptrs[3].value)
        ctx.read_hdr()
        res = by_name(ctx)
        for name in ("albedoRoughness", "normalMetalness", "depth", "velocity"):
            assert res[name][1].valid == 0 and res[name][1].width == 0, name
        with pytest.raises(Exception, match="not valid"):
            ctx.texture_readback("depth", 1.0, 1.0)
        assert res["illumination"][1].valid == 1  # the others are untouched
    finally:
        frame(ctx, cam)  # back to the context's own targets before the buffers go
        ctx.read_hdr()
        for p in ptrs:
            hip.hipFree(p)
    res = by_name(ctx)
    assert all(res[name][1].valid == 1 for name in ("albedoRoughness", "normalMetalness", "depth", "velocity"))


def test_the_tone_mapped_image_is_listed_only_while_the_context_keeps_it(setup):
    from prosper_amd import dds
    ctx, _ = setup
    g = np.linspace(0.0, 1.0, 8)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    ctx.set_tone_map_lut(dds.encode_r9g9b9e5(np.stack([r, gg, b], axis=-1)))
    kept = ctx.tone_map(1.0, 1.0)  # a host copy alone: the image stays in the context
    index, entry = by_name(ctx)["toneMapped"]
    assert entry.valid == 1 and (entry.width, entry.height, entry.levelCount, entry.format) == (W, H, 1, S.DEBUG_FORMAT_RGBA8_UNORM)
    assert kept.nbytes == W * H * R.FORMAT_BYTES[entry.format]
    for px, py in ((0.0, 0.0), (20.5, 11.0), (float(W), float(H))):
        got = read_texel(ctx, index, px, py)
        assert same_bits(got, R.texture_readback(kept, F(px), F(py))).all(), (px, py)
    hip = C.CDLL("libamdhip64.so")
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(W * H * 4)) == 0
    try:
        ctx.tone_map(1.0, 1.0, device_ptr=p.value, to_host=False)  # into the caller's buffer: nothing is kept
        ctx.read_hdr()
        assert by_name(ctx)["toneMapped"][1].valid == 0
    finally:
        hip.hipFree(p)
