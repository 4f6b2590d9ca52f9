"""The texture viewer on the GPU (prosper_pt_texture_debug; pt_debug_view.hip): after one frame of the
quad-and-sky scene at 48 x 32 (traced velocity G-buffer, deferred shading, sky, bloom, TAA, depth of field, and a tone
map kept by the context), one entry of every stored format is viewed through a curated list of settings and compared
bit for bit with tests/debug_view_reference.py applied to the GPU's own read-back of that entry."""
import ctypes as C

import numpy as np
import pytest

import debug_view_reference as R
from debug_view_scene import H, W, by_name, camera, frame, quad_world, read_back
from prosper_amd import capi, dds, structs as S

pytestmark = pytest.mark.gpu

F = np.float32
RGB, ABS, ZOOM, MAG = S.TEXTURE_DEBUG_CHANNEL_RGB, S.TEXTURE_DEBUG_ABS_BEFORE_RANGE, S.TEXTURE_DEBUG_ZOOM, S.TEXTURE_DEBUG_MAGNIFIER
OUT_EXTENTS = ((W, H), (37, 23), (23, 37))
# one entry per stored format
ENTRIES = {"RGBA32F": "illumination", "RG32F": "velocity", "R32F": "depth", "RGBA16F": "HalfResIllumination",
           "RG16F": "dilatedTileMinMaxCoC", "R16F": "HalfResCircleOfConfusion", "RG16_UNORM": "SpecularBrdfLut",
           "RGBA8_UNORM": "toneMapped"}


@pytest.fixture(scope="module")
def setup(gpu_ctx, oracle):
    gpu_ctx.upload_scene(quad_world())
    gpu_ctx.generate_ibl()
    cam = camera(oracle)
    # the camera came from up and to the left: the velocity target holds both signs
    cam.previousWorldToCamera.col[3].x += 0.05
    cam.previousWorldToCamera.col[3].y -= 0.03
    frame(gpu_ctx, cam)
    g = np.linspace(0.0, 1.0, 8)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    gpu_ctx.set_tone_map_lut(dds.encode_r9g9b9e5(np.stack([r, gg, b], axis=-1)))
    kept = gpu_ctx.tone_map(1.0, 1.0)  # a host copy alone: the context keeps the image
    return gpu_ctx, cam, kept


def image_of(ctx, name, kept, level=0):
    return kept if name == "toneMapped" else read_back(ctx, name, level)


def combinations(last_level):
    """(out extent, range, lod, flags, bilinear): at most 40 per format"""
    combos = []
    for out in OUT_EXTENTS:
        for bilinear in (False, True):
            combos.append((out, (0.0, 1.0), 0, RGB, bilinear))
            combos.append((out, (-2.0, 3.0), 0, RGB | ZOOM, bilinear))
    for channel in range(4):
        combos.append(((37, 23), (0.0, 1.0), 0, channel, channel % 2 == 1))
    for rng in ((1.0, 0.0), (0.5, 0.5), (-2.0, 3.0)):
        combos.append(((W, H), rng, 0, RGB, False))
        combos.append(((23, 37), rng, 0, RGB | ABS, True))
    combos.append(((W, H), (0.0, 1.0), 0, 0 | ABS | ZOOM, True))
    if last_level:
        for out in OUT_EXTENTS:
            combos.append((out, (0.0, 1.0), last_level, RGB, out[0] == 37))
        combos.append(((37, 23), (0.0, 0.25), last_level // 2, 1 | ZOOM, True))
    assert len(combos) <= 40
    return combos


@pytest.mark.parametrize("fmt", list(ENTRIES))
def test_the_view_of_one_entry_per_format_equals_the_restatement_bit_for_bit(setup, fmt):
    ctx, _, kept = setup
    name = ENTRIES[fmt]
    index, r = by_name(ctx)[name]
    assert r.valid == 1 and r.format == list(ENTRIES).index(fmt), name
    levels = {}
    for out, rng, lod, flags, bilinear in combinations(r.levelCount - 1):
        if lod not in levels:
            levels[lod] = image_of(ctx, name, kept, lod)
        got = ctx.texture_debug(index, out, rng, lod, flags, bilinear=bilinear)
        want, _ = R.texture_debug(levels[lod], out, rng, flags, bilinear=bilinear)
        assert got.shape == want.shape == (out[1], out[0], 4)
        bad = (got != want).any(2)
        assert not bad.any(), "%s %s: %d texels differ, first at %s: %s against %s" % (
            name, (out, rng, lod, flags, bilinear), bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])
        assert (got[..., 3] == 255).all()


def test_abs_matters_on_velocity_and_the_zero_span_range_saturates(setup):
    ctx, _, _ = setup
    velocity = read_back(ctx, "velocity")
    assert (velocity < 0).any() and (velocity > 0).any()  # the design: the camera moved
    channel = 0 if (velocity[..., 0] < 0).any() else 1
    negative = velocity[..., channel] < 0
    span = float(np.abs(velocity[..., channel]).max())
    plain = ctx.texture_debug("velocity", (W, H), (0.0, span), 0, channel)
    absolute = ctx.texture_debug("velocity", (W, H), (0.0, span), 0, channel | ABS)
    assert (plain[negative][:, :3] == 0).all() and (absolute[negative][:, :3] > 0).any()
    flat = ctx.texture_debug("depth", (W, H), (0.5, 0.5), 0, 0)  # (c - 0.5) / 0: +inf, -inf or NaN
    assert set(np.unique(flat[..., 0]).tolist()) <= {0, 255}


def test_no_output_texel_is_left_out_and_two_calls_are_identical(setup):
    ctx, _, _ = setup
    hip = C.CDLL("libamdhip64.so")
    for out in OUT_EXTENTS:
        n = out[0] * out[1] * 4
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), C.c_size_t(n + 64)) == 0
        try:
            results = []
            for fill in (0x00, 0x5A):  # whatever the buffer held, every texel is written (alpha 255) and nothing past the end
                assert hip.hipMemset(ptr, fill, C.c_size_t(n + 64)) == 0
                ctx.texture_debug("illumination", out, (0.0, 1.0), 0, RGB | MAG, cursor_uv=(0.4, 0.6), bilinear=True,
                                  device_ptr=ptr.value, to_host=False)
                ctx.read_hdr()  # (synchronises)
                raw = np.empty(n + 64, np.uint8)
                assert hip.hipMemcpy(C.c_void_p(raw.ctypes.data), ptr, C.c_size_t(n + 64), 2) == 0
                assert (raw[n:] == fill).all()
                results.append(raw[:n].reshape(out[1], out[0], 4))
            assert (results[0][..., 3] == 255).all() and results[0].tobytes() == results[1].tobytes()
            host = ctx.texture_debug("illumination", out, (0.0, 1.0), 0, RGB | MAG, cursor_uv=(0.4, 0.6), bilinear=True)
            assert host.tobytes() == results[0].tobytes()
        finally:
            hip.hipFree(ptr)


@pytest.mark.parametrize("zoom", (0, ZOOM))
@pytest.mark.parametrize("out", OUT_EXTENTS)
def test_the_magnifier_peeks_the_snapped_texel_and_marks_it(setup, out, zoom):
    ctx, _, _ = setup
    image = read_back(ctx, "illumination")
    # a corner, the centre, a texel boundary, and cursors whose snapped uv lies outside [0, 1): past the end, and - with
    # another aspect - in the bars beside the image
    for cursor in ((0.0, 0.0), (0.5, 0.5), (0.25, 0.75), (0.999, 0.999), (1.0, 1.0), (1.0, 0.5), (0.01, 0.5), (0.5, 0.01), (-0.2, 0.3)):
        got = ctx.texture_debug("illumination", out, (0.0, 1.0), 0, RGB | MAG | zoom, cursor_uv=cursor)
        peek = ctx.texture_debug_peek()
        want, want_peek = R.texture_debug(image, out, (0.0, 1.0), RGB | MAG | zoom, cursor_uv=cursor)
        assert peek.view(np.uint32).tolist() == want_peek.view(np.uint32).tolist(), (cursor, peek, want_peek)
        assert (got == want).all(), cursor
        su, sv = R.snapped_cursor(cursor, (W, H), out, bool(zoom))
        if not (0 <= su < 1 and 0 <= sv < 1):
            assert np.isposinf(peek).all(), cursor
    # the marker: a white square of 2 inside a black one of 3 around the centre's texel
    got = ctx.texture_debug("illumination", (W, H), (0.0, 1.0), 0, RGB | MAG, cursor_uv=(0.5, 0.5))
    plain = ctx.texture_debug("illumination", (W, H), (0.0, 1.0), 0, RGB)
    changed = (got != plain).any(2)
    ys, xs = np.nonzero(changed)
    assert 22 <= xs.min() and xs.max() <= 27 and 14 <= ys.min() and ys.max() <= 19
    assert (got[16, 24, :3] == 255).all() and (got[14, 22, :3] == 0).all()


def test_refusals(setup, oracle):
    ctx, cam, _ = setup
    lib = capi.lib()
    res = by_name(ctx)
    index, r = res["HalfResIllumination"]

    def call(resource, in_res, out_res, lod=0, flags=RGB, bilinear=0):
        pc = S.TextureDebugPC((C.c_int32 * 2)(*in_res), (C.c_int32 * 2)(*out_res), (C.c_float * 2)(0.0, 1.0), lod, flags, (C.c_float * 2)(0.0, 0.0))
        out = np.empty((max(out_res[1], 1), max(out_res[0], 1), 4), np.uint8)
        return lib.prosper_pt_texture_debug(ctx._h, resource, C.byref(pc), bilinear, None, out.ctypes.data, out.nbytes, None)

    ok = (r.width, r.height)
    assert call(index, ok, (8, 8), lod=r.levelCount - 1) == 0
    assert call(index, ok, (8, 8), lod=r.levelCount) == -1 and b"lod" in lib.prosper_pt_last_error()
    assert call(res["depth"][0], (W, H), (8, 8), lod=1) == -1
    assert call(len(res), ok, (8, 8)) == -1 and b"no such resource" in lib.prosper_pt_last_error()
    assert call(index, (r.width + 1, r.height), (8, 8)) == -1 and b"inRes" in lib.prosper_pt_last_error()
    assert call(index, ok, (0, 8)) == -1 and call(index, ok, (8, 40000)) == -1
    assert call(index, ok, (8, 8), flags=64) == -1 and call(index, ok, (8, 8), bilinear=2) == -1
    # an entry whose pass has not run: the FFT technique's on a fresh context, and everything before any pass
    fresh = capi.Context(device=0)
    try:
        with pytest.raises(Exception, match="not valid"):
            fresh.texture_debug("depth", (8, 8))
        with pytest.raises(capi.ProsperPtError) as e:
            fresh.texture_debug_peek()
        assert e.value.code == -4  # NO_SCENE before any magnifier call
    finally:
        fresh.close()
    # a stale entry: the history after it was released
    taa = res["previousResolvedIllumination"][0]
    ctx.texture_debug(taa, (8, 8))
    ctx.taa_release_history()
    with pytest.raises(Exception, match="not valid"):
        ctx.texture_debug(taa, (8, 8))
    frame(ctx, cam)
    ctx.texture_debug(taa, (8, 8))


def test_the_cpp_texture_debug_keeps_settings_per_name_and_views_what_the_direct_call_views(setup):
    ctx, _, _ = setup
    lib = capi.lib()
    h = C.c_void_p()
    assert lib.prosper_host_texture_debug_create(ctx._h, C.byref(h)) == 0
    try:
        out = np.zeros((23, 37, 4), np.uint8)
        pc = S.TextureDebugPC()

        def record(cursor=None):
            c = None if cursor is None else (C.c_float * 2)(*cursor)
            return lib.prosper_host_texture_debug_record(h, 37, 23, c, None, out.ctypes.data, out.nbytes, None, C.byref(pc))

        assert lib.prosper_host_texture_debug_texture_selected(h) == 0
        assert record() == -1 and b"no texture is selected" in lib.prosper_host_last_error()
        lib.prosper_host_texture_debug_set_target(h, b"noSuchImage")
        assert lib.prosper_host_texture_debug_texture_selected(h) == 1 and record() == -3
        # the defaults of a name seen for the first time: range (0, 1), lod 0, RGB, nearest
        lib.prosper_host_texture_debug_set_target(h, b"illumination")
        assert record() == 0 and (pc.range[0], pc.range[1], pc.lod, pc.flags) == (0.0, 1.0, 0, RGB)
        assert out.tobytes() == ctx.texture_debug("illumination", (37, 23)).tobytes()
        # settings stay with their name; the LOD is clamped to the image's last level
        lib.prosper_host_texture_debug_set_settings(h, b"HalfResIllumination", -2.0, 3.0, 99, 1, 1, 1)
        lib.prosper_host_texture_debug_set_target(h, b"HalfResIllumination")
        lib.prosper_host_texture_debug_set_zoom(h, 1)
        last = by_name(ctx)["HalfResIllumination"][1].levelCount - 1
        assert record((0.4, 0.6)) == 0 and pc.lod == last and pc.flags == 1 | ABS | ZOOM | MAG
        assert (pc.inRes[0], pc.inRes[1], pc.outRes[0], pc.outRes[1]) == (W // 2, H // 2, 37, 23)
        want = ctx.texture_debug("HalfResIllumination", (37, 23), (-2.0, 3.0), last, 1 | ABS | ZOOM | MAG, (0.4, 0.6), bilinear=True)
        assert out.tobytes() == want.tobytes()
        peek = (C.c_float * 4)()
        assert lib.prosper_host_texture_debug_peeked_value(h, C.byref(peek)) == 0
        assert np.array(peek[:], F).view(np.uint32).tolist() == ctx.texture_debug_peek().view(np.uint32).tolist()
        lib.prosper_host_texture_debug_set_zoom(h, 0)
        lib.prosper_host_texture_debug_set_target(h, b"illumination")
        assert record() == 0 and (pc.range[0], pc.lod, pc.flags) == (0.0, 0, RGB)  # its own settings, untouched
        lib.prosper_host_texture_debug_set_target(h, b"")
        assert lib.prosper_host_texture_debug_texture_selected(h) == 0
    finally:
        lib.prosper_host_texture_debug_destroy(h)
