"""Temporal anti-aliasing without a GPU: the jitter, the host camera's jitter and previous-frame state, the struct sizes,
the refusals that need no context, the numpy restatement's known answers and what the test design
(tests/taa_reference.py) reaches of the pass.  The GPU side: tests/test_taa.py."""
import ctypes as C

import numpy as np
import pytest

import taa_reference as R
from prosper_amd import capi, structs as S
from test_bloom_cpu import header_struct_size

NEW_SYMBOLS = ("prosper_pt_taa_resolve", "prosper_pt_taa_release_history", "prosper_pt_read_taa_history", "prosper_pt_get_taa_info",
               "prosper_pt_taa_jitter", "prosper_host_camera_set_jitter", "prosper_host_taa_create", "prosper_host_taa_destroy",
               "prosper_host_taa_draw_ui", "prosper_host_taa_record", "prosper_host_taa_release_preserved")
# the smallest extents at which each rule can go wrong (see tests/test_taa.py)
EXTENTS = ((1, 1), (3, 2), (17, 9), (101, 71), (130, 33), (33, 130))
ALL_VARIANT_EXTENTS = ((17, 9), (101, 71))
FRAMES = 3
# what every extent from 17 x 9 up must hold in each of the frames that read a history
KINDS = ("zero", "sub_pixel", "whole_pixels", "lands_on_edge", "step_outside", "plus_minus_one", "largest_ties", "closest_ties",
         "all_zero_depths", "history_above", "history_below", "flat", "resolved", "fallback")


def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4


def test_struct_sizes_equal_the_headers():
    assert C.sizeof(S.TaaPC) == header_struct_size("prosper_pt_taa_pc") == 20
    assert C.sizeof(S.TaaInfo) == header_struct_size("prosper_pt_taa_info") == 28
    assert C.sizeof(S.TaaInputs) == 32
    pc = S.TaaPC.default()
    assert (pc.catmullRom, pc.colorClipping, pc.velocitySampling, pc.luminanceWeighting, pc.resetHistory) == (1, 2, 2, 1, 0)
    assert (pc.catmullRom, pc.colorClipping, pc.velocitySampling, pc.luminanceWeighting) == R.DEFAULT


def radical_inverse(i, base):
    """Halton's sequence from its definition: the digits of i in `base`, mirrored about the point."""
    value, scale = 0.0, 1.0 / base
    while i:
        value += (i % base) * scale
        i //= base
        scale /= base
    return value


def test_the_jitter_is_the_halton_2_3_cycle():
    table = R.halton23()
    assert table.shape == (8, 2)
    for i in range(8):
        assert table[i, 0] == np.float32(radical_inverse(i + 1, 2)) and table[i, 1] == np.float32(radical_inverse(i + 1, 3))
    for w, h in ((1920, 1080), (101, 71), (1, 1)):
        for i in range(20):
            s = np.array([radical_inverse(i % 8 + 1, 2), radical_inverse(i % 8 + 1, 3)], np.float32)
            want = (s * np.float32(2) - np.float32(1)) / np.array([w, h], np.float32)
            got = capi.taa_jitter(i, w, h)
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes() == R.jitter(i, w, h).tobytes(), (w, h, i)
    # the cycle is centred: every sample within half a pixel (2 / res in NDC is one pixel)
    assert (np.abs(np.array([capi.taa_jitter(i, 100, 50) for i in range(8)])) < np.array([0.01, 0.02])).all()


def mat(m):
    """A prosper_mat4 (column-major) as float64 [4, 4]."""
    return np.array([[m.col[c].x, m.col[c].y, m.col[c].z, m.col[c].w] for c in range(4)], np.float64).T


def make_camera(w=160, h=96):
    from prosper_amd.rt_reference import Camera
    cam = Camera()
    cam.look_at((0.3, 1.0, 3.4), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0))
    cam.set_parameters(np.radians(40.0), 0.1, 100.0, 0.00001, 1.0)
    cam.update_resolution(w, h)
    return cam


def test_a_camera_that_never_jitters_is_unchanged():
    plain, off = make_camera(), make_camera()
    off.set_jitter(False)
    u, _ = plain.update_buffer()
    first = bytes(u)
    assert bytes(off.update_buffer()[0]) == first
    assert bytes(u.previousWorldToCamera) == bytes(u.worldToCamera) and bytes(u.previousCameraToClip) == bytes(u.cameraToClip)
    assert list(u.currentJitter) == [0.0, 0.0] and list(u.previousJitter) == [0.0, 0.0]
    assert bytes(C.c_float(u.cameraToClip.col[2].x)) == bytes(C.c_float(0.0)) == bytes(C.c_float(u.cameraToClip.col[2].y))
    # frames of a still camera: the previous matrices are the same ones
    for _ in range(3):
        plain.end_frame()
        assert bytes(plain.update_buffer()[0]) == first
    plain.close()
    off.close()


def test_end_frame_hands_the_matrices_and_the_jitter_to_the_previous_fields():
    w, h = 160, 96
    cam = make_camera(w, h)
    cam.set_jitter(True)
    u0 = S.CameraUniforms.from_buffer_copy(bytes(cam.update_buffer()[0]))
    assert np.array(u0.currentJitter[:], np.float32).tobytes() == capi.taa_jitter(0, w, h).tobytes()
    # until the first end_frame the previous matrices are the current ones
    assert bytes(u0.previousCameraToClip) == bytes(u0.cameraToClip) and bytes(u0.previousWorldToCamera) == bytes(u0.worldToCamera)
    assert list(u0.previousJitter) == [0.0, 0.0]
    cam.end_frame()
    cam.look_at((0.5, 1.1, 3.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0))
    u1 = S.CameraUniforms.from_buffer_copy(bytes(cam.update_buffer()[0]))
    cam.end_frame()
    cam.look_at((0.7, 1.2, 2.8), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0))
    u2 = S.CameraUniforms.from_buffer_copy(bytes(cam.update_buffer()[0]))
    for before, after, index in ((u0, u1, 1), (u1, u2, 2)):
        assert bytes(after.previousWorldToCamera) == bytes(before.worldToCamera) != bytes(after.worldToCamera)
        assert bytes(after.previousCameraToClip) == bytes(before.cameraToClip) != bytes(after.cameraToClip)
        assert list(after.previousJitter) == list(before.currentJitter)
        assert np.array(after.currentJitter[:], np.float32).tobytes() == capi.taa_jitter(index, w, h).tobytes()
    # the index wraps after eight frames
    for _ in range(6):
        cam.end_frame()
    assert np.array(cam.update_buffer()[0].currentJitter[:], np.float32).tobytes() == capi.taa_jitter(0, w, h).tobytes()
    cam.close()


def test_the_jittered_projection_moves_ndc_by_the_jitter():
    w, h = 160, 96
    plain, jittered = make_camera(w, h), make_camera(w, h)
    jittered.set_jitter(True)
    for index in range(8):
        u, uj = plain.update_buffer()[0], jittered.update_buffer()[0]
        jitter = np.array(uj.currentJitter[:], np.float64)
        assert jitter.any()
        for point in ((0.1, 1.2, 0.3, 1.0), (-0.8, 0.4, -2.0, 1.0), (1.5, 2.0, 1.0, 1.0)):
            clip = mat(u.cameraToClip) @ mat(u.worldToCamera) @ np.array(point)
            clip_j = mat(uj.cameraToClip) @ mat(uj.worldToCamera) @ np.array(point)
            assert clip[3] > 0 and clip_j[3] == clip[3] and clip_j[2] == clip[2]
            # ndc_jittered = ndc_unjittered + currentJitter on both axes, after the y-flip
            assert np.allclose(clip_j[:2] / clip_j[3] - clip[:2] / clip[3], jitter, rtol=0, atol=1e-12), index
        plain.end_frame()
        jittered.end_frame()
    plain.close()
    jittered.close()


def test_bad_arguments_are_rejected_before_touching_the_gpu():
    lib = capi.lib()
    ve = np.zeros((8, 8, 2), np.float32)

    def refused(rc, words):
        return rc == -1 and words in lib.prosper_pt_last_error().decode()

    def resolve(pc=S.TaaPC.default(), w=8, h=8, inputs=S.TaaInputs(None, ve.ctypes.data, None, 0)):
        return lib.prosper_pt_taa_resolve(None, None if pc is None else C.byref(pc), w, h, None if inputs is None else C.byref(inputs), None)

    assert refused(resolve(), "null argument")  # only the context is missing
    assert refused(resolve(pc=None), "null argument")
    assert refused(resolve(inputs=None), "null argument")
    for field in ("catmullRom", "luminanceWeighting", "resetHistory"):
        pc = S.TaaPC.default()
        setattr(pc, field, 2)
        assert refused(resolve(pc=pc), "0 or 1"), field
    assert refused(resolve(pc=S.TaaPC.default(color_clipping=3)), "unknown color clipping")
    assert refused(resolve(pc=S.TaaPC.default(velocity_sampling=3)), "unknown velocity sampling")
    assert refused(resolve(w=0), "empty extent") and refused(resolve(h=0), "empty extent")
    assert refused(resolve(w=32769), "above 32768") and refused(resolve(h=32769), "above 32768")
    assert refused(resolve(inputs=S.TaaInputs(None, None, None, 0)), "null argument")  # (the traced velocity target is the context's)
    buf = np.zeros(16, np.uint8)
    assert lib.prosper_pt_read_taa_history(None, buf.ctypes.data, 16, None) == -1
    assert lib.prosper_pt_get_taa_info(None, None) == -1
    lib.prosper_pt_taa_release_history(None)  # (a no-op)
    lib.prosper_pt_taa_jitter(0, 8, 8, None)
    handle = C.c_void_p()
    assert lib.prosper_host_taa_create(None, C.byref(handle)) == -1 and handle.value is None
    assert "null context" in lib.prosper_host_last_error().decode()
    assert lib.prosper_host_taa_record(None, 8, 8, None, None, None) == -1
    lib.prosper_host_taa_release_preserved(None)
    lib.prosper_host_taa_destroy(None)


def test_the_specialization_index_is_prospers():
    indices = [R.specialization_index(0, *v) for v in R.VARIANTS]
    assert len(R.VARIANTS) == len(set(indices)) == 36 and max(indices) < 128
    assert R.specialization_index(0, *R.DEFAULT) == 2 | (2 << 2) | (2 << 4) | (1 << 6)
    assert R.specialization_index(1, *R.CHEAPEST) == 1


# ---- the restatement's known answers ----

def still(w, h):
    return np.zeros((h, w, 2), np.float32), np.full((h, w), 0.5, np.float32)


@pytest.mark.parametrize("variant", R.VARIANTS, ids=lambda v: "%d%d%d%d" % v)
def test_a_constant_image_stays_constant(variant):
    w, h = 7, 5
    illum = np.empty((h, w, 4), np.float32)
    illum[...] = (0.75, 1.5, 0.25, 0.5)
    vel, depth = R.design(w, h, 1)[1:]
    r = R.resolve(illum, vel, depth, R.half(illum), variant)
    assert r["inside"].any() and not r["inside"].all()
    assert np.allclose(r["v"], illum[..., :3], rtol=1e-12, atol=0)
    assert np.isfinite(r["a"]).all() and (r["a"][r["inside"]] > 0).all() and (r["a"][~r["inside"]] == 0).all()


def test_zero_velocity_with_catmull_rom_returns_the_history_texel():
    w, h = 9, 6
    rng = np.random.default_rng(3)
    hist = R.half(rng.uniform(0.1, 4.0, (h, w, 4)))
    illum = R.design(w, h, 0)[0]
    vel, depth = still(w, h)
    r = R.resolve(illum, vel, depth, hist, (1, R.NONE, R.CENTER, 0))
    assert r["inside"].all()
    assert np.allclose(r["previous"], hist[..., :3].astype(np.float64), rtol=1e-6, atol=0)
    # f = 0: w1 = 1 and the other weights vanish
    w0, w12, w3, t = R.catmull_axis(np.float32(0))
    assert (w0, w12, w3, t) == (0, 1, 0, 0)
    cw, hw = float(np.float32(0.1)), float(np.float32(1) - np.float32(0.1))
    want = (illum[..., :3].astype(np.float64) * cw + hist[..., :3].astype(np.float64) * hw) / (cw + hw)
    assert np.allclose(r["v"], want, rtol=1e-6, atol=0)


def test_a_history_outlier_is_clipped_to_the_neighbourhood():
    w, h = 5, 5
    illum = R.design(w, h, 0)[0]
    n = R.neighbourhood(illum)
    vel, depth = still(w, h)
    for factor, bound in ((100.0, n.max(axis=0)), (0.001, n.min(axis=0))):
        hist = R.half(illum[..., :3].astype(np.float64) * factor)
        r = R.resolve(illum, vel, depth, hist, (0, R.MIN_MAX, R.CENTER, 0))
        clipped = np.minimum(np.maximum(r["previous"], r["lo"]), r["hi"])
        assert np.array_equal(clipped, bound)
        want = (illum[..., :3].astype(np.float64) * float(np.float32(0.1)) + bound * float(np.float32(1) - np.float32(0.1)))
        assert np.allclose(r["v"], want, rtol=1e-6, atol=0)


def test_a_flat_neighbourhood_has_sigma_zero_and_no_nan():
    w, h = 4, 4
    illum = np.empty((h, w, 4), np.float32)
    illum[...] = (0.1, 0.7, 1.3, 1.0)  # (m2 / 9 - mu mu goes negative in float32 for such values)
    lo, hi, a = R.clip_bounds(illum, R.VARIANCE)
    assert np.array_equal(lo, hi) and np.isfinite(a).all() and (a > 0).all()
    vel, depth = still(w, h)
    r = R.resolve(illum, vel, depth, R.half(illum[..., :3] * 3.0), R.DEFAULT)
    assert np.isfinite(r["v"]).all() and np.allclose(r["v"], illum[..., :3], rtol=1e-12, atol=0)
    c = illum[0, 0, :3]
    m2 = sum(c * c for _ in range(9))
    assert ((np.float32(m2) / np.float32(9) - c * c) != 0).any()  # what the stated max(., 0) is for


# ---- the design ----

def histories(w, h, variant):
    """The fp16 history each frame of the design reads when the restatement runs the sequence itself."""
    out, hist = [], None
    for frame in range(FRAMES):
        out.append(hist)
        hist = R.half(R.resolve(*R.design(w, h, frame), hist, variant)["v"])
    return out


@pytest.mark.parametrize("w,h", [e for e in EXTENTS if e[0] * e[1] >= 17 * 9], ids=lambda v: str(v))
def test_the_design_holds_every_kind_of_texel(w, h):
    for variant in (R.DEFAULT, R.CHEAPEST):
        hist = histories(w, h, variant)
        for frame in range(1, FRAMES):
            c = R.coverage(w, h, frame, hist[frame], variant)
            print(w, h, variant, frame, c)
            for kind in KINDS:
                assert c[kind] >= 1, (kind, frame, variant)
            r = R.resolve(*R.design(w, h, frame), hist[frame], variant)
            if variant[3]:
                assert (1.0 + r["history_luminance"]).min() > 0.25  # the blend's weights stay away from their pole


@pytest.mark.parametrize("w,h", ALL_VARIANT_EXTENTS, ids=lambda v: str(v))
def test_every_variant_stays_inside_fp16_and_away_from_the_luminance_pole(w, h):
    for variant in R.VARIANTS:
        hist = None
        for frame in range(FRAMES):
            r = R.resolve(*R.design(w, h, frame), hist, variant)
            assert (np.abs(r["v"]) + r["a"]).max() < 6e4, (variant, frame)
            if variant[3] and hist is not None:
                assert (1.0 + r["history_luminance"])[r["inside"]].min() > 0.25, (variant, frame)
            hist = R.half(r["v"])


def test_the_small_extents_hold_what_they_can():
    # 1 x 1: the one texel is its own neighbourhood; its velocity kind moves on with the frame (zero, sub-pixel, whole pixels)
    kinds = [int(R.velocity_kinds(1, 1, f)[0, 0]) for f in range(FRAMES)]
    assert kinds == [R.V_ZERO, R.V_SUB_PIXEL, R.V_WHOLE_PIXELS]
    hist = histories(1, 1, R.DEFAULT)
    assert R.resolve(*R.design(1, 1, 1), hist[1], R.DEFAULT)["inside"].all()  # 0.37 of a texel: still inside
    assert not R.resolve(*R.design(1, 1, 2), hist[2], R.DEFAULT)["inside"].any()  # two texels: outside a 1-wide image
    # 3 x 2: every texel's neighbourhood is clamped on at least two sides, and both outcomes occur
    hist = histories(3, 2, R.CHEAPEST)
    inside = [R.resolve(*R.design(3, 2, f), hist[f], R.CHEAPEST)["inside"] for f in (1, 2)]
    assert any(i.any() for i in inside) and any((~i).any() for i in inside)
    for w, h in EXTENTS:
        illum = np.concatenate([R.design(w, h, f)[0].ravel() for f in range(FRAMES)])
        assert 0 < illum.min() and illum.max() < 6e4
