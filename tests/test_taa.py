"""The temporal anti-aliasing resolve on the GPU (prosper_pt_taa_resolve).

Three consecutive calls per case over the per-pixel design of tests/taa_reference.py, a new frame of it each: the first
ignores the history, the next two read what the call before wrote.  Each call is checked against the numpy restatement
fed with the GPU's own read-back of the history the call read.  The resolved image is fp16: a texel passes when its code
lies between the fp16 roundings of v - a and v + a, v the restatement's unrounded value and a its allowance (relative
2e-4 of the sum of absolute terms, carried through the clamps: tests/taa_reference.py); a texel that falls back to the
illumination must be its rounding exactly.  No texel is left out.  The HDR image must be the float32 expansion of the
new history bit for bit, with alpha 1.

Extents, the smallest at which each rule can go wrong: 1 x 1, 3 x 2 (every neighbourhood clamped), 17 x 9, 101 x 71 (odd),
130 x 33 and 33 x 130 (more than one 32 x 8 tile with its halo on each axis, the last one partial).  All 36 variants on
17 x 9 and 101 x 71, the default and the cheapest variant on every extent.  The CPU side and the design:
tests/test_taa_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import taa_reference as R
from prosper_amd import capi, scenes, structs as S
from test_depth_of_field import DeviceCopy, check_half
from test_taa_cpu import ALL_VARIANT_EXTENTS, EXTENTS, FRAMES

pytestmark = pytest.mark.gpu

CASES = [(w, h, v) for w, h in ALL_VARIANT_EXTENTS for v in R.VARIANTS] + [
    (w, h, v) for w, h in EXTENTS if (w, h) not in ALL_VARIANT_EXTENTS for v in (R.DEFAULT, R.CHEAPEST)]
IDS = ["%dx%d-cr%d-clip%d-vel%d-lw%d" % ((w, h) + v) for w, h, v in CASES]


def pc_of(variant, reset=0):
    return S.TaaPC.default(*variant, reset_history=reset)


def expansion(history16):
    """What the HDR image must hold beside a history: its float32 expansion."""
    return np.asarray(history16, np.float16).astype(np.float32)


def call(ctx, variant, w, h, frame, reset=0, how="host"):
    """One resolve of frame `frame` of the design; (the history the call wrote, the HDR image)."""
    illum, vel, depth = R.design(w, h, frame)
    if how == "host":
        ctx.taa_resolve(pc_of(variant, reset), w, h, vel, depth, illum)
    elif how == "device":
        with DeviceCopy(illum) as il, DeviceCopy(vel) as ve, DeviceCopy(depth) as dp:
            ctx.taa_resolve(pc_of(variant, reset), w, h, velocity_ptr=ve, depth_ptr=dp, illumination_ptr=il)
            return ctx.read_taa_history(), ctx.read_hdr()
    else:  # in place: the illumination is put into the HDR image first
        put_hdr(ctx, illum)
        with DeviceCopy(vel) as ve, DeviceCopy(depth) as dp:
            ctx.taa_resolve(pc_of(variant, reset), w, h, velocity_ptr=ve, depth_ptr=dp)
            return ctx.read_taa_history(), ctx.read_hdr()
    return ctx.read_taa_history(), ctx.read_hdr()


def put_hdr(ctx, illum):
    """The image into the context's HDR image, byte for byte.  (When the HDR image has another extent, a resolve with host
    inputs makes it first; its history is released again.)"""
    h, w = illum.shape[:2]
    if tuple(ctx.local_extent()) != (w, h):
        ctx.taa_resolve(pc_of(R.CHEAPEST, 1), w, h, np.zeros((h, w, 2), np.float32), None, illum)
        ctx.taa_release_history()
    ptr, size = ctx.hdr_device_ptr()
    assert size == illum.nbytes
    with DeviceCopy(illum):  # (loads the runtime)
        assert DeviceCopy.hip.hipMemcpy(C.c_void_p(ptr), C.c_void_p(illum.ctypes.data), C.c_size_t(illum.nbytes), 1) == 0
    assert ctx.read_hdr().tobytes() == illum.tobytes()


def check_call(label, illum, vel, depth, before, after, hdr, variant):
    r = R.resolve(illum, vel, depth, before, variant)
    assert after.shape == illum.shape and (after[..., 3] == 1).all(), label
    check_half(label, after[..., :3], r["v"], r["a"])
    # a texel that took the illumination holds its rounding
    keep = ~r["inside"]
    assert np.array_equal(after[..., :3][keep].view(np.uint16), R.half(illum[..., :3])[keep].view(np.uint16)), label
    assert hdr.tobytes() == expansion(after).tobytes(), label + ": the HDR image is not the expansion of the history"
    return r


@pytest.mark.parametrize("w,h,variant", CASES, ids=IDS)
def test_three_consecutive_calls_equal_the_restatement_over_the_history_they_read(gpu_ctx, w, h, variant):
    gpu_ctx.taa_release_history()
    before, resolved = None, 0
    for frame in range(FRAMES):
        after, hdr = call(gpu_ctx, variant, w, h, frame)
        info = gpu_ctx.taa_info()
        assert (info.valid, info.width, info.height, info.historyValid, info.ignoredHistory) == (1, w, h, 1, 1 if frame == 0 else 0)
        assert np.isfinite(info.resolveMs) and info.resolveMs >= 0 and np.isfinite(info.expandMs) and info.expandMs >= 0
        r = check_call("%s frame %d" % (IDS[CASES.index((w, h, variant))], frame), *R.design(w, h, frame), before, after, hdr, variant)
        resolved += int(r["inside"].sum())
        before = after
    assert resolved > 0 or (w, h) == (1, 1)


def first_call_is_the_rounded_input(ctx, w, h, frame, **kw):
    after, hdr = call(ctx, R.DEFAULT, w, h, frame, **kw)
    illum = R.design(w, h, frame)[0]
    assert ctx.taa_info().ignoredHistory == 1
    assert np.array_equal(after[..., :3].view(np.uint16), R.half(illum[..., :3]).view(np.uint16)) and (after[..., 3] == 1).all()
    assert hdr.tobytes() == expansion(after).tobytes()


def reads_history(ctx, w, h, frame):
    call(ctx, R.DEFAULT, w, h, frame)
    assert ctx.taa_info().ignoredHistory == 0


def test_history_is_ignored_when_there_is_none_to_read(gpu_ctx):
    w, h = 17, 9
    gpu_ctx.taa_release_history()
    assert gpu_ctx.taa_info().historyValid == 0
    with pytest.raises(capi.ProsperPtError):
        gpu_ctx.read_taa_history()
    first_call_is_the_rounded_input(gpu_ctx, w, h, 0)  # the first call
    reads_history(gpu_ctx, w, h, 1)
    first_call_is_the_rounded_input(gpu_ctx, 101, 71, 1)  # a changed extent
    reads_history(gpu_ctx, 101, 71, 2)
    first_call_is_the_rounded_input(gpu_ctx, w, h, 2)  # ... and back to a smaller one
    reads_history(gpu_ctx, w, h, 0)
    first_call_is_the_rounded_input(gpu_ctx, w, h, 1, reset=1)  # resetHistory
    reads_history(gpu_ctx, w, h, 2)
    gpu_ctx.taa_release_history()
    first_call_is_the_rounded_input(gpu_ctx, w, h, 0)  # after a release
    reads_history(gpu_ctx, w, h, 1)


def test_a_scene_upload_drops_the_history():
    w, h = 17, 9
    ctx = capi.Context(device=0)
    try:
        first_call_is_the_rounded_input(ctx, w, h, 0)
        reads_history(ctx, w, h, 1)
        ctx.upload_scene(scenes.cornell(with_skybox=True))
        assert ctx.taa_info().historyValid == 0
        first_call_is_the_rounded_input(ctx, w, h, 2)
        reads_history(ctx, w, h, 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("w,h", [(3, 2), (101, 71), (130, 33)], ids=lambda v: str(v))
def test_in_place_device_and_host_inputs_give_the_same_bytes(gpu_ctx, w, h):
    results = {}
    for how in ("host", "device", "in place"):
        gpu_ctx.taa_release_history()
        results[how] = [call(gpu_ctx, R.DEFAULT, w, h, frame, how=how) for frame in range(FRAMES)]
    for how in ("device", "in place"):
        for frame in range(FRAMES):
            assert results[how][frame][0].tobytes() == results["host"][frame][0].tobytes(), (how, frame, "history")
            assert results[how][frame][1].tobytes() == results["host"][frame][1].tobytes(), (how, frame, "HDR image")
    # the HDR image passed explicitly behaves as in place
    gpu_ctx.taa_release_history()
    for frame in range(FRAMES):
        illum, vel, depth = R.design(w, h, frame)
        put_hdr(gpu_ctx, illum)
        with DeviceCopy(vel) as ve, DeviceCopy(depth) as dp:
            gpu_ctx.taa_resolve(pc_of(R.DEFAULT), w, h, velocity_ptr=ve, depth_ptr=dp, illumination_ptr=gpu_ctx.hdr_device_ptr()[0])
            assert gpu_ctx.read_taa_history().tobytes() == results["host"][frame][0].tobytes()
            assert gpu_ctx.read_hdr().tobytes() == results["host"][frame][1].tobytes()


def test_two_identical_sequences_give_the_same_bytes(gpu_ctx):
    w, h = 101, 71
    runs = []
    for _ in range(2):
        gpu_ctx.taa_release_history()
        runs.append([call(gpu_ctx, R.DEFAULT, w, h, frame) for frame in range(FRAMES)])
    for frame in range(FRAMES):
        assert runs[0][frame][0].tobytes() == runs[1][frame][0].tobytes() and runs[0][frame][1].tobytes() == runs[1][frame][1].tobytes()


def test_bad_arguments_are_refused_and_change_nothing(gpu_ctx):
    w, h = 17, 9
    gpu_ctx.taa_release_history()
    call(gpu_ctx, R.DEFAULT, w, h, 0)
    history, hdr, info = gpu_ctx.read_taa_history(), gpu_ctx.read_hdr(), bytes(gpu_ctx.taa_info())
    illum, vel, depth = R.design(w, h, 1)

    def refused(words, fn):
        with pytest.raises(capi.ProsperPtError) as e:
            fn()
        assert e.value.code == -1 and words in str(e.value), str(e.value)

    refused("unknown color clipping", lambda: gpu_ctx.taa_resolve(S.TaaPC.default(color_clipping=3), w, h, vel, depth, illum))
    refused("unknown velocity sampling", lambda: gpu_ctx.taa_resolve(S.TaaPC.default(velocity_sampling=3), w, h, vel, depth, illum))
    refused("0 or 1", lambda: gpu_ctx.taa_resolve(S.TaaPC.default(catmull_rom=2), w, h, vel, depth, illum))
    refused("another extent", lambda: gpu_ctx.taa_resolve(pc_of(R.DEFAULT), 64, 48, np.zeros((48, 64, 2), np.float32), np.zeros((48, 64), np.float32)))
    assert capi.lib().prosper_pt_read_taa_history(gpu_ctx._h, history.ctypes.data, history.nbytes - 8, None) == -1
    assert gpu_ctx.read_taa_history().tobytes() == history.tobytes() and gpu_ctx.read_hdr().tobytes() == hdr.tobytes()
    assert bytes(gpu_ctx.taa_info()) == info
    reads_history(gpu_ctx, w, h, 1)


def test_the_mirror_with_defaults_equals_a_direct_call(gpu_ctx):
    from prosper_amd.rt_reference import TemporalAntiAliasing
    w, h = 101, 71
    gpu_ctx.taa_release_history()
    want = [call(gpu_ctx, R.DEFAULT, w, h, frame) for frame in range(FRAMES)]
    taa = TemporalAntiAliasing(gpu_ctx)
    try:
        taa.release_preserved()
        assert gpu_ctx.taa_info().historyValid == 0
        for frame in range(FRAMES):
            illum, vel, depth = R.design(w, h, frame)
            pc = taa.record(w, h, vel, depth, illum)
            assert bytes(pc) == bytes(pc_of(R.DEFAULT))
            assert gpu_ctx.read_taa_history().tobytes() == want[frame][0].tobytes() and gpu_ctx.read_hdr().tobytes() == want[frame][1].tobytes()
        # the setters reach the push constants
        taa.draw_ui(catmull_rom=False, color_clipping=S.TAA_CLIPPING_NONE, velocity_sampling=S.TAA_VELOCITY_CENTER, luminance_weighting=False)
        taa.release_preserved()
        gpu_ctx.taa_release_history()
        cheapest = [call(gpu_ctx, R.CHEAPEST, w, h, frame) for frame in range(2)]
        taa.release_preserved()
        for frame in range(2):
            illum, vel, depth = R.design(w, h, frame)
            assert bytes(taa.record(w, h, vel, depth, illum)) == bytes(pc_of(R.CHEAPEST))
            assert gpu_ctx.read_taa_history().tobytes() == cheapest[frame][0].tobytes()
    finally:
        taa.close()
