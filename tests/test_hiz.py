"""The depth pyramid on the GPU (prosper_pt_hiz_downsample; pt_culling.hip): designed depths - random with
planted unique minima at tile corners and along the clamped right and bottom edges - and every level of the pyramid
against the footprint-minimum definition of tests/culling_reference.py, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import culling_reference as R
from debug_view_scene import H, W, camera, quad_world
from prosper_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
# width x height.  130 x 70 has 8 levels, so the second launch runs; 96 x 64 and 1920 x 1080 have float4 rows and tiles
# right of and below the image; 2 x 2, 3 x 5, 65 x 33 and 130 x 70 take the kernel for rows that are not whole float4s
SIZES = [(2, 2), (3, 5), (64, 64), (65, 33), (130, 70), (96, 64), (1920, 1080)]


class DeviceArray:
    """device memory through the HIP runtime the library itself uses"""

    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0

    def upload(self, a, byte_offset=0):
        a = np.ascontiguousarray(a)
        assert self.hip.hipMemcpy(C.c_void_p(self.ptr.value + byte_offset), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def check(ctx, depth, slot, what=""):
    """the slot's pyramid is the definition's over `depth`"""
    h, w = depth.shape
    want = R.hiz_pyramid(depth)
    info = ctx.hiz_info(slot)
    assert (info.valid, info.sourceWidth, info.sourceHeight, info.levelCount) == (1, w, h, len(want))
    assert (info.width, info.height) == R.hiz_extents(w, h)[0]
    assert info.launches == (2 if len(want) > 6 else 1)
    got = ctx.read_hiz(slot)
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, l)
        bad = a.view(np.uint32) != b.view(np.uint32)
        assert not bad.any(), "%s level %d: %d texels differ, first at %s" % (what, l, bad.sum(), np.argwhere(bad)[0])


@pytest.mark.parametrize("w,h", SIZES)
def test_every_level_is_the_minimum_of_its_clamped_footprint(gpu_ctx, w, h):
    depth = R.designed_depth(w, h, seed=w * 7 + h)
    gpu_ctx.hiz_downsample(w, h, slot=0, depth=depth)  # a host array, copied by the call
    check(gpu_ctx, depth, 0, "host")
    dev = DeviceArray(depth.nbytes + 16)
    try:
        dev.upload(depth)
        gpu_ctx.hiz_downsample(w, h, slot=1, depth_ptr=dev.ptr.value)  # the caller's device array
        check(gpu_ctx, depth, 1, "device")
        if w % 4 == 0 and w <= 128:
            # the same rows four bytes on: no longer 16-byte aligned, so the other kernel
            dev.upload(depth, byte_offset=4)
            gpu_ctx.hiz_downsample(w, h, slot=1, depth_ptr=dev.ptr.value + 4)
            check(gpu_ctx, depth, 1, "unaligned")
    finally:
        dev.free()


def test_both_slots_hold_their_own_pyramid_and_a_repeated_call_gives_the_same(gpu_ctx):
    a, b = R.designed_depth(130, 70, seed=1), R.designed_depth(65, 33, seed=2)
    gpu_ctx.hiz_downsample(130, 70, slot=0, depth=a)
    gpu_ctx.hiz_downsample(65, 33, slot=1, depth=b)
    check(gpu_ctx, a, 0)
    check(gpu_ctx, b, 1)
    first = gpu_ctx.read_hiz(0)
    gpu_ctx.hiz_downsample(130, 70, slot=0, depth=a)
    for x, y in zip(first, gpu_ctx.read_hiz(0)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    check(gpu_ctx, b, 1)  # untouched
    # a smaller, then a larger pyramid in the same slot: the buffer only grows and the extents follow the call
    gpu_ctx.hiz_downsample(3, 5, slot=0, depth=a[:5, :3])
    check(gpu_ctx, np.ascontiguousarray(a[:5, :3]), 0)
    big = R.designed_depth(200, 150, seed=3)
    gpu_ctx.hiz_downsample(200, 150, slot=0, depth=big)
    check(gpu_ctx, big, 0)
    # the device pointer of a level is where the read-back reads
    ptr, lw, lh = gpu_ctx.hiz_device_ptr(0, 2)
    assert (lw, lh) == R.hiz_extents(200, 150)[2] and ptr
    out = np.empty((lh, lw), F)
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    assert np.array_equal(out, R.hiz_pyramid(big)[2])


def test_calls_on_two_streams_into_one_slot_do_not_overwrite_each_other(gpu_ctx):
    hip = C.CDLL("libamdhip64.so")
    s1, s2 = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s1), 1) == 0 and hip.hipStreamCreateWithFlags(C.byref(s2), 1) == 0
    try:
        a, b = R.designed_depth(130, 70, seed=11), R.designed_depth(260, 140, seed=12)
        for _ in range(3):  # the second call grows the buffer the first still writes; nothing waits on the host between
            gpu_ctx.hiz_downsample(130, 70, slot=0, depth=a, stream=s1.value)
            gpu_ctx.hiz_downsample(260, 140, slot=0, depth=b, stream=s2.value)
            got = [gpu_ctx.read_hiz_level(0, l, stream=s1.value) for l in range(gpu_ctx.hiz_info(0).levelCount)]
            for x, y in zip(got, R.hiz_pyramid(b)):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    finally:
        assert hip.hipStreamSynchronize(s1) == 0 and hip.hipStreamSynchronize(s2) == 0
        hip.hipStreamDestroy(s1)
        hip.hipStreamDestroy(s2)


def test_the_pyramid_of_a_traced_depth(gpu_ctx, oracle):
    """quad and sky at 48 x 32: the default input is the last traced G-buffer's depth"""
    gpu_ctx.upload_scene(quad_world())
    assert gpu_ctx.hiz_info(0).valid == 0 and gpu_ctx.hiz_info(1).valid == 0  # a new scene invalidates both slots
    with pytest.raises(capi.ProsperPtError, match="holds no pyramid"):
        gpu_ctx.read_hiz_level(0, 0)
    cam = camera(oracle)
    gpu_ctx.trace_gbuffer(cam, W, H)
    depth = gpu_ctx.read_gbuffer()[2]
    assert (depth == 0).any() and (depth > 0).any()  # sky and quad
    gpu_ctx.hiz_downsample(W, H, slot=1)
    check(gpu_ctx, depth, 1)
    levels = gpu_ctx.read_hiz(1)
    assert levels[-1][0, 0] == 0  # the farthest of everything is the sky
    assert (levels[0][:, :8] > 0).all()  # the left of the view is all quad
    with pytest.raises(capi.ProsperPtError, match="another extent"):
        gpu_ctx.hiz_downsample(W, H + 1, slot=1)
    assert gpu_ctx.hiz_info(1).valid == 1  # a refused call leaves the slot as it was
    check(gpu_ctx, depth, 1)


def test_the_cpp_downsampler_makes_what_the_direct_call_makes(gpu_ctx):
    from prosper_amd import rt_reference
    depth = R.designed_depth(130, 70, seed=21)
    pass_ = rt_reference.HierarchicalDepthDownsampler(gpu_ctx)
    try:
        for next_frame in (0, 1, 2):
            mips = pass_.record(130, 70, next_frame=next_frame, depth=depth)
            slot = next_frame & 1
            check(gpu_ctx, depth, slot)
            assert mips == [gpu_ctx.hiz_device_ptr(slot, l)[0] for l in range(8)]
        with pytest.raises(capi.ProsperPtError, match="above 1"):
            pass_.record(1, 70, depth=depth[:, :1])
    finally:
        pass_.close()


def test_refusals(gpu_ctx):
    depth = R.designed_depth(8, 8, seed=5)
    gpu_ctx.hiz_downsample(8, 8, slot=0, depth=depth)
    with pytest.raises(capi.ProsperPtError, match="slot is 0 or 1"):
        gpu_ctx.hiz_downsample(8, 8, slot=2, depth=depth)
    for w, h in ((1, 8), (8, 1), (0, 8)):
        with pytest.raises(capi.ProsperPtError, match="above 1"):
            capi._check(capi.lib().prosper_pt_hiz_downsample(gpu_ctx._h, 0, C.c_void_p(depth.ctypes.data), 0, w, h, None))
    with pytest.raises(capi.ProsperPtError, match="at most 4096"):
        capi._check(capi.lib().prosper_pt_hiz_downsample(gpu_ctx._h, 0, C.c_void_p(depth.ctypes.data), 0, 4097, 2, None))
    with pytest.raises(capi.ProsperPtError, match="level beyond"):
        gpu_ctx.read_hiz_level(0, 3)
    out = np.empty((4, 4), F)
    with pytest.raises(capi.ProsperPtError, match="too small"):
        capi._check(capi.lib().prosper_pt_read_hiz_level(gpu_ctx._h, 0, 0, C.c_void_p(out.ctypes.data), 63, None))
    check(gpu_ctx, depth, 0)  # the refusals left the slot alone


def test_before_any_gbuffer_the_default_input_is_refused():
    ctx = capi.Context(device=0)
    try:
        rc = capi.lib().prosper_pt_hiz_downsample(ctx._h, 0, None, 1, 48, 32, None)
        assert rc == -4  # PROSPER_PT_ERR_NO_SCENE
        assert ctx.hiz_info(0).valid == 0
    finally:
        ctx.close()
