"""The spatiotemporal denoiser on the GPU (prosper_pt_denoise).

Consecutive calls over the per-pixel design of tests/denoise_design.py, a new frame of it each: the first ignores the
history, the following read what the call before wrote.  Every stage's read-back must equal the NumPy statement
(prosper_amd/denoise.py) bit for bit, the statement being fed with the GPU's own read-back of what that stage read: the
history images for the temporal stage, the guide, moments and temporal colour for the variance estimate, the previous
image for an a-trous pass, the last image for the stored result.  No texel is left out; lengths, flags and the info's counts
are compared exactly.  The a-trous passes ping-pong between two images, so a call holds its last two passes' images: an
earlier pass is checked through the statement's own chain from the read-back variance image, and directly in the run
whose `iterations` makes it one of the last two (all of 0 .. 5 run on every extent).

Extents, the smallest at which each rule can go wrong: 1 x 1, 3 x 2 (every tap outside or skipped), 17 x 9 (steps 8 and 16
never land inside), 101 x 71 (odd, with pixels of full reach at step 16), 130 x 33 and 33 x 130 (several 32 x 8 tiles per
axis, the last one partial).  The CPU side and the design: tests/test_denoise_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import debug_view_scene as V
import denoise_design as D
import test_denoise_cpu as P
from prosper_amd import capi, dds, denoise as R, scenes, structs as S
from test_depth_of_field import DeviceCopy

pytestmark = pytest.mark.gpu

KEYS = ("illumination", "albedo", "normal_metallic", "depth", "velocity")


def both(**kw):
    """the same parameters for the library and for the statement"""
    ref = R.PC(**kw)
    return S.DenoisePC.default(**kw), ref


def design_camera():
    cam = S.CameraUniforms()
    cam.cameraToClip.col[2].z = float(D.C22)
    cam.cameraToClip.col[3].z = float(D.C32)
    return cam


def assert_same(label, got, want):
    g, w = R.bits(got), R.bits(want)
    assert g.shape == w.shape, label
    bad = g != w
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: got %r, the statement %r" % (
            label, int(bad.sum()), bad.size, at, np.asarray(got, np.float32)[at], np.asarray(want, np.float32)[at]))


def read_all(ctx, iterations):
    r = {"guide_a": ctx.read_denoise_stage(S.DENOISE_GUIDE_A), "guide_b": ctx.read_denoise_stage(S.DENOISE_GUIDE_B),
         "moments": ctx.read_denoise_stage(S.DENOISE_MOMENTS), "temporal": ctx.read_denoise_stage(S.DENOISE_TEMPORAL),
         "colour": ctx.read_denoise_stage(S.DENOISE_HISTORY_COLOUR), "out": ctx.read_hdr(), "atrous": {}}
    for i in range(max(iterations - 2, 0), iterations):
        r["atrous"][i] = ctx.read_denoise_stage(S.DENOISE_ATROUS_0 + i)
    r["info"] = ctx.denoise_info()
    return r


def history_of(r):
    return {k: r[k] for k in ("colour", "moments", "guide_a", "guide_b")}


def check_call(label, ref, c22, c32, d, before, got):
    """every stage of one call against the statement over what the GPU's stage before it wrote"""
    t = R.temporal_stage(ref, c22, c32, *[d[k] for k in KEYS], history=before)
    for k in ("guide_a", "guide_b", "moments"):
        assert_same(label + " " + k, got[k], t[k])
    assert_same(label + " temporal colour", got["temporal"][..., :3], t["temporal"][..., :3])
    assert (got["info"].historyPixels, got["info"].noHistoryPixels) == t["counts"], label
    unestimated = np.concatenate([got["temporal"][..., :3], R.temporal_variance(got["moments"])[..., None]], -1)
    assert_same(label + " variance", got["temporal"], R.variance_stage(ref, got["guide_a"], got["guide_b"], got["moments"], unestimated))
    image, feedback = got["temporal"], unestimated
    for i in range(ref.iterations):
        image = R.atrous_pass(ref, i, got["guide_a"], got["guide_b"], image)
        if i in got["atrous"]:
            assert_same(label + " a-trous pass %d" % i, got["atrous"][i], image)
            image = got["atrous"][i]  # the next pass is checked over what it read
        if i == ref.feedback_iteration:
            feedback = image
    assert_same(label + " colour history", got["colour"], feedback)
    assert_same(label + " result", got["out"], R.finish(ref, d["illumination"], d["albedo"], got["guide_a"], image))
    return t


def run_design(ctx, w, h, frames, how="host", **kw):
    """`frames` consecutive calls over the design, each checked; the read-backs of the last"""
    pc, ref = both(**kw)
    cam = design_camera()
    ctx.denoise_release_history()
    before, got = None, None
    for k in range(frames):
        d = D.design(w, h, k)
        call(ctx, pc, cam, w, h, d, how)
        got = read_all(ctx, ref.iterations)
        i = got["info"]
        assert (i.valid, i.width, i.height, i.historyValid, i.ignoredHistory, i.iterations) == (1, w, h, 1, 1 if k == 0 else 0, ref.iterations)
        times = [i.temporalMs, i.varianceMs, i.finishMs, i.totalMs] + list(i.atrousMs)
        assert all(np.isfinite(t) and t >= 0 for t in times)
        check_call("%dx%d frame %d" % (w, h, k), ref, D.C22, D.C32, d, before, got)
        before = history_of(got)
    return got


def call(ctx, pc, cam, w, h, d, how="host"):
    if how == "host":
        ctx.denoise(pc, cam, w, h, *[d[k] for k in KEYS])
    elif how == "device":
        with DeviceCopy(d["illumination"]) as il, DeviceCopy(d["albedo"]) as al, DeviceCopy(d["normal_metallic"]) as nm, \
                DeviceCopy(d["depth"]) as dp, DeviceCopy(d["velocity"]) as ve:
            ctx.denoise(pc, cam, w, h, illumination_ptr=il, albedo_roughness_ptr=al, normal_metallic_ptr=nm, depth_ptr=dp, velocity_ptr=ve)
            ctx.read_hdr()  # (synchronises before the copies are freed)
    else:  # in place: the illumination is put into the HDR image first
        put_hdr(ctx, d["illumination"])
        with DeviceCopy(d["albedo"]) as al, DeviceCopy(d["normal_metallic"]) as nm, DeviceCopy(d["depth"]) as dp, DeviceCopy(d["velocity"]) as ve:
            ctx.denoise(pc, cam, w, h, albedo_roughness_ptr=al, normal_metallic_ptr=nm, depth_ptr=dp, velocity_ptr=ve)
            ctx.read_hdr()


def put_hdr(ctx, illum):
    """The image into the context's HDR image, byte for byte.  (A TAA resolve with host inputs makes an HDR image of the
    extent when there is none.)"""
    h, w = illum.shape[:2]
    if tuple(ctx.local_extent()) != (w, h):
        ctx.taa_resolve(S.TaaPC.default(0, 0, 0, 0, 1), w, h, np.zeros((h, w, 2), np.float32), None, illum)
        ctx.taa_release_history()
    ptr, size = ctx.hdr_device_ptr()
    assert size == illum.nbytes
    with DeviceCopy(illum):  # (loads the runtime)
        assert DeviceCopy.hip.hipMemcpy(C.c_void_p(ptr), C.c_void_p(illum.ctypes.data), C.c_size_t(illum.nbytes), 1) == 0
    assert ctx.read_hdr().tobytes() == illum.tobytes()


# ---- the restatement ----

PLAIN = dict(demodulate=0, feedback_iteration=9, max_history_length=4)
CASES = [(w, h, kw) for w, h in D.EXTENTS for kw in (dict(max_history_length=4), PLAIN)] + [
    (w, h, dict(iterations=n, max_history_length=4, feedback_iteration=f)) for w, h in D.EXTENTS for n, f in ((0, 0), (1, 0), (2, 1), (3, 2), (4, 3))]
IDS = ["%dx%d-%s" % (w, h, "-".join("%s%s" % (k[:4], v) for k, v in kw.items())) for w, h, kw in CASES]


@pytest.mark.parametrize("w,h,kw", CASES, ids=IDS)
def test_consecutive_calls_equal_the_statement_stage_by_stage(gpu_ctx, w, h, kw):
    got = run_design(gpu_ctx, w, h, D.FRAMES, **kw)
    if (w, h) == D.FULL:
        length = R.bits(got["moments"][..., 2])
        assert (length == 4).any() and (length == 1).any() and got["info"].historyPixels > 0 and got["info"].noHistoryPixels > 0


# ---- the properties that need no restatement (the checks of tests/test_denoise_cpu.py, on the GPU) ----

def on_gpu(ctx):
    def denoise(ref, frames):
        pc = S.DenoisePC.default(ref.iterations, ref.demodulate, ref.max_history_length, ref.feedback_iteration, ref.normal_power_log2,
                                 ref.reset_history, *[float(v) for v in (ref.min_alpha, ref.depth_tolerance, ref.normal_threshold,
                                                                         ref.sigma_depth, ref.sigma_luminance)])
        ctx.denoise_release_history()
        for d in frames:
            h, w = d["depth"].shape
            call(ctx, pc, design_camera(), w, h, d)
        return ctx.read_hdr()
    return denoise


@pytest.mark.parametrize("check", [P.check_passthrough, P.check_half_planes, P.check_sky, P.check_outliers])
def test_properties_on_the_gpu(gpu_ctx, check):
    check(on_gpu(gpu_ctx))


# ---- input paths ----

def test_host_device_and_in_place_inputs_give_the_same_bytes(gpu_ctx):
    w, h = 130, 33
    images = ("guide_a", "guide_b", "moments", "temporal", "colour", "out")
    want = run_design(gpu_ctx, w, h, 3)
    again = run_design(gpu_ctx, w, h, 3)  # two identical sequences
    for how in ("device", "in place"):
        got = run_design(gpu_ctx, w, h, 3, how=how)
        for k in images:
            assert got[k].tobytes() == want[k].tobytes() == again[k].tobytes(), (how, k)
        for i, image in want["atrous"].items():
            assert got["atrous"][i].tobytes() == image.tobytes() == again["atrous"][i].tobytes(), (how, i)


# ---- history ----

def info_of(ctx):
    i = ctx.denoise_info()
    return i.valid, i.width, i.height, i.historyValid, i.ignoredHistory


def test_every_way_of_dropping_the_history(gpu_ctx):
    ctx, cam = gpu_ctx, design_camera()
    pc, _ = both()
    step = lambda w, h, k, p=pc: call(ctx, p, cam, w, h, D.design(w, h, k))
    ctx.denoise_release_history()
    assert ctx.denoise_info().historyValid == 0
    step(17, 9, 0)
    assert info_of(ctx) == (1, 17, 9, 1, 1)  # the first call
    assert ctx.denoise_info().historyPixels == 0
    step(17, 9, 1)
    assert info_of(ctx) == (1, 17, 9, 1, 0) and ctx.denoise_info().historyPixels > 0
    step(17, 9, 2, both(reset_history=1)[0])
    assert info_of(ctx) == (1, 17, 9, 1, 1)  # resetHistory
    step(17, 9, 3)
    assert info_of(ctx) == (1, 17, 9, 1, 0)
    ctx.denoise_release_history()
    assert info_of(ctx) == (1, 17, 9, 0, 0)  # released: the last call's fields stand, the history is gone
    with pytest.raises(capi.ProsperPtError):
        ctx.read_denoise_stage(S.DENOISE_HISTORY_COLOUR)
    step(17, 9, 4)
    assert info_of(ctx) == (1, 17, 9, 1, 1)
    step(33, 17, 0)
    assert info_of(ctx) == (1, 33, 17, 1, 1)  # a changed extent
    step(33, 17, 1)
    assert info_of(ctx) == (1, 33, 17, 1, 0)
    # an a-trous image that a later pass has written over, and one that did not run
    with pytest.raises(capi.ProsperPtError):
        ctx.read_denoise_stage(S.DENOISE_ATROUS_0)
    step(33, 17, 2, both(iterations=2)[0])
    with pytest.raises(capi.ProsperPtError):
        ctx.read_denoise_stage(S.DENOISE_ATROUS_0 + 2)


def test_a_scene_upload_drops_the_history_and_refusals_change_nothing():
    ctx, cam = capi.Context(device=0), design_camera()
    try:
        pc, _ = both()
        w, h = 17, 9
        d = D.design(w, h, 0)
        assert ctx.denoise_info().valid == 0
        with pytest.raises(capi.ProsperPtError):
            ctx.read_denoise_stage(S.DENOISE_TEMPORAL)
        # NULL inputs before anything has been traced, and an in-place call without an HDR image of the extent
        for kw in (dict(illumination=d["illumination"]), dict(illumination=d["illumination"], velocity=d["velocity"]),
                   dict(albedo_roughness=d["albedo"], normal_metallic=d["normal_metallic"], depth=d["depth"], velocity=d["velocity"])):
            with pytest.raises(capi.ProsperPtError):
                ctx.denoise(pc, cam, w, h, **kw)
        assert ctx.denoise_info().valid == 0
        call(ctx, pc, cam, w, h, d)
        call(ctx, pc, cam, w, h, D.design(w, h, 1))
        assert info_of(ctx) == (1, w, h, 1, 0)
        before = ctx.read_hdr().tobytes()
        with pytest.raises(capi.ProsperPtError):  # in place at another extent
            ctx.denoise(pc, cam, w + 1, h, albedo_roughness=np.zeros((h, w + 1, 4), np.float32), normal_metallic=np.zeros((h, w + 1, 4), np.float32),
                        depth=np.zeros((h, w + 1), np.float32), velocity=np.zeros((h, w + 1, 2), np.float32))
        assert info_of(ctx) == (1, w, h, 1, 0) and ctx.read_hdr().tobytes() == before
        ctx.upload_scene(scenes.cornell())
        assert info_of(ctx) == (1, w, h, 0, 0)
        call(ctx, pc, cam, w, h, D.design(w, h, 2))
        assert info_of(ctx) == (1, w, h, 1, 1)
        # the traced targets of another extent
        cornell = scenes.cornell().camera
        ctx.trace_gbuffer_velocity(cam_of(cornell, 24, 16)[0], 24, 16)
        with pytest.raises(capi.ProsperPtError):
            ctx.denoise(pc, cam, w, h, illumination=d["illumination"])
        with pytest.raises(capi.ProsperPtError):
            ctx.denoise(pc, cam, w, h, illumination=d["illumination"], velocity=d["velocity"])
        assert info_of(ctx) == (1, w, h, 1, 1)
    finally:
        ctx.close()


# ---- real scenes ----

def cam_of(c, w, h, target=None):
    from oracle import binding
    return binding.camera_uniforms(c["eye"], target or c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)


def one_spp(focal, frame):
    return S.ReferencePC(0, S.PC_FLAG_SKIP_HISTORY | S.PC_FLAG_ACCUMULATE | S.PC_FLAG_CLAMP_INDIRECT | S.PC_FLAG_IBL, frame, 1e-5, 1.0, focal, 3, 4)


def test_a_traced_scene_with_a_pan_equals_the_statement():
    """the quad-and-sky scene at 48 x 32 and 1 spp: G-buffer and velocity from prosper_pt_trace_gbuffer_velocity, every
    input NULL; frames 0 .. 2 with a still camera, 3 and 4 panning"""
    w, h = V.W, V.H
    pc, ref = both()
    look = dict(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=V.FOV, zN=0.1, zF=100.0)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(V.quad_world())
        before, previous = None, None
        for k in range(5):
            cam, focal = cam_of(look, w, h, target=(-0.06 * max(k - 2, 0), 0.0, -1.0))  # pans to the left
            if previous is not None:
                cam.previousWorldToCamera, cam.previousCameraToClip = previous.worldToCamera, previous.cameraToClip
            previous = cam
            ctx.trace_gbuffer_velocity(cam, w, h)
            ctx.render(one_spp(focal, 100 + k), cam, w, h)
            albedo, normal, depth = ctx.read_gbuffer()
            d = dict(illumination=ctx.read_hdr(), albedo=albedo, normal_metallic=normal, depth=depth, velocity=ctx.read_velocity())
            ctx.denoise(pc, cam, w, h)
            got = read_all(ctx, ref.iterations)
            assert got["info"].ignoredHistory == (1 if k == 0 else 0)
            check_call("quad frame %d" % k, ref, cam.cameraToClip.col[2].z, cam.cameraToClip.col[3].z, d, before, got)
            before = history_of(got)
            geometry, length = R.flag_of(got["guide_a"]), R.bits(got["moments"][..., 2])
            assert geometry.any() and (~geometry).any() and (got["guide_a"][..., 0][geometry] > 0).all()
            if k == 2:
                assert (length[geometry] == 3).all()
        # after the pan: reprojected texels and reset ones
        assert (length[geometry] > 1).any() and (length[geometry] == 1).any()
    finally:
        ctx.close()


def test_eight_noisy_frames_come_out_closer_to_the_converged_image_than_one():
    """Cornell at 96 x 64, eight 1-spp frames with a still camera against 2048 accumulated frames: over geometry pixels the
    luminance mean squared error of the denoised eighth frame must be lower than that of the raw eighth frame."""
    w, h = 96, 64
    world = scenes.cornell()
    cam, focal = cam_of(world.camera, w, h)
    pc, _ = both()
    ctx, reference = capi.Context(device=0), capi.Context(device=0)
    try:
        reference.upload_scene(world)
        reference.render(one_spp(focal, 1), cam, w, h, frames=2048)
        want = R.luminance(reference.read_hdr()[..., :3].astype(np.float64))
        ctx.upload_scene(world)
        raws = []
        for k in range(8):
            ctx.trace_gbuffer_velocity(cam, w, h)
            ctx.render(one_spp(focal, 3001 + k), cam, w, h)
            raws.append(ctx.read_hdr())
            ctx.denoise(pc, cam, w, h)
        out = ctx.read_hdr()
        geometry = ctx.read_gbuffer()[2] != 0
        assert geometry.sum() > w * h // 2 and np.isfinite(out[..., :3]).all()
        mse = lambda image: float(((R.luminance(image[..., :3].astype(np.float64)) - want)[geometry] ** 2).mean())
        denoised, raw, mean = mse(out), mse(raws[-1]), mse(np.mean(np.stack(raws).astype(np.float64), 0))
        print("denoise noise: mse denoised %.6g, raw 1 spp %.6g (ratio %.4f), mean of the 8 frames %.6g (ratio %.4f)" % (
            denoised, raw, denoised / raw, mean, denoised / mean))
        assert denoised < raw
        assert R.bits(ctx.read_denoise_stage(S.DENOISE_MOMENTS)[..., 2])[geometry].max() == 8
    finally:
        ctx.close()
        reference.close()


# ---- the chain ----

def test_the_passes_after_it_accept_the_image_and_the_passes_without_it_are_unchanged(gpu_ctx):
    ctx, cam = gpu_ctx, design_camera()
    w, h = 33, 17
    d = D.design(w, h, 0)
    d["illumination"] = np.nan_to_num(d["illumination"], nan=0.5, posinf=2.0, neginf=0.0)
    taa = S.TaaPC.default(1, S.TAA_CLIPPING_VARIANCE, S.TAA_VELOCITY_CENTER, 1, 1)
    g = np.linspace(0.0, 1.0, 8)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    ctx.set_tone_map_lut(dds.encode_r9g9b9e5(np.stack([r, gg, b], axis=-1)))  # an identity LUT

    def resolve_alone():
        ctx.taa_resolve(taa, w, h, d["velocity"], None, d["illumination"])
        return ctx.read_hdr().tobytes(), ctx.tone_map().tobytes()
    before = resolve_alone()
    call(ctx, both()[0], cam, w, h, d)
    denoised = ctx.read_hdr()
    toned = ctx.tone_map()
    assert toned.shape == (h, w, 4)
    with DeviceCopy(d["velocity"]) as ve:
        ctx.taa_resolve(taa, w, h, velocity_ptr=ve)  # in place over the denoised image
        resolved = ctx.read_hdr()
    assert np.isfinite(resolved).all()
    assert np.array_equal(resolved[..., :3], np.asarray(denoised[..., :3], np.float16).astype(np.float32))  # IGNORE_HISTORY: the rounded input
    assert resolve_alone() == before
