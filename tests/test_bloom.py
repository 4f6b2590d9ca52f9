"""Bloom on the GPU (prosper_pt_bloom).

Each stage is checked against the numpy restatement (tests/bloom_reference.py) fed with the GPU's own read-back of that
stage's inputs: separate over the input image, reduce level k over the stored level 0, the horizontal blur over
`highlights`, the vertical one over `horizontal`, compose over the input and the stored levels.  Every working image is
fp16: a texel passes when its code lies between the fp16 roundings of v - a and v + a, v the restatement's unrounded
value and a the allowance of tests/test_deferred_shading.py, relative 2e-4 of the texel's sum of absolute terms; compose
passes within a in float32.  No texel is left out.

Extents, the smallest at which each rule can go wrong.  Half: 8 x 8 (the minimum, level 3 is 1 x 1), 17 x 9, 101 x 71
(odd: compose's res differs from the level size, the streak's fractions vary), 130 x 33 (crosses a 64-wide reduce tile),
258 x 20 (streak half-width 32 on a 10-row image), 2100 x 8 (a level-0 row of 1050 texels and 524 streak taps: three
staged pieces).  Quarter: 32 x 32 (the minimum), 100 x 70, 258 x 36.  Biquadratic sampling on all of them, bilinear on
101 x 71 and 100 x 70.  The CPU side and the design: tests/test_bloom_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import bloom_reference as R
from prosper_amd import capi, flight_helmet, structs as S
from test_bloom_cpu import CASES, SEED
from test_depth_of_field import DeviceCopy, check_half, share

pytestmark = pytest.mark.gpu

IDS = ["%dx%d-%s-%s" % (w, h, "half" if s == R.HALF else "quarter", "biquadratic" if b else "bilinear") for w, h, s, b in CASES]
WORKING = ((S.BLOOM_HIGHLIGHTS, "highlights"), (S.BLOOM_HORIZONTAL, "horizontal"), (S.BLOOM_BLURRED, "blurred"))
_runs = {}


def default_pc(scale=R.HALF, biquadratic=1, threshold=R.THRESHOLD, blend=R.DEFAULT_BLEND):
    return S.BloomPC.default(threshold, blend, scale, biquadratic)


def read_back(ctx):
    info = ctx.bloom_info()
    assert info.valid == 1
    blurred_levels = range(info.firstLevel, info.firstLevel + 3)
    rb = {"info": info, "highlights": {l: ctx.read_bloom_stage(S.BLOOM_HIGHLIGHTS, l) for l in range(R.LEVELS)},
          "horizontal": {l: ctx.read_bloom_stage(S.BLOOM_HORIZONTAL, l) for l in blurred_levels},
          "blurred": {l: ctx.read_bloom_stage(S.BLOOM_BLURRED, l) for l in blurred_levels}}
    rb["out"] = ctx.read_hdr()
    return rb


def run(ctx, w, h, scale, biquadratic):
    """One bloom call per case and session, with everything it left behind."""
    key = (w, h, scale, biquadratic)
    if key not in _runs:
        illum, pc = R.design(w, h, SEED), default_pc(scale, biquadratic)
        ctx.bloom(pc, w, h, illum)
        rb = read_back(ctx)
        rb.update(pc=pc, illum=illum)
        _runs[key] = rb
    return _runs[key]


def same_bytes(a, b):
    return all(a[name][l].tobytes() == b[name][l].tobytes() for _, name in WORKING for l in a[name]) and (
        a["out"].tobytes() == b["out"].tobytes())


def check_stages(ctx, rb, illum, pc, label):
    """Every stage of one call against the restatement over the read-back of that stage's inputs."""
    h, w = illum.shape[:2]
    scale, first = pc.resolutionScale, R.first_level(pc.resolutionScale)
    ww, wh = R.working_extent(w, h, scale)
    info = rb["info"]
    assert (info.width, info.height, info.workingWidth, info.workingHeight, info.firstLevel, info.streakHalfWidth) == (
        w, h, ww, wh, first, R.streak_half_width(ww))
    times = [info.separateMs, info.reduceMs, info.composeMs] + list(info.blurHorizontalMs) + list(info.blurVerticalMs)
    assert all(np.isfinite(t) and t >= 0 for t in times)
    hl, hz, bl = rb["highlights"], rb["horizontal"], rb["blurred"]
    for l in range(R.LEVELS):
        lw, lh = R.level_extent(ww, wh, l)
        assert hl[l].shape == (lh, lw, 4) and (hl[l][..., 3] == 0).all()
    assert sorted(hz) == sorted(bl) == [first, first + 1, first + 2]
    # a level the blur passes did not write is refused
    buf = np.zeros(8, np.uint8)
    for stage in (S.BLOOM_HORIZONTAL, S.BLOOM_BLURRED):
        for l in set(range(R.LEVELS + 1)) - set(hz):
            assert capi.lib().prosper_pt_read_bloom_stage(ctx._h, stage, l, buf.ctypes.data, 8, None) == -1
    assert capi.lib().prosper_pt_read_bloom_stage(ctx._h, S.BLOOM_HIGHLIGHTS, R.LEVELS, buf.ctypes.data, 8, None) == -1
    # separate
    v, s = R.separate(illum, pc.threshold, scale)
    check_half(label + " separate", hl[0][..., :3], v, R.REL * s)
    # reduce: every level from the stored level 0
    for k in range(1, R.LEVELS):
        v, s = R.reduce_level(k, hl[0])
        check_half(label + " reduce level %d" % k, hl[k][..., :3], v, R.REL * s)
    # blur
    for l in range(first, first + 3):
        lw, lh = R.level_extent(ww, wh, l)
        assert hz[l].shape == bl[l].shape == (lh, lw, 4) and (hz[l][..., 3] == 1).all() and (bl[l][..., 3] == 1).all()
        v, s = R.blur_pass(hl[l], False, hl[0] if l == 1 else None)[:2]
        check_half(label + " horizontal level %d%s" % (l, " (streak)" if l == 1 else ""), hz[l][..., :3], v, R.REL * s)
        v, s = R.blur_pass(hz[l], True)[:2]
        check_half(label + " vertical level %d" % l, bl[l][..., :3], v, R.REL * s)
    # compose
    read = [bl[l] if l in bl else hl[l] for l in range(3)]
    v, s, _ = R.compose(illum, read, list(pc.blendFactors), scale, pc.biquadratic)
    a = R.REL * s
    err = np.abs(rb["out"][..., :3].astype(np.float64) - v)
    print("%s compose: worst error %.3f of the allowance" % (label, share(rb["out"][..., :3], v, a)))
    assert (err <= a).all(), label + " compose"
    assert (rb["out"][..., 3] == 1).all()


@pytest.mark.parametrize("w,h,scale,biquadratic", CASES, ids=IDS)
def test_every_stage_equals_the_restatement_over_its_read_back_inputs(gpu_ctx, w, h, scale, biquadratic):
    rb = run(gpu_ctx, w, h, scale, biquadratic)
    check_stages(gpu_ctx, rb, rb["illum"], rb["pc"], IDS[CASES.index((w, h, scale, biquadratic))])


def test_two_calls_give_the_same_bytes(gpu_ctx):
    for key in ((101, 71, R.HALF, 1), (258, 36, R.QUARTER, 1)):
        first = run(gpu_ctx, *key)
        gpu_ctx.bloom(first["pc"], key[0], key[1], first["illum"])
        assert same_bytes(first, read_back(gpu_ctx)), key


@pytest.mark.parametrize("scale", [R.HALF, R.QUARTER])
def test_nothing_above_the_threshold_and_zero_blend_factors_return_the_input(gpu_ctx, scale):
    w, h = 101, 71
    illum = R.design(w, h, SEED)
    want = illum.copy()
    want[..., 3] = 1.0
    # the threshold above everything the image holds
    gpu_ctx.bloom(default_pc(scale, threshold=float(illum[..., :3].max()) + 1.0), w, h, illum)
    assert gpu_ctx.read_hdr().tobytes() == want.tobytes()
    assert not any(gpu_ctx.read_bloom_stage(S.BLOOM_HIGHLIGHTS, l).any() for l in range(R.LEVELS))
    # highlights, but nothing of them blended in
    gpu_ctx.bloom(default_pc(scale, blend=(0.0, 0.0, 0.0)), w, h, illum)
    assert gpu_ctx.read_hdr().tobytes() == want.tobytes()
    assert gpu_ctx.read_bloom_stage(S.BLOOM_BLURRED, 1).any()


def test_in_place_and_device_inputs_equal_the_host_call(gpu_ctx):
    w, h = 101, 71
    want = run(gpu_ctx, w, h, R.HALF, 1)
    pc, illum = want["pc"], want["illum"]
    with DeviceCopy(illum) as il:
        gpu_ctx.bloom(pc, w, h, illumination_ptr=il)
        assert same_bytes(want, read_back(gpu_ctx))
    # in place: zero blend factors first put the input's rgb into the HDR image (alpha 1, which bloom does not read)
    gpu_ctx.bloom(default_pc(blend=(0.0, 0.0, 0.0)), w, h, illum)
    gpu_ctx.bloom(pc, w, h)
    assert same_bytes(want, read_back(gpu_ctx))
    # ... and with the HDR image passed explicitly
    gpu_ctx.bloom(default_pc(blend=(0.0, 0.0, 0.0)), w, h, illum)
    gpu_ctx.bloom(pc, w, h, illumination_ptr=gpu_ctx.hdr_device_ptr()[0])
    assert same_bytes(want, read_back(gpu_ctx))


def test_bad_arguments_are_refused_and_change_nothing(gpu_ctx):
    w, h = 101, 71
    want = run(gpu_ctx, w, h, R.HALF, 1)
    pc, illum = want["pc"], want["illum"]
    gpu_ctx.bloom(pc, w, h, illum)
    before, info_before = read_back(gpu_ctx), bytes(gpu_ctx.bloom_info())
    lib = capi.lib()

    def refused(words, call):
        with pytest.raises(capi.ProsperPtError) as e:
            call()
        assert e.value.code == -1 and words in str(e.value), str(e.value)

    assert lib.prosper_pt_bloom(gpu_ctx._h, None, w, h, illum.ctypes.data, 0, None) == -1
    reserved = default_pc()
    reserved.reserved[0] = 7
    for bad, words in ((default_pc(threshold=np.nan), "non-finite"), (default_pc(blend=(0.9, np.inf, 0.04)), "non-finite"),
                       (default_pc(threshold=-0.5), "negative"), (default_pc(blend=(-0.9, 0.04, 0.04)), "negative"),
                       (default_pc(scale=2), "unknown resolution scale"), (reserved, "reserved")):
        refused(words, lambda: gpu_ctx.bloom(bad, w, h, illum))
    refused("empty extent", lambda: gpu_ctx.bloom(pc, 0, h, illumination_ptr=gpu_ctx.hdr_device_ptr()[0]))
    refused("another extent", lambda: gpu_ctx.bloom(pc, 64, 48))
    small = np.ones((32, 32, 4), np.float32)
    refused("blurred level empty", lambda: gpu_ctx.bloom(pc, 7, 8, small[:8, :7]))
    refused("blurred level empty", lambda: gpu_ctx.bloom(pc, 8, 7, small[:7, :8]))
    refused("blurred level empty", lambda: gpu_ctx.bloom(default_pc(R.QUARTER), 31, 32, small[:, :31]))
    refused("blurred level empty", lambda: gpu_ctx.bloom(default_pc(R.QUARTER), 32, 31, small[:31]))
    assert same_bytes(before, read_back(gpu_ctx)) and bytes(gpu_ctx.bloom_info()) == info_before
    # the smallest extents are not refused
    gpu_ctx.bloom(pc, 8, 8, small[:8, :8])
    gpu_ctx.bloom(default_pc(R.QUARTER), 32, 32, small)
    assert gpu_ctx.bloom_info().workingWidth == 8


def test_the_mirrors_with_defaults_equal_a_direct_call(gpu_ctx):
    from prosper_amd.rt_reference import Bloom
    w, h = 101, 71
    want = run(gpu_ctx, w, h, R.HALF, 1)  # the direct call with {1, {.9, .04, .04}, Half, biquadratic}
    direct = S.BloomPC(1.0, (C.c_float * 3)(0.9, 0.04, 0.04), 0, 1, (C.c_uint32 * 2)(0, 0))
    assert bytes(want["pc"]) == bytes(direct)
    bloom = Bloom(gpu_ctx)
    try:
        got = bloom.record(w, h, want["illum"])
        assert bytes(got) == bytes(direct) and same_bytes(want, read_back(gpu_ctx))
        # the setters reach the push constants
        bloom.draw_ui(threshold=1.0, blend_factors=R.DEFAULT_BLEND, biquadratic=False, resolution_scale=S.BLOOM_QUARTER)
        quarter = run(gpu_ctx, 100, 70, R.QUARTER, 0)
        got = bloom.record(100, 70, quarter["illum"])
        assert (got.resolutionScale, got.biquadratic) == (1, 0)
        assert same_bytes(quarter, read_back(gpu_ctx))
    finally:
        bloom.close()


def test_flight_helmet_from_trace_to_tone_map(oracle):
    from prosper_amd import dds
    from prosper_amd.rt_reference import Bloom, Camera, DepthOfField
    w, h = 160, 96
    world = flight_helmet.load_fixture(sky_size=16)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        c = world.camera
        hcam = Camera.from_world(world, w, h)
        focus = float(np.linalg.norm(np.asarray(c["eye"], np.float64) - np.asarray(c["target"], np.float64)))
        hcam.set_parameters(c["fov"], c["zN"], c["zF"], 0.02, focus)
        cam, _ = hcam.update_buffer()
        ctx.deferred_shading_traced(cam, w, h)
        ctx.skybox_fill(cam, w, h)
        illum = ctx.read_hdr()
        assert np.isfinite(illum).all()
        # a threshold that leaves highlights on about a third of the image
        threshold = float(np.quantile(illum[..., :3].max(axis=-1), 0.65))
        bloom = Bloom(ctx)
        bloom.draw_ui(threshold=threshold)
        pc = bloom.record(w, h)  # in place
        rb = read_back(ctx)
        lit = rb["highlights"][0][..., :3].any(axis=-1).mean()
        print("flight helmet: threshold %.4f, highlights on %.0f %% of level 0" % (threshold, 100 * lit))
        assert 0.1 < lit < 0.6
        check_stages(ctx, rb, illum, pc, "flight helmet %dx%d" % (w, h))
        added = rb["out"][..., :3].astype(np.float64) - illum[..., :3]
        assert (added >= 0).all() and (added > 0).mean() > 0.1
        DepthOfField(ctx).record(hcam, w, h)
        after_dof = ctx.read_hdr()
        assert np.isfinite(after_dof).all() and (after_dof[..., 3] == 1).all()
        g = np.linspace(0.0, 1.0, 16)
        b, gg, r = np.meshgrid(g, g, g, indexing="ij")
        ctx.set_tone_map_lut(dds.encode_r9g9b9e5(np.stack([r, gg, b], axis=-1)))
        ldr = ctx.tone_map()
        assert ldr.shape == (h, w, 4) and (ldr[..., 3] == 255).all() and ldr[..., :3].any()
        bloom.close()
    finally:
        ctx.close()
