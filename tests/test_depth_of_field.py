"""Depth of field and the skybox fill on the GPU (prosper_pt_depth_of_field, prosper_pt_skybox_fill).

Each stage is checked against the numpy restatement (tests/dof_reference.py) fed with the GPU's own read-back of that
stage's inputs.  Flatten, dilate and filter are exact.  Setup, every reduce level and both gathers store fp16: a texel
passes when its code lies between the fp16 roundings of v - a and v + a, v the restatement's unrounded value and a the
allowance of tests/test_deferred_shading.py, relative 2e-4 of the texel's sum of absolute terms.  No texel is left out.
The CPU side and the design: tests/test_depth_of_field_cpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

import dof_reference as R
import gbuffer_sweep as G
import ibl_reference as I
from prosper_amd import capi, flight_helmet, scenes, structs as S
from test_depth_of_field_cpu import EXTENTS, dof_camera, dof_pc, reach_pc

pytestmark = pytest.mark.gpu

# (w, h, configuration): the banded design with maxBackgroundCoC 8 on every extent and 3 on the first, and the reach
# variant (wide bands, a gatherRadius of one tile: the outer buckets of rings 4 and 5) where tiles are three apart
CASES = [(w, h, "banded8") for w, h in EXTENTS] + [(100, 70, "banded3")] + [(w, h, "reach") for w, h in EXTENTS[:3]]
IDS = ["%dx%d-%s" % c for c in CASES]
_runs = {}


def case_inputs(oracle, w, h, config):
    cam = dof_camera(oracle, w, h)
    if config == "reach":
        return cam, reach_pc(), R.reach_design(cam, w, h)
    return cam, dof_pc(8.0 if config == "banded8" else 3.0), R.design(cam, w, h)


def read_back(ctx):
    info = ctx.dof_info()
    assert info.valid == 1
    rb = {"info": info, "mips": [ctx.read_dof_stage(S.DOF_HALF_ILLUMINATION, l) for l in range(info.mips)]}
    for name, stage in (("coc", S.DOF_HALF_COC), ("tiles", S.DOF_TILE_MIN_MAX), ("dilated", S.DOF_DILATED_TILE_MIN_MAX),
                        ("fg", S.DOF_FG_GATHER), ("bg", S.DOF_BG_GATHER), ("fg_filtered", S.DOF_FG_FILTERED),
                        ("bg_filtered", S.DOF_BG_FILTERED)):
        rb[name] = ctx.read_dof_stage(stage)
    rb["out"] = ctx.read_hdr()
    return rb


def run(ctx, oracle, w, h, config):
    """One depth-of-field call per case and session, with everything it left behind."""
    key = (w, h, config)
    if key not in _runs:
        cam, pc, (illum, depth) = case_inputs(oracle, w, h, config)
        ctx.depth_of_field(pc, cam, w, h, illum, depth)
        rb = read_back(ctx)
        rb.update(cam=cam, pc=pc, illum=illum, depth=depth)
        _runs[key] = rb
    return _runs[key]


def same_halves(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


def share(got, v, a):
    """The worst |got - v| as a share of the allowance (0 where both are exactly equal)."""
    err = np.abs(np.asarray(got, np.float64) - v)
    with np.errstate(all="ignore"):
        s = np.where(err == 0, 0.0, err / a)
    return float(np.nanmax(s)) if s.size else 0.0


def needed_share(got16, v, a):
    """The smallest allowance that lets every stored texel pass, as a share of the one it has: 0 where the code is the
    rounding of v itself, else how far v lies from the values that round to the stored code."""
    got = np.asarray(got16, np.float16)
    v = np.broadcast_to(np.asarray(v, np.float64), got.shape)
    a = np.broadcast_to(np.asarray(a, np.float64), got.shape)
    off = got != R.half(v)
    if not off.any():
        return 0.0
    g, vv = got[off], v[off]
    toward = np.nextafter(g, np.where(vv > g.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    need = np.abs(vv - 0.5 * (g.astype(np.float64) + toward.astype(np.float64)))
    with np.errstate(all="ignore"):
        return float(np.max(need / a[off]))


def check_half(name, got16, v, a):
    ok = R.within_half(got16, v, a)
    print("%s: needs %.3f of the allowance, %d of %d texels outside" % (name, needed_share(got16, v, a), (~ok).sum(), ok.size))
    assert ok.all(), name


def check_stages(rb, illum, depth, pc, cam, label):
    """Every stage of one call against the restatement over the read-back of that stage's inputs."""
    h, w = depth.shape
    hw, hh, tw, th, levels = R.extents(w, h)
    info = rb["info"]
    assert (info.width, info.height, info.halfWidth, info.halfHeight, info.tileWidth, info.tileHeight, info.mips) == (
        w, h, hw, hh, tw, th, levels)
    # setup
    s = R.setup(illum, depth, pc, cam)
    check_half(label + " setup colour", rb["mips"][0][..., :3], s["colour"], s["colour_a"])
    check_half(label + " setup coc", rb["coc"], s["coc"], s["coc_a"])
    assert (rb["mips"][0][..., 3] == 1).all()
    # reduce: every level from the stored level 0 (levels 1-6) or the stored level below (7 and up)
    for k in range(1, levels):
        v = R.reduce_level(k, rb["mips"][0], rb["mips"][k - 1])
        assert rb["mips"][k].shape[:2] == v.shape[:2]
        check_half(label + " reduce level %d" % k, rb["mips"][k][..., :3], v, R.REL * np.abs(v))
        assert (rb["mips"][k][..., 3] == 1).all()
    # flatten, dilate: exact
    assert same_halves(rb["tiles"], R.flatten(rb["coc"])), label + " flatten"
    assert same_halves(rb["dilated"], R.dilate(rb["tiles"], pc.gatherRadius)), label + " dilate"
    # gathers
    for name, background in (("fg", False), ("bg", True)):
        v, a = R.gather(rb["mips"], rb["coc"], rb["dilated"], background)
        check_half(label + " gather " + name, rb[name], v, a)
    # filter: exact
    assert same_halves(rb["fg_filtered"], R.median_filter(rb["fg"])), label + " filter fg"
    assert same_halves(rb["bg_filtered"], R.median_filter(rb["bg"])), label + " filter bg"
    # combine, the last row and column (where the clamp rule acts on even extents) included
    v, a = R.combine(illum, rb["coc"], rb["fg_filtered"], rb["bg_filtered"])
    err = np.abs(rb["out"][..., :3].astype(np.float64) - v)
    print("%s combine: worst error %.3f of the allowance" % (label, share(rb["out"][..., :3], v, a)))
    assert (err <= a).all(), label + " combine"
    assert np.array_equal(rb["out"][..., 3].view(np.uint32), np.ascontiguousarray(illum[..., 3]).view(np.uint32))


@pytest.mark.parametrize("w,h,config", CASES, ids=IDS)
def test_every_stage_equals_the_restatement_over_its_read_back_inputs(gpu_ctx, oracle, w, h, config):
    rb = run(gpu_ctx, oracle, w, h, config)
    check_stages(rb, rb["illum"], rb["depth"], rb["pc"], rb["cam"], "%dx%d %s" % (w, h, config))


def test_reduce_levels_past_seven_read_the_stored_level_below(gpu_ctx, oracle):
    """514 x 6: half width 257, nine levels: level 7 reads the stored level 6, level 8 the stored level 7, each clamped to
    its own extent (2 x 1 and 1 x 1 texels)."""
    w, h = 514, 6
    cam, pc, (illum, depth) = case_inputs(oracle, w, h, "banded8")
    gpu_ctx.depth_of_field(pc, cam, w, h, illum, depth)
    rb = read_back(gpu_ctx)
    assert rb["info"].mips == 9 and rb["mips"][7].shape == (1, 2, 4) and rb["mips"][8].shape == (1, 1, 4)
    check_stages(rb, illum, depth, pc, cam, "514x6")


def test_two_calls_give_the_same_bytes(gpu_ctx, oracle):
    first = run(gpu_ctx, oracle, 100, 70, "banded8")
    cam, pc, (illum, depth) = case_inputs(oracle, 100, 70, "banded8")
    gpu_ctx.depth_of_field(pc, cam, 100, 70, illum, depth)
    again = read_back(gpu_ctx)
    for name in ("coc", "tiles", "dilated", "fg", "bg", "fg_filtered", "bg_filtered", "out"):
        assert first[name].tobytes() == again[name].tobytes(), name
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first["mips"], again["mips"]))


@pytest.mark.parametrize("w,h", EXTENTS)
def test_every_depth_at_focus_leaves_the_image_bit_identical(gpu_ctx, oracle, w, h):
    cam = dof_camera(oracle, w, h)
    illum, depth = R.design(cam, w, h, depths=(R.FOCUS,))
    gpu_ctx.depth_of_field(dof_pc(8.0), cam, w, h, illum, depth)
    assert gpu_ctx.read_hdr().tobytes() == illum.tobytes()
    assert not gpu_ctx.read_dof_stage(S.DOF_FG_GATHER).any() and not gpu_ctx.read_dof_stage(S.DOF_BG_GATHER).any()


def test_a_constant_colour_stays_constant(gpu_ctx, oracle):
    """... but for the pixels whose foreground upscale averages an empty texel in (dof_reference.constant_colour_bounds)."""
    w, h = 100, 70
    cam = dof_camera(oracle, w, h)
    colour = np.array([0.75, 2.5, 0.125])
    illum, depth = R.design(cam, w, h, constant=colour)
    gpu_ctx.depth_of_field(dof_pc(8.0), cam, w, h, illum, depth)
    out = gpu_ctx.read_hdr()[..., :3].astype(np.float64)
    lo, hi = R.constant_colour_bounds(colour, h, w, gpu_ctx.read_dof_stage(S.DOF_FG_FILTERED))
    assert ((out >= lo) & (out <= hi)).all()
    for stage in (S.DOF_FG_GATHER, S.DOF_BG_GATHER):
        layer = gpu_ctx.read_dof_stage(stage)
        used = layer[..., :3].any(axis=-1)
        assert used.any() and (layer[used][:, :3].astype(np.float64) == colour).all()


class DeviceCopy:
    """A host array in device memory for the length of a `with` block."""
    hip = None

    def __init__(self, array):
        if DeviceCopy.hip is None:
            DeviceCopy.hip = C.CDLL("libamdhip64.so")
        self.array = np.ascontiguousarray(array)
        self.ptr = C.c_void_p()

    def __enter__(self):
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.array.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, C.c_void_p(self.array.ctypes.data), C.c_size_t(self.array.nbytes), 1) == 0
        return self.ptr.value

    def __exit__(self, *exc):
        self.hip.hipDeviceSynchronize()
        self.hip.hipFree(self.ptr)


def test_in_place_and_device_inputs_equal_the_host_call(gpu_ctx, oracle):
    w, h = 100, 70
    want = run(gpu_ctx, oracle, w, h, "banded8")
    cam, pc, illum, depth = want["cam"], want["pc"], want["illum"], want["depth"]
    # device inputs
    with DeviceCopy(illum) as il, DeviceCopy(depth) as dp:
        gpu_ctx.depth_of_field(pc, cam, w, h, illumination_ptr=il, depth_ptr=dp)
        assert gpu_ctx.read_hdr().tobytes() == want["out"].tobytes()
    # in place: every depth at focus first puts the input itself into the HDR image
    _, focus_depth = R.design(cam, w, h, depths=(R.FOCUS,))
    gpu_ctx.depth_of_field(pc, cam, w, h, illum, focus_depth)
    assert gpu_ctx.read_hdr().tobytes() == illum.tobytes()
    gpu_ctx.depth_of_field(pc, cam, w, h, depth=depth)
    assert gpu_ctx.read_hdr().tobytes() == want["out"].tobytes()
    # ... and with the HDR image passed explicitly
    gpu_ctx.depth_of_field(pc, cam, w, h, illum, focus_depth)
    with DeviceCopy(depth) as dp:
        gpu_ctx.depth_of_field(pc, cam, w, h, illumination_ptr=gpu_ctx.hdr_device_ptr()[0], depth_ptr=dp)
        assert gpu_ctx.read_hdr().tobytes() == want["out"].tobytes()


def test_bad_arguments_are_refused_without_a_launch(gpu_ctx, oracle):
    w, h = 100, 70
    want = run(gpu_ctx, oracle, w, h, "banded8")
    cam, pc, illum, depth = want["cam"], want["pc"], want["illum"], want["depth"]
    gpu_ctx.depth_of_field(pc, cam, w, h, illum, depth)
    before = read_back(gpu_ctx)

    def refused(words, call):
        with pytest.raises(capi.ProsperPtError) as e:
            call()
        assert words in str(e.value), str(e.value)

    small = np.zeros((35, 50), np.float32)
    refused("another extent", lambda: gpu_ctx.depth_of_field(pc, dof_camera(oracle, 50, 35), 50, 35, depth=small))
    for bad, words in ((S.DofPC(np.nan, 8, 16, 2), "non-finite"), (S.DofPC(0, 8, 16, 2), "focusDistance"),
                       (S.DofPC(2, -8, 16, 2), "negative"), (S.DofPC(2, 8, 16, 0), "gatherRadius")):
        refused(words, lambda: gpu_ctx.depth_of_field(bad, cam, w, h, illum, depth))
    lib, buf = capi.lib(), np.zeros(16, np.uint8)
    assert lib.prosper_pt_read_dof_stage(gpu_ctx._h, S.DOF_HALF_COC, 0, buf.ctypes.data, 16, None) == -1
    assert lib.prosper_pt_read_dof_stage(gpu_ctx._h, S.DOF_HALF_ILLUMINATION, 99, buf.ctypes.data, 16, None) == -1
    after = read_back(gpu_ctx)
    assert all(before[k].tobytes() == after[k].tobytes() for k in ("coc", "dilated", "fg", "bg", "out"))


# ---- skybox fill ----

def fill_check(ctx, cam, world, w, h, depth, label):
    """After a fill over `depth`: miss texels hold the sky within the allowance, hit texels are bit-unchanged."""
    before = ctx.read_hdr()
    if depth is None:
        ctx.skybox_fill(cam, w, h)
        depth = ctx.read_gbuffer()[2]
    else:
        ctx.skybox_fill(cam, w, h, depth=depth)
    after = ctx.read_hdr()
    miss = depth == 0
    assert np.array_equal(after[~miss].view(np.uint32), before[~miss].view(np.uint32)), label
    if world.skybox is None:
        assert (after[miss] == np.array([0, 0, 0, 1], np.float32)).all(), label
        return int(miss.sum())
    want = I.sample_cube(I.sky64(world), R.sky_directions(cam, w, h)[miss])
    got = after[miss]
    err = np.abs(got[:, :3].astype(np.float64) - want)
    print("%s: %d miss texels, worst error %.3f of the allowance" % (label, miss.sum(), share(got[:, :3], want, R.REL * np.abs(want))))
    assert (err <= R.REL * np.abs(want)).all() and (got[:, 3] == 1).all(), label
    return int(miss.sum())


def checker_depth(w, h):
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.where(((xs // 3) + (ys // 2)) % 2 == 0, 0.0, 0.25).astype(np.float32)


@pytest.mark.parametrize("sky", ["cornell", "sweep", "none"])
def test_skybox_fill(oracle, sky):
    world = {"cornell": lambda: scenes.cornell(with_skybox=True), "sweep": G.ibl_world, "none": scenes.cornell}[sky]()
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        for w, h in ((100, 70), (17, 9)):
            c = world.camera
            cam, _ = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)
            ctx.deferred_shading_traced(cam, w, h)
            # the last traced G-buffer's depth, then a checkerboard of misses over the same image
            fill_check(ctx, cam, world, w, h, None, "%s %dx%d traced" % (sky, w, h))
            assert fill_check(ctx, cam, world, w, h, checker_depth(w, h), "%s %dx%d checker" % (sky, w, h)) > w * h // 3
        # a NULL depth whose G-buffer has another extent than the image
        ctx.trace_gbuffer(cam, 16, 8, jitter=False)
        with pytest.raises(capi.ProsperPtError) as e:
            ctx.skybox_fill(cam, w, h)
        assert "the last traced G-buffer has another extent" in str(e.value)
        # an image of another extent
        for bad in (lambda: ctx.skybox_fill(cam, 16, 8), lambda: ctx.skybox_fill(cam, 16, 8, depth=np.zeros((8, 16), np.float32))):
            with pytest.raises(capi.ProsperPtError) as e:
                bad()
            assert "another extent" in str(e.value)
    finally:
        ctx.close()


def test_skybox_fill_takes_a_device_depth_like_a_host_one(oracle):
    """The caller's depth as a device pointer gives, bit for bit, the image the same depth gives as a host array."""
    w, h = 50, 35
    world = scenes.cornell(with_skybox=True)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        c = world.camera
        cam, _ = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)
        depth = checker_depth(w, h)
        ctx.deferred_shading_traced(cam, w, h)
        before = ctx.read_hdr()
        ctx.skybox_fill(cam, w, h, depth=depth)
        host = ctx.read_hdr()
        ctx.deferred_shading_traced(cam, w, h)  # the same image again under the second fill
        assert ctx.read_hdr().tobytes() == before.tobytes()
        with DeviceCopy(depth) as dp:
            ctx.skybox_fill(cam, w, h, depth_ptr=dp)
            device = ctx.read_hdr()
        assert host.tobytes() != before.tobytes()  # (the fill wrote the misses)
        assert device.tobytes() == host.tobytes()
    finally:
        ctx.close()


# ---- end to end ----

def hand_pc(hcam, w):
    """The push constants from dof/Setup.cpp's and dof/Dilate.cpp's formulas, in float32."""
    f = np.float32
    hw = (w + 1) // 2
    units = (f(hcam.aperture) * f(hcam.focal_length)) / (f(hcam.focus) - f(hcam.focal_length))
    max_bg = (units / f(0.035)) * f(hw)
    in_tiles = math.ceil(float((units / f(0.035)) * f((hw + 7) // 8)))
    return S.DofPC(hcam.focus, float(max_bg), float(max_bg * f(2)), max(in_tiles * 2, 1))


def test_flight_helmet_end_to_end_and_the_host_mirrors(oracle):
    from prosper_amd.rt_reference import Camera, DeferredShading, DepthOfField, GBufferTracer, SkyboxRenderer
    w, h = 160, 96
    world = flight_helmet.load_fixture(sky_size=16)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        c = world.camera
        hcam = Camera()
        hcam.look_at(c["eye"], c["target"], c["up"])
        hcam.update_resolution(w, h)
        hcam.set_parameters(c["fov"], c["zN"], c["zF"])
        _, focal = hcam.update_buffer()
        # an aperture that gives the far background a circle of 6 half-resolution texels, focused on the helmet
        focus = float(np.linalg.norm(np.asarray(c["eye"], np.float64) - np.asarray(c["target"], np.float64)))
        aperture = 6.0 / ((w + 1) // 2) * 0.035 * (focus - focal) / focal
        hcam.set_parameters(c["fov"], c["zN"], c["zF"], aperture, focus)
        cam, focal = hcam.update_buffer()
        hcam.aperture, hcam.focus, hcam.focal_length = aperture, focus, focal
        pc = hand_pc(hcam, w)
        assert 5.9 < pc.maxBackgroundCoC < 6.1 and pc.gatherRadius == 2

        # direct calls: trace, shade, fill, depth of field in place over the traced depth
        ctx.deferred_shading_traced(cam, w, h)
        ctx.skybox_fill(cam, w, h)
        illum, depth = ctx.read_hdr(), ctx.read_gbuffer()[2]
        assert 0.05 < (depth == 0).mean() < 0.95
        ctx.depth_of_field(pc, cam, w, h)
        rb = read_back(ctx)
        check_stages(rb, illum, depth, pc, cam, "flight helmet %dx%d" % (w, h))
        both = (rb["fg"][..., 3] > 0).mean(), rb["bg"][..., :3].any(axis=-1).mean()
        print("flight helmet: foreground weight on %.0f %%, background colour on %.0f %% of the half-resolution texels" % (
            100 * both[0], 100 * both[1]))
        assert both[1] > 0.02  # (the sky behind the helmet: its circle is nearly the largest)

        # the mirrors
        gb = GBufferTracer(ctx).record(hcam, w, h, jitter=False)
        DeferredShading(ctx).record_device(hcam, gb, w, h)
        SkyboxRenderer(ctx).record(hcam, w, h)
        assert ctx.read_hdr().tobytes() == illum.tobytes()
        got = DepthOfField(ctx).record(hcam, w, h)
        assert bytes(got) == bytes(pc)
        assert ctx.read_hdr().tobytes() == rb["out"].tobytes()
        # ... and over host arrays
        got = DepthOfField(ctx).record(hcam, w, h, illum, depth)
        assert bytes(got) == bytes(pc) and ctx.read_hdr().tobytes() == rb["out"].tobytes()
    finally:
        ctx.close()
