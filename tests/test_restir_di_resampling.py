"""ReSTIR-DI initial reservoirs and spatial reuse (res/shader/restir_di/{initial_reservoirs,spatial_reuse}.comp) and the
record that chains them with the trace (src/render/rtdi/RtDirectIllumination.cpp:70-115): the C-ABI surface on the
CPU, and with -m gpu the HIP kernels against tests/restir_resampling_reference.py, the chain bit for bit against the
oracle's trace, and the unbiasedness of the initial pass."""
import ctypes as C

import numpy as np
import pytest

import restir_resampling_reference as R
from conftest import same_bits
from prosper_amd import capi, scenes, structs as S

FLAG_SKIP_HISTORY, FLAG_ACCUMULATE = 1, 2
W, H = 160, 96
NEW_SYMBOLS = ("prosper_pt_restir_di_resample", "prosper_pt_restir_di_record",
               "prosper_pt_get_restir_reservoirs_device_ptr", "prosper_pt_read_restir_reservoirs",
               "prosper_host_rt_direct_illumination_create", "prosper_host_rt_direct_illumination_destroy",
               "prosper_host_rt_direct_illumination_draw_ui", "prosper_host_rt_direct_illumination_record",
               "prosper_host_rt_direct_illumination_recompile_shaders",
               "prosper_host_rt_direct_illumination_release_preserved")


def make_world(scene, point_lights=None):
    if scene == "cornell":
        return scenes.cornell()
    world = scenes.sponza_class(lights=True, foliage=True, texture_size=64, sky_size=32, detail=0.25)
    if point_lights is not None:
        world.point_lights.count = point_lights
    return world


def index_of(res):
    return np.ascontiguousarray(res[..., 0]).view(np.int32)


class DeviceBuffer:
    """Device memory through the HIP runtime the library runs on (hipMalloc / hipMemcpy on the null stream)."""

    def __init__(self, host=None, nbytes=None):
        self.hip = hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        self.nbytes = host.nbytes if host is not None else nbytes
        self.ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.ptr), self.nbytes) == 0
        if host is not None:
            host = np.ascontiguousarray(host)
            assert hip.hipMemcpy(self.ptr, host.ctypes.data, self.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def read(self, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        assert out.nbytes == self.nbytes and self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = C.c_void_p()


def pack(index, weight):
    return np.stack([np.ascontiguousarray(index, np.int32).view(np.float32), weight.astype(np.float32)], axis=-1)


# ---- CPU ----

def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    assert (S.RESTIR_INITIAL, S.RESTIR_SPATIAL, S.RESTIR_SPATIAL_REUSE) == (0, 1, 1)


def test_bad_arguments_are_rejected_before_touching_the_gpu():
    lib = capi.lib()
    cam = S.CameraUniforms()
    inp = S.RestirInputs(None, None, None, None, 0, 0)
    pc = S.RestirTracePC(0, 1, 1)
    assert lib.prosper_pt_restir_di_resample(None, 0, 1, C.byref(cam), 4, 4, C.byref(inp), None, None) == -1
    assert lib.prosper_pt_restir_di_resample(None, 0, 1, None, 4, 4, None, None, None) == -1
    assert lib.prosper_pt_restir_di_record(None, C.byref(pc), 1, C.byref(cam), 4, 4, C.byref(inp), None) == -1
    assert lib.prosper_pt_restir_di_record(None, None, 0, None, 4, 4, None, None) == -1
    ptr, n = C.c_void_p(), C.c_size_t()
    assert lib.prosper_pt_get_restir_reservoirs_device_ptr(None, C.byref(ptr), C.byref(n)) == -1
    assert lib.prosper_pt_read_restir_reservoirs(None, None, 0, None) == -1
    h = C.c_void_p()
    assert lib.prosper_host_rt_direct_illumination_create(None, C.byref(h)) == -1 and not h.value


def test_reference_rng_matches_the_oracle_bit_for_bit(oracle):
    """pcg3d / rnd01 / rnd2d01 of the NumPy restatement against eval_fn(PROSPER_PT_FN_RNG), the hook pinned to the
    device: one rnd01 then one rnd2d01 from uvec3(px, py, frame)."""
    rng = np.random.default_rng(5)
    seeds = rng.integers(0, 2 ** 32, size=(4096, 3), dtype=np.uint64).astype(np.uint32)
    seeds[:4] = [[0, 0, 0], [1, 2, 3], [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], [1919, 1079, 4095]]
    want = oracle.eval_fn("RNG", seeds.view(np.float32))
    r = R.Rng(seeds[:, 0], seeds[:, 1], 0)
    r.s[2] = seeds[:, 2].copy()
    a = r.rnd01()
    b0, b1 = r.rnd2d01()
    assert same_bits(a, want[:, 0]).all() and same_bits(b0, want[:, 1]).all() and same_bits(b1, want[:, 2]).all()
    # the candidate pick never leaves [0, lightCount) even for rnd01() == 1 (float(0xFFFFFFFF) rounds to 2^32)
    assert R.rng_to_01(np.array([0xFFFFFFFF], np.uint32))[0] == 1.0


# ---- GPU ----

def _gbuffer(oracle, world):
    return R.make_gbuffer(oracle, world, W, H)


def _check_against_reference(got, want_idx, want_w, margin, lights):
    idx = index_of(got)
    weight = got[..., 1]
    assert np.isfinite(weight).all() and (weight >= 0).all()
    assert ((idx >= -1) & (idx < lights)).all()
    decided = margin >= 1e-4
    assert decided.mean() >= 0.99, "only %.4f of the pixels decided" % decided.mean()
    bad = decided & (idx != want_idx)
    assert not bad.any(), "%d decided pixels pick another light" % bad.sum()
    same = idx == want_idx
    with np.errstate(all="ignore"):
        rel = np.abs(weight.astype(np.float64) - want_w) / np.maximum(np.abs(want_w), 1e-30)
    wrong = same & decided & (rel > 1e-4)
    assert not wrong.any(), "%d pixels: W off by up to %.3g" % (wrong.sum(), rel[wrong].max())
    assert (idx >= 0).mean() > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "sponza_small"])
def test_gpu_resampling_passes_match_the_reference(gpu_ctx, oracle, scene):
    world = make_world(scene)
    cam, fl, osc, ar, nm, depth, _ = _gbuffer(oracle, world)
    gpu_ctx.upload_scene(world)
    lights = R.Lights(world).count
    for frame in (1, 2, 3):
        ref_i, ref_w, ref_m = R.initial(world, cam, ar, nm, depth, frame)
        got = gpu_ctx.restir_di_resample(S.RESTIR_INITIAL, frame, cam, ar, nm, depth)
        _check_against_reference(got, ref_i, ref_w, ref_m, lights)
        # the spatial pass is fed the REFERENCE's initial reservoirs: an error of one pass cannot hide in the other
        ref_res = pack(ref_i, ref_w)
        sp_i, sp_w, sp_m, _ = R.spatial(world, cam, ar, nm, depth, ref_res, frame, oracle)
        got_sp = gpu_ctx.restir_di_resample(S.RESTIR_SPATIAL, frame, cam, ar, nm, depth, ref_res)
        _check_against_reference(got_sp, sp_i, sp_w, sp_m, lights)
        # every light the spatial pass picks is one its offsets can reach: the radius-60 disc around (-30, -30),
        # rows and columns > 0
        chosen = index_of(got_sp)
        rng = np.random.default_rng(frame)
        ys, xs = np.nonzero(chosen >= 0)
        for k in rng.choice(len(ys), size=min(len(ys), 1500), replace=False):
            y, x = ys[k], xs[k]
            y0, y1 = max(1, y - 91), min(H, y + 32)
            x0, x1 = max(1, x - 91), min(W, x + 32)
            gy, gx = np.mgrid[y0:y1, x0:x1]
            reach = np.hypot(gx - x + 30, gy - y + 30) <= 60 + 1.5
            assert (ref_i[y0:y1, x0:x1][reach] == chosen[y, x]).any(), (y, x)


@pytest.mark.gpu
def test_gpu_record_bit_exact_chain(gpu_ctx, oracle):
    """record (initial, optional spatial, trace) for 3 accumulating frames: the HDR bit for bit what the oracle's trace
    makes of the reservoirs the record traced with, and what separate resample + resample + trace calls make (host and
    device inputs)."""
    world = make_world("cornell")
    cam, fl, osc, ar, nm, depth, _ = _gbuffer(oracle, world)
    gpu_ctx.upload_scene(world)
    dev = [DeviceBuffer(a) for a in (ar, nm, depth)]
    out0, out1 = DeviceBuffer(nbytes=W * H * 8), DeviceBuffer(nbytes=W * H * 8)
    ptrs = [d.ptr.value for d in dev]
    try:
        _record_chain(gpu_ctx, osc, cam, ar, nm, depth, ptrs, out0, out1)
    finally:
        for d in dev + [out0, out1]:
            d.free()


def _record_chain(gpu_ctx, osc, cam, ar, nm, depth, ptrs, out0, out1):
    for spatial in (True, False):
        want = None
        recorded = []
        frames = ((1, FLAG_SKIP_HISTORY | FLAG_ACCUMULATE), (2, FLAG_ACCUMULATE), (3, FLAG_ACCUMULATE))
        for frame, flags in frames:
            pc = S.RestirTracePC(0, frame, flags)
            gpu_ctx.restir_di_record(pc, cam, ar, nm, depth, spatial_reuse=spatial)
            res = gpu_ctx.read_restir_reservoirs()
            recorded.append(res)
            want = osc.restir_di_trace((0, frame, flags), cam, ar, nm, depth, res, history=want)
        got = gpu_ctx.read_hdr()
        ok = same_bits(got, want).all(axis=2)
        assert ok.all(), "spatial=%s: %d of %d pixels differ from the oracle's trace" % (spatial, (~ok).sum(), ok.size)
        assert (index_of(recorded[0]) >= 0).mean() > 0.1
        assert not np.array_equal(recorded[0], recorded[1])  # the frame index reaches the resampling passes
        # the same chain as separate calls
        for (frame, flags), res_rec in zip(frames, recorded):
            res = gpu_ctx.restir_di_resample(S.RESTIR_INITIAL, frame, cam, ar, nm, depth)
            if spatial:
                res = gpu_ctx.restir_di_resample(S.RESTIR_SPATIAL, frame, cam, ar, nm, depth, res)
            assert same_bits(res, res_rec).all()
            gpu_ctx.restir_di_trace(S.RestirTracePC(0, frame, flags), cam, ar, nm, depth, res)
        sep = gpu_ctx.read_hdr()
        assert same_bits(sep, got).all()
        # device inputs
        for (frame, flags), res_rec in zip(frames, recorded):
            gpu_ctx.restir_di_record_device(S.RestirTracePC(0, frame, flags), cam, W, H, *ptrs, spatial_reuse=spatial)
            assert same_bits(gpu_ctx.read_restir_reservoirs(), res_rec).all()
        assert same_bits(gpu_ctx.read_hdr(), got).all()
        # device resample into caller buffers, the spatial pass reading the initial pass's
        p0, p1 = out0.ptr.value, out1.ptr.value
        gpu_ctx.restir_di_resample_device(S.RESTIR_INITIAL, 3, cam, W, H, *ptrs, out_ptr=p0)
        gpu_ctx.restir_di_resample_device(S.RESTIR_SPATIAL, 3, cam, W, H, *ptrs, res_ptr=p0, out_ptr=p1)
        last = (out1 if spatial else out0).read((H, W, 2))  # (hipMemcpy waits for the null stream)
        assert same_bits(last, recorded[-1]).all()
    with pytest.raises(capi.ProsperPtError):  # the spatial pass cannot write the reservoirs it reads
        gpu_ctx.restir_di_resample_device(S.RESTIR_SPATIAL, 1, cam, W, H, *ptrs, res_ptr=out0.ptr.value,
                                          out_ptr=out0.ptr.value)


@pytest.mark.gpu
def test_gpu_light_count_change_reaches_every_stage(gpu_ctx, oracle):
    """update_lights between two records: the initial pass draws from the new count, the spatial pass weighs with the
    new lights, the trace shades with them."""
    world = make_world("sponza_small")
    cam, fl, osc, ar, nm, depth, _ = _gbuffer(oracle, world)
    gpu_ctx.upload_scene(world)
    gpu_ctx.restir_di_record(S.RestirTracePC(0, 1, FLAG_SKIP_HISTORY), cam, ar, nm, depth)
    before = index_of(gpu_ctx.read_restir_reservoirs())
    fewer = make_world("sponza_small", point_lights=8)
    lights = R.Lights(fewer).count
    assert lights < R.Lights(world).count and (before >= lights).any()
    gpu_ctx.update_lights(fewer)
    osc2 = oracle.OracleScene(fewer, brute_force=True)
    ref_i, ref_w, ref_m = R.initial(fewer, cam, ar, nm, depth, 2)
    try:
        for spatial in (False, True):
            gpu_ctx.restir_di_record(S.RestirTracePC(0, 2, FLAG_SKIP_HISTORY), cam, ar, nm, depth, spatial_reuse=spatial)
            res = gpu_ctx.read_restir_reservoirs()
            idx = index_of(res)
            assert ((idx >= -1) & (idx < lights)).all()
            want = osc2.restir_di_trace((0, 2, FLAG_SKIP_HISTORY), cam, ar, nm, depth, res)
            assert same_bits(gpu_ctx.read_hdr(), want).all()
            if not spatial:
                _check_against_reference(res, ref_i, ref_w, ref_m, lights)
            else:  # (fed the GPU's initial reservoirs: a neighbour's undecided pick may differ)
                sp_i, sp_w, sp_m, _ = R.spatial(fewer, cam, ar, nm, depth, pack(ref_i, ref_w), 2, oracle)
                decided = sp_m >= 1e-4
                assert decided.mean() >= 0.99 and (idx[decided] == sp_i[decided]).mean() >= 0.99
    finally:
        gpu_ctx.update_lights(world)
        osc2.close()


@pytest.mark.gpu
def test_gpu_initial_pass_is_unbiased(gpu_ctx, oracle):
    """E[f(X) W] = sum over lights of f(l) per pixel and channel (f = irradiance * BRDF * NoL, float64 test-side),
    over 512 frame indices on ~1000 pixels that several lights reach: within 4 standard errors on >= 99 % of them.
    The atrium with 16 point and 16 spot lights: with all 1024, a light that dominates a pixel is among the 5 candidates
    of 2 or 3 frames in 512, and the sample standard error of so skewed an estimate understates its spread."""
    world = make_world("sponza_small", point_lights=16)
    world.spot_lights.count = 16
    cam, fl, osc, ar, nm, depth, _ = _gbuffer(oracle, world)
    gpu_ctx.upload_scene(world)
    sf = R.Surfaces(cam, ar, nm, depth)
    lights = R.Lights(world)
    rng = np.random.default_rng(9)
    cand = rng.choice(W * H, size=4000, replace=False)
    all_lights = np.arange(lights.count)
    target, reach = np.zeros((cand.size, 3)), np.zeros(cand.size, np.int64)
    for k, p in enumerate(cand):
        idx = np.full(lights.count, p)
        f, _ = R.light_contribution(sf, lights, all_lights, idx)
        target[k] = f.sum(axis=0)
        reach[k] = (f.sum(axis=1) > 0).sum()
    keep = np.nonzero(reach >= 4)[0][:1000]
    assert keep.size >= 500
    pix, target = cand[keep], target[keep]
    frames = 512
    est = np.zeros((frames, pix.size, 3))
    for t in range(frames):
        res = gpu_ctx.restir_di_resample(S.RESTIR_INITIAL, t + 1, cam, ar, nm, depth).reshape(-1, 2)[pix]
        idx = res[:, 0].copy().view(np.int32)
        f, _ = R.light_contribution(sf, lights, idx, pix)
        est[t] = np.where((idx >= 0)[:, None], f * res[:, 1:2].astype(np.float64), 0.0)
    mean = est.mean(axis=0)
    se = est.std(axis=0, ddof=1) / np.sqrt(frames)
    outside = np.abs(mean - target) > 4.0 * se + 1e-6 * np.abs(target)
    frac = outside.any(axis=1).mean()
    assert frac <= 0.01, "%.3f of the pixels outside 4 standard errors" % frac
    assert abs(mean.sum() / target.sum() - 1.0) < 0.01  # and over all of them together
    # a wrong selection probability would move the mean on most pixels: the estimate is not just noise around 0
    assert (mean.sum(axis=1) > 0).mean() > 0.9


@pytest.mark.gpu
def test_gpu_host_mirror_equals_the_c_abi_record(oracle):
    """render::rtdi::RtDirectIllumination::record (host layer) against prosper_pt_restir_di_record with the TracePC it
    pushed: the same image bit for bit, spatial reuse on (the default) and off."""
    from prosper_amd.rt_reference import Camera, RtDirectIllumination
    world = make_world("cornell")
    cam0, fl, osc, ar, nm, depth, _ = _gbuffer(oracle, world)
    host_ctx, abi_ctx = capi.Context(0), capi.Context(0)
    try:
        host_ctx.upload_scene(world)
        abi_ctx.upload_scene(world)
        camera = Camera.from_world(world, W, H)
        cam, _ = camera.update_buffer()
        pass_ = RtDirectIllumination(host_ctx)
        pcs = []
        for spatial in (True, True, False, False):
            if not spatial:
                pass_.draw_ui(spatial_reuse=False)
            pc = pass_.record(camera, ar, nm, depth)
            pcs.append((pc.frameIndex, pc.flags))
            abi_ctx.restir_di_record(pc, cam, ar, nm, depth, spatial_reuse=spatial)
            assert same_bits(host_ctx.read_hdr(), abi_ctx.read_hdr()).all()
            assert same_bits(host_ctx.read_restir_reservoirs(), abi_ctx.read_restir_reservoirs()).all()
        # frame index steps per record; the first record skips history (m_resetAccumulation, a changed camera)
        assert [f for f, _ in pcs] == [1, 2, 3, 4]
        assert pcs[0][1] & FLAG_SKIP_HISTORY and not pcs[1][1] & FLAG_SKIP_HISTORY and not pcs[1][1] & FLAG_ACCUMULATE
        pass_.recompile_shaders()
        assert pass_.record(camera, ar, nm, depth).flags & FLAG_SKIP_HISTORY
        pass_.close()
    finally:
        host_ctx.close()
        abi_ctx.close()
