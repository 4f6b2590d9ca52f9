"""Image-based lighting (prosper_pt_generate_ibl, prosper_pt_read_ibl, prosper_pt_deferred_shading with ibl = 1;
ibl_irradiance_kernel, ibl_prefilter_kernel, ibl_brdf_lut_kernel, deferred_shading_ibl_kernel): the C-ABI surface and
the reference's known answers on the CPU, and with -m gpu the maps and the shaded image against tests/ibl_reference.py,
the lifecycle of the maps and the host mirrors."""
import ctypes as C

import numpy as np
import pytest

import deferred_shading_reference as D
import ibl_reference as I
import restir_resampling_reference as R
from prosper_amd import capi, flight_helmet, scenes, structs as S

NEW_SYMBOLS = ("prosper_pt_generate_ibl", "prosper_pt_get_ibl_info", "prosper_pt_read_ibl",
               "prosper_host_image_based_lighting_create", "prosper_host_image_based_lighting_destroy",
               "prosper_host_image_based_lighting_is_generated", "prosper_host_image_based_lighting_record_generation")
IRR_BYTES, RAD_BYTES, LUT_BYTES = 6 * 64 * 64 * 8, sum(6 * (512 >> m) ** 2 for m in range(10)) * 8, 512 * 512 * 4
# shading tolerance of test_deferred_shading.py
REL = 2e-4
ABS = 1e-6


def constant_sky(value, n=8):
    sky = np.full((6, n, n, 4), value, np.float16)
    sky[..., 3] = 1.0
    return sky


def sky_world(kind):
    world = scenes.cornell(with_skybox=True)
    if kind == "sky512":
        world.skybox = scenes.sky_cube(512)
    return world


def edge_texels(n):
    """(face, i, j) of every face's border texels (corners included)."""
    k = np.arange(n)
    i = np.concatenate([k, k, np.zeros(n, int), np.full(n, n - 1)])
    j = np.concatenate([np.zeros(n, int), np.full(n, n - 1), k, k])
    ij = np.unique(np.stack([i, j], -1), axis=0)
    f = np.repeat(np.arange(6), len(ij))
    return f, np.tile(ij[:, 0], 6), np.tile(ij[:, 1], 6)


def checked_texels(n, seed, count=512):
    """Every texel of a level of at most 8 x 8 per face; otherwise every face's edges and corners and `count` seeded
    random texels."""
    if n * n * 6 <= 6 * 64:
        f, j, i = np.meshgrid(np.arange(6), np.arange(n), np.arange(n), indexing="ij")
        return f.ravel(), i.ravel(), j.ravel()
    f, i, j = edge_texels(n)
    rng = np.random.default_rng(seed)
    return (np.concatenate([f, rng.integers(0, 6, count)]), np.concatenate([i, rng.integers(0, n, count)]),
            np.concatenate([j, rng.integers(0, n, count)]))


# ---- CPU ----

def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    assert C.sizeof(S.IblInfo) == 32


def test_bad_arguments_are_rejected_before_touching_the_gpu():
    lib = capi.lib()

    def refused(rc, words, code=-1):
        return rc == code and words in lib.prosper_pt_last_error().decode()

    buf = np.zeros(LUT_BYTES // 2, np.uint16)
    assert refused(lib.prosper_pt_generate_ibl(None, None), "null argument")
    assert refused(lib.prosper_pt_get_ibl_info(None, None), "null argument")
    assert refused(lib.prosper_pt_read_ibl(None, None, 0, None, 0, None, 0, None), "null argument")
    assert refused(lib.prosper_pt_read_ibl(None, buf.ctypes.data, IRR_BYTES - 8, None, 0, None, 0, None), "irradiance_bytes")
    assert refused(lib.prosper_pt_read_ibl(None, None, 0, buf.ctypes.data, RAD_BYTES + 8, None, 0, None), "radiance_bytes")
    assert refused(lib.prosper_pt_read_ibl(None, None, 0, None, 0, buf.ctypes.data, LUT_BYTES // 2, None), "lut_bytes")
    assert refused(lib.prosper_pt_read_ibl(None, None, 0, None, 0, buf.ctypes.data, LUT_BYTES, None), "null argument")
    # ibl = 1 without a context (or without maps) is still refused as unsupported, naming the generation step
    cam = S.CameraUniforms()
    ar = np.zeros((4, 4, 4), np.float32)
    gb = S.RestirInputs(ar.ctypes.data, ar.ctypes.data, ar.ctypes.data, None, 0, 0)
    rc = lib.prosper_pt_deferred_shading(None, C.byref(S.DeferredShadingPC(0, 1)), 0, 0, C.byref(cam), 4, 4,
                                         C.byref(gb), None)
    assert refused(rc, "ImageBasedLighting", code=-6) and "prosper_pt_generate_ibl" in lib.prosper_pt_last_error().decode()
    out = C.c_void_p()
    assert lib.prosper_host_image_based_lighting_create(None, C.byref(out)) == -1 and not out.value
    assert lib.prosper_host_image_based_lighting_is_generated(None) == -1
    assert lib.prosper_host_image_based_lighting_record_generation(None, None) == -1


@pytest.mark.parametrize("value", [0.5, 20.0])
def test_reference_constant_sky(value):
    """A constant sky c gives irradiance c * pi * sum(cos sin) / 8192 (~c) and c at every radiance mip; above 10 the
    clamp gives the answers for 10."""
    sky = constant_sky(value).astype(np.float64)
    c = min(value, 10.0)
    theta = 0.5 * I.PI * np.arange(64) / 64.0
    want = c * I.PI * 128 * (np.cos(theta) * np.sin(theta)).sum() / 8192.0
    assert abs(want - c) < 0.02 * c
    f, i, j = np.array([0, 2, 3, 5]), np.array([0, 31, 63, 7]), np.array([0, 12, 63, 40])
    got, _ = I.irradiance(sky, f, i, j)
    assert np.allclose(got, want, rtol=1e-12)
    for mip in (0, 1, 5, 9):
        n = 512 >> mip
        got, _ = I.prefilter(sky, mip, f, np.minimum(i, n - 1), np.minimum(j, n - 1))
        assert np.allclose(got, c, rtol=1e-12), mip


def test_reference_lut_row_zero_closed_form_and_column_zero():
    """Row 0 (alpha 0: every H = N): A = (1 - Fc) G, B = Fc G, G = (NoV / (NoV (1 - k) + k))^2, k = 1e-4,
    Fc = (1 - NoV)^5; column 0 (NoV = 0) is (0, 0)."""
    rows = I.brdf_lut([0, 1, 300, 511])
    NoV = np.arange(1, 512) / 512.0
    k = 1e-4
    G = (NoV / (NoV * (1 - k) + k)) ** 2
    fc = (1 - NoV) ** 5
    assert np.allclose(rows[0, 1:, 0], np.clip((1 - fc) * G, 0, 1), rtol=1e-9, atol=1e-12)
    assert np.allclose(rows[0, 1:, 1], np.clip(fc * G, 0, 1), rtol=1e-9, atol=1e-12)
    assert (rows[:, 0] == 0.0).all()
    assert np.isfinite(rows).all() and (rows[1:, 1:, 0] > 0).all()


# ---- GPU ----

def _generate(ctx, world):
    ctx.upload_scene(world)
    ctx.generate_ibl()
    info = ctx.ibl_info()
    assert (info.generated, info.irradianceSize, info.radianceSize, info.radianceMips, info.lutSize) == (1, 64, 512, 10, 512)
    return ctx.read_ibl()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cornell_sky", "sky512"])
def test_gpu_irradiance_matches_the_reference(gpu_ctx, kind):
    world = sky_world(kind)
    maps = _generate(gpu_ctx, world)
    f, i, j = checked_texels(64, 11)
    want, near = I.irradiance(I.sky64(world), f, i, j)
    d = I.half_ulps(maps["irradiance"][f, j, i, :3], want)
    print("%s irradiance: %d texels, max %d ulp, %d near the frame switch" % (kind, len(f), d.max(), near))
    assert d.max() <= 1
    assert (maps["irradiance"][..., 3] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cornell_sky", "sky512"])
def test_gpu_radiance_matches_the_reference(gpu_ctx, kind):
    world = sky_world(kind)
    maps = _generate(gpu_ctx, world)
    sky = I.sky64(world)
    worst, nears = 0, 0
    for mip in range(10):
        n = 512 >> mip
        f, i, j = checked_texels(n, 100 + mip)
        want, near = I.prefilter(sky, mip, f, i, j)
        d = I.half_ulps(maps["radiance"][mip][f, j, i, :3], want)
        assert d.max() <= 1, (mip, d.max())
        worst, nears = max(worst, int(d.max())), nears + near
        if mip == 0:
            # mip 0 is the clamped sky at the texel's direction
            sky_at = np.minimum(I.sample_cube(sky, I.normalize(I.texel_dirs(f, i, j, n))), 10.0)
            assert I.half_ulps(maps["radiance"][0][f, j, i, :3], sky_at).max() <= 1
    print("%s radiance: max %d ulp, %d texels near the sampler switch" % (kind, worst, nears))


@pytest.mark.gpu
def test_gpu_brdf_lut_matches_the_reference(gpu_ctx):
    """Rows 0, 1 and 511 and column 0 whole, and 512 seeded texels.  The texels of the first columns of the low-roughness
    rows are ill-conditioned (NoV of a few 1/512 against half vectors a few degrees from N: float32 and float64 part
    there by up to 100 codes), so the seeded ones lie at NoV >= 16 / 512."""
    maps = _generate(gpu_ctx, sky_world("cornell_sky"))
    lut = maps["lut"].astype(np.int64)
    assert (lut[:, 0] == 0).all(), "column 0 is (0, 0)"
    rng = np.random.default_rng(5)
    ys, xs = rng.integers(0, 512, 512), rng.integers(16, 512, 512)
    rows = sorted(set([0, 1, 511]) | set(ys.tolist()))
    want = dict(zip(rows, I.lut_codes(I.brdf_lut(rows))))
    whole = {y: int(np.abs(lut[y] - want[y]).max()) for y in (0, 1, 511)}
    seeded = np.array([np.abs(lut[y, x] - want[y][x]).max() for y, x in zip(ys, xs)])
    print("LUT: max codes off in rows 0, 1, 511: %s; seeded texels: %d" % (whole, seeded.max()))
    assert max(whole.values()) <= 1 and seeded.max() <= 1


@pytest.mark.gpu
def test_gpu_known_answers_constant_and_missing_sky_and_determinism():
    ctx = capi.Context(device=0)
    try:
        world = scenes.cornell()
        luts = []
        for value in (0.5, 20.0):
            world.skybox = constant_sky(value)
            maps = _generate(ctx, world)
            c = np.float16(min(value, 10.0)).astype(np.float64)
            theta = 0.5 * I.PI * np.arange(64) / 64.0
            irr = c * I.PI * 128 * (np.cos(theta) * np.sin(theta)).sum() / 8192.0
            assert I.half_ulps(maps["irradiance"][..., :3], np.full((6, 64, 64, 3), irr)).max() <= 1, value
            for m, level in enumerate(maps["radiance"]):
                assert I.half_ulps(level[..., :3], np.full(level[..., :3].shape, c)).max() <= 1, (value, m)
            luts.append(maps["lut"])
        world.skybox = None
        maps = _generate(ctx, world)
        assert not maps["irradiance"].any() and not any(level.any() for level in maps["radiance"])
        luts.append(maps["lut"])
        assert all(np.array_equal(luts[0], x) for x in luts[1:]), "the LUT does not depend on the sky"
        world.skybox = scenes.sky_cube(64)
        a = _generate(ctx, world)
        ctx.generate_ibl()
        b = ctx.read_ibl()
        assert a["irradiance"].tobytes() == b["irradiance"].tobytes() and a["lut"].tobytes() == b["lut"].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a["radiance"], b["radiance"]))
        info = ctx.ibl_info()
        assert info.irradianceMs > 0 and info.radianceMs > 0 and info.lutMs > 0
    finally:
        ctx.close()


def _ibl_check(got, sf, idx, maps, base, base_total, what):
    ibl, ibl_total, _ = I.eval_ibl(sf, idx, maps)
    want = base + ibl
    total = base_total + ibl_total
    g = got[..., :3].reshape(-1, 3)[idx].astype(np.float64)
    assert np.isfinite(g).all(), what
    err = np.abs(g - want).max(-1)
    # within the LUT's first texel interval (NoV < 1.5 / 512) the LUT climbs from column 0's (0, 0) to ~0.9 in 1 / 512
    # of NoV: float32's NoV moves the term there by far more than the fp32 surface moves the other terms
    NoV = np.clip((sf.n[idx] * sf.v[idx]).sum(-1), 0.0, 1.0)
    grazing = NoV < 1.5 / 512
    bad = err > np.where(grazing, 1e-2, REL) * total + ABS
    print("%s: %d pixels (%d grazing), worst error %.3g" % (what, len(idx), grazing.sum(), err.max()))
    for k in np.nonzero(bad)[0][:10]:
        print("  off: pixel %d err %.3g total %.3g NoV %.6f roughness %.4f" % (idx[k], err[k], total[k], NoV[k],
                                                                           sf.rough[idx[k]]))
    assert not bad.any(), "%s: %d pixels off, worst %.3g" % (what, bad.sum(), err[bad].max())
    assert (ibl.sum(-1) > 0).mean() > 0.9, "the IBL term lights the hits"


@pytest.mark.gpu
def test_gpu_shading_with_ibl_matches_the_reference(oracle):
    world = sky_world("cornell_sky")
    w, h = 160, 96
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        ctx.generate_ibl()
        maps = ctx.read_ibl()
        cam = camera_for(oracle, world, w, h)
        ar, nm, depth = ctx.trace_gbuffer(cam, w, h, jitter=False)
        ctx.deferred_shading(cam, ar, nm, depth, ibl=1)
        got = ctx.read_hdr()
        lists = D.membership(ctx.read_light_clusters(), world.point_lights.count, world.spot_lights.count)
    finally:
        ctx.close()
    base, base_total, margin = D.shade(world, cam, ar, nm, depth, lists=lists)
    sf = R.Surfaces(cam, ar, nm, depth)
    idx = np.nonzero((depth.ravel() != 0.0) & (margin.ravel() > 1e-4))[0]
    assert len(idx) > 0.5 * w * h
    _ibl_check(got, sf, idx, maps, base.reshape(-1, 3)[idx], base_total.ravel()[idx], "cornell with sky")
    assert (got[..., 3] == 1.0).all()


def camera_for(oracle, world, w, h):
    c = world.camera
    cam, _ = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)
    return cam


@pytest.mark.gpu
def test_gpu_shading_with_ibl_flight_helmet_full_size(oracle):
    world = flight_helmet.load_fixture()
    w, h = 1920, 1080
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        ctx.generate_ibl()
        maps = ctx.read_ibl()
        cam = camera_for(oracle, world, w, h)
        ar, nm, depth = ctx.trace_gbuffer(cam, w, h, jitter=False)
        ctx.deferred_shading(cam, ar, nm, depth, ibl=1)
        got = ctx.read_hdr()
    finally:
        ctx.close()
    assert world.point_lights.count == 0 and world.spot_lights.count == 0
    hits = np.nonzero(depth.ravel() != 0.0)[0]
    idx = np.sort(np.random.default_rng(9).choice(hits, 20000, replace=False))
    sf = R.Surfaces(cam, ar, nm, depth)
    L = R.Lights(world)
    b, _ = R.brdf_times_nol(sf, np.broadcast_to(L.sun_l, (len(idx), 3)), idx)
    base = L.rad[0] * b
    _ibl_check(got, sf, idx, maps, base, np.abs(base).sum(-1), "FlightHelmet 1920x1080")


@pytest.mark.gpu
def test_gpu_ibl_off_is_unchanged_by_generation_and_the_lifecycle(oracle):
    world = sky_world("cornell_sky")
    w, h = 96, 64
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        cam = camera_for(oracle, world, w, h)
        ar, nm, depth = ctx.trace_gbuffer(cam, w, h, jitter=False)
        assert ctx.ibl_info().generated == 0
        with pytest.raises(capi.ProsperPtError):
            ctx.deferred_shading(cam, ar, nm, depth, ibl=1)
        ctx.deferred_shading(cam, ar, nm, depth)
        before = ctx.read_hdr()
        ctx.generate_ibl()
        assert ctx.ibl_info().generated == 1
        ctx.deferred_shading(cam, ar, nm, depth)
        assert ctx.read_hdr().tobytes() == before.tobytes(), "ibl = 0 is byte-identical after generation"
        ctx.deferred_shading(cam, ar, nm, depth, ibl=1)
        lit = ctx.read_hdr()
        assert (lit[..., :3] > before[..., :3]).mean() > 0.5
        world.point_lights.lights[0].radianceAndRadius.x *= 2.0
        ctx.update_lights(world)  # updates keep the maps
        assert ctx.ibl_info().generated == 1
        ctx.deferred_shading(cam, ar, nm, depth, ibl=1)
        ctx.upload_scene(world)  # the maps describe the old sky
        assert ctx.ibl_info().generated == 0
        with pytest.raises(capi.ProsperPtError):
            ctx.deferred_shading(cam, ar, nm, depth, ibl=1)
        with pytest.raises(capi.ProsperPtError):
            ctx.read_ibl()
        ctx.generate_ibl()
        ctx.deferred_shading(cam, ar, nm, depth, ibl=1)
        assert np.isfinite(ctx.read_hdr()[depth != 0.0]).all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_host_mirrors_equal_direct_calls():
    from prosper_amd.rt_reference import Camera, DeferredShading, ImageBasedLighting
    world = sky_world("cornell_sky")
    w, h = 128, 80
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        hcam = Camera.from_world(world, w, h)
        cam, _ = hcam.update_buffer()
        ar, nm, depth = ctx.trace_gbuffer(cam, w, h, jitter=False)
        ctx.generate_ibl()
        direct_maps = ctx.read_ibl()
        ctx.deferred_shading(cam, ar, nm, depth, ibl=1)
        direct = ctx.read_hdr()

        ctx.upload_scene(world)
        ibl = ImageBasedLighting(ctx)
        shading = DeferredShading(ctx)
        assert not ibl.is_generated()
        with pytest.raises(capi.ProsperPtError):
            shading.record(hcam, ar, nm, depth, apply_ibl=True)
        ibl.record_generation()
        assert ibl.is_generated()
        maps = ctx.read_ibl()
        assert maps["irradiance"].tobytes() == direct_maps["irradiance"].tobytes()
        assert maps["lut"].tobytes() == direct_maps["lut"].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(maps["radiance"], direct_maps["radiance"]))
        pc = shading.record(hcam, ar, nm, depth, apply_ibl=True)
        assert (pc.drawType, pc.ibl) == (0, 1)
        assert ctx.read_hdr().tobytes() == direct.tobytes()
        ibl.close()
        shading.close()
    finally:
        ctx.close()
