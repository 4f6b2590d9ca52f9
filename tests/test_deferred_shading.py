"""Clustered lighting and deferred shading (prosper_pt_cluster_lights, prosper_pt_deferred_shading;
light_clustering_kernel, deferred_shading_kernel): the C-ABI surface and the restatement's geometry on the CPU, and with
-m gpu the cluster lists and the shaded image against tests/deferred_shading_reference.py, the overflow rule, the
conservative culling, the traced path, queued light updates and the host mirrors."""
import ctypes as C

import numpy as np
import pytest

import deferred_shading_reference as D
import restir_resampling_reference as R
from prosper_amd import capi, scenes, structs as S

W, H = 160, 96
NEW_SYMBOLS = ("prosper_pt_cluster_lights", "prosper_pt_get_light_cluster_dims", "prosper_pt_read_light_clusters",
               "prosper_pt_deferred_shading", "prosper_host_light_clustering_create",
               "prosper_host_light_clustering_destroy", "prosper_host_light_clustering_record",
               "prosper_host_deferred_shading_create", "prosper_host_deferred_shading_destroy",
               "prosper_host_deferred_shading_record")
# per-pixel tolerance, relative to the pixel's sum of absolute terms: fp32 surface reconstruction and BRDF against float64
REL = 2e-4
ABS = 1e-6


def camera(oracle, world, w=W, h=H, zN=None, zF=None, resolution=None):
    c = world.camera
    rw, rh = resolution or (w, h)
    cam, _ = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], zN or c["zN"], zF or c["zF"], rw, rh)
    return cam


def make_world(scene):
    if scene == "c2":
        return scenes.cornell()
    return scenes.sponza_class(lights=(64, 32), foliage=True, texture_size=64, sky_size=32, detail=0.25)


def view_points(cam, px, py, depth, w, h):
    """worldPos (uv = px / size, no half-pixel offset) taken to view space, float64 [n, 3]."""
    clip = np.stack([px / w * 2.0 - 1.0, py / h * 2.0 - 1.0, depth, np.ones(len(px))], axis=-1)
    v = clip @ D.mat(cam.clipToWorld).T
    p = np.concatenate([v[:, :3] / v[:, 3:4], np.ones((len(px), 1))], axis=-1)
    return (p @ D.mat(cam.worldToCamera).T)[:, :3]


# ---- CPU ----

def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    assert C.sizeof(S.DeferredShadingPC) == 8
    assert (S.DEFERRED_TRACE_GBUFFER, S.DEFERRED_JITTER_GBUFFER) == (1, 2)


def test_bad_arguments_are_rejected_before_touching_the_gpu(oracle):
    lib = capi.lib()
    cam = camera(oracle, scenes.cornell())
    ar, nm, dp = np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32), np.zeros((4, 4), np.float32)
    gb = S.RestirInputs(ar.ctypes.data, nm.ctypes.data, dp.ctypes.data, None, 0, 0)
    pc = S.DeferredShadingPC(0, 0)

    def refused(rc, words, code=-1):
        return rc == code and words in lib.prosper_pt_last_error().decode()

    def shade(pc_=C.byref(pc), flags=0, cam_=C.byref(cam), w=4, h=4, g=C.byref(gb)):
        return lib.prosper_pt_deferred_shading(None, pc_, flags, 0, cam_, w, h, g, None)

    assert refused(lib.prosper_pt_cluster_lights(None, C.byref(cam), 4, 4, None), "null argument")
    assert refused(lib.prosper_pt_cluster_lights(None, None, 4, 4, None), "null argument")
    assert refused(lib.prosper_pt_cluster_lights(None, C.byref(cam), 0, 4, None), "empty extent")
    assert refused(lib.prosper_pt_get_light_cluster_dims(None, None, None, None), "null argument")
    assert refused(lib.prosper_pt_read_light_clusters(None, None, None, None, None, None, 0, None), "null argument")
    assert refused(shade(), "null argument")
    assert refused(shade(pc_=None), "null argument")
    assert refused(shade(cam_=None), "null argument")
    assert refused(shade(g=None), "null argument")
    assert refused(shade(w=0), "empty extent")
    assert refused(shade(flags=4), "unknown flags")
    assert refused(shade(flags=S.DEFERRED_JITTER_GBUFFER), "JITTER_GBUFFER without TRACE_GBUFFER")
    assert refused(shade(pc_=C.byref(S.DeferredShadingPC(len(S.DRAW_TYPES), 0))), "drawType out of range")
    assert refused(shade(pc_=C.byref(S.DeferredShadingPC(0, 2))), "ibl is 0 or 1")
    assert refused(shade(pc_=C.byref(S.DeferredShadingPC(0, 1))), "ImageBasedLighting", code=-6)  # UNSUPPORTED
    bad = S.CameraUniforms.from_buffer_copy(bytes(cam))
    bad.far_ = bad.near_
    assert refused(shade(cam_=C.byref(bad)), "near_ < far_")
    assert refused(lib.prosper_pt_cluster_lights(None, C.byref(bad), 4, 4, None), "near_ < far_")
    # the traced path needs no G-buffer, so only the context is missing
    assert refused(shade(flags=S.DEFERRED_TRACE_GBUFFER, g=None), "null argument")
    assert lib.prosper_host_deferred_shading_record(None, None, 4, 4, None, 0, 0, None, None) == -1
    assert lib.prosper_host_light_clustering_record(None, None, 4, 4, None) == -1


def test_slice_boundaries(oracle):
    cam = camera(oracle, scenes.cornell())
    near, far = float(cam.near_), float(cam.far_)
    z = -np.array([near, near * 1.0001, far * 0.9999, far, far * 2.0, near * 0.5, near * 1e-3,
                   float(D.slice_start(cam, 5)) * 1.001, float(D.slice_start(cam, 5)) * 0.999, np.nan])
    s, beyond, _ = D.slices(cam, z)
    assert list(s[:4]) == [0, 0, 15, 16] and list(beyond[:5]) == [False, False, False, False, True]
    assert list(s[5:]) == [0, 0, 5, 4, 0] and not beyond[5:].any()
    # slice 16 holds exactly the far plane; past it, at far * (far / near)^(1 / 16), the robust load's empty cluster
    assert D.slices(cam, [-float(D.slice_start(cam, 17)) * 1.001])[1].all()
    assert not D.slices(cam, [-float(D.slice_start(cam, 17)) * 0.999])[1].any()


def test_a_hand_placed_point_light_lands_in_the_expected_clusters(oracle):
    world = scenes.cornell()
    world.point_lights.count = 0
    world.spot_lights.count = 0
    w = h = 256
    c = world.camera
    cam, _ = oracle.camera_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), c["fov"], 0.1, 100.0, w, h)
    world.add_point_light((1.0, 1.0, 1.0), 1.0, (0.0, 0.0, -5.0), light_range=0.1)
    vis, _ = D.clusters(world, cam, w, h)
    got = {tuple(int(v) for v in k) for k in zip(*np.nonzero(vis[..., 0]))}
    # the centre (uv 0.5, pixel 128) of a sphere well inside slice 9: clusterFrustum's planes bound x' = px / 32 - cx to
    # [-1, 1], i.e. pixels [32 (cx - 1), 32 (cx + 1)]: tile cx and the one before it, so tiles 3, 4 and 5 list it
    assert got == {(9, y, x) for y in (3, 4, 5) for x in (3, 4, 5)}, sorted(got)
    # a light the size of the view crosses slices 7-11 and every tile
    world.point_lights.lights[0].radianceAndRadius.w = 2.0
    vis, _ = D.clusters(world, cam, w, h)
    zs = sorted(set(np.nonzero(vis[..., 0])[0].tolist()))
    assert zs == [k for k in range(17) if D.slice_start(cam, k) <= 7.0 and D.slice_start(cam, k + 1) >= 3.0]
    assert vis[zs[len(zs) // 2], :, :, 0].all()
    # behind the camera: nowhere
    world.point_lights.lights[0].position.z = 5.0
    world.point_lights.lights[0].radianceAndRadius.w = 1.0
    assert not D.clusters(world, cam, w, h)[0].any()


@pytest.mark.parametrize("resolution_scale", [1, 2])
def test_every_pixel_lies_inside_its_own_cluster(oracle, resolution_scale):
    """20 000 random texels: the view-space point of (px, py, depth) inside the frustum of its cluster.  The frustum's
    tiles come from camera.resolution: at the extent, a pixel's cluster is (px / 32, py / 32, slice); with a resolution
    of twice the extent it is the tile of uv * resolution / 32 (the lookup's px / 32 then names another cluster)."""
    world = scenes.cornell()
    w, h = 200, 120
    cam = camera(oracle, world, w, h, resolution=(w * resolution_scale, h * resolution_scale))
    rng = np.random.default_rng(7)
    n = 20000
    px, py = rng.integers(0, w, n).astype(np.float64), rng.integers(0, h, n).astype(np.float64)
    lin = -np.exp(rng.uniform(np.log(cam.near_ * 1.0001), np.log(cam.far_ * 0.9999), n))
    c2c = D.mat(cam.cameraToClip)
    depth = -c2c[2, 3] / lin - c2c[2, 2]  # linearizeDepth inverted
    p = view_points(cam, px, py, depth, w, h)
    assert np.allclose(p[:, 2], lin, rtol=1e-4)
    s, beyond, _ = D.slices(cam, p[:, 2])
    assert not beyond.any()
    tx = np.floor(px * resolution_scale / D.DIM).astype(int)
    ty = np.floor(py * resolution_scale / D.DIM).astype(int)
    failures = 0
    for k in range(n):
        d = D.signed_distances(D.frustum(cam, tx[k], ty[k], s[k]), p[k:k + 1])[0]
        failures += (d < -1e-9 * max(1.0, -p[k, 2])).any()
    assert failures == 0


# ---- GPU ----

def _cluster_check(got, world, cam, w, h, eps=1e-3):
    n_point, n_spot = world.point_lights.count, world.spot_lights.count
    nx, ny, nz = D.dims(w, h)
    ptrs, idx = got["pointers"], got["indices"]
    assert ptrs.shape == (nz, ny, nx, 2)
    pc, sc = ptrs[..., 1] >> 16, ptrs[..., 1] & 0xFFFF
    linear = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    assert ((ptrs[..., 0] == np.where(pc + sc > 0, linear * D.SLOT, 0))).all(), "fixed slots"
    assert (sc == min(n_spot, D.MAX_SPOTS)).all(), "every spot in every cluster"
    assert got["count"] == int((pc + sc).sum()) and got["dropped"] == 0 and got["overflowing"] == 0
    want, margin = D.clusters(world, cam, w, h)
    for c in np.ndindex(nz, ny, nx):
        pts = idx[c][:pc[c]].astype(np.int64)
        assert (np.diff(pts) > 0).all(), ("ascending", c)
        assert (idx[c][pc[c]:pc[c] + sc[c]] == np.arange(sc[c])).all(), c
        listed = np.zeros(n_point, bool)
        listed[pts] = True
        differ = listed != want[c]
        assert not (differ & (np.abs(margin[c]) > eps)).any(), (c, np.nonzero(differ)[0])
    return D.membership(got, n_point, n_spot)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["c2", "c4"])
def test_gpu_cluster_lists_match_the_reference(gpu_ctx, oracle, scene):
    world = make_world(scene)
    gpu_ctx.upload_scene(world)
    for w, h, res in ((W, H, None), (W, H, (2 * W, 2 * H)), (1920 // 4, 1080 // 4, None)):
        cam = camera(oracle, world, w, h, resolution=res)
        gpu_ctx.cluster_lights(cam, w, h)
        assert gpu_ctx.light_cluster_dims() == D.dims(w, h)
        _cluster_check(gpu_ctx.read_light_clusters(), world, cam, w, h)


@pytest.mark.gpu
def test_gpu_overflow_keeps_the_lowest_indices(oracle):
    world = scenes.cornell()
    world.point_lights.count = 0
    world.spot_lights.count = 0
    rng = np.random.default_rng(3)
    for i in range(200):  # every third light sits behind the camera (no cluster), the others reach 60 m
        p = rng.uniform(-1.0, 1.0, 3) + [0.0, 1.0, 0.0 if i % 3 else 10.0]
        world.add_point_light((1.0, 1.0, 1.0), 1.0, tuple(p), light_range=60.0 if i % 3 else 0.5)
    for _ in range(150):
        world.add_spot_light((1.0, 1.0, 1.0), 1.0, (0.0, 1.9, 0.0), (0.0, -1.0, 0.0), 0.3, 0.6)
    ctx = capi.Context(device=0)  # a fresh index buffer: every entry past a cluster's counts still holds 0xFFFF
    try:
        ctx.upload_scene(world)
        cam = camera(oracle, world)
        ctx.cluster_lights(cam, W, H)
        got = ctx.read_light_clusters()
    finally:
        ctx.close()
    want, margin = D.clusters(world, cam, W, H)
    assert (np.abs(margin) > 1e-3).all()
    ptrs, idx = got["pointers"], got["indices"]
    pc, sc = ptrs[..., 1] >> 16, ptrs[..., 1] & 0xFFFF
    visible = want.sum(-1)
    assert (visible == 133).any() and (pc == np.minimum(visible, D.MAX_POINTS)).all() and (sc == D.MAX_SPOTS).all()
    k = np.arange(D.SLOT)
    for c in np.ndindex(pc.shape):
        # the 128 lowest of the visible lights (every third index is not among them)
        assert (idx[c][:pc[c]] == np.nonzero(want[c])[0][:D.MAX_POINTS]).all(), c
        assert (idx[c][pc[c]:pc[c] + sc[c]] == np.arange(D.MAX_SPOTS)).all(), c
        assert (idx[c][k >= pc[c] + sc[c]] == 0xFFFF).all(), ("written outside the lists", c)
    dropped = np.maximum(visible - D.MAX_POINTS, 0) + (150 - D.MAX_SPOTS)
    assert got["dropped"] == int(dropped.sum()) and got["overflowing"] == pc.size
    assert got["count"] == int((pc + sc).sum())


def _shade_check(got, want, total, margin, what, depth):
    """`margin`: how close each pixel's slice pick was to another (deferred_shading_reference.slices).  Within 1e-4 the
    GPU's fp32 log may pick the neighbour, whose lists differ only by point lights that add ~0 at that depth (a texel
    at the far plane, e.g. every miss, sits exactly on slice 16's start); those pixels are checked too, but the test
    insists that nearly every hit is decided."""
    assert (got[..., 3] == 1.0).all(), what
    ok = margin > 1e-4
    assert ok[depth != 0.0].mean() > 0.99, what
    g = got[..., :3].astype(np.float64)
    finite = np.isfinite(want).all(-1)
    assert (np.isfinite(g).all(-1) == finite).all(), what
    err = np.abs(g - want).max(-1)
    bad = finite & (err > REL * total + ABS)
    assert not bad.any(), "%s: %d pixels off, worst %.3g of %.3g" % (
        what, bad.sum(), err[bad].max(), total[bad][np.argmax(err[bad])])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["c2", "c4"])
@pytest.mark.parametrize("planes", ["scene", "far_cuts", "near_cuts"])
def test_gpu_shading_matches_the_reference(gpu_ctx, oracle, scene, planes):
    world = make_world(scene)
    if planes != "scene":
        world.camera = dict(world.camera)
        # slice 17 would start at far * (far / near)^(1 / 16): C2's back wall (4.4 from the eye) and C4's far end lie past
        # it with these far planes; C2's front edge (2.4) and C4's nearest pillars lie before these near planes
        key, value = {"c2": {"far_cuts": ("zF", 2.5), "near_cuts": ("zN", 2.9)},
                      "c4": {"far_cuts": ("zF", 4.0), "near_cuts": ("zN", 3.0)}}[scene][planes]
        world.camera[key] = value
    cam, fl, osc, ar, nm, depth, _ = R.make_gbuffer(oracle, world, W, H)
    gpu_ctx.upload_scene(world)
    gpu_ctx.deferred_shading(cam, ar, nm, depth)
    got = gpu_ctx.read_hdr()
    lists = _cluster_check(gpu_ctx.read_light_clusters(), world, cam, W, H)
    want, total, margin = D.shade(world, cam, ar, nm, depth, lists=lists)
    _shade_check(got, want, total, margin, "%s %s" % (scene, planes), depth)
    s, beyond, _ = D.slices(cam, R.Surfaces(cam, ar, nm, depth).lin_depth.astype(np.float64))
    hit = depth.ravel() != 0.0
    if planes == "far_cuts":
        assert (beyond & hit).sum() >= 50
    if planes == "near_cuts":
        near = hit & (-R.Surfaces(cam, ar, nm, depth).lin_depth < cam.near_)
        assert near.mean() > 0.02 and (s[near] == 0).all()
    # culling is conservative: the clustered image is the brute force over every light
    brute, btotal, _ = D.shade(world, cam, ar, nm, depth, lists=None)
    _shade_check(got, brute, btotal, margin, "%s %s brute force" % (scene, planes), depth)


@pytest.mark.gpu
def test_gpu_every_draw_type(gpu_ctx, oracle):
    world = make_world("c2")
    cam, fl, osc, ar, nm, depth, _ = R.make_gbuffer(oracle, world, W, H)
    gpu_ctx.upload_scene(world)
    for dt in range(len(S.DRAW_TYPES)):
        gpu_ctx.deferred_shading(cam, ar, nm, depth, draw_type=dt)
        got = gpu_ctx.read_hdr()
        if dt == 0:
            want, total, margin = D.shade(world, cam, ar, nm, depth)
            _shade_check(got, want, total, margin, "Default", depth)
        elif dt == S.DrawType["Position"]:
            want = R.Surfaces(cam, ar, nm, depth).pos.reshape(H, W, 3)
            hit = depth != 0.0
            err = np.abs(got[..., :3] - want)[hit].max()
            assert err <= 1e-5 * np.abs(want[hit]).max() and (got[..., 3] == 1.0).all()
        else:
            assert (got[..., :3] == ar[..., :3]).all() and (got[..., 3] == 1.0).all(), dt


@pytest.mark.gpu
def test_gpu_a_point_light_adds_exactly_zero_past_its_radius(oracle):
    world = scenes.cornell()
    world.spot_lights.count = 0
    world.point_lights.lights[0].radianceAndRadius.w = 0.8
    cam, fl, osc, ar, nm, depth, _ = R.make_gbuffer(oracle, world, W, H)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        ctx.deferred_shading(cam, ar, nm, depth)
        got = ctx.read_hdr()
    finally:
        ctx.close()
    pos = R.Surfaces(cam, ar, nm, depth).pos.reshape(H, W, 3)
    L = world.point_lights.lights[0].position
    d = np.linalg.norm(pos - np.array([L.x, L.y, L.z]), axis=-1)
    outside = (depth != 0.0) & (d > 0.8 * 1.0001)
    inside = (depth != 0.0) & (d < 0.8 * 0.9)
    assert outside.mean() > 0.3 and inside.any()
    assert (got[outside][:, :3] == 0.0).all()
    assert (got[inside][:, :3] > 0.0).any()


@pytest.mark.gpu
def test_gpu_traced_path_is_the_traced_gbuffer_shaded(gpu_ctx, oracle):
    world = make_world("c4")
    gpu_ctx.upload_scene(world)
    cam = camera(oracle, world)
    for jitter in (False, True):
        gpu_ctx.deferred_shading_traced(cam, W, H, frame_index=3, jitter=jitter)
        a = gpu_ctx.read_hdr()
        gpu_ctx.deferred_shading_traced(cam, W, H, frame_index=3, jitter=jitter)
        b = gpu_ctx.read_hdr()
        assert a.tobytes() == b.tobytes(), "two runs differ"
        ar, nm, depth = gpu_ctx.trace_gbuffer(cam, W, H, frame_index=3, jitter=jitter)
        inp, _, _ = gpu_ctx.gbuffer_device_ptrs()
        gpu_ctx.deferred_shading_device(cam, W, H, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
        assert gpu_ctx.read_hdr().tobytes() == a.tobytes()
        gpu_ctx.deferred_shading(cam, ar, nm, depth)
        assert gpu_ctx.read_hdr().tobytes() == a.tobytes()
    assert np.isfinite(a).all() and (a[..., :3].sum(-1) > 0).mean() > 0.5


@pytest.mark.gpu
def test_gpu_queued_light_update_reaches_both_kernels(oracle):
    world = make_world("c4")
    cam, fl, osc, ar, nm, depth, _ = R.make_gbuffer(oracle, world, W, H)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        ctx.deferred_shading(cam, ar, nm, depth)
        before = ctx.read_hdr()
        world.point_lights.count = 40  # queued: the next call flushes it before clustering
        world.spot_lights.count = 20
        for i in range(40):
            world.point_lights.lights[i].radianceAndRadius.x *= 3.0
        ctx.update_lights(world)
        ctx.deferred_shading(cam, ar, nm, depth)
        got = ctx.read_hdr()
        lists = _cluster_check(ctx.read_light_clusters(), world, cam, W, H)
    finally:
        ctx.close()
    assert before.tobytes() != got.tobytes()
    want, total, margin = D.shade(world, cam, ar, nm, depth, lists=lists)
    _shade_check(got, want, total, margin, "after update_lights", depth)


@pytest.mark.gpu
def test_gpu_host_mirrors_equal_direct_calls(oracle):
    from prosper_amd.rt_reference import Camera, DeferredShading, GBufferTracer, LightClustering
    world = make_world("c4")
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(world)
        hcam = Camera.from_world(world, W, H)
        cam, _ = hcam.update_buffer()
        ar, nm, depth = ctx.trace_gbuffer(cam, W, H, jitter=False)
        ctx.cluster_lights(cam, W, H)
        direct_clusters = ctx.read_light_clusters()
        ctx.deferred_shading(cam, ar, nm, depth)
        direct = ctx.read_hdr()

        clustering = LightClustering(ctx)
        clustering.record(hcam, W, H)
        mirrored = ctx.read_light_clusters()
        assert all(np.array_equal(mirrored[k], direct_clusters[k]) for k in direct_clusters)
        shading = DeferredShading(ctx)
        pc = shading.record(hcam, ar, nm, depth)
        assert (pc.drawType, pc.ibl) == (0, 0)
        assert ctx.read_hdr().tobytes() == direct.tobytes()
        gb = GBufferTracer(ctx).record(hcam, W, H, jitter=False)
        shading.record_device(hcam, gb, W, H)
        assert ctx.read_hdr().tobytes() == direct.tobytes()
        with pytest.raises(capi.ProsperPtError):
            shading.record(hcam, ar, nm, depth, apply_ibl=True)
        shading.record(hcam, ar, nm, depth, draw_type="Albedo")
        assert (ctx.read_hdr()[..., :3] == ar[..., :3]).all()
        clustering.close()
        shading.close()
    finally:
        ctx.close()
