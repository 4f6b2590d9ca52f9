"""The rasteriser over the meshlet draw lists on the GPU (prosper_pt_raster_meshlets, prosper_pt_raster_visibility;
pt_raster.hip).

The rule: the designed scene S1 (tests/raster_scenes.py) through the unculled list against tests/raster_reference.py at every
pixel, ids and depth bits, and the counts of prosper_pt_get_raster_info.  The property: after both culling phases over the
rasteriser's own depth the image is byte for byte the one drawn with nothing culled."""
import ctypes as C

import numpy as np
import pytest

import culling_reference as CR
import culling_scenes as CS
import raster_reference as R
import raster_scenes as RS
from prosper_amd import capi, structs as S

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = ("triangles", "culledBackface", "culledZeroArea", "culledOutside", "clipped", "queued", "fragments")


def counts_of(draw):
    assert draw.valid == 1 and draw.queueOverflow == 0
    return {k: getattr(draw, k) for k in COUNTS}


def draw_unculled(ctx, cam, stream=None):
    ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE, stream=stream)
    ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True, stream=stream)
    return ctx.read_raster_visibility(int(cam.resolution[0]), int(cam.resolution[1]), stream=stream)


def assert_is_the_restatement(ctx, world, cam, ids, depth):
    want = R.rasterise(world, cam, CR.generate(world, CR.MODE_OPAQUE))
    want_ids, want_depth = R.decode(world, want["keys"])
    assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32))
    assert np.array_equal(ids, want_ids)
    info = ctx.raster_info()  # (the read-back has waited for the draw: the counts have landed)
    assert info is not None and (info.width, info.height) == (ids.shape[1], ids.shape[0])
    assert counts_of(info.draw[0]) == want["counts"] and info.draw[1].valid == 0
    return want


@pytest.fixture(scope="module")
def s1(gpu_ctx):
    world, names = RS.s1_world()
    gpu_ctx.upload_scene(world)
    return gpu_ctx, world, names


@pytest.mark.parametrize("extent", [(48, 32), (33, 17), (1, 1), (96, 64)])
def test_s1_is_the_restatement_s_at_every_pixel(s1, extent):
    ctx, world, names = s1
    cam = RS.s1_camera(*extent)
    ids, depth = draw_unculled(ctx, cam)
    want = assert_is_the_restatement(ctx, world, cam, ids, depth)
    if extent != (1, 1):
        c = want["counts"]
        assert c["clipped"] >= 3 and c["queued"] >= c["clipped"] and c["culledZeroArea"] >= 1 and c["culledBackface"] >= 3
        if extent == (96, 64):
            assert c["queued"] > c["clipped"]  # the triangle over the whole image is past the medium class: the tiles' path
    # a second, identical call is byte-identical
    ids2, depth2 = draw_unculled(ctx, cam)
    assert ids2.tobytes() == ids.tobytes() and depth2.tobytes() == depth.tobytes()
    # and so is the same list drawn again WITHOUT a clear: nothing beats its own key
    ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=False)
    ids3, depth3 = ctx.read_raster_visibility(*extent)
    assert ids3.tobytes() == ids.tobytes() and depth3.tobytes() == depth.tobytes()
    info = ctx.raster_info()
    assert counts_of(info.draw[1]) == want["counts"] and counts_of(info.draw[0]) == want["counts"]


def test_refusals(s1):
    ctx, world, names = s1
    lib = capi.lib()
    cam = RS.s1_camera()
    ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
    with pytest.raises(capi.ProsperPtError, match="unknown flags"):
        lib_rc = lib.prosper_pt_raster_meshlets(ctx._h, S.DRAW_LIST_GENERATED, 2, C.byref(cam), None)
        capi._check(lib_rc)
    assert lib.prosper_pt_raster_meshlets(ctx._h, S.DRAW_LIST_SECOND_PHASE_INPUT, 1, C.byref(cam), None) == -1
    assert lib.prosper_pt_raster_meshlets(ctx._h, 4, 1, C.byref(cam), None) == -1
    assert lib.prosper_pt_raster_meshlets(None, 0, 1, C.byref(cam), None) == -1
    assert lib.prosper_pt_raster_meshlets(ctx._h, 0, 1, None, None) == -1
    assert lib.prosper_pt_raster_visibility(None, C.byref(cam), None) == -1
    with pytest.raises(capi.ProsperPtError, match="did not produce"):
        ctx.raster_meshlets(cam, S.DRAW_LIST_SECOND_PHASE)  # no pyramid, no second phase
    ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True)
    before = ctx.read_raster_visibility(48, 32)
    other = RS.s1_camera(40, 32)
    with pytest.raises(capi.ProsperPtError, match="without PROSPER_PT_RASTER_CLEAR"):
        ctx.raster_meshlets(other, S.DRAW_LIST_GENERATED, clear=False)
    empty = RS.s1_camera(48, 32)
    empty.resolution[0] = 0
    with pytest.raises(capi.ProsperPtError, match="resolution"):
        ctx.raster_meshlets(empty, S.DRAW_LIST_GENERATED)
    one = RS.s1_camera(1, 1)
    with pytest.raises(capi.ProsperPtError, match="above 1"):
        ctx.raster_visibility(one)
    ids = np.empty((32, 48, 3), np.uint32)
    assert lib.prosper_pt_read_raster_visibility(ctx._h, ids.ctypes.data, None, 48 * 32 - 1, None) == -1  # too small
    assert lib.prosper_pt_read_raster_visibility(ctx._h, None, None, 48 * 32, None) == -1
    assert lib.prosper_pt_get_raster_info(ctx._h, None) == -1
    # a refused call leaves everything as it was
    after = ctx.read_raster_visibility(48, 32)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    fresh = capi.Context(device=0)
    try:
        info = S.RasterInfo()
        assert lib.prosper_pt_raster_meshlets(fresh._h, 0, 1, C.byref(cam), None) == -4  # no scene
        assert lib.prosper_pt_raster_visibility(fresh._h, C.byref(cam), None) == -4
        assert lib.prosper_pt_get_raster_info(fresh._h, C.byref(info)) == -4
        assert lib.prosper_pt_read_raster_visibility(fresh._h, ids.ctypes.data, None, ids.size, None) == -4
        # a scene without meshlets
        from prosper_amd import scenes
        plain = scenes.World()
        m = plain.add_material()
        plain.add_instance(plain.add_model([(scenes._add(plain, scenes.quad((-1, -1, -3), (1, -1, -3), (1, 1, -3), (-1, 1, -3)), m), m)]))
        plain.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 5.0, 0.0))
        fresh.upload_scene(plain)
        fresh.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
        with pytest.raises(capi.ProsperPtError, match="no meshlets") as e:
            fresh.raster_meshlets(cam)
        assert e.value.code == -4
        # MASK materials without a texture (alpha 1 against the cutoff): drawn, every fragment kept
        masked, _ = CS.sweep_world(CS.camera_at())
        masked = masked.with_meshes_loaded([i for i in range(len(masked.metadatas))])
        fresh.upload_scene(masked)
        fresh.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
        fresh.raster_meshlets(cam)
    finally:
        fresh.close()


def test_two_streams_into_one_context(s1):
    ctx, world, names = s1
    hip = C.CDLL("libamdhip64.so")
    s1_, s2_ = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s1_), 1) == 0 and hip.hipStreamCreateWithFlags(C.byref(s2_), 1) == 0
    try:
        small, big = RS.s1_camera(33, 17), RS.s1_camera(96, 64)
        want = R.decode(world, R.rasterise(world, big, CR.generate(world, CR.MODE_OPAQUE))["keys"])
        for _ in range(2):  # the second call grows the image the first still writes; nothing waits on the host between
            ctx.cull_first_phase(small, S.CULL_MODE_OPAQUE, stream=s1_.value)
            ctx.raster_meshlets(small, S.DRAW_LIST_GENERATED, stream=s1_.value)
            ctx.cull_first_phase(big, S.CULL_MODE_OPAQUE, stream=s2_.value)
            ctx.raster_meshlets(big, S.DRAW_LIST_GENERATED, stream=s2_.value)
            ids, depth = ctx.read_raster_visibility(96, 64, stream=s1_.value)
            assert np.array_equal(ids, want[0]) and np.array_equal(depth.view(np.uint32), want[1].view(np.uint32))
    finally:
        assert hip.hipStreamSynchronize(s1_) == 0 and hip.hipStreamSynchronize(s2_) == 0
        hip.hipStreamDestroy(s1_)
        hip.hipStreamDestroy(s2_)


# (from here on the tests upload scenes of their own into the session's context)
@pytest.mark.parametrize("count", [0, 1, 65, 257])
def test_lists_of_every_length_around_a_wave(gpu_ctx, count):
    world = RS.list_world(count)
    gpu_ctx.upload_scene(world)
    cam = CS.camera_at()
    ids, depth = draw_unculled(gpu_ctx, cam)
    pairs, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_GENERATED)
    assert len(pairs) == count
    want = assert_is_the_restatement(gpu_ctx, world, cam, ids, depth)
    assert want["counts"]["triangles"] == count
    assert (ids[..., 0] != R.NO_ID).any() == (count != 0)


def test_two_phases_draw_what_no_culling_draws(gpu_ctx):
    world, inst = CS.property_world()
    gpu_ctx.upload_scene(world)
    fresh = capi.Context(device=0)
    try:
        fresh.upload_scene(world)
        second_total = 0
        for frame, eye_x in enumerate((0.0, 0.3, 0.6)):
            cam = CS.camera_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0))
            gpu_ctx.raster_visibility(cam)
            ids, depth = gpu_ctx.read_raster_visibility(CS.WIDTH, CS.HEIGHT)
            want_ids, want_depth = draw_unculled(fresh, cam)
            assert ids.tobytes() == want_ids.tobytes() and depth.tobytes() == want_depth.tobytes(), frame
            assert (ids[..., 0] != R.NO_ID).sum() > 0.5 * ids.shape[0] * ids.shape[1]
            first, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_FIRST_PHASE)
            gen, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_GENERATED)
            stats = gpu_ctx.draw_stats()
            info = gpu_ctx.raster_info()
            kept = gpu_ctx.hiz_info(0 if frame % 2 == 0 else 1)
            assert kept.valid == 1 and (kept.sourceWidth, kept.sourceHeight) == (CS.WIDTH, CS.HEIGHT)
            if frame == 0:
                assert stats.drawnMeshletCount == len(first) and info.draw[1].valid == 0
                with pytest.raises(capi.ProsperPtError, match="did not produce"):
                    gpu_ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE)
            else:
                second, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE)
                second_total += len(second)
                assert stats.drawnMeshletCount == len(first) + len(second)
                assert len(first) + len(second) < len(gen)  # something was culled
                assert info.draw[0].valid == 1 and info.draw[1].valid == 1
                # the two draws are the restatement's: the second on top of the first
                a = R.rasterise(world, cam, first)
                b = R.rasterise(world, cam, second, keys=a["keys"])
                assert counts_of(info.draw[0]) == a["counts"] and counts_of(info.draw[1]) == b["counts"]
                assert np.array_equal(R.decode(world, b["keys"])[0], ids)
            # the kept pyramid is the image's depth's
            levels = gpu_ctx.read_hiz(0 if frame % 2 == 0 else 1)
            for x, y in zip(levels, CR.hiz_pyramid(depth)):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert second_total > 0  # else the test shows nothing: the camera's step disoccluded something
        # the culling call over a TRACED depth shares the kept slot and is what it was
        gpu_ctx.trace_gbuffer(cam, CS.WIDTH, CS.HEIGHT, jitter=False)
        gpu_ctx.cull_gbuffer(cam)
        fresh.trace_gbuffer(cam, CS.WIDTH, CS.HEIGHT, jitter=False)
        fresh.cull_gbuffer(cam)
        assert sorted(map(tuple, gpu_ctx.read_draw_list(S.DRAW_LIST_GENERATED)[0].tolist())) == \
            sorted(map(tuple, fresh.read_draw_list(S.DRAW_LIST_GENERATED)[0].tolist()))
        # a new scene forgets the image and the kept pyramid
        gpu_ctx.upload_scene(world)
        with pytest.raises(capi.ProsperPtError, match="nothing has been drawn"):
            gpu_ctx.read_raster_visibility(CS.WIDTH, CS.HEIGHT)
        assert gpu_ctx.hiz_info(0).valid == 0 and gpu_ctx.hiz_info(1).valid == 0
    finally:
        fresh.close()
