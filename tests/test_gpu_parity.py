"""HIP path vs the CPU oracle on the same seeded inputs (bit-exact: DESIGN.md "Arithmetic contract").

All calls go through the C-ABI (libprosper_pt.so); the oracle is only the checker.
"""
import os

import numpy as np
import pytest

from conftest import default_pc, same_bits
from prosper_amd import capi, scenes, structs as S

pytestmark = pytest.mark.gpu


def _camera(oracle, world, w, h):
    c = world.camera
    return oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)


def _rand_inputs(fn, n, rng):
    in_stride, _ = FN_SHAPES[fn]
    return rng.standard_normal((n, in_stride)).astype(np.float32)


FN_SHAPES = {0: (1, 2), 1: (2, 1), 2: (1, 1), 3: (3, 3), 4: (1, 4), 5: (3, 9), 6: (5, 3), 7: (6, 3), 8: (7, 1),
             9: (14, 3), 10: (6, 3), 11: (10, 7), 12: (14, 7), 13: (17, 4), 14: (1, 2), 15: (3, 4)}


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _fn_inputs(fn, n, rng):
    """Inputs in the domain each function sees on the path."""
    u = lambda *shape: rng.random(shape, dtype=np.float32)
    g = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    if fn == 0:   # sincos: angles in [0, 2pi] plus a wider range
        return np.concatenate([u(n // 2, 1) * 6.2831855, g(n - n // 2, 1) * 50.0]).astype(np.float32)
    if fn == 1:   # pow
        return np.stack([u(n) * 4.0, g(n) * 3.0], axis=1).astype(np.float32)
    if fn == 2:   # srgb: every 8-bit code plus random
        codes = (np.arange(256, dtype=np.float32) / np.float32(255.0))[:, None]
        return np.concatenate([codes, u(n, 1)]).astype(np.float32)
    if fn == 3:
        return g(n, 3) * np.float32(10.0)
    if fn == 4:   # snorm10 bit patterns
        bits = rng.integers(0, 2**32, size=(n, 1), dtype=np.uint64).astype(np.uint32)
        return bits.view(np.float32)
    if fn == 5:
        return _unit(g(n, 3)).astype(np.float32)
    if fn == 6:
        return np.concatenate([_unit(g(n, 3)), u(n, 2)], axis=1).astype(np.float32)
    if fn == 7:
        ve = _unit(g(n, 3))
        ve[:, 2] = np.abs(ve[:, 2])
        return np.concatenate([ve, (u(n, 1) * 0.99 + 0.0025), u(n, 2)], axis=1).astype(np.float32)
    if fn == 8:
        ve, le = _unit(g(n, 3)), _unit(g(n, 3))
        ve[:, 2], le[:, 2] = np.abs(ve[:, 2]), np.abs(le[:, 2])
        return np.concatenate([ve, le, (u(n, 1) * 0.99 + 0.0025)], axis=1).astype(np.float32)
    if fn == 9:
        nrm = _unit(g(n, 3))
        l = _unit(nrm + 0.8 * g(n, 3))
        v = _unit(nrm + 0.8 * g(n, 3))
        return np.concatenate([l, nrm, v, u(n, 3), u(n, 1) * 0.95 + 0.05, u(n, 1)], axis=1).astype(np.float32)
    if fn == 10:
        p = g(n, 3) * np.float32(5.0)
        p[: n // 4] *= np.float32(0.004)  # exercise the |p| < 1/32 branch
        return np.concatenate([p, _unit(g(n, 3))], axis=1).astype(np.float32)
    if fn == 11:
        return np.concatenate([g(n, 3) * 4, u(n, 3) * 3, u(n, 1) * 20 + 0.5, g(n, 3) * 4], axis=1).astype(np.float32)
    if fn == 12:
        return np.concatenate([g(n, 3) * 4, g(n, 1), u(n, 3) * 3, u(n, 1) * 8, _unit(g(n, 3)), g(n, 3) * 4],
                              axis=1).astype(np.float32)
    if fn == 13:
        o, tgt = g(n, 3) * 3, g(n, 3)
        v0, v1, v2 = tgt + g(n, 3), tgt + g(n, 3), tgt + g(n, 3)
        # second half: 2-5 cm triangles 10-40 units away, aimed at their interior, an edge or just past a
        # vertex (where the rounding of the edge functions decides), some axis-aligned and flat: the
        # population the box guard of the hit contract exists for
        h, m = n // 2, n - n // 2
        far = _unit(g(m, 3)) * (u(m, 1) * 30 + 10)
        e1, e2 = g(m, 3) * np.float32(0.03), g(m, 3) * np.float32(0.03)
        flat = np.arange(m) % 4 == 0
        e1[flat, 1] = 0.0
        e2[flat, 1] = 0.0
        a, b = u(m, 1) * 1.2 - 0.1, u(m, 1) * 1.2 - 0.1   # barycentrics slightly outside [0, 1] too
        b[np.arange(m) % 3 == 0] = 0.0                     # exactly on the v0-v1 edge (before rounding)
        tgt[h:] = far + a * e1 + b * e2
        v0[h:], v1[h:], v2[h:] = far, far + e1, far + e2
        d = _unit(tgt - o)
        return np.concatenate([o, d, v0, v1, v2, np.zeros((n, 1)), np.full((n, 1), np.inf)], axis=1).astype(np.float32)
    if fn == 14:
        x = g(n, 1) * np.float32(100.0)
        x[: n // 8] *= np.float32(1e-6)
        x[n // 8: n // 4] *= np.float32(1e4)
        return x.astype(np.float32)
    if fn == 15:
        return rng.integers(0, 4096, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    raise AssertionError(fn)


@pytest.mark.parametrize("fn", sorted(FN_SHAPES))
def test_device_functions_match_oracle_bitwise(gpu_ctx, oracle, fn):
    """Every device function of pt_device.hpp agrees with the oracle's restatement bit for bit."""
    rng = np.random.default_rng(1234 + fn)
    x = _fn_inputs(fn, 20000, rng)
    in_stride, out_stride = FN_SHAPES[fn]
    want = oracle.eval_fn(fn, x)
    got = gpu_ctx.eval_device_fn(fn, x, in_stride, out_stride)
    ok = same_bits(got, want)
    bad = np.argwhere(~ok)
    assert bad.size == 0, "fn %d: %d mismatches, first at %s: gpu=%r oracle=%r in=%r" % (
        fn, len(bad), bad[0], got[bad[0][0]], want[bad[0][0]], x[bad[0][0]])


DRAW_TYPES = ["PrimitiveID", "MeshID", "MaterialID", "Position", "ShadingNormal", "TexCoord0", "Albedo", "Roughness",
              "Metallic"]


@pytest.mark.parametrize("draw_type", DRAW_TYPES)
def test_cornell_debug_draw_types_bit_exact(gpu_ctx, oracle, cornell_world, draw_type):
    """C1-size DrawType images: traversal + fetch + decode + material, RNG-free after the jitter."""
    w = h = 256
    cam, fl = _camera(oracle, cornell_world, w, h)
    pc = default_pc(S, fl, draw_type=S.DrawType[draw_type], max_bounces=1)
    gpu_ctx.upload_scene(cornell_world)
    gpu_ctx.render(pc, cam, w, h)
    got = gpu_ctx.read_hdr()
    osc = oracle.OracleScene(cornell_world, brute_force=True)
    want, _ = osc.render(pc, cam, w, h)
    ok = same_bits(got, want).all(axis=2)
    assert ok.all(), "%s: %d of %d pixels differ" % (draw_type, (~ok).sum(), ok.size)


@pytest.mark.parametrize("draw_type", ["Albedo", "Roughness", "ShadingNormal", "Default"])
def test_texture_addressing_bit_exact(gpu_ctx, oracle, draw_type):
    """Every wrap mode x filter, power-of-two and odd texture sizes, UVs several periods either side of
    zero (scenes.texture_wall): texel addressing and bilinear weights, bit for bit."""
    world = scenes.texture_wall()
    w, h = 384, 256
    cam, fl = _camera(oracle, world, w, h)
    pc = default_pc(S, fl, draw_type=S.DrawType[draw_type], max_bounces=2)
    gpu_ctx.upload_scene(world)
    gpu_ctx.render(pc, cam, w, h)
    got = gpu_ctx.read_hdr()
    want, _ = oracle.OracleScene(world, brute_force=True).render(pc, cam, w, h)
    ok = same_bits(got, want).all(axis=2)
    assert ok.all(), "%s: %d of %d pixels differ" % (draw_type, (~ok).sum(), ok.size)
    if draw_type == "Albedo":  # the quads really are textured
        assert len(np.unique(got[..., :3].reshape(-1, 3), axis=0)) > 1000


@pytest.mark.parametrize("max_bounces,ibl,dof", [(1, False, False), (4, False, False), (6, True, True)])
def test_cornell_radiance_bit_exact_over_accumulated_frames(gpu_ctx, oracle, cornell_world, max_bounces, ibl, dof):
    """C1 (256x256, 1 bounce) and deeper variants: four accumulated frames, every pixel identical."""
    w = h = 256
    cam, fl = _camera(oracle, cornell_world, w, h)
    gpu_ctx.upload_scene(cornell_world)
    osc = oracle.OracleScene(cornell_world, brute_force=True)
    want = None
    for frame in range(1, 5):
        pc = default_pc(S, fl, frame_index=frame, max_bounces=max_bounces, ibl=ibl, dof=dof,
                        skip_history=(frame == 1), roulette=2)
        pc.apertureDiameter = 0.05 if dof else 1e-5
        pc.focusDistance = 3.0
        gpu_ctx.render(pc, cam, w, h)
        want, _ = osc.render(pc, cam, w, h, history=want)
    got = gpu_ctx.read_hdr()
    ok = same_bits(got, want).all(axis=2)
    assert ok.all(), "%d of %d pixels differ; max abs diff %g" % (
        (~ok).sum(), ok.size, np.nanmax(np.abs(got - want)))
    assert np.isfinite(got).all()
    assert (got[..., 3] == 4.0).all()


@pytest.mark.parametrize("factor", [0.01, 100.0, 3000.0])
def test_scene_scale_sweep_bit_exact(gpu_ctx, oracle, factor):
    """S-cornell scaled through its instance transforms (lights and camera with it): the BVH padding, the node-local
    fp16 boxes and the box guard are all relative to coordinate magnitude, so parity must hold at 2 cm, 200 m
    and 6 km scene size alike (positions stay fp16 in object space)."""
    from prosper_amd.world import scale as scale_matrix
    world = scenes.cornell(with_skybox=True)
    sm = scale_matrix((factor, factor, factor))
    world.model_instances = [(mi, sm @ m) for mi, m in world.model_instances]
    for i in range(world.point_lights.count):
        p = world.point_lights.lights[i].position
        p.x, p.y, p.z = p.x * factor, p.y * factor, p.z * factor
        r = world.point_lights.lights[i].radianceAndRadius
        r.x, r.y, r.z, r.w = r.x * factor * factor, r.y * factor * factor, r.z * factor * factor, r.w * factor
    for i in range(world.spot_lights.count):
        p = world.spot_lights.lights[i].positionAndAngleOffset
        p.x, p.y, p.z = p.x * factor, p.y * factor, p.z * factor
        r = world.spot_lights.lights[i].radianceAndAngleScale
        r.x, r.y, r.z = r.x * factor * factor, r.y * factor * factor, r.z * factor * factor
    c = world.camera
    world.camera = dict(c, eye=tuple(v * factor for v in c["eye"]), target=tuple(v * factor for v in c["target"]))
    w, h = 192, 128
    cam, fl = _camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    osc = oracle.OracleScene(world, brute_force=True)
    want = None
    for frame in (1, 2):
        pc = default_pc(S, fl, frame_index=frame, max_bounces=4, ibl=True, skip_history=(frame == 1))
        gpu_ctx.render(pc, cam, w, h)
        want, _ = osc.render(pc, cam, w, h, history=want)
    ok = same_bits(gpu_ctx.read_hdr(), want).all(axis=2)
    assert ok.all(), "scale %g: %d of %d pixels differ" % (factor, (~ok).sum(), ok.size)
    pos_pc = default_pc(S, fl, draw_type=S.DrawType["PrimitiveID"], max_bounces=1)
    gpu_ctx.render(pos_pc, cam, w, h)
    want_id, _ = osc.render(pos_pc, cam, w, h)
    assert same_bits(gpu_ctx.read_hdr(), want_id).all() and (want_id[..., :3].sum(axis=2) > 0).mean() > 0.5


@pytest.mark.parametrize("draw_type", ["ShadingNormal", "Position", "TexCoord0", "Default"])
def test_instance_transform_zoo_bit_exact(gpu_ctx, oracle, draw_type):
    """Rotations, non-uniform scales, a shear and mirrored instances of a normal-mapped box (scenes.transform_zoo)."""
    world = scenes.transform_zoo()
    w, h = 320, 200
    cam, fl = _camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    osc = oracle.OracleScene(world, brute_force=True)
    want = None
    for frame in (1, 2):
        pc = default_pc(S, fl, frame_index=frame, draw_type=S.DrawType[draw_type], max_bounces=3, skip_history=(frame == 1))
        gpu_ctx.render(pc, cam, w, h)
        want, _ = osc.render(pc, cam, w, h, history=want)
    ok = same_bits(gpu_ctx.read_hdr(), want).all(axis=2)
    assert ok.all(), "%s: %d of %d pixels differ" % (draw_type, (~ok).sum(), ok.size)
    assert (want[..., :3].sum(axis=2) != 0).mean() > 0.05


@pytest.mark.parametrize("kw", [
    dict(accumulate=False, skip_history=False),           # no running mean: (colour, 1) every frame
    dict(clamp=False, max_bounces=6, roulette=0),          # unclamped indirect, roulette from the second bounce
    dict(max_bounces=9, roulette=6),                       # PC above the shader's MAX_BOUNCES cap: 6 bounces, no roulette
    dict(max_bounces=2, ibl=True, dof=True, roulette=0),
    dict(max_bounces=1, ibl=True, clamp=False),
])
def test_push_constant_flag_matrix_bit_exact(gpu_ctx, oracle, cornell_world, kw):
    """ReferencePC flag / bound combinations (RtReference.cpp:77-88, main.rgen:26-30,241-244,269-276): three frames each."""
    w, h = 128, 96
    cam, fl = _camera(oracle, cornell_world, w, h)
    gpu_ctx.upload_scene(cornell_world)
    osc = oracle.OracleScene(cornell_world, brute_force=True)
    want = None
    for frame in (1, 2, 3):
        args = dict(kw)
        args.setdefault("skip_history", frame == 1)
        pc = default_pc(S, fl, frame_index=frame, **args)
        pc.apertureDiameter = 0.08 if kw.get("dof") else 1e-5
        pc.focusDistance = 2.5
        gpu_ctx.render(pc, cam, w, h)
        want, _ = osc.render(pc, cam, w, h, history=want)
    ok = same_bits(gpu_ctx.read_hdr(), want).all(axis=2)
    assert ok.all(), "%r: %d of %d pixels differ" % (kw, (~ok).sum(), ok.size)


def test_render_frames_equals_repeated_render(gpu_ctx, oracle, cornell_world):
    """prosper_pt_render_frames(n) == n x prosper_pt_render (history kept in registers vs HBM)."""
    w, h = 320, 200
    cam, fl = _camera(oracle, cornell_world, w, h)
    gpu_ctx.upload_scene(cornell_world)
    for frame in range(1, 6):
        pc = default_pc(S, fl, frame_index=frame, skip_history=(frame == 1))
        gpu_ctx.render(pc, cam, w, h)
    one_by_one = gpu_ctx.read_hdr()
    pc = default_pc(S, fl, frame_index=1, skip_history=True)
    gpu_ctx.render(pc, cam, w, h, frames=5)
    batched = gpu_ctx.read_hdr()
    assert same_bits(one_by_one, batched).all()


def test_counters_match_oracle(gpu_ctx, oracle, cornell_world):
    """BVH-independent work counters are exact integers shared by both implementations."""
    w = h = 128
    cam, fl = _camera(oracle, cornell_world, w, h)
    pc = default_pc(S, fl, max_bounces=4)
    gpu_ctx.upload_scene(cornell_world)
    gpu_ctx.reset_counters()
    gpu_ctx.render(pc, cam, w, h, flags=S.RENDER_COUNT_WORK)
    got = gpu_ctx.counters().as_dict()
    counted = gpu_ctx.read_hdr()
    gpu_ctx.render(pc, cam, w, h)
    assert same_bits(counted, gpu_ctx.read_hdr()).all(), "instrumented kernel changed the image"
    osc = oracle.OracleScene(cornell_world, brute_force=False)
    _, oc = osc.render(pc, cam, w, h)
    want = oc.as_dict()
    for key in ("paths", "closestRays", "shadowRays", "closestHits", "lightSamples", "spotLightSamples", "skyLookups",
                "pixelsWritten", "historyReads"):
        assert got[key] == want[key], key
    assert got["nodeVisits"] > 0 and got["triangleTests"] > 0


# ---------------------------------------------------------------------------------------------
# committed goldens, larger scenes, tiles, host class, full-size properties
# ---------------------------------------------------------------------------------------------

import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_gpu_reproduces_committed_goldens(gpu_ctx, cornell_world):
    """tests/golden/cornell_48.npz (every DrawType + Default radiance), bit for bit."""
    spec = importlib.util.spec_from_file_location("make_images", os.path.join(HERE, "golden", "make_images.py"))
    make_images = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make_images)
    golden = np.load(os.path.join(HERE, "golden", "cornell_48.npz"))
    cam = S.CameraUniforms.from_buffer_copy(golden["camera"].tobytes())
    gpu_ctx.upload_scene(cornell_world)

    def render(pc, hist):
        # history lives in the context's HDR buffer: frames are rendered in golden order
        gpu_ctx.render(pc, cam, 48, 48)
        return gpu_ctx.read_hdr()

    images = make_images.render_all(render)
    for name, img in images.items():
        assert same_bits(img, golden[name]).all(), name


@pytest.fixture(scope="module")
def sponza_small():
    from prosper_amd import scenes
    return scenes.sponza_class(lights=True, foliage=True, texture_size=64, sky_size=32, detail=0.25)


@pytest.mark.parametrize("draw_type", ["PrimitiveID", "ShadingNormal", "Albedo", "Roughness", "TexCoord0"])
def test_sponza_class_debug_draw_types_bit_exact(gpu_ctx, oracle, sponza_small, draw_type):
    """Instancing, u16+u32 indices, two geometry buffers, textures, normal maps, alpha foliage."""
    w, h = 240, 136
    cam, fl = _camera(oracle, sponza_small, w, h)
    pc = default_pc(S, fl, draw_type=S.DrawType[draw_type], max_bounces=1)
    gpu_ctx.upload_scene(sponza_small)
    gpu_ctx.render(pc, cam, w, h)
    got = gpu_ctx.read_hdr()
    want, _ = oracle.OracleScene(sponza_small).render(pc, cam, w, h)
    ok = same_bits(got, want).all(axis=2)
    assert ok.all(), "%s: %d of %d pixels differ" % (draw_type, (~ok).sum(), ok.size)


def test_sponza_class_radiance_bit_exact(gpu_ctx, oracle, sponza_small):
    """C4-style: 1024 punctual lights + sun + IBL + stochastic foliage, 3 accumulated frames."""
    w, h = 240, 136
    cam, fl = _camera(oracle, sponza_small, w, h)
    gpu_ctx.upload_scene(sponza_small)
    st = gpu_ctx.scene_stats()
    assert st.triangleCount == sponza_small.triangle_count() and st.maxDepth <= 96
    osc = oracle.OracleScene(sponza_small)
    want = None
    for frame in (1, 2, 3):
        pc = default_pc(S, fl, frame_index=frame, max_bounces=4, ibl=True, skip_history=(frame == 1))
        gpu_ctx.render(pc, cam, w, h)
        want, _ = osc.render(pc, cam, w, h, history=want)
    got = gpu_ctx.read_hdr()
    ok = same_bits(got, want).all(axis=2)
    assert ok.all(), "%d of %d pixels differ; max abs diff %g" % ((~ok).sum(), ok.size, np.nanmax(np.abs(got - want)))


def test_traversal_semantics_on_gpu(gpu_ctx, oracle):
    """The tiny-scene cases of test_oracle_traversal.py seen through whole renders."""
    from prosper_amd import scenes
    world = scenes.tiny_triangles()
    w = h = 64
    cam, fl = _camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    osc = oracle.OracleScene(world, brute_force=True)
    for frame in (1, 7, 4095, 0):  # frameIndex wraps mod 4096 (RtReference.cpp:170)
        pc = default_pc(S, fl, frame_index=frame, draw_type=S.DrawType["MeshID"], max_bounces=1)
        gpu_ctx.render(pc, cam, w, h)
        want, _ = osc.render(pc, cam, w, h)
        assert same_bits(gpu_ctx.read_hdr(), want).all()
    # an instance whose mesh has no indices yet (inactive TLAS instance, World.cpp:878-928) is invisible;
    # seen from behind (no face culling) the scene still renders
    from test_oracle_traversal import _with_inactive_instance
    world2 = _with_inactive_instance()
    gpu_ctx.upload_scene(world2)
    gpu_ctx.render(pc, cam, w, h)
    assert same_bits(gpu_ctx.read_hdr(), want).all()
    world.camera = dict(world.camera, eye=(0.0, 0.0, -5.0))
    cam2, fl2 = _camera(oracle, world, w, h)
    pc2 = default_pc(S, fl2, draw_type=S.DrawType["PrimitiveID"], max_bounces=1)
    gpu_ctx.upload_scene(world)
    gpu_ctx.render(pc2, cam2, w, h)
    back, _ = osc.render(pc2, cam2, w, h)
    assert same_bits(gpu_ctx.read_hdr(), back).all() and (back[..., :3].sum(axis=2) > 0).any()


def test_stripe_tiles_equal_whole_image(gpu_ctx, oracle, cornell_world):
    """prosper_pt_tile_desc: the union of the ranks' tiles is the single-GPU image, bit for bit."""
    from prosper_amd import tiling
    w, h = 256, 72
    cam, fl = _camera(oracle, cornell_world, w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    gpu_ctx.upload_scene(cornell_world)
    gpu_ctx.render(pc, cam, w, h, frames=2)
    whole = gpu_ctx.read_hdr()
    for world_size in (2, 4, 8):
        tiles = []
        for r in range(world_size):
            gpu_ctx.render(pc, cam, w, h, tile=tiling.tile_for_rank(r, world_size), frames=2)
            t = gpu_ctx.read_hdr()
            assert t.shape == (h, w // world_size, 4)
            tiles.append(t)
        assert same_bits(tiling.deinterleave(tiles, w), whole).all(), world_size


def test_rgba16f_blit_rounds_to_nearest_even(gpu_ctx, oracle, cornell_world):
    w, h = 64, 64
    cam, fl = _camera(oracle, cornell_world, w, h)
    gpu_ctx.upload_scene(cornell_world)
    gpu_ctx.render(default_pc(S, fl), cam, w, h)
    f32 = gpu_ctx.read_hdr()
    f16 = gpu_ctx.blit_rgba16f()
    assert (f16.view(np.uint16) == f32.astype(np.float16).view(np.uint16)).all()


def test_rt_reference_host_class_semantics(oracle, cornell_world):
    """render::RtReference (C++ host): frame index, history dirtiness, drawUi, releasePreserved —
    RtReference.cpp:148-159,170,189-216,278-298,385-391."""
    from prosper_amd.rt_reference import Camera, RtReference
    w, h = 96, 64
    rt = RtReference()
    rt.init(0)
    rt.set_world(cornell_world)
    cam = Camera.from_world(cornell_world, w, h)
    rt.draw_ui(maxBounces=4)
    pcs = [rt.record(cam, w, h) for _ in range(3)]
    assert [p.frameIndex for p in pcs] == [1, 2, 3]                    # pre-incremented: first frame is 1
    assert [p.flags & 1 for p in pcs] == [1, 0, 0]                     # skipHistory on the first frame only
    assert all(p.flags & 2 and p.flags & 16 for p in pcs)              # accumulate + clampIndirect defaults
    assert pcs[0].maxBounces == 4 and pcs[0].rouletteStartBounce == 3
    got = rt.context.read_hdr()
    assert (got[..., 3] == 3.0).all()
    # the same three frames straight through the C-ABI + oracle
    cu, fl = cam.update_buffer()
    osc = oracle.OracleScene(cornell_world, brute_force=True)
    want = None
    for p in pcs:
        want, _ = osc.render(p, cu, w, h, history=want)
    assert same_bits(got, want).all()
    # drawUi: changing anything but `accumulate` restarts history
    rt.draw_ui(maxBounces=4, accumulate=True)
    assert rt.record(cam, w, h).flags & 1 == 0
    rt.draw_ui(maxBounces=4, clampIndirect=False)
    p = rt.record(cam, w, h)
    assert p.flags & 1 == 1 and p.flags & 16 == 0 and p.frameIndex == 5
    # camera move, colorDirty, extent change, recompile and releasePreserved all skip history
    cam.look_at((0.0, 1.0, 3.0), (0.0, 1.0, 0.0))
    assert rt.record(cam, w, h).flags & 1 == 1
    assert rt.record(cam, w, h).flags & 1 == 0
    assert rt.record(cam, w, h, RtReference.Options(colorDirty=True)).flags & 1 == 1
    assert rt.record(cam, w + 16, h).flags & 1 == 1
    assert rt.record(cam, w + 16, h).flags & 1 == 0
    rt.recompile_shaders()
    assert rt.record(cam, w + 16, h).flags & 1 == 1
    rt.release_preserved()
    assert rt.record(cam, w + 16, h).flags & 1 == 1
    # a batch of frames advances the frame index by its length
    before = rt.record(cam, w + 16, h).frameIndex
    after = rt.record(cam, w + 16, h, frame_count=4)
    assert after.frameIndex == before + 1
    assert rt.record(cam, w + 16, h).frameIndex == before + 5
    # options reach the push constants (RtReference.cpp:278-298)
    p = rt.record(cam, w + 16, h, RtReference.Options(depthOfField=True, ibl=True, drawType="Albedo"))
    assert p.drawType == 8 and p.flags & 4 and p.flags & 8
    rt.close()


def test_error_paths_through_the_c_abi(gpu_ctx, oracle, cornell_world):
    import ctypes as C
    from prosper_amd import capi, world as W
    lib = capi.lib()
    fresh = capi.Context(device=0)
    cam, fl = _camera(oracle, cornell_world, 32, 32)
    pc = default_pc(S, fl)
    with pytest.raises(capi.ProsperPtError) as e:
        fresh.render(pc, cam, 32, 32)
    assert e.value.code == -4  # PROSPER_PT_ERR_NO_SCENE
    # a draw instance pointing past the mesh table is rejected by validation, not by a GPU fault
    bad = W.World()
    m = bad.add_material()
    from prosper_amd import scenes
    b = scenes.box()
    mesh = bad.add_mesh(b[0], b[4], m)
    bad.add_instance(bad.add_model([(mesh + 5, m)]))
    with pytest.raises(capi.ProsperPtError) as e:
        fresh.upload_scene(bad)
    assert e.value.code == -5 and "draw instance" in str(e.value)
    with pytest.raises(capi.ProsperPtError):
        fresh.render(S.ReferencePC(99, 0, 1, 0, 0, 0, 0, 1), cam, 32, 32)
    # empty scene renders (every ray misses)
    empty = W.World()
    fresh.upload_scene(empty)
    fresh.render(default_pc(S, fl), cam, 32, 32)
    img = fresh.read_hdr()
    assert (img[..., :3] == 0).all() and (img[..., 3] == 1).all()
    fresh.close()


def test_full_size_c2_properties(gpu_ctx, oracle, cornell_world):
    """BASELINE C2 size (1920x1080, 8 spp, 4 bounces): properties that do not need the oracle to
    trace 16.6 M paths — frame batching, determinism, counter identities — plus an exact check of a
    sampled set of rows against the oracle."""
    w, h, spp = 1920, 1080, 8
    cam, fl = _camera(oracle, cornell_world, w, h)
    gpu_ctx.upload_scene(cornell_world)
    pc = default_pc(S, fl, max_bounces=4)
    gpu_ctx.reset_counters()
    gpu_ctx.render(pc, cam, w, h, frames=spp, flags=S.RENDER_COUNT_WORK)
    a = gpu_ctx.read_hdr()
    c = gpu_ctx.counters().as_dict()
    assert c["paths"] == w * h * spp and c["pixelsWritten"] == w * h * spp and c["historyReads"] == w * h * (spp - 1)
    assert c["closestRays"] >= c["paths"] and c["closestHits"] <= c["closestRays"]
    assert c["shadowRays"] <= c["closestHits"] and c["lightSamples"] + c["spotLightSamples"] <= c["closestHits"]
    gpu_ctx.render(pc, cam, w, h, frames=spp)
    b = gpu_ctx.read_hdr()
    assert same_bits(a, b).all()                       # run-to-run determinism, counting kernel == timed kernel
    assert np.isfinite(b).all() and (b[..., 3] == spp).all()
    # two half batches == one batch (history through HBM vs registers)
    gpu_ctx.render(pc, cam, w, h, frames=3)
    pc2 = default_pc(S, fl, frame_index=4, max_bounces=4, skip_history=False)
    gpu_ctx.render(pc2, cam, w, h, frames=5)
    assert same_bits(gpu_ctx.read_hdr(), b).all()
    # exact oracle check on a 1920x24 band in the middle of the image (rendered as its own frames:
    # seeds are absolute pixel coordinates, so compare rows of a reduced-height oracle run is not
    # possible; instead compare full-width rows via a 2-frame render of the same extent)
    osc = oracle.OracleScene(cornell_world, brute_force=True)
    want = None
    for frame in (1, 2):
        p = default_pc(S, fl, frame_index=frame, max_bounces=4, skip_history=(frame == 1))
        gpu_ctx.render(p, cam, w, h)
    got2 = gpu_ctx.read_hdr()
    # oracle renders the whole 1920x1080 twice in a few seconds with all cores
    for frame in (1, 2):
        p = default_pc(S, fl, frame_index=frame, max_bounces=4, skip_history=(frame == 1))
        want, _ = osc.render(p, cam, w, h, history=want)
    assert same_bits(got2, want).all()


def test_c5_rank_tile_chunked_batch_properties(gpu_ctx, oracle, cornell_world):
    """BASELINE C5 as one of its 8 ranks sees it: 3840x2160, 64 spp, stripe 3 of 8.  66 M path slots exceed
    the 64 M-slot workspace cap, so the batch runs as two chunks: it must equal the same 64 frames
    accumulated 16 at a time, bit for bit, and the first stripe columns must equal a whole-width render."""
    from prosper_amd import tiling
    w, h, spp = 3840, 2160, 64
    cam, fl = _camera(oracle, cornell_world, w, h)
    gpu_ctx.upload_scene(cornell_world)
    tile = tiling.tile_for_rank(3, 8)
    pc = default_pc(S, fl, max_bounces=4)
    gpu_ctx.reset_counters()
    gpu_ctx.render(pc, cam, w, h, tile=tile, frames=spp, flags=S.RENDER_COUNT_WORK)
    a = gpu_ctx.read_hdr()
    lw = tiling.local_width(w, 3, 8)
    assert a.shape == (h, lw, 4) and np.isfinite(a).all() and (a[..., 3] == spp).all()
    c = gpu_ctx.counters().as_dict()
    assert c["paths"] == lw * h * spp and c["historyReads"] == lw * h * (spp - 1)
    for k in range(4):
        p = default_pc(S, fl, frame_index=1 + 16 * k, max_bounces=4, skip_history=(k == 0))
        gpu_ctx.render(p, cam, w, h, tile=tile, frames=16)
    assert same_bits(gpu_ctx.read_hdr(), a).all()
    # 2 spp of the same rank tile against the untiled image (absolute pixel seeds): stripe 3 = columns 48..63, ...
    gpu_ctx.render(pc, cam, w, h, tile=tile, frames=2)
    t2 = gpu_ctx.read_hdr()
    gpu_ctx.render(pc, cam, w, h, frames=2)
    full = gpu_ctx.read_hdr()
    cols = np.concatenate([np.arange(16) + 16 * (3 + 8 * j) for j in range(lw // 16)])
    assert same_bits(t2, full[:, cols]).all()


@pytest.fixture(scope="module")
def sponza_full():
    """S-sponza-class as BASELINE C3/C5 name it: 262 k triangles, 75 x 1024^2 textures, 512^2 sky."""
    return scenes.sponza_class()


def test_c5_own_workload_rank_tile(gpu_ctx, oracle, sponza_full):
    """BASELINE C5 on its OWN scene, as one of its 8 ranks sees it: S-sponza-class (full detail, 1024^2 textures, IBL),
    3840x2160, stripe set 3 of 8.  2 spp of the rank tile against the oracle, bit for bit; then the 64-spp batch
    (66 M path slots: two workspace chunks) against the same 64 frames accumulated 16 at a time, and the tile's columns
    against an untiled render."""
    from prosper_amd import tiling
    w, h, spp = 3840, 2160, 64
    cam, fl = _camera(oracle, sponza_full, w, h)
    gpu_ctx.upload_scene(sponza_full)
    st = gpu_ctx.scene_stats()
    assert st.triangleCount == sponza_full.triangle_count() and abs(st.triangleCount - 262144) < 2622
    tile = tiling.tile_for_rank(3, 8)
    lw = tiling.local_width(w, 3, 8)
    osc = oracle.OracleScene(sponza_full)
    want = None
    for frame in (1, 2):
        pc = default_pc(S, fl, frame_index=frame, max_bounces=4, ibl=True, skip_history=(frame == 1))
        want, _ = osc.render(pc, cam, w, h, history=want, tile=tile)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    gpu_ctx.render(pc, cam, w, h, tile=tile, frames=2)
    t2 = gpu_ctx.read_hdr()
    assert t2.shape == (h, lw, 4)
    ok = same_bits(t2, want).all(axis=2)
    assert ok.all(), "%d of %d pixels of the rank tile differ from the oracle" % ((~ok).sum(), ok.size)
    # the same 2 spp untiled: stripe 3 = columns 48..63, 176..191, ...
    gpu_ctx.render(pc, cam, w, h, frames=2)
    full = gpu_ctx.read_hdr()
    cols = np.concatenate([np.arange(16) + 16 * (3 + 8 * j) for j in range(lw // 16)])
    assert same_bits(t2, full[:, cols]).all()
    del full
    # 64 spp: one call (two chunks) == four calls of 16 frames
    gpu_ctx.reset_counters()
    gpu_ctx.render(pc, cam, w, h, tile=tile, frames=spp, flags=S.RENDER_COUNT_WORK)
    a = gpu_ctx.read_hdr()
    assert np.isfinite(a).all() and (a[..., 3] == spp).all()
    c = gpu_ctx.counters().as_dict()
    assert c["paths"] == lw * h * spp and c["historyReads"] == lw * h * (spp - 1)
    for k in range(4):
        p = default_pc(S, fl, frame_index=1 + 16 * k, max_bounces=4, ibl=True, skip_history=(k == 0))
        gpu_ctx.render(p, cam, w, h, tile=tile, frames=16, flags=S.RENDER_PIPELINED)
    assert same_bits(gpu_ctx.read_hdr(), a).all()


def test_two_launch_chains_equal_one_chain(gpu_ctx, oracle, sponza_small):
    """The default pipeline runs the segment groups as two chains of launches on two internal streams
    (tails of one overlap the other); PROSPER_PT_CREATE_SINGLE_CHAIN runs one chain on the caller's stream.
    Same pixels, same counters - also when the traversal stacks spill to the (per-chain) global overflow
    region, which a 16-entry LDS stack forces on this tree."""
    from prosper_amd import capi
    w, h = 1920, 1080  # 16 k segments: large enough for the split to happen
    cam, fl = _camera(oracle, sponza_small, w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    single = capi.Context(device=0, flags=S.CREATE_SINGLE_CHAIN)
    try:
        for forced in (None, "16"):
            if forced:
                capi.debug(ldsStackEntries=int(forced))
            out = []
            for ctx in (gpu_ctx, single):
                ctx.upload_scene(sponza_small)
                ctx.reset_counters()
                ctx.set_kernel_timing(True)
                ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_COUNT_WORK)
                total, per = ctx.last_render_timing()
                ctx.set_kernel_timing(False)
                out.append((ctx.read_hdr(), ctx.counters().as_dict(), per))
            assert same_bits(out[0][0], out[1][0]).all(), forced
            for k in ("paths", "closestRays", "shadowRays", "closestHits", "nodeVisits", "triangleTests", "skyLookups"):
                assert out[0][1][k] == out[1][1][k], (forced, k)
            assert out[0][2]["wf_trace"][1] == 2 * out[1][2]["wf_trace"][1]  # twice the launches, half the size
    finally:
        capi.debug(ldsStackEntries=None)
        single.close()


def test_pipelined_renders_equal_in_order_renders(gpu_ctx, oracle, sponza_small):
    """PROSPER_PT_RENDER_PIPELINED (up to three frames in flight: the path stages of a render overlap the previous
    renders, taking the context's three workspaces in turn): an accumulation sequence - every frame reads the previous frame's image
    as history - and a sequence of independent frames into alternating output buffers give the same bits as the
    in-order default, also with spilled traversal stacks and with per-launch timing events on."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")  # the runtime the library already uses (torch would bring a second one)
    w, h = 640, 360
    nbytes = w * h * 16
    cam, fl = _camera(oracle, sponza_small, w, h)
    gpu_ctx.upload_scene(sponza_small)
    bufs = []
    for _ in range(2):
        ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(nbytes)) == 0
        bufs.append(ptr)

    def download(ptr):
        out = np.empty((h, w, 4), np.float32)
        assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ptr, ctypes.c_size_t(nbytes), 2) == 0  # device to host
        return out
    for forced in (None, "16"):
        if forced:
            capi.debug(ldsStackEntries=int(forced))
        results = []
        for flags in (0, S.RENDER_PIPELINED):
            gpu_ctx.set_kernel_timing(flags != 0)
            # (1) accumulation: frames 1..6, the first skips history; the pipelined pass mixes in an in-order and a
            # counted render (the flag is ignored with PROSPER_PT_RENDER_COUNT_WORK) between pipelined ones
            mixed = [flags, flags, 0, flags, flags | S.RENDER_COUNT_WORK, flags]
            for f in range(1, 7):
                pc = default_pc(S, fl, frame_index=f, max_bounces=3, ibl=True, skip_history=(f == 1))
                gpu_ctx.render(pc, cam, w, h, frames=1 + (f % 2), flags=mixed[f - 1] if flags else 0)
            acc = gpu_ctx.read_hdr()
            # (2) independent frames into two caller-owned buffers, used alternately, no sync in between
            for f in range(8):
                gpu_ctx.set_output_buffer(bufs[f % 2].value, nbytes)
                pc = default_pc(S, fl, frame_index=10 + f, max_bounces=2 + f % 3, ibl=True)
                gpu_ctx.render(pc, cam, w, h, flags=flags)
            assert hip.hipDeviceSynchronize() == 0
            results.append((acc, download(bufs[0]), download(bufs[1])))
            gpu_ctx.set_output_buffer(None, 0)
            gpu_ctx.set_kernel_timing(False)
        for a, b in zip(*results):
            assert same_bits(a, b).all(), forced
        assert (results[0][0][..., 3] == 9.0).all()  # 2+1+2+1+2+1 accumulated samples
    capi.debug(ldsStackEntries=None)
    for ptr in bufs:
        hip.hipFree(ptr)
    # and the last pipelined frame equals the oracle's
    pc = default_pc(S, fl, frame_index=17, max_bounces=2 + 7 % 3, ibl=True)
    want, _ = oracle.OracleScene(sponza_small).render(pc, cam, w, h)
    assert same_bits(results[1][2], want).all()


@pytest.mark.parametrize("draw_type", ["Default", "Albedo", "ShadingNormal", "MaterialID"])
def test_gltf_scene_bit_exact(gpu_ctx, oracle, draw_type):
    """A scene that came in through the glTF ingest (tests/golden/tiny_scene.gltf: MASK + BLEND materials, a
    nearest/mirrored sampler, an instanced mesh under a matrix node, sun + point + spot lights, its own
    camera): the same bits from the HIP path and the oracle."""
    import os
    from prosper_amd import gltf
    world = gltf.load_gltf(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_scene.gltf"))
    w, h = 320, 240
    cam, fl = _camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    osc = oracle.OracleScene(world, brute_force=True)
    want = None
    for frame in (1, 2, 3):
        pc = default_pc(S, fl, frame_index=frame, draw_type=S.DrawType[draw_type], max_bounces=4,
                        skip_history=(frame == 1))
        gpu_ctx.render(pc, cam, w, h)
        want, _ = osc.render(pc, cam, w, h, history=want)
    ok = same_bits(gpu_ctx.read_hdr(), want).all(axis=2)
    assert ok.all(), "%s: %d of %d pixels differ" % (draw_type, (~ok).sum(), ok.size)


def test_banded_batches_give_the_same_pixels(gpu_ctx, oracle, sponza_small):
    """Debug option bandedBatches (default: by scene size): every XCD's segments take the camera-ray batches of one band of
    the image instead of batches strided over all of it (pt_wavefront.hip, WavefrontBuffers::bandSegments).  Which segment
    a path lives in never decides a pixel: the same bits with and without, in order and with frames in flight, for frame
    counts that are not powers of two, for a rank's stripes, for an image smaller than a band, and equal to the oracle."""
    from prosper_amd import tiling
    cases = ((640, 360, 8, None), (200, 120, 5, None), (256, 144, 3, tiling.tile_for_rank(1, 2)), (72, 40, 70, None), (1920, 1080, 2, None))
    gpu_ctx.upload_scene(sponza_small)
    for w, h, frames, tile in cases:
        cam, fl = _camera(oracle, sponza_small, w, h)
        pc = default_pc(S, fl, max_bounces=3, ibl=True)
        images = []
        for banded in (0, 1):
            capi.debug(bandedBatches=banded)
            for flags in (0, S.RENDER_PIPELINED, S.RENDER_PIPELINED):
                gpu_ctx.render(pc, cam, w, h, tile=tile, frames=frames, flags=flags)
                images.append(gpu_ctx.read_hdr())
        capi.debug(bandedBatches=None)
        for other in images[1:]:
            assert same_bits(images[0], other).all(), (w, h, frames)
        assert (images[0][..., 3] == frames).all()
    w, h, frames, tile = cases[1]
    cam, fl = _camera(oracle, sponza_small, w, h)
    osc = oracle.OracleScene(sponza_small)
    want = None
    for f in range(frames):
        want, _ = osc.render(default_pc(S, fl, frame_index=1 + f, max_bounces=3, ibl=True, skip_history=(f == 0)), cam, w, h, history=want)
    capi.debug(bandedBatches=1)
    gpu_ctx.render(default_pc(S, fl, max_bounces=3, ibl=True), cam, w, h, frames=frames, flags=S.RENDER_PIPELINED)
    assert same_bits(gpu_ctx.read_hdr(), want).all()


def test_all_pipelines_produce_identical_pixels(gpu_ctx, oracle, cornell_world):
    """The default wavefront pipeline and PROSPER_PT_CREATE_MEGAKERNEL are the same function of (pixel, frame):
    identical images, identical counters, both equal to the oracle.  PROSPER_PT_CREATE_PERSISTENT is reserved."""
    from prosper_amd import capi
    w, h = 200, 120  # not a multiple of the 8x8 / 16x16 tiles: exercises partial tiles
    cam, fl = _camera(oracle, cornell_world, w, h)
    with pytest.raises(capi.ProsperPtError) as refused:
        capi.Context(device=0, flags=S.CREATE_PERSISTENT)
    assert refused.value.code == -6  # PROSPER_PT_ERR_UNSUPPORTED
    others = [capi.Context(device=0, flags=S.CREATE_MEGAKERNEL)]
    images, counts = [], []
    for ctx in [gpu_ctx] + others:
        ctx.upload_scene(cornell_world)
        ctx.reset_counters()
        ctx.render(default_pc(S, fl, max_bounces=5, ibl=True, roulette=1), cam, w, h, frames=3, flags=S.RENDER_COUNT_WORK)
        images.append(ctx.read_hdr())
        counts.append(ctx.counters().as_dict())
    for ctx in others:
        ctx.close()
    assert all(same_bits(images[0], other).all() for other in images[1:])
    # schedule-independent counters are identical; node visits / triangle tests / any-hit calls depend on
    # the order candidates are found in (slab test form, traversal scheduler) and only need to be close
    stable = [k for k in counts[0] if k not in ("nodeVisits", "triangleTests", "anyHitCalls", "shortIndexHits", "shortIndexTriangleTests",
                                                   "nodePhaseSteps", "trianglePhaseSteps")]
    for c in counts[1:]:
        assert {k: c[k] for k in stable} == {k: counts[0][k] for k in stable}
        assert abs(c["nodeVisits"] - counts[0]["nodeVisits"]) < 0.01 * counts[0]["nodeVisits"]
    osc = oracle.OracleScene(cornell_world, brute_force=True)
    want = None
    for f in (1, 2, 3):
        want, _ = osc.render(default_pc(S, fl, frame_index=f, max_bounces=5, ibl=True, roulette=1, skip_history=(f == 1)),
                             cam, w, h, history=want)
    assert same_bits(images[0], want).all()
    # maxBounces = 0 never traces: black image, count 1
    gpu_ctx.render(default_pc(S, fl, max_bounces=0), cam, w, h)
    z = gpu_ctx.read_hdr()
    assert (z[..., :3] == 0).all() and (z[..., 3] == 1).all()


@pytest.mark.parametrize("mode,create_flags,render_flags,want", [
    ("in_order", 0, 0, (1, 3, 3, 1)),
    ("single_chain", S.CREATE_SINGLE_CHAIN, 0, (1, 3, 3, 1)),
    ("pipelined", 0, S.RENDER_PIPELINED, (1, 3, 3, 1)),
    ("megakernel", S.CREATE_MEGAKERNEL, 0, (1, 0, 0, 0)),
])
def test_timing_readout_counts_the_launches_of_every_pipeline(oracle, cornell_world, mode, create_flags, render_flags, want):
    """prosper_pt_get_last_render_timing on a 64 x 64 Cornell render of 3 bounces (too small to split into chains): one
    generate, three shades, three traces and one accumulate launch in every wavefront mode, the one kernel of the
    megakernel pipeline; finite times >= 0 and a total > 0; the same numbers when read again, and still after timing was
    switched off and an untimed render ran.  A context without a timed render refuses the readout."""
    w = h = 64
    cam, fl = _camera(oracle, cornell_world, w, h)
    pc = default_pc(S, fl, max_bounces=3)
    names = ("wf_generate_extend", "wf_shade", "wf_trace", "wf_accumulate")
    ctx = capi.Context(device=0, flags=create_flags)
    try:
        ctx.upload_scene(cornell_world)
        ctx.render(pc, cam, w, h, flags=render_flags)
        with pytest.raises(capi.ProsperPtError) as refused:
            ctx.last_render_timing()
        assert refused.value.code == -1  # PROSPER_PT_ERR_INVALID_ARGUMENT
        ctx.set_kernel_timing(True)
        ctx.render(pc, cam, w, h, flags=render_flags)
        total, per = ctx.last_render_timing()
        print(mode, total, per)
        assert tuple(per[n][1] for n in names) == want
        assert np.isfinite(total) and total > 0
        assert all(np.isfinite(per[n][0]) and per[n][0] >= 0 for n in names)
        assert ctx.last_render_timing() == (total, per)
        ctx.set_kernel_timing(False)
        ctx.render(pc, cam, w, h, flags=render_flags)
        assert ctx.last_render_timing() == (total, per)
    finally:
        ctx.close()


def test_reserved_debug_options_are_refused():
    """The debug options of the removed experiments are reserved: each one, set alone on a fresh context before any
    upload or render, fails with PROSPER_PT_ERR_UNSUPPORTED and leaves the context's options as they were."""
    ctx = capi.Context(device=0)
    try:
        for name in ("poolVariant", "rawRecords", "tileOrder", "hipGraph", "pipelinedChains", "mergeLimit"):
            with pytest.raises(capi.ProsperPtError) as refused:
                ctx.set_debug(**{name: 1})
            assert refused.value.code == -6, name  # PROSPER_PT_ERR_UNSUPPORTED
            assert getattr(ctx.debug_options(), name) == 0, name
            ctx.set_debug()
    finally:
        ctx.close()


def test_lds_stack_variants_agree(gpu_ctx, oracle, sponza_small):
    """The traversal kernels are instantiated for 16/24/32-entry LDS stacks and picked by BVH depth;
    forcing the deeper variants must not change a pixel."""
    w, h = 160, 96
    cam, fl = _camera(oracle, sponza_small, w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    gpu_ctx.upload_scene(sponza_small)
    assert gpu_ctx.scene_stats().maxDepth <= 96
    gpu_ctx.render(pc, cam, w, h, frames=2)
    base = gpu_ctx.read_hdr()
    for forced in ("16", "24", "32"):  # 16 pushes the deeper entries of this tree into the global overflow array
        capi.debug(ldsStackEntries=int(forced))
        gpu_ctx.render(pc, cam, w, h, frames=2)
        assert same_bits(gpu_ctx.read_hdr(), base).all(), forced
    capi.debug(ldsStackEntries=None)


def test_lds_staged_tables_equal_global_memory_tables(gpu_ctx, oracle):
    """wf_shade stages draw instances, transforms, materials and lights in LDS when they fit in 16 KB.  The scene
    here is S-sponza-class with the first 24 + 24 lights of C4's sequences (about 8 KB of tables: the LDS variant
    is the one that runs - asserted through prosper_pt_scene_stats.variantFlags);
    debug option noLdsTables reads the tables from global memory.  Same bits, and the oracle's."""
    world = scenes.sponza_class(lights=(24, 24), foliage=True, texture_size=64, sky_size=32, detail=0.25)
    assert world.point_lights.count == 24 and world.spot_lights.count == 24
    w, h = 200, 120
    cam, fl = _camera(oracle, world, w, h)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    gpu_ctx.upload_scene(world)
    assert gpu_ctx.scene_stats().variantFlags & S.VARIANT_LDS_TABLES
    gpu_ctx.render(pc, cam, w, h, frames=2)
    base = gpu_ctx.read_hdr()
    capi.debug(noLdsTables=1)
    assert not (gpu_ctx.scene_stats().variantFlags & S.VARIANT_LDS_TABLES)
    gpu_ctx.render(pc, cam, w, h, frames=2)
    capi.debug(noLdsTables=None)
    assert same_bits(gpu_ctx.read_hdr(), base).all()
    osc = oracle.OracleScene(world)
    want = None
    for frame in (1, 2):
        want, _ = osc.render(default_pc(S, fl, frame_index=frame, max_bounces=4, ibl=True, skip_history=(frame == 1)),
                             cam, w, h, history=want)
    assert same_bits(base, want).all()
    # C4's 1024 lights (40 KB of light tables) do not fit: they stay in global memory while the instance / transform /
    # material tables are staged (the third variant of the kernel) - same bits again
    big = scenes.sponza_class(lights=True, foliage=False, texture_size=64, sky_size=32, detail=0.25)
    cam, fl = _camera(oracle, big, w, h)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    gpu_ctx.upload_scene(big)
    assert gpu_ctx.scene_stats().variantFlags & S.VARIANT_LDS_TABLES
    gpu_ctx.render(pc, cam, w, h, frames=2)
    staged = gpu_ctx.read_hdr()
    capi.debug(noLdsTables=1)
    gpu_ctx.render(pc, cam, w, h, frames=2)
    capi.debug(noLdsTables=None)
    assert same_bits(gpu_ctx.read_hdr(), staged).all()


def test_texture_packs_equal_separate_textures(gpu_ctx, oracle, sponza_small):
    """Materials whose base / MR / normal textures share extent and sampler are sampled from an interleaved copy
    (pt_scene.hpp MaterialPack: one footprint, four 8-byte loads for an opaque material - the compact pack - or four
    12-byte ones).  Same texels, same filter arithmetic: the images with the compact packs, the wide ones
    (debug option widePacks = 0 / 1) and without packs (noTexturePacks = 1; both read at upload) are
    bit-equal - on S-sponza-class and on a wall of odd-sized textures under every wrap mode and both filters, which also
    equals the oracle with either pack."""
    from prosper_amd.world import World
    w, h = 240, 136
    cam, fl = _camera(oracle, sponza_small, w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    images = []
    for variant, value in (("widePacks", 0), ("widePacks", 1), ("noTexturePacks", 1)):
        # opaque materials: the compact pack (8 bytes per texel; the default of big texture sets), the 12-of-16-byte one,
        # the textures themselves
        capi.debug(**{variant: value})
        gpu_ctx.upload_scene(sponza_small)
        assert bool(gpu_ctx.scene_stats().variantFlags & S.VARIANT_TEXTURE_PACKS) == (variant != "noTexturePacks")
        gpu_ctx.render(pc, cam, w, h, frames=2)
        images.append(gpu_ctx.read_hdr())
        capi.debug(**{variant: None})
    assert same_bits(images[0], images[1]).all() and same_bits(images[0], images[2]).all()

    rng = np.random.default_rng(7)
    world = World()
    k = 0
    for size in ((10, 7), (9, 16), (33, 8)):                      # (width, height): not multiples of the 4 x 2 tiles
        for mag in (S.FILTER_LINEAR, S.FILTER_NEAREST):
            for wrap in (S.WRAP_REPEAT, S.WRAP_MIRRORED_REPEAT, S.WRAP_CLAMP_TO_EDGE):
                smp = world.add_sampler(mag, mag, wrap, wrap)
                tex = [world.add_texture(rng.integers(0, 256, size=(size[1], size[0], 4), dtype=np.uint8)) for _ in range(3)]
                mat = world.add_material(base_color=(1, 1, 1, 1), metallic=1.0, roughness=1.0, base_tex=(tex[0], smp),
                                         mr_tex=(tex[1], smp), normal_tex=(tex[2], smp))
                x, y = (k % 6) * 1.1 - 3.3, (k // 6) * 1.1 - 1.65
                mesh = scenes._add(world, scenes.quad((x, y, 0), (x + 1, y, 0), (x + 1, y + 1, 0), (x, y + 1, 0), uv_scale=2.5), mat)
                world.add_instance(world.add_model([(mesh, mat)]))
                k += 1
    world.set_directional_light((1.0, 1.0, 1.0), 3.0, (-0.3, -0.4, -1.0))
    world.camera = dict(eye=(0.0, 0.0, 6.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=0.9, zN=0.1, zF=100.0)
    w, h = 384, 192
    cam, fl = _camera(oracle, world, w, h)
    osc = oracle.OracleScene(world, brute_force=True)
    wanted = {}
    for wide in (False, True):
        capi.debug(widePacks=1 if wide else 0)
        gpu_ctx.upload_scene(world)
        assert gpu_ctx.scene_stats().variantFlags & S.VARIANT_TEXTURE_PACKS
        for draw_type in ("Albedo", "Roughness", "Metallic", "ShadingNormal", "Default"):
            pc = default_pc(S, fl, draw_type=S.DrawType[draw_type], max_bounces=2)
            gpu_ctx.render(pc, cam, w, h)
            if draw_type not in wanted:
                wanted[draw_type], _ = osc.render(pc, cam, w, h)
            ok = same_bits(gpu_ctx.read_hdr(), wanted[draw_type]).all(axis=2)
            assert ok.all(), "%s (%s pack): %d of %d pixels differ" % (draw_type, "wide" if wide else "compact", (~ok).sum(), ok.size)
    capi.debug(widePacks=None)


def test_moved_instances_refit_equals_fresh_upload(gpu_ctx, oracle):
    """prosper_pt_update_transforms (prosper: World::updateScene + the per-frame TLAS rebuild, World.cpp:359-466,749-802):
    a refit on the GPU - new world triangles and new boxes for the unchanged tree, no host build.  After moving two
    instances the image equals a fresh upload of the moved scene, the flat (round-1) hierarchy's image and the
    oracle's, bit for bit; so does the image after the explicit host-side rebuild."""
    from prosper_amd import capi
    from prosper_amd.world import rotate_y, translate

    def build(moved):
        world = scenes.sponza_class(lights=(8, 8), foliage=True, texture_size=64, sky_size=32, detail=0.5)
        if moved:
            for i, delta in ((3, translate((0.4, 0.25, -0.3)) @ rotate_y(0.6)), (17, translate((-0.2, 0.0, 0.5)))):
                model, m = world.model_instances[i]
                world.model_instances[i] = (model, delta @ m)
        return world
    still, moved = build(False), build(True)
    w, h = 320, 180
    cam, fl = _camera(oracle, still, w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    gpu_ctx.upload_scene(still)
    full_build = gpu_ctx.scene_stats().bvhBuildSeconds
    nodes_at_upload = gpu_ctx.read_nodes()
    gpu_ctx.render(pc, cam, w, h, frames=2)
    before = gpu_ctx.read_hdr()
    gpu_ctx.update_transforms(moved)
    st = gpu_ctx.scene_stats()
    hs = gpu_ctx.hierarchy_state()
    assert st.triangleCount == moved.triangle_count() and st.bvhBuildSeconds == 0.0 and st.buildSeconds < full_build
    assert hs.refits == 1 and hs.rebuilds == 0 and hs.costRatio > 1.0 and hs.levels >= 3
    gpu_ctx.render(pc, cam, w, h, frames=2)
    refit = gpu_ctx.read_hdr()
    assert not same_bits(refit, before).all()  # the instances are in view: something moved
    fresh = capi.Context(device=0)
    try:
        images = []
        for flat in (False, True):
            if flat:
                capi.debug(flatBvh=1)
            fresh.upload_scene(moved)
            fresh.render(pc, cam, w, h, frames=2)
            images.append(fresh.read_hdr())
        capi.debug(flatBvh=None)
    finally:
        fresh.close()
    assert same_bits(refit, images[0]).all() and same_bits(refit, images[1]).all()
    osc = oracle.OracleScene(moved)
    want = None
    for frame in (1, 2):
        want, _ = osc.render(default_pc(S, fl, frame_index=frame, max_bounces=3, ibl=True, skip_history=(frame == 1)),
                             cam, w, h, history=want)
    assert same_bits(refit, want).all()
    # the host-side rebuild (re-split of the two moved instances): same image, a tree as good as a fresh one
    gpu_ctx.rebuild_hierarchy()
    hs = gpu_ctx.hierarchy_state()
    assert hs.rebuilds == 1 and abs(hs.costRatio - 1.0) < 1e-6 and gpu_ctx.scene_stats().bvhBuildSeconds > 0.0
    gpu_ctx.render(pc, cam, w, h, frames=2)
    assert same_bits(gpu_ctx.read_hdr(), refit).all()
    # moving them back restores the first image
    gpu_ctx.update_transforms(still)
    gpu_ctx.render(pc, cam, w, h, frames=2)
    assert same_bits(gpu_ctx.read_hdr(), before).all()
    # an unchanged table is a no-op; a table of the wrong length is refused
    refits = gpu_ctx.hierarchy_state().refits
    gpu_ctx.update_transforms(still)
    assert gpu_ctx.hierarchy_state().refits == refits
    with pytest.raises(capi.ProsperPtError):
        capi._check(capi.lib().prosper_pt_update_transforms(gpu_ctx._h, None, 3))
    # a rebuild that fails half way (forced) must not be mistaken for done: renders are refused until an update has gone
    # through, and then show the moved scene
    capi.debug(failNextUpdate=1)
    capi.debug(alwaysRebuild=1)
    with pytest.raises(capi.ProsperPtError):
        gpu_ctx.update_transforms(moved)
    capi.debug(failNextUpdate=None)
    capi.debug(alwaysRebuild=None)
    with pytest.raises(capi.ProsperPtError):
        gpu_ctx.render(pc, cam, w, h, frames=2)
    gpu_ctx.update_transforms(moved)
    gpu_ctx.render(pc, cam, w, h, frames=2)
    assert same_bits(gpu_ctx.read_hdr(), refit).all()
    # upload: the refit that runs right after the build rewrote every node with the bytes the emitter had written
    gpu_ctx.upload_scene(still)
    assert np.array_equal(gpu_ctx.read_nodes(), nodes_at_upload)


def test_refit_writes_the_emitters_bytes(gpu_ctx):
    """The device encoder of a node's child boxes (bvh_encode.hpp through encode_nodes_kernel) and the host emitter are
    the same code: with the refit at upload switched off (debug option noUploadRefit) the node array is the
    emitter's own, and it equals the refitted one byte for byte - on a scene with instancing, scaling and a skewed
    transform, and on the big one."""
    from prosper_amd.world import World
    empty = World()  # no geometry at all: the root the emitter writes (origin 0, child boxes at +inf) must survive the upload
    empty.add_material(base_color=(1.0, 1.0, 1.0, 1.0))
    empty.camera = dict(eye=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=0.9, zN=0.1, zF=100.0)
    for world in (scenes.transform_zoo(), scenes.sponza_class(foliage=True, texture_size=64, sky_size=32, detail=0.5), empty):
        capi.debug(noUploadRefit=1)
        gpu_ctx.upload_scene(world)
        emitted = gpu_ctx.read_nodes()
        capi.debug(noUploadRefit=None)
        gpu_ctx.upload_scene(world)
        refitted = gpu_ctx.read_nodes()
        assert emitted.shape == refitted.shape and (emitted.shape[0] > 8 or world is empty)
        if world is empty:
            assert emitted.shape[0] == 1 and (emitted[0, :3] == 0).all() and np.isfinite(emitted[0, :3].view(np.float32)).all()
            assert gpu_ctx.hierarchy_state().builtCost == 0.0
        differing = np.argwhere(emitted != refitted)
        assert differing.size == 0, "node %d word %d: emitter %08x, refit %08x" % (
            differing[0][0], differing[0][1], emitted[tuple(differing[0])], refitted[tuple(differing[0])])


def test_update_enqueued_on_a_stream_of_the_callers(gpu_ctx, oracle):
    """prosper_pt_update_transforms_async with a stream: the refit is enqueued by the call itself on that stream (not left
    to the next render), the renders that follow - on the same stream or, pipelined, on the library's own - wait for it."""
    import ctypes
    from prosper_amd.world import rotate_y, translate
    hip = ctypes.CDLL("libamdhip64.so")
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    try:
        still, moved = scenes.transform_zoo(), scenes.transform_zoo()
        for k in (0, 5):
            model, m = moved.model_instances[k]
            moved.model_instances[k] = (model, translate((0.5, 0.4, 0.3)) @ rotate_y(0.7) @ m)
        w, h = 256, 160
        cam, fl = _camera(oracle, still, w, h)
        pc = default_pc(S, fl, max_bounces=3)
        gpu_ctx.upload_scene(still)
        gpu_ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_PIPELINED, stream=stream.value)
        gpu_ctx.update_transforms(moved, stream=stream.value)
        assert gpu_ctx._world is moved
        images = []
        for flags in (S.RENDER_PIPELINED, 0):
            gpu_ctx.render(pc, cam, w, h, frames=2, flags=flags, stream=stream.value)
            images.append(gpu_ctx.read_hdr(stream.value))
        osc = oracle.OracleScene(moved, brute_force=True)
        want = None
        for frame in (1, 2):
            want, _ = osc.render(default_pc(S, fl, frame_index=frame, max_bounces=3, skip_history=(frame == 1)), cam, w, h,
                                 history=want)
        assert same_bits(images[0], want).all() and same_bits(images[1], want).all()
        assert gpu_ctx.hierarchy_state().refits == 1
    finally:
        assert hip.hipStreamSynchronize(stream) == 0
        assert hip.hipStreamDestroy(stream) == 0


def test_far_moves_trigger_the_host_side_rebuild(gpu_ctx, oracle):
    """A refit keeps the tree's shape: instances that travel far leave it with fat boxes.  The refit's surface-area measure
    notices (costRatio well above 1.3 after three instances crossed the hall), and the NEXT update has them re-split on the
    host - in the background, switched in once done (rebuilds == 1, the measure back at 1): the image is the oracle's before
    and after."""
    from prosper_amd.world import translate

    def pose(shift):
        world = scenes.sponza_class(lights=(4, 4), texture_size=64, sky_size=32, detail=0.25)
        for k in (2, 9, 14):
            model, m = world.model_instances[k]
            world.model_instances[k] = (model, translate((shift, 0.3 * shift, -0.5 * shift)) @ m)
        return world
    still, far, farther = pose(0.0), pose(14.0), pose(14.05)
    w, h = 256, 144
    cam, fl = _camera(oracle, still, w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    gpu_ctx.upload_scene(still)
    for world, rebuilds in ((far, 0), (farther, 1)):
        gpu_ctx.update_transforms(world)
        gpu_ctx.finish_mesh_updates()  # (the re-split runs on the context's worker thread: wait for it)
        gpu_ctx.render(pc, cam, w, h, frames=2)
        got = gpu_ctx.read_hdr()
        hs = gpu_ctx.hierarchy_state()
        assert hs.rebuilds == rebuilds, (hs.rebuilds, hs.costRatio)
        if rebuilds == 0:
            assert hs.costRatio > 1.3, hs.costRatio
        else:
            assert hs.costRatio < 1.05, hs.costRatio
        osc = oracle.OracleScene(world)
        want = None
        for frame in (1, 2):
            want, _ = osc.render(default_pc(S, fl, frame_index=frame, max_bounces=3, ibl=True, skip_history=(frame == 1)),
                                 cam, w, h, history=want)
        assert same_bits(got, want).all()


def test_refit_of_a_flat_tree_and_of_alpha_geometry(gpu_ctx, oracle):
    """The refit does not care how the tree was built: on the one-tree-over-everything hierarchy (debug option flatBvh)
    moved instances give the oracle's image of the moved scene too - here on the instance-transform zoo (mirrors, shears,
    non-uniform scales) and with MASK / BLEND quads among the movers (their any-hit records are object-space and stay)."""
    from prosper_amd.world import rotate_z, translate
    capi.debug(flatBvh=1)
    for builder, picks in ((scenes.transform_zoo, (1, 4, 6)), (scenes.alpha_wall, (0, 3, 17, 30))):
        still, moved = builder(), builder()
        for k in picks:
            model, m = moved.model_instances[k]
            moved.model_instances[k] = (model, translate((0.3, -0.2, 0.25)) @ rotate_z(0.4) @ m)
        w, h = 256, 160
        cam, fl = _camera(oracle, still, w, h)
        gpu_ctx.upload_scene(still)
        gpu_ctx.update_transforms(moved)
        want = None
        osc = oracle.OracleScene(moved, brute_force=True)
        for frame in (1, 2):
            pc = default_pc(S, fl, frame_index=frame, max_bounces=3, skip_history=(frame == 1))
            gpu_ctx.render(pc, cam, w, h)
            want, _ = osc.render(pc, cam, w, h, history=want)
        assert gpu_ctx.hierarchy_state().refits == 1
        ok = same_bits(gpu_ctx.read_hdr(), want).all(axis=2)
        assert ok.all(), "%s: %d of %d pixels differ" % (builder.__name__, (~ok).sum(), ok.size)


def test_moving_instances_between_frames_in_flight(gpu_ctx, oracle):
    """Updates interleaved with pipelined renders on one stream, as a frame loop makes them (App.cpp:516-578: update the
    scene, then record the pass): every frame shows the scene of ITS update - frames in flight neither see the next
    update nor delay it.  Each image equals a fresh context's render of that pose."""
    from prosper_amd import capi
    from prosper_amd.world import rotate_y, translate

    def pose(k):
        world = scenes.sponza_class(lights=(4, 4), texture_size=64, sky_size=32, detail=0.25)
        model, m = world.model_instances[5]
        world.model_instances[5] = (model, translate((0.15 * k, 0.05 * k, 0.0)) @ rotate_y(0.2 * k) @ m)
        return world
    poses = [pose(k) for k in range(4)]
    w, h = 256, 144
    cam, fl = _camera(oracle, poses[0], w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")  # the runtime the library itself uses: plain device buffers for the four images
    nbytes = w * h * 16
    outs = []
    for _ in poses:
        ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(nbytes)) == 0
        outs.append(ptr)
    gpu_ctx.upload_scene(poses[0])
    for k, world in enumerate(poses):
        gpu_ctx.update_transforms(world)
        gpu_ctx.set_output_buffer(outs[k].value, nbytes)
        gpu_ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_PIPELINED)
    assert hip.hipDeviceSynchronize() == 0
    gpu_ctx.set_output_buffer(0, 0)
    images = []
    for ptr in outs:
        img = np.zeros((h, w, 4), np.float32)
        assert hip.hipMemcpy(ctypes.c_void_p(img.ctypes.data), ptr, ctypes.c_size_t(nbytes), 2) == 0  # hipMemcpyDeviceToHost
        assert hip.hipFree(ptr) == 0
        images.append(img)
    fresh = capi.Context(device=0)
    try:
        for k, world in enumerate(poses):
            fresh.upload_scene(world)
            fresh.render(pc, cam, w, h, frames=2)
            assert same_bits(images[k], fresh.read_hdr()).all(), "pose %d" % k
    finally:
        fresh.close()


def test_drifting_instances_trigger_the_rebuild_with_frames_in_flight(gpu_ctx, oracle):
    """A GPU-bound frame loop that moves instances EVERY frame, three frames in flight, no host synchronisation: the refit
    whose measure says "the tree has degraded" is never the newest one - that has only just been enqueued when the next
    update arrives - so the measure is kept per scene version and the newest FINISHED one is read.  Instances carried far
    out of the hall must make an update rebuild by itself (prosper_pt_hierarchy_state.rebuilds), and every frame still
    shows its own pose."""
    from prosper_amd.world import translate

    def pose(k):
        world = scenes.sponza_class(lights=(4, 4), texture_size=64, sky_size=32, detail=0.25)
        for i in (3, 5, 7):
            model, m = world.model_instances[i]
            world.model_instances[i] = (model, translate((1.5 * k, 0.2 * k, 0.4 * k)) @ m)
        return world
    poses = [pose(k) for k in range(14)]  # 21 units in the end: far past the 30 % growth of the measure
    w, h = 192, 108
    cam, fl = _camera(oracle, poses[0], w, h)
    pc = default_pc(S, fl, max_bounces=2, ibl=True)
    gpu_ctx.upload_scene(poses[0])
    before = gpu_ctx.hierarchy_state()
    for world in poses[1:]:
        gpu_ctx.update_transforms(world)  # staged; the refit runs at the head of the render's own chain
        gpu_ctx.render(pc, cam, w, h, frames=8, flags=S.RENDER_PIPELINED)
    last = gpu_ctx.read_hdr()
    gpu_ctx.finish_mesh_updates()  # (a re-split may still be under way on the worker thread)
    after = gpu_ctx.hierarchy_state()
    assert after.rebuilds > before.rebuilds, "refits %d, rebuilds %d, measure x%.3f" % (after.refits, after.rebuilds, after.costRatio)
    assert after.costRatio < 1.3  # the tree is good again
    fresh = capi.Context(device=0)
    try:
        fresh.upload_scene(poses[-1])
        fresh.render(pc, cam, w, h, frames=8)
        assert same_bits(last, fresh.read_hdr()).all()
    finally:
        fresh.close()


def test_lights_updated_between_frames_in_flight(gpu_ctx, oracle):
    """prosper rewrites the three light buffers every frame (World.cpp:531-535).  prosper_pt_update_lights stages a
    changed set (an unchanged one is a no-op) and the next render copies it into the next of three device versions at the
    head of its own chain: every frame of a pipelined sequence shows the lights of ITS update - equal to the oracle's
    image of that light set - and nothing synchronises the device."""
    import ctypes
    import copy

    def lit(k):
        world = scenes.cornell(with_skybox=True)
        if k >= 1:
            world.add_point_light((0.2, 0.9, 0.3), 30.0 + 10.0 * k, (0.4 - 0.3 * k, 1.2, 0.6))
        if k >= 2:
            world.add_spot_light((0.9, 0.3, 0.2), 120.0, (-0.6, 1.7, 0.9), (0.3, -0.8, -0.4), 0.3, 0.6)
        if k >= 3:
            world.set_directional_light((1.0, 0.9, 0.8), 1.5, (-0.4, -1.0, -0.3))
        return world
    worlds = [lit(k) for k in range(4)]
    w, h = 224, 160
    cam, fl = _camera(oracle, worlds[0], w, h)
    pc = default_pc(S, fl, max_bounces=3)
    hip = ctypes.CDLL("libamdhip64.so")
    nbytes = w * h * 16
    outs = []
    for _ in worlds:
        ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(nbytes)) == 0
        outs.append(ptr)
    gpu_ctx.upload_scene(worlds[0])
    for k, world in enumerate(worlds):
        gpu_ctx.update_lights(world)
        gpu_ctx.update_lights(world)  # again: nothing changed, nothing happens
        gpu_ctx.set_output_buffer(outs[k].value, nbytes)
        gpu_ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_PIPELINED)
    assert hip.hipDeviceSynchronize() == 0
    gpu_ctx.set_output_buffer(0, 0)
    for k, world in enumerate(worlds):
        img = np.zeros((h, w, 4), np.float32)
        assert hip.hipMemcpy(ctypes.c_void_p(img.ctypes.data), outs[k], ctypes.c_size_t(nbytes), 2) == 0
        assert hip.hipFree(outs[k]) == 0
        osc = oracle.OracleScene(world, brute_force=True)
        want = None
        for frame in (1, 2):
            want, _ = osc.render(default_pc(S, fl, frame_index=frame, max_bounces=3, skip_history=(frame == 1)), cam, w, h,
                                 history=want)
        ok = same_bits(img, want).all(axis=2)
        assert ok.all(), "light set %d: %d of %d pixels differ" % (k, (~ok).sum(), ok.size)
    # in-order renders and the counting kernels see the staged set too
    gpu_ctx.update_lights(worlds[1])
    gpu_ctx.render(pc, cam, w, h, frames=2)
    osc = oracle.OracleScene(worlds[1], brute_force=True)
    want = None
    for frame in (1, 2):
        want, _ = osc.render(default_pc(S, fl, frame_index=frame, max_bounces=3, skip_history=(frame == 1)), cam, w, h, history=want)
    assert same_bits(gpu_ctx.read_hdr(), want).all()


def test_every_kind_of_update_between_frames_in_flight_wraps_the_rings(gpu_ctx, oracle):
    """Nine states of one scene, each with another pose of one instance, another light set and another base colour (and
    alpha: the any-hit records follow) of one material than the state before, each updated and rendered pipelined into
    a buffer of its own with no host synchronisation in between: the three-version rings of transforms, lights and
    material tables wrap three times and the four-buffer staging rings twice, so versions and pinned buffers are REUSED
    behind frames in flight.  Every image equals a fresh context's in-order render of an upload of its state."""
    import copy
    import ctypes
    from prosper_amd.world import rotate_y, translate

    def state(k):
        world = scenes.cornell(with_skybox=True)
        model, m = world.model_instances[2]
        world.model_instances[2] = (model, translate((-0.05 * k, 0.02 * k, 0.03 * k)) @ rotate_y(0.2 * k) @ m)
        world.add_point_light((0.3 + 0.07 * k, 0.9 - 0.05 * k, 0.4), 10.0 + 4.0 * k, (0.7 - 0.15 * k, 1.3, 0.5))
        if k % 3 == 2:
            world.add_spot_light((0.9, 0.3, 0.2), 60.0 + k, (-0.6, 1.7, 0.9), (0.3, -0.8, -0.4), 0.3, 0.6)
        i = [j for j, mat in enumerate(world.materials) if mat.alphaMode == S.ALPHA_MODE_BLEND][0]
        mat = copy.copy(world.materials[i])
        mat.baseColorFactor = S.Vec4(0.2 + 0.08 * k, 0.4, 0.9 - 0.06 * k, 0.3 + 0.05 * k)
        world.materials[i] = mat
        return world
    states = [state(k) for k in range(9)]
    w, h = 96, 64
    cam, fl = _camera(oracle, states[0], w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    hip = ctypes.CDLL("libamdhip64.so")
    nbytes = w * h * 16
    outs = []
    for _ in states:
        ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(ptr), ctypes.c_size_t(nbytes)) == 0
        outs.append(ptr)
    gpu_ctx.upload_scene(scenes.cornell(with_skybox=True))
    for k, world in enumerate(states):
        gpu_ctx.update_transforms(world)
        gpu_ctx.update_lights(world)
        gpu_ctx.update_materials(world.materials, 0)
        gpu_ctx.set_output_buffer(outs[k].value, nbytes)
        gpu_ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_PIPELINED)
    assert hip.hipDeviceSynchronize() == 0
    gpu_ctx.set_output_buffer(0, 0)
    images = []
    for ptr in outs:
        img = np.zeros((h, w, 4), np.float32)
        assert hip.hipMemcpy(ctypes.c_void_p(img.ctypes.data), ptr, ctypes.c_size_t(nbytes), 2) == 0  # hipMemcpyDeviceToHost
        assert hip.hipFree(ptr) == 0
        images.append(img)
    fresh = capi.Context(device=0)
    try:
        for k, world in enumerate(states):
            fresh.upload_scene(world)
            fresh.render(pc, cam, w, h, frames=2)
            ok = same_bits(images[k], fresh.read_hdr()).all(axis=2)
            assert ok.all(), "state %d: %d of %d pixels differ" % (k, (~ok).sum(), ok.size)
        assert not same_bits(images[0], images[8]).all()  # (the states do differ)
    finally:
        fresh.close()


def test_pipelined_renders_survive_changing_extents(gpu_ctx, oracle, cornell_world):
    """Frames in flight while the image extent (and with it every slot's workspace size) changes from call to call,
    growing and shrinking: each image equals the in-order render of the same call."""
    gpu_ctx.upload_scene(cornell_world)
    extents = [(64, 64), (320, 200), (96, 48), (640, 360), (640, 360), (33, 17), (512, 288), (128, 128)]
    images = {}
    for flags in (0, S.RENDER_PIPELINED):
        out = []
        for k, (w, h) in enumerate(extents):
            cam, fl = _camera(oracle, cornell_world, w, h)
            pc = default_pc(S, fl, frame_index=1 + k, max_bounces=2 + k % 3)
            gpu_ctx.render(pc, cam, w, h, frames=1 + k % 2, flags=flags)
            out.append(gpu_ctx.read_hdr())
        images[flags] = out
    for a, b in zip(images[0], images[S.RENDER_PIPELINED]):
        assert same_bits(a, b).all()


def test_zero_throughput_rule_does_not_change_the_image(gpu_ctx, oracle, sponza_small):
    """Arithmetic contract: a path whose throughput is exactly (0, 0, 0) ends.  With debug option traceDeadPaths
    the kernels keep tracing such paths like the GLSL does: more rays (the counters say how many), the same bits in
    every pixel with clampIndirect on, the reference's default (without it the traced paths' NaN sky terms survive:
    DESIGN.md section 3) - on the small S-sponza-class scene with lights, foliage and IBL and on S-cornell, both pipelines."""
    from prosper_amd import capi
    for world, kw in ((sponza_small, dict(max_bounces=5, ibl=True, roulette=6)),
                      (scenes.cornell(with_skybox=True), dict(max_bounces=6, ibl=True, roulette=2))):
        w, h = 480, 270
        cam, fl = _camera(oracle, world, w, h)
        pc = default_pc(S, fl, **kw)
        for create in (0, S.CREATE_MEGAKERNEL):
            ctx = capi.Context(device=0, flags=create)
            try:
                ctx.upload_scene(world)
                out = []
                for audit in ("0", "1"):
                    capi.debug(traceDeadPaths=int(audit))
                    ctx.reset_counters()
                    ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_COUNT_WORK)
                    out.append((ctx.read_hdr(), ctx.counters().as_dict()))
                capi.debug(traceDeadPaths=None)
            finally:
                ctx.close()
            assert same_bits(out[0][0], out[1][0]).all(), create
            assert out[1][1]["closestRays"] > out[0][1]["closestRays"] * 1.1, create  # the dead paths are many
            assert out[1][1]["paths"] == out[0][1]["paths"]


def test_batched_texture_fetches_equal_sequential_ones(gpu_ctx, oracle, sponza_small):
    """sample_material<true> (big texture sets: the twelve texel loads of a hit's three textures in flight together)
    against the one-texture-after-the-other path, forced either way on the texture-addressing wall (every wrap mode
    and filter, odd sizes) and on the small S-sponza-class scene: same bits, and the wall equals the oracle."""
    for world, extent, kw in ((scenes.texture_wall(), (384, 256), dict(max_bounces=2)),
                              (sponza_small, (480, 270), dict(max_bounces=3, ibl=True))):
        w, h = extent
        cam, fl = _camera(oracle, world, w, h)
        pc = default_pc(S, fl, **kw)
        images = []
        for forced in ("0", "1"):
            capi.debug(batchedTextures=int(forced))
            gpu_ctx.upload_scene(world)
            gpu_ctx.render(pc, cam, w, h, frames=2)
            images.append(gpu_ctx.read_hdr())
        capi.debug(batchedTextures=None)
        assert same_bits(images[0], images[1]).all()
        if world is not sponza_small:
            want = None
            osc = oracle.OracleScene(world, brute_force=True)
            for f in range(2):
                p2 = default_pc(S, fl, frame_index=1 + f, skip_history=(f == 0), **kw)
                want, _ = osc.render(p2, cam, w, h, history=want)
            assert same_bits(images[1], want).all()


def test_hits_do_not_depend_on_the_hierarchy(gpu_ctx, oracle, sponza_small):
    """Hit contract: the box guard bounds where a triangle can be hit, so fatter BVH boxes (a different
    tree: other culling, other traversal order) must give the same bits."""
    w, h = 160, 96
    cam, fl = _camera(oracle, sponza_small, w, h)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    images, nodes = [], []
    for pad in (None, "1e-4", "3e-3"):
        if pad is None:
            capi.debug(boxPad=None)
        else:
            capi.debug(boxPad=float(pad))
        gpu_ctx.upload_scene(sponza_small)
        gpu_ctx.reset_counters()
        gpu_ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_COUNT_WORK)
        images.append(gpu_ctx.read_hdr())
        nodes.append(gpu_ctx.counters().nodeVisits)
    capi.debug(boxPad=None)
    assert nodes[0] < nodes[1] < nodes[2]  # the hierarchies really differ
    assert same_bits(images[0], images[1]).all() and same_bits(images[0], images[2]).all()


def test_lds_resident_scene_equals_global_memory_traversal(gpu_ctx, oracle, cornell_world):
    """Scenes of a few KB are traversed out of LDS (LdsGeom); same pixels as the HBM path."""
    w, h = 224, 128
    cam, fl = _camera(oracle, cornell_world, w, h)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    gpu_ctx.upload_scene(cornell_world)
    gpu_ctx.render(pc, cam, w, h, frames=2)
    lds = gpu_ctx.read_hdr()
    capi.debug(noLdsScene=1)
    gpu_ctx.render(pc, cam, w, h, frames=2)
    assert same_bits(gpu_ctx.read_hdr(), lds).all()
    capi.debug(noLdsScene=None)


def test_full_sponza_class_scene_parity(gpu_ctx, oracle):
    """The full 262 k-triangle S-sponza-class scene (64^2 textures) at reduced resolution: grazing rays
    over tessellated flats are where a traversal could disagree with the oracle about hit selection
    (DESIGN.md "hit contract"); every pixel must still match bit for bit."""
    from prosper_amd import scenes
    world = scenes.sponza_class(texture_size=64, sky_size=64)
    w, h = 320, 180
    cam, fl = _camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    osc = oracle.OracleScene(world)
    want = None
    for frame in (1, 2):
        pc = default_pc(S, fl, frame_index=frame, max_bounces=4, ibl=True, skip_history=(frame == 1))
        gpu_ctx.render(pc, cam, w, h)
        want, _ = osc.render(pc, cam, w, h, history=want)
    got = gpu_ctx.read_hdr()
    ok = same_bits(got, want).all(axis=2)
    assert ok.all(), "%d of %d pixels differ" % ((~ok).sum(), ok.size)


def test_random_configurations_bit_exact():
    """A fixed-seed slice of scripts/parity_fuzz.py (random poses, flags, bounces, frame counts, extents, rank tiles and
    moved instances over seven scenes); profiles/r03_parity_fuzz.txt keeps the long runs."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "parity_fuzz.py")
    spec = importlib.util.spec_from_file_location("parity_fuzz", path)
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    lines = []
    bad, pixels = fuzz.run(28, 11, ["cornell", "sponza", "foliage", "wall", "zoo", "alpha", "helmet"], log=lines.append)
    assert bad == 0, "\n".join(l for l in lines if "DIFFER" in l)
    assert pixels > 100000


def _full_size_parity(gpu_ctx, oracle, world, frames, label):
    """1920x1080 (BASELINE's extent), `frames` accumulated frames, maxBounces 4, IBL: every texel == the oracle's."""
    w, h = 1920, 1080
    cam, fl = _camera(oracle, world, w, h)
    gpu_ctx.upload_scene(world)
    osc = oracle.OracleScene(world)
    want = None
    for frame in range(1, frames + 1):
        pc = default_pc(S, fl, frame_index=frame, max_bounces=4, ibl=True, skip_history=(frame == 1))
        want, oracle_counters = osc.render(pc, cam, w, h, history=want)
    osc.close()
    # the batched entry point bench.py times (all frames resident at once, three frames in flight) ...
    gpu_ctx.render(default_pc(S, fl, max_bounces=4, ibl=True), cam, w, h, frames=frames, flags=S.RENDER_PIPELINED)
    got = gpu_ctx.read_hdr()
    ok = same_bits(got, want).all(axis=2)
    assert ok.all(), "%s: %d of %d pixels differ from the oracle (batched)" % (label, (~ok).sum(), ok.size)
    # ... and one record() per frame, as prosper makes them (RtReference.cpp:161-383)
    for frame in range(1, frames + 1):
        pc = default_pc(S, fl, frame_index=frame, max_bounces=4, ibl=True, skip_history=(frame == 1))
        gpu_ctx.render(pc, cam, w, h)
    assert same_bits(gpu_ctx.read_hdr(), want).all(), "%s: per-frame renders differ from the oracle" % label
    return got, oracle_counters.as_dict()


def test_full_size_c3_parity(gpu_ctx, oracle, sponza_full):
    """BASELINE C3 as bench.py times it - S-sponza-class, 262 k triangles, 75 x 1024^2 textures, 512^2 sky, 1920x1080 -
    2 spp against the oracle, bit for bit."""
    got, _ = _full_size_parity(gpu_ctx, oracle, sponza_full, 2, "C3")
    assert np.isfinite(got).all() and (got[..., 3] == 2).all()


def test_full_size_c4_parity(gpu_ctx, oracle):
    """BASELINE C4 at its own size: the C3 scene + 1024 point / spot lights + 20 k alpha-tested / blended foliage quads
    (302 k triangles, 1024^2 leaf masks), 1920x1080: 7.5 any-hit candidates per camera ray (rt/scene.rahit:18-39), the
    light pick over 1025 lights (main.rgen:195-223).  1 spp against the oracle, bit for bit, and the work counters that do
    not depend on the hierarchy."""
    world = scenes.sponza_class(lights=True, foliage=True)
    got, oc = _full_size_parity(gpu_ctx, oracle, world, 1, "C4")
    assert np.isfinite(got).all() and (got[..., 3] == 1).all()
    w, h = 1920, 1080
    cam, fl = _camera(oracle, world, w, h)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    gpu_ctx.reset_counters()
    gpu_ctx.render(pc, cam, w, h, flags=S.RENDER_COUNT_WORK)
    assert same_bits(gpu_ctx.read_hdr(), got).all()
    c = gpu_ctx.counters().as_dict()
    for k in ("paths", "closestRays", "closestHits", "shadowRays", "lightSamples", "spotLightSamples", "skyLookups",
              "pixelsWritten"):
        assert c[k] == oc[k], (k, c[k], oc[k])


def test_full_size_flight_helmet_parity(gpu_ctx, oracle):
    """The reference's one bundled asset (src/main.cpp:32-33) at 1920x1080, Default draw type + IBL, 2 spp."""
    from prosper_amd import flight_helmet
    got, _ = _full_size_parity(gpu_ctx, oracle, flight_helmet.load_fixture(), 2, "FlightHelmet")
    assert np.isfinite(got).all() and (got[..., 3] == 2).all()
