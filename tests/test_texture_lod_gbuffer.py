"""The traced G-buffer through the textures' mip chains: lambda read off a flat-roughness chain against
float64, the sampled material against the restatement fed the GPU's own uv and derivatives, and what must not change."""
import ctypes as C
import math

import numpy as np
import pytest

import texture_lod_reference as R
from prosper_amd import capi, scenes, structs as S
from prosper_amd.world import World

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 64, 48
LAMBDA_CAP = 2.0 ** -7  # what the bound may not exceed
LAMBDA_BOUND = 3.2e-3   # DESIGN.md (f14), "the derivative bound": the running error analysis' largest pixel, 3.11e-3


def corner_uvs(scale):
    return [(0.0, 0.0), (scale, 0.0), (scale, scale), (0.0, scale)]
# One tilted quad that fills the view; every coordinate and uv is a binary16 value.  uv is affine over the quad:
# u = scale * (x + 16) / 32, v = scale * (y + 8) / 24.
P = [(-16.0, -8.0, -6.0), (16.0, -8.0, -6.0), (16.0, 16.0, -22.0), (-16.0, 16.0, -22.0)]
NORMAL = np.cross(np.subtract(P[1], P[0]), np.subtract(P[3], P[0]))


def camera(oracle):
    return oracle.camera_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), math.radians(50.0), 0.1, 100.0, W, H)[0]


def quad_world(rng, uv_scale, mr_chain=None, normal_texture=False, alpha_mode=S.ALPHA_MODE_OPAQUE):
    w = World()
    base = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    mr = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    tb = w.add_texture(base)
    tm = w.add_texture_chain(mr_chain) if mr_chain is not None else w.add_texture(mr)
    tn = w.add_texture(rng.integers(100, 156, (64, 64, 4), dtype=np.uint8)) if normal_texture else 0
    m = w.add_material(base_color=(0.9, 0.8, 0.7, 1.0), metallic=0.75, roughness=1.0, base_tex=(tb, 0), mr_tex=(tm, 0),
                       normal_tex=(tn, 0), alpha_mode=alpha_mode)
    q = scenes._add(w, scenes.quad(*P, uv_scale=uv_scale), m)
    w.add_instance(w.add_model([(q, m)]))
    return w, base, (mr_chain if mr_chain is not None else mr)


def uv_of(scale):
    return lambda p: np.stack([scale * (p[..., 0] + 16.0) / 32.0, scale * (p[..., 1] + 8.0) / 24.0], axis=-1)


def mips_context(world, **debug):
    ctx = capi.Context(device=0, flags=S.CREATE_TEXTURE_MIPS)
    if debug:
        ctx.set_debug(**debug)
    ctx.upload_scene(world)
    return ctx


def test_lambda_read_off_a_flat_roughness_chain_against_float64(oracle):
    """|lambda_gpu - lambda_float64| <= the running forward error bound of the written-down sequence, pixel by pixel;
    its largest pixel is LAMBDA_BOUND = 3.2e-3 < 2^-7.  Measured: 2.6e-5."""
    rng = np.random.default_rng(31)
    chain = [np.zeros((64 >> l, 64 >> l, 4), np.uint8) for l in range(5)]
    for l, a in enumerate(chain):
        a[..., 1] = 40 + 20 * l
    world, _, _ = quad_world(rng, 8.0, mr_chain=chain)
    cam = camera(oracle)
    # float64 first: every pixel's lambda lies strictly inside (0, last level), so no pixel is excluded
    _, d64 = R.analytic_derivatives(cam, W, H, P[0], NORMAL, uv_of(8.0))
    lam64 = R.lambda64(64, 64, d64)
    print("lambda64 range %.4f .. %.4f" % (lam64.min(), lam64.max()))
    assert lam64.min() > 0.05 and lam64.max() < 3.95
    bound, _ = R.quad_error_bounds(cam, W, H, P, corner_uvs(8.0), (64, 64))
    print("error bound %.3e .. %.3e" % (bound.min(), bound.max()))
    assert bound.max() <= LAMBDA_BOUND <= LAMBDA_CAP
    ctx = mips_context(world)
    try:
        ctx.set_texture_lod(True, 0.0)
        ar, nm, depth = ctx.trace_gbuffer(cam, W, H, jitter=False)
        assert (depth > 0).all()
        lam = (ar[..., 3].astype(np.float64) * 255.0 - 40.0) / 20.0
        err = np.abs(lam - lam64)
        print("max |lambda_gpu - lambda64| = %.3e (bound %.3e)" % (err.max(), LAMBDA_BOUND))
        assert (err <= bound).all() and err.max() <= LAMBDA_BOUND
        # bias -1 moves every pixel down by one level (all stay above 0 where lambda64 > 1)
        ctx.set_texture_lod(True, -1.0)
        ar1 = ctx.trace_gbuffer(cam, W, H, jitter=False)[0]
        lam1 = (ar1[..., 3].astype(np.float64) * 255.0 - 40.0) / 20.0
        inside = lam64 > 1.05
        assert inside.any() and (np.abs(lam1 - (lam64 - 1.0)) <= bound + 1e-6)[inside].all()
        assert (np.abs(lam1[lam64 < 0.95]) <= 1e-6).all()  # lambda <= 0: level 0, code 40
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["unpacked", "packed", "compact"])
def test_the_sampled_material_is_the_restatement_fed_the_gpus_uv_and_derivatives(oracle, case):
    rng = np.random.default_rng(32)
    scale = 8.0 if case == "unpacked" else 2.0  # the packed cases straddle lambda = 0 and 1: level 0 out of the pack
    world, base, mr = quad_world(rng, scale, normal_texture=case != "unpacked")
    cam = camera(oracle)
    uv64, d64 = R.analytic_derivatives(cam, W, H, P[0], NORMAL, uv_of(scale))
    debug = {} if case == "unpacked" else {"widePacks": 1 if case == "packed" else 0}
    ctx = mips_context(world, **debug)
    try:
        assert bool(ctx.scene_stats().variantFlags & S.VARIANT_TEXTURE_PACKS) == (case != "unpacked")
        ctx.set_texture_lod(True, 0.0)
        ctx.set_texture_lod_debug(True)
        uv = ctx.trace_gbuffer(cam, W, H, draw_type=S.DRAW_TYPES.index("TexCoord0"), jitter=False)[0][..., :2]
        d = ctx.read_texture_lod_derivatives(W, H)
        # the derivatives against float64, within the bound of the same analysis expressed in uv: the four differences'
        # own running error bounds
        _, tol = R.quad_error_bounds(cam, W, H, P, corner_uvs(scale), (64, 64))
        print("max derivative error / bound = %.3e" % (np.abs(d - d64) / tol).max())
        assert (np.abs(d - d64) <= tol).all()
        assert np.abs(uv - uv64).max() <= 8 * 2.0 ** -20
        chains = (R.generate_chain(base, True), R.generate_chain(mr, False))
        smp = (1, 1, 0, 0)
        albedo, rough, metal, _ = R.sample_material_lod(chains, (smp, smp), ((0.9, 0.8, 0.7), 1.0, 0.75), uv.reshape(-1, 2), d.reshape(-1, 4), 0.0)
        lam = R.texture_lambda(64, 64, d.reshape(-1, 4), 0.0)
        assert (lam > 0).any() and (case == "unpacked" or ((lam <= 0).any() and ((lam > 0) & (lam < 1)).any()))
        got_albedo = ctx.trace_gbuffer(cam, W, H, draw_type=S.DRAW_TYPES.index("Albedo"), jitter=False)[0][..., :3]
        ar, nm, _ = ctx.trace_gbuffer(cam, W, H, jitter=False)
        assert (got_albedo.reshape(-1, 3).view(np.uint32) == albedo.view(np.uint32)).all()
        assert (ar[..., :3].reshape(-1, 3).view(np.uint32) == albedo.view(np.uint32)).all()
        assert (ar[..., 3].reshape(-1).view(np.uint32) == rough.view(np.uint32)).all()
        assert (nm[..., 2].reshape(-1).view(np.uint32) == metal.view(np.uint32)).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["unpacked", "packed", "compact"])
def test_what_must_not_change(gpu_ctx, oracle, case):
    rng = np.random.default_rng(33)
    cam = camera(oracle)
    debug = {} if case == "unpacked" else {"widePacks": 1 if case == "packed" else 0}
    # minified: depth, velocity and the geometric-normal case (no normal texture) are the same bytes off and on
    world, _, _ = quad_world(rng, 8.0, normal_texture=False)
    ctx = mips_context(world, **debug)
    try:
        off = ctx.trace_gbuffer(cam, W, H, jitter=True, frame_index=3)
        off_v = ctx.trace_gbuffer_velocity(cam, W, H)
        ctx.set_texture_lod(True, -1.0)
        on = ctx.trace_gbuffer(cam, W, H, jitter=True, frame_index=3)
        on_v = ctx.trace_gbuffer_velocity(cam, W, H)
        assert off[2].tobytes() == on[2].tobytes() and off_v[2].tobytes() == on_v[2].tobytes() and off_v[3].tobytes() == on_v[3].tobytes()
        assert off[1][..., [0, 1, 3]].tobytes() == on[1][..., [0, 1, 3]].tobytes()  # the encoded normal
        assert off[0].tobytes() != on[0].tobytes()  # (the material did change)
        for k in ("Position", "PrimitiveID", "TexCoord0"):
            ctx.set_texture_lod(False)
            a = ctx.trace_gbuffer(cam, W, H, draw_type=S.DRAW_TYPES.index(k), jitter=False)[0]
            ctx.set_texture_lod(True, 0.0)
            assert a.tobytes() == ctx.trace_gbuffer(cam, W, H, draw_type=S.DRAW_TYPES.index(k), jitter=False)[0].tobytes()
    finally:
        ctx.close()
    # magnified (texels larger than pixels everywhere, checked in float64): every target is the same bytes off and on,
    # and LOD off on a mips context is a context without the flag
    world, _, _ = quad_world(rng, 0.5, normal_texture=case != "unpacked")
    _, d64 = R.analytic_derivatives(cam, W, H, P[0], NORMAL, uv_of(0.5))
    assert R.lambda64(64, 64, d64).max() < -0.5
    gpu_ctx.set_debug(**debug) if debug else gpu_ctx.set_debug()
    gpu_ctx.upload_scene(world)
    plain = gpu_ctx.trace_gbuffer(cam, W, H, jitter=True, frame_index=5) + gpu_ctx.trace_gbuffer_velocity(cam, W, H)
    gpu_ctx.set_debug()
    ctx = mips_context(world, **debug)
    try:
        assert bool(ctx.scene_stats().variantFlags & S.VARIANT_TEXTURE_PACKS) == (case != "unpacked")
        off = ctx.trace_gbuffer(cam, W, H, jitter=True, frame_index=5) + ctx.trace_gbuffer_velocity(cam, W, H)
        ctx.set_texture_lod(True, 0.0)
        on = ctx.trace_gbuffer(cam, W, H, jitter=True, frame_index=5) + ctx.trace_gbuffer_velocity(cam, W, H)
        for a, b, c in zip(plain, off, on):
            assert a.tobytes() == b.tobytes() == c.tobytes()
    finally:
        ctx.close()


def test_enabling_needs_the_mips_flag(gpu_ctx):
    with pytest.raises(capi.ProsperPtError) as e:
        gpu_ctx.set_texture_lod(True, 0.0)
    assert e.value.code == -6
    gpu_ctx.set_texture_lod(False, -1.0)  # switching it off is always fine
    with pytest.raises(capi.ProsperPtError):
        gpu_ctx.read_texture_lod_derivatives(W, H)


def test_the_host_mirror_traces_with_its_bias(oracle):
    from prosper_amd.rt_reference import Camera, GBufferTracer, renderer_lod_bias
    rng = np.random.default_rng(34)
    world, _, _ = quad_world(rng, 8.0)
    world.camera = dict(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=math.radians(50.0), zN=0.1, zF=100.0)
    ctx = mips_context(world)
    try:
        hcam = Camera.from_world(world, W, H)
        cam, _ = hcam.update_buffer()
        cam = S.CameraUniforms.from_buffer_copy(bytes(cam))
        tracer = GBufferTracer(ctx)
        want = {}
        for taa in (False, True):
            ctx.set_texture_lod(True, -1.0 if taa else 0.0)
            want[taa] = ctx.trace_gbuffer(cam, W, H, jitter=False)[0]
        assert want[False].tobytes() != want[True].tobytes()
        for taa in (True, False):
            tracer.set_texture_lod(True, renderer_lod_bias(taa))
            tracer.record(hcam, W, H, jitter=False)
            assert ctx.read_gbuffer()[0].tobytes() == want[taa].tobytes()
        tracer.set_texture_lod(False)
        tracer.record(hcam, W, H, jitter=False)
        ctx.set_texture_lod(False)
        assert ctx.read_gbuffer()[0].tobytes() == ctx.trace_gbuffer(cam, W, H, jitter=False)[0].tobytes()
    finally:
        ctx.close()


# ---- the mapped normal: a quad square to the view axis, whose frame is (0, 0, 1) / (1, 0, 0) exactly ----
FLAT = [(-16.0, -12.0, -8.0), (16.0, -12.0, -8.0), (16.0, 12.0, -8.0), (-16.0, 12.0, -8.0)]


def flat_world(rng, uv_scale, alpha_mode=S.ALPHA_MODE_OPAQUE, smooth=False):
    w = World()
    if smooth:
        tex = [scenes.noise_texture(64, 5, alpha=255), scenes.metallic_roughness_texture(64, 6), scenes.normal_texture(64, 7)]
        tex[0][..., 3] = 128 + (np.arange(64)[None, :] + np.arange(64)[:, None])  # alpha 128 .. 254, never 0
    else:
        tex = [rng.integers(0, 256, (64, 64, 4), dtype=np.uint8) for _ in range(3)]
        tex[2][..., 2] = rng.integers(128, 256, (64, 64))  # the tangent-space normal points out of the surface
    ids = [w.add_texture(t) for t in tex]
    m = w.add_material(base_color=(0.9, 0.8, 0.7, 0.6 if alpha_mode == S.ALPHA_MODE_BLEND else 1.0), metallic=0.75, roughness=1.0,
                       base_tex=(ids[0], 0), mr_tex=(ids[1], 0), normal_tex=(ids[2], 0), alpha_mode=alpha_mode)
    q = scenes._add(w, scenes.quad(*FLAT, uv_scale=uv_scale), m)
    w.add_instance(w.add_model([(q, m)]))
    return w, tex


@pytest.mark.parametrize("case,scale", [("unpacked", 8.0), ("packed", 4.0), ("packed", 8.0), ("compact", 4.0), ("compact", 8.0)])
def test_the_mapped_normal_is_the_restatement_bit_for_bit(oracle, case, scale):
    """Every target of the G-buffer, the encoded mapped normal included, for a material with a normal texture: level 0
    out of the pack and level 1 (scale 4: lambda about 0.73), two chain levels (scale 8: about 1.73), and unpacked."""
    rng = np.random.default_rng(35)
    world, tex = flat_world(rng, scale)
    cam = camera(oracle)
    debug = {"noTexturePacks": 1} if case == "unpacked" else {"widePacks": 1 if case == "packed" else 0}
    ctx = mips_context(world, **debug)
    try:
        assert bool(ctx.scene_stats().variantFlags & S.VARIANT_TEXTURE_PACKS) == (case != "unpacked")
        ctx.set_texture_lod(True, 0.0)
        ctx.set_texture_lod_debug(True)
        uv = ctx.trace_gbuffer(cam, W, H, draw_type=S.DRAW_TYPES.index("TexCoord0"), jitter=False)[0][..., :2]
        d = ctx.read_texture_lod_derivatives(W, H)
        ar, nm, depth = ctx.trace_gbuffer(cam, W, H, jitter=False)
        assert (depth > 0).all()
        lam = R.texture_lambda(64, 64, d.reshape(-1, 4), 0.0)
        print("lambda %.3f .. %.3f" % (lam.min(), lam.max()))
        assert (lam > 0).all() and (lam < 4).all() and ((lam < 1).all() if scale == 4.0 else (lam > 1).all())
        chains = (R.generate_chain(tex[0], True), R.generate_chain(tex[1], False))
        smp = (1, 1, 0, 0)
        albedo, rough, metal, tsn, _ = R.sample_material_lod(
            chains, (smp, smp), ((0.9, 0.8, 0.7), 1.0, 0.75), uv.reshape(-1, 2), d.reshape(-1, 4), 0.0,
            normal_chain=R.generate_chain(tex[2], False), normal_sampler=smp)
        assert (ar[..., :3].reshape(-1, 3).view(np.uint32) == albedo.view(np.uint32)).all()
        assert (ar[..., 3].reshape(-1).view(np.uint32) == rough.view(np.uint32)).all()
        assert (nm[..., 2].reshape(-1).view(np.uint32) == metal.view(np.uint32)).all()
        # The bitangent's sign is the INTERPOLATED tangent.w, ((1 - bu) - bv + bu) + bv of the hit's barycentrics: 1 up to
        # two roundings, which no target reports.  Every pixel must be the restatement, bit for bit, for one of the
        # floats that sum can be, and for 1 itself in nearly all of them.
        got = nm[..., [0, 1, 3]].reshape(-1, 3)
        signs = [1.0] + [1.0 + k * 2.0 ** -24 for k in (-1, -2, -3, -4)] + [1.0 + k * 2.0 ** -23 for k in (1, 2)]
        matched = np.zeros(len(got), bool)
        for i, sign in enumerate(signs):
            enc = R.signed_oct_encode(R.mapped_normal_axis_frame(tsn, sign))
            same = (got.view(np.uint32) == enc.view(np.uint32)).all(axis=1)
            if i == 0:
                print("%d of %d encoded normals are the restatement with sign 1" % (same.sum(), len(got)))
                assert same.mean() >= 0.9
            matched |= same
        assert matched.all(), "%d encoded normals are no restatement" % (~matched).sum()
        # and LOD off gives another normal (the chain is read)
        ctx.set_texture_lod(False)
        assert ctx.trace_gbuffer(cam, W, H, jitter=False)[1].tobytes() != nm.tobytes()
    finally:
        ctx.close()


# ---- the forward transparent pass ----
def transparent_frame(ctx, cam, keep=2):
    """The deferred frame up to the pass and the pass in debug mode, as tests/test_transparent.py runs it."""
    import test_transparent as TT
    return TT.run_pass(ctx, cam, W, H, mode="centre", keep=keep)


def test_the_transparent_pass_magnified_is_byte_identical_off_and_on(oracle):
    rng = np.random.default_rng(36)
    world, _ = flat_world(rng, 0.25, alpha_mode=S.ALPHA_MODE_BLEND)
    cam = camera(oracle)
    _, d64 = R.analytic_derivatives(cam, W, H, FLAT[0], (0.0, 0.0, 1.0), lambda p: np.stack([0.25 * (p[..., 0] + 16.0) / 32.0, 0.25 * (p[..., 1] + 12.0) / 24.0], axis=-1))
    assert R.lambda64(64, 64, d64).max() < -0.5
    ctx = mips_context(world)
    try:
        off = transparent_frame(ctx, cam)
        ctx.set_texture_lod(True, 0.0)
        on = transparent_frame(ctx, cam)
        assert (off[2] == 1).all()
        for a, b in zip(off, on):
            assert a.tobytes() == b.tobytes()
    finally:
        ctx.close()


def test_a_minified_blend_quad_is_the_lod_restatement_composited(oracle):
    """One BLEND quad, lambda about 1.73: its layer's material against the LOD restatement at the float64 uv and
    derivatives, and the image against transparent_reference.composite over those restated layers, with
    tests/test_transparent.py's tolerances (REL of the pixel's sum of absolute terms + ABS)."""
    import test_transparent as TT
    import transparent_reference as T
    rng = np.random.default_rng(37)
    scale = 8.0
    world, tex = flat_world(rng, scale, alpha_mode=S.ALPHA_MODE_BLEND, smooth=True)
    cam = camera(oracle)
    uv64, d64 = R.analytic_derivatives(cam, W, H, FLAT[0], (0.0, 0.0, 1.0), lambda p: np.stack([scale * (p[..., 0] + 16.0) / 32.0, scale * (p[..., 1] + 12.0) / 24.0], axis=-1))
    lam64 = R.lambda64(64, 64, d64)
    assert lam64.min() > 1.5 and lam64.max() < 2.0
    ctx = mips_context(world)
    try:
        off = transparent_frame(ctx, cam)
        ctx.set_texture_lod(True, 0.0)
        before, after, counts, layers, depth = transparent_frame(ctx, cam)
        assert (counts == 1).all() and (depth == 0).all()
        assert off[1].tobytes() != after.tobytes()
        smp = (1, 1, 0, 0)
        chains = (R.generate_chain(tex[0], True), R.generate_chain(tex[1], False))
        albedo, rough, metal, tsn, alpha = R.sample_material_lod(
            chains, (smp, smp), ((0.9, 0.8, 0.7), 1.0, 0.75), uv64.reshape(-1, 2).astype(F), d64.reshape(-1, 4).astype(F), 0.0,
            normal_chain=R.generate_chain(tex[2], False), normal_sampler=smp, alpha_factor=0.6)
        want = layers.copy()
        first = want[..., 0]
        first["albedo"] = albedo.reshape(H, W, 3)
        first["roughness"] = rough.reshape(H, W)
        first["metallic"] = metal.reshape(H, W)
        first["alpha"] = alpha.reshape(H, W)
        first["normal"] = R.mapped_normal_axis_frame(tsn).reshape(H, W, 3)
        want[..., 0] = first
        # the layer the GPU recorded against the restated one: float32 uv and lambda against float64 ones
        for k in ("albedo", "roughness", "metallic", "alpha", "normal"):
            err = np.abs(layers[..., 0][k].astype(np.float64) - want[..., 0][k]).max()
            print("layer %s: max difference %.3g" % (k, err))
            assert err <= 2e-4, k
        rgb, a, scale_, margin = T.composite(world, cam, counts, want, before)
        err = np.abs(after[..., :3].astype(np.float64) - rgb).max(-1)
        print("worst error %.3g of scale %.3g" % (err.max(), scale_.reshape(-1)[np.argmax(err)]))
        assert (err <= TT.REL * scale_ + TT.ABS).all()
        assert np.abs(after[..., 3].astype(np.float64) - a).max() <= 1e-6
    finally:
        ctx.close()
