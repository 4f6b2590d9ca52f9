"""Loop-invariant work hoisted out of the wavefront kernels: stored guard boxes of LDS-resident
triangles, the sun's direction once per workgroup, divisions by a launch's tile counts as multiplications, 32-bit record
offsets, a hit's BRDF terms shared by the light sample and the bounce sample.  Every one is the same operations on the
same operands, only earlier: the images must not change by a bit."""
import numpy as np
import pytest

from conftest import default_pc, same_bits
from prosper_amd import capi, scenes, structs as S


def _camera(oracle, world, w, h):
    c = world.camera
    return oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)


def _oracle_frames(oracle, world, fl, cam, w, h, frames, **kw):
    osc = oracle.OracleScene(world, brute_force=True)
    want = None
    for f in range(frames):
        pc = default_pc(S, fl, frame_index=1 + f, skip_history=(f == 0), **kw)
        want, _ = osc.render(pc, cam, w, h, history=want)
    return want


# ---- divisions by launch constants: the host function that makes the multipliers (no GPU) ----

def _divides_like_python(divisors, rng):
    for d in divisors:
        d = int(d)
        mul, sh1, sh2 = capi.magic_divisor(d)
        n = np.concatenate([np.array([0, d - 1, d, min(d + 1, 2**32 - 1), 2**32 - 1], np.uint64),
                            rng.integers(0, 2**32, size=10000, dtype=np.uint64)])
        t = (n * np.uint64(mul)) >> np.uint64(32)  # n, mul < 2^32: the product fits 64 bits
        q = (t + ((n - t) >> np.uint64(sh1))) >> np.uint64(sh2)
        assert sh1 < 32 and sh2 < 32 and t.max() < 2**32 and (t + ((n - t) >> np.uint64(sh1))).max() < 2**32, d
        bad = q != n // np.uint64(d)
        assert not bad.any(), (d, mul, sh1, sh2, n[bad][:4])


def test_magic_divisors_divide_exactly_small_divisors():
    _divides_like_python(range(1, 4097), np.random.default_rng(25))


def test_magic_divisors_divide_exactly_random_divisors():
    rng = np.random.default_rng(26)
    _divides_like_python(rng.integers(1, 2**31 + 1, size=2000, dtype=np.uint64), rng)
    assert capi.magic_divisor(0) == capi.magic_divisor(1)  # an empty band of tiles divides nothing


# ---- the kernels that use them: tile rows that are no power of two, partial frame groups ----

@pytest.mark.gpu
@pytest.mark.parametrize("frames", (1, 3, 8, 65))
@pytest.mark.parametrize("width", (8, 24, 1000, 1928))
def test_slot_and_batch_decoding_by_multiplication(gpu_ctx, oracle, cornell_world, width, frames):
    h = 16
    cam, fl = _camera(oracle, cornell_world, width, h)
    kw = dict(max_bounces=2, ibl=True)
    gpu_ctx.upload_scene(cornell_world)
    gpu_ctx.render(default_pc(S, fl, **kw), cam, width, h, frames=frames)
    got = gpu_ctx.read_hdr()
    want = _oracle_frames(oracle, cornell_world, fl, cam, width, h, frames, **kw)
    ok = same_bits(got, want).all(axis=2)
    assert ok.all(), "%d of %d pixels differ" % ((~ok).sum(), ok.size)


# ---- stored guard boxes (LDS-resident scene) against the recomputed ones (global memory) ----

def _cornell_with_a_large_slab():
    """S-cornell plus a slab under and around the room whose corners lie 1200 units out: there the guard pad
    (2^-16 of the largest |coordinate|) is no longer negligible against the box it pads."""
    w = scenes.cornell(with_skybox=True)
    model = w.model_instances[1][0]  # the white block's model: a unit box
    w.add_instance(model, scenes.translate((0.0, -1.0, 0.0)) @ scenes.scale((2400.0, 0.5, 2400.0)))
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ("cornell", "large_slab"))
def test_stored_guard_box_equals_the_recomputed_one(gpu_ctx, oracle, cornell_world, scene):
    world = cornell_world if scene == "cornell" else _cornell_with_a_large_slab()
    w, h = 64, 48
    cam, fl = _camera(oracle, world, w, h)
    pc = default_pc(S, fl, max_bounces=3, ibl=True)
    out = []
    for no_lds in (0, 1):
        capi.debug(noLdsScene=no_lds)
        gpu_ctx.upload_scene(world)
        in_lds = bool(gpu_ctx.scene_stats().variantFlags & S.VARIANT_LDS_SCENE)
        assert in_lds == (no_lds == 0)  # five float4s per triangle still fit the LDS budget
        gpu_ctx.reset_counters()
        gpu_ctx.render(pc, cam, w, h, frames=2, flags=S.RENDER_COUNT_WORK)
        out.append((gpu_ctx.read_hdr(), gpu_ctx.counters().as_dict()))
    capi.debug(noLdsScene=None)
    if scene == "large_slab":
        tris, _ = gpu_ctx.read_hierarchy_arrays()
        assert np.abs(tris.view(np.float32)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).max() >= 1024.0
    assert (out[0][0].view(np.uint32) == out[1][0].view(np.uint32)).all()
    assert out[0][1] == out[1][1]
    assert out[0][1]["triangleTests"] > 0 and out[0][1]["shadowRays"] > 0


# ---- the sun's direction, normalised once per workgroup ----

SUN_DIRECTIONS = {"axis": (0.0, -1.0, 0.0), "generic": (-0.3, -1.7, 0.45), "tiny_component": (1e-25, -1.0, 0.3)}


@pytest.mark.gpu
def test_sun_direction_normalised_once_equals_the_oracle(gpu_ctx, oracle):
    w, h = 64, 48
    uploaded = False
    for name, direction in SUN_DIRECTIONS.items():
        world = scenes.cornell(with_skybox=True)
        world.set_directional_light((1.0, 0.95, 0.9), 3.0, direction)
        cam, fl = _camera(oracle, world, w, h)
        kw = dict(max_bounces=3, ibl=True)
        if not uploaded:
            gpu_ctx.upload_scene(world)
            uploaded = True
        else:
            gpu_ctx.update_lights(world)  # the next light block: the direction is worked out from what the render reads
        gpu_ctx.reset_counters()
        gpu_ctx.render(default_pc(S, fl, **kw), cam, w, h, frames=2, flags=S.RENDER_COUNT_WORK)
        got = gpu_ctx.read_hdr()
        assert gpu_ctx.counters().lightSamples > 0
        want = _oracle_frames(oracle, world, fl, cam, w, h, 2, **kw)
        assert same_bits(got, want).all(), name


# ---- 32-bit record offsets at the far end of a large workspace ----

@pytest.mark.gpu
def test_records_at_high_offsets_of_a_large_workspace(oracle, cornell_world):
    """2^25 path slots in 64-slot segments (half a million of them; records up to 512 MB into their arrays, 6.7 GB of
    workspace) against the same render in the default segments: the record addressing must not depend on where in the
    workspace a segment lies."""
    w, h, frames = 2048, 1024, 16
    cam, fl = _camera(oracle, cornell_world, w, h)
    pc = default_pc(S, fl, max_bounces=4, ibl=True)
    ctx = capi.Context(device=0)
    try:
        ctx.upload_scene(cornell_world)
        ctx.render(pc, cam, w, h, frames=frames)
        want = ctx.read_hdr()
        ctx.set_debug(segmentLength=64)
        ctx.render(pc, cam, w, h, frames=frames)
        got = ctx.read_hdr()
    finally:
        ctx.close()
    assert np.isfinite(want).all() and float(want[..., :3].mean()) > 0.0
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
