"""The particle system without a GPU: the entry points exist and refuse bad arguments before they touch
the device, structs.Particle mirrors the header, and tests/particles_reference.py gives the answers worked by hand for
coverage, facing, the dither and the freelist."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import particles_reference as P
from prosper_amd import capi, scenes, structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def camera(oracle, w, h, eye=(0.0, 1.0, 3.0), target=(0.0, 1.0, 0.0)):
    return oracle.camera_uniforms(eye, target, (0.0, 1.0, 0.0), math.radians(59.0), 0.1, 100.0, w, h)[0]


def test_the_symbols_exist_and_bad_arguments_are_rejected_before_touching_the_gpu(oracle):
    lib = capi.lib()
    for name in ("prosper_pt_particles", "prosper_pt_get_particles_info", "prosper_pt_read_particles", "prosper_pt_set_particles",
                 "prosper_host_particles_create", "prosper_host_particles_destroy", "prosper_host_particles_record",
                 "prosper_host_particles_set_source", "prosper_host_particles_set_max_particle_count"):
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    cam = camera(oracle, 4, 4)
    pc = S.ParticlesPC(600, 0, 0, 1.0 / 60.0, 1, 1)

    def call(pc_ref, stages, cam_ref, w, h):
        return lib.prosper_pt_particles(None, pc_ref, stages, cam_ref, w, h, None, None)

    assert call(None, S.PARTICLES_ALL, C.byref(cam), 4, 4) == -1
    assert call(C.byref(pc), 16, C.byref(cam), 4, 4) == -1  # an unknown stage bit
    assert b"unknown stage bits" in lib.prosper_pt_last_error()
    assert call(C.byref(pc), S.PARTICLES_RENDER, None, 4, 4) == -1
    assert b"camera" in lib.prosper_pt_last_error()
    assert call(C.byref(pc), S.PARTICLES_RENDER, C.byref(cam), 0, 4) == -1
    assert b"empty extent" in lib.prosper_pt_last_error()
    bad = S.ParticlesPC(600, 0, 2, 0.0, 0, 0)
    assert call(C.byref(bad), S.PARTICLES_DECAY, None, 0, 0) == -1
    assert b"reset" in lib.prosper_pt_last_error()
    assert call(C.byref(pc), S.PARTICLES_DECAY, None, 0, 0) == -1  # everything else is fine: the null context
    assert lib.prosper_pt_get_particles_info(None, None) == -1
    assert lib.prosper_pt_read_particles(None, None, None, 0, None) == -1
    # a freelist that would index outside the pool
    rec, count, idx = P.fresh_pool(8)
    for freelist in ([9] + list(idx), [-1] + list(idx), [8] + list(idx[:-1]) + [8], [8] + list(idx[:-1]) + [-1]):
        fl = np.array(freelist, np.int32)
        assert lib.prosper_pt_set_particles(None, rec.ctypes.data, fl.ctypes.data, 8, None) == -1
        assert b"freelist" in lib.prosper_pt_last_error()
    h = C.c_void_p()
    assert lib.prosper_host_particles_create(None, C.byref(h)) == -1


def test_the_particle_struct_is_64_bytes_in_the_headers_field_order():
    assert C.sizeof(S.Particle) == 64 and S.PARTICLE_DTYPE.itemsize == 64
    text = open(os.path.join(ROOT, "include", "prosper_pt", "shader_structs.h")).read()
    body = text[text.index("typedef struct prosper_pt_particle"):text.index("} prosper_pt_particle;")]
    names = re.findall(r"\b(?:prosper_vec4|uint32_t)\s+([A-Za-z_0-9]+);", body)
    assert names == [n for n, _ in S.Particle._fields_]
    assert [S.Particle.position_lifetime.offset, S.Particle.normal_spawnRateS.offset, S.Particle.velocity_spawnTimerS.offset,
            S.Particle.mask.offset] == [0, 16, 32, 48]
    assert [S.PARTICLE_DTYPE.fields[k][1] for k in ("position_lifetime", "normal_spawnRateS", "velocity_spawnTimerS", "mask")] == [0, 16, 32, 48]
    # particle.h's mask bits and the reference's 500 000 slots
    assert (S.PARTICLE_MASK_GRAVITY, S.PARTICLE_MASK_DECAY, S.PARTICLE_MASK_EMIT) == (1, 2, 4)
    assert S.MAX_PARTICLE_COUNT == 500000
    text = open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()
    body = text[text.index("typedef struct prosper_pt_particles_pc"):text.index("} prosper_pt_particles_pc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(?:uint32_t|float)\s+([A-Za-z_]+);", body) == [n for n, _ in S.ParticlesPC._fields_]
    body = text[text.index("typedef struct prosper_pt_particles_info"):text.index("} prosper_pt_particles_info;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for line in re.findall(r"\b(?:uint32_t|float)\s+([A-Za-z_, ]+);", body) for n in line.replace(" ", "").split(",")]
    assert fields == [n for n, _ in S.ParticlesInfo._fields_]


def test_fma_is_rounded_once():
    """The restatement's fmaf against exact rational arithmetic."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(F)
    b = rng.standard_normal(4000).astype(F)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.standard_normal(4000) * 1e-7)).astype(F)  # heavy cancellation
    got = P.fma(a, b, c)
    for k in range(0, 4000, 7):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo, hi = np.nextafter(got[k], F(-np.inf)), np.nextafter(got[k], F(np.inf))
        err = abs(Fraction(float(got[k])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
    assert P.fma(F(3.0), F(4.0), F(5.0)) == 17.0


def test_a_quad_on_pixel_centres_covers_what_the_top_left_rule_gives():
    """Corners (in the strip's order 0 1 / 2 3 as the camera puts them: see the facing test) on the centres of pixels
    (2, 1), (6, 1), (2, 4), (6, 4): a left or top edge through a centre includes it, a right or bottom edge does not, and
    the diagonal's pixels belong to exactly one triangle."""
    c = lambda p: p * 256 + 128
    # front-facing strip: 0 = right top, 1 = left top, 2 = right bottom, 3 = left bottom
    X, Y = [c(6), c(2), c(6), c(2)], [c(1), c(1), c(4), c(4)]
    assert all(P.triangle_area2(X, Y, t) < 0 for t in P.STRIP)
    py, px = P.quad_coverage(X, Y, 16, 16)
    want = {(y, x) for y in range(1, 4) for x in range(2, 6)}
    assert set(zip(py.tolist(), px.tolist())) == want and len(py) == len(want)
    # the same quad wound the other way is culled whole
    Xb = [c(2), c(6), c(2), c(6)]
    assert all(P.triangle_area2(Xb, Y, t) > 0 for t in P.STRIP)
    assert len(P.quad_coverage(Xb, Y, 16, 16)[0]) == 0
    # clipped by the image: only the part inside
    py, px = P.quad_coverage(X, Y, 4, 3)
    assert set(zip(py.tolist(), px.tolist())) == {(y, x) for y in range(1, 3) for x in range(2, 4)}


def test_a_quad_smaller_than_a_pixel_covers_one_pixel_or_none():
    def quad(x0, y0, size):
        return [x0 + size, x0, x0 + size, x0], [y0, y0, y0 + size, y0 + size]
    # 100/256 of a pixel around the centre of pixel (5, 3)
    X, Y = quad(5 * 256 + 128 - 50, 3 * 256 + 128 - 50, 100)
    py, px = P.quad_coverage(X, Y, 16, 16)
    assert (py.tolist(), px.tolist()) == ([3], [5])
    # the same size between the centres
    X, Y = quad(5 * 256 + 140, 3 * 256 + 140, 100)
    assert len(P.quad_coverage(X, Y, 16, 16)[0]) == 0
    # its left edge exactly on the centre: included; its right edge exactly on it: not
    X, Y = quad(5 * 256 + 128, 3 * 256 + 100, 100)
    assert (P.quad_coverage(X, Y, 16, 16)[1].tolist()) == [5]
    X, Y = quad(5 * 256 + 28, 3 * 256 + 100, 100)
    assert len(P.quad_coverage(X, Y, 16, 16)[0]) == 0
    # an empty quad covers nothing
    X, Y = quad(5 * 256 + 128, 3 * 256 + 128, 0)
    assert len(P.quad_coverage(X, Y, 16, 16)[0]) == 0


def test_a_particle_in_front_of_the_camera_is_front_facing(oracle):
    """prosper's particles are visible, so render.vert's strip must come out front-facing under (f12)'s sign rule
    (Vulkan's a = -1/2 sum(x_i y_i+1 - x_i+1 y_i) > 0 with y down): triangle_area2 = -2 a < 0 for both triangles."""
    rng = np.random.default_rng(11)
    for eye, target in (((0.0, 1.0, 3.0), (0.0, 1.0, 0.0)), ((2.0, 3.0, -1.0), (0.5, 0.0, 0.25)), ((-1.0, 0.2, 0.5), (4.0, 1.0, 2.0))):
        w, h = 512, 384
        cam = camera(oracle, w, h, eye, target)
        e, t = np.array(eye), np.array(target)
        fwd = (t - e) / np.linalg.norm(t - e)
        seen = 0
        for _ in range(40):
            pos = e + fwd * rng.uniform(0.3, 6.0) + rng.uniform(-0.05, 0.05, 3)
            q = P.quad_corners(pos.astype(F), cam, w, h)
            assert q is not None
            depth, X, Y = q
            assert 0.0 < depth <= 1.0
            assert all(P.triangle_area2(X, Y, tri) < 0 for tri in P.STRIP), (X, Y)
            # corner 0 is above corner 2 on screen (world up is a smaller pixel y) and the strip closes into a rectangle
            assert Y[0] < Y[2] and Y[1] < Y[3] and X[0] != X[1]
            seen += len(P.quad_coverage(X, Y, w, h)[0])
        assert seen > 0
        # behind the camera and in front of the near plane: dropped whole
        assert P.quad_corners((e - fwd).astype(F), cam, w, h) is None
        assert P.quad_corners((e + fwd * 0.05).astype(F), cam, w, h) is None


def test_the_dither_passes_ceil_alpha_64_cells_and_shifts_with_the_frame_index():
    py, px = np.mgrid[0:8, 0:8]
    for f in (0, 1, 9, 63):
        for k in range(65):
            alpha = F(k / 64.0)
            passed = P.dither_passes(alpha, py + 16, px + 40, f)
            # The thresholds are 0/64 .. 63/64, each once, and step() passes on equality, so alpha = k/64 passes the
            # k + 1 thresholds 0 .. k: one more than ceil(alpha * 64) = k, which is the count for every alpha that is
            # not itself a threshold (below).  render.frag is the authority: step(threshold, alpha) == 0 discards.
            assert passed.sum() == min(k + 1, 64)
            assert k < 64 or passed.all()
            if k < 64:
                between = F((k + 0.5) / 64.0)
                assert P.dither_passes(between, py + 16, px + 40, f).sum() == math.ceil(float(between) * 64) == k + 1
        assert P.dither_passes(F(1.0), py, px, f).all()
        assert P.dither_passes(F(0.0), py, px, f).sum() == 1  # the cell whose threshold is 0 (a dying particle's last pixel)
    # as written: f % 8 offsets the column and f / 8 the row
    one = P.dither_passes(F(0.0), py, px, 0)
    assert one[0, 0]
    assert P.dither_passes(F(0.0), py, px, 1)[0, 7] and P.dither_passes(F(0.0), py, px, 9)[7, 7]
    assert P.dither_passes(F(0.0), py, px, 63)[1, 1]
    assert (P.BAYER64.reshape(-1).tolist().count(0), sorted(P.BAYER64.reshape(-1).tolist())) == (1, list(range(64)))
    # strictly between two thresholds: ceil(alpha * 64) cells
    assert P.dither_passes(F(10.5 / 64.0), py, px, 0).sum() == 11


def test_pop_grants_min_and_push_appends_as_sets():
    rec, count, idx = P.fresh_pool(16)
    assert count == 16 and idx.tolist() == list(range(16)) and not P.live(rec).any()
    assert (rec["position_lifetime"] == -9999.0).all() and not rec["mask"].any()
    assert [P.pop_grants(k, c) for k, c in ((0, 5), (3, 5), (5, 5), (40, 5), (7, 0))] == [0, 3, 5, 5, 0]
    # decay: the freed slots are exactly the Decay slots at or below 0 and nothing dead
    rec["position_lifetime"][:6, 3] = [0.25, 0.0, -0.5, 0.0, 1.0, -0.5]
    rec["mask"][:6] = [S.PARTICLE_MASK_DECAY] * 3 + [S.PARTICLE_MASK_EMIT] + [3, 0]
    out, freed = P.decay(rec, 0)
    assert set(freed.tolist()) == {1, 2}
    assert (out["position_lifetime"][[1, 2]] == -9999.0).all() and out["position_lifetime"][0, 3] == F(0.25)
    out, freed = P.decay(rec, 1)
    assert set(freed.tolist()) == {0, 1, 2, 3, 4, 5}  # decayAll: everything that is not dead already
    again, freed = P.decay(out, 1)
    assert len(freed) == 0 and (again["position_lifetime"] == out["position_lifetime"]).all()


def test_simulate_by_hand():
    """One emitter and one child, dt = 1/4, every number checked against the shader's text in plain float32."""
    rec, _, _ = P.fresh_pool(4)
    rec["position_lifetime"][1] = [1.0, 2.0, 3.0, 0.0]
    rec["normal_spawnRateS"][1] = [0.0, 1.0, 0.0, 0.25]
    rec["mask"][1] = S.PARTICLE_MASK_EMIT
    rec["position_lifetime"][2] = [0.0, 1.0, 0.0, 0.125]
    rec["velocity_spawnTimerS"][2] = [0.5, 0.0, -0.25, 0.0]
    rec["mask"][2] = S.PARTICLE_MASK_GRAVITY | S.PARTICLE_MASK_DECAY
    out, children, parents = P.simulate(rec, 0.25, 7)
    # the child: moved by its velocity, gravity 9.81 * .01 * dt off y, lifetime less dt (crossing 0)
    assert out["position_lifetime"][2].tolist() == [0.125, 1.0, -0.0625, -0.125]
    assert out["velocity_spawnTimerS"][2, 1] == F(0.0) - (F(9.81) * F(0.01)) * F(0.25)
    # dead slots are untouched
    assert (out[0].tobytes(), out[3].tobytes()) == (rec[0].tobytes(), rec[3].tobytes())
    # the emitter: speed clamped to 0.05 along its new direction, timer at the rate spawns and returns to 0
    v = out["velocity_spawnTimerS"][1]
    assert abs(float(np.linalg.norm(v[:3].astype(np.float64))) - 0.05) < 1e-8 and v[3] == 0.0
    assert parents.tolist() == [1] and len(children) == 1
    c = children[0]
    assert c["position_lifetime"].tolist() == [1.0, 2.0, 3.0, 4.0] and c["mask"] == 3  # the emitter had no velocity yet
    assert (c["normal_spawnRateS"][:3] == out["normal_spawnRateS"][1, :3]).all() and c["normal_spawnRateS"][3] == 0.0
    assert np.allclose(c["velocity_spawnTimerS"][:3], out["normal_spawnRateS"][1, :3] * 0.1, rtol=1e-6)
    # the rng: pcg3d of (slot, slot % 256, frame)
    r, _ = P.rnd3d01(np.array([[1, 1, 7]], np.uint32))
    assert ((r >= 0) & (r <= 1)).all()
    x = (1 * 1664525 + 1013904223) & 0xFFFFFFFF
    assert int(P.pcg3d(np.array([[1, 1, 7]], np.uint32))[0, 0]) != x  # (mixed, not the bare LCG)
    assert (P.pcg3d(np.array([[300, 44, 7]], np.uint32)) == P.pcg3d(np.array([[300, 300 % 256, 7]], np.uint32))).all()


def test_init_records_of_a_quad():
    """scenes.quad through an instance transform: positions and normals as instances.glsl transforms them."""
    w = scenes.World()
    m = w.add_material(base_color=(1, 1, 1, 1))
    mesh = scenes._add(w, scenes.quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1)), m)
    t = np.eye(4)
    t[:3, 3] = (0.5, 2.0, -1.0)
    t[0, 0] = t[1, 1] = t[2, 2] = 2.0
    w.add_instance(w.add_model([(mesh, m)]), t)
    rec = P.init_records(w, 0)
    assert len(rec) == 4
    assert sorted(map(tuple, rec["position_lifetime"].tolist())) == sorted(
        [(-1.5, 2.0, 1.0, 0.0), (2.5, 2.0, 1.0, 0.0), (2.5, 2.0, -3.0, 0.0), (-1.5, 2.0, -3.0, 0.0)])
    assert np.allclose(rec["normal_spawnRateS"][:, :3], (0, 1, 0), atol=1e-6) and (rec["normal_spawnRateS"][:, 3] == F(0.1)).all()
    assert (rec["mask"] == S.PARTICLE_MASK_EMIT).all() and not rec["velocity_spawnTimerS"].any()
