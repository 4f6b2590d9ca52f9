"""The particle system on the GPU (prosper_pt_particles; pt_particles.hip): every stage over designed
states against tests/particles_reference.py, bit for bit.  Slot assignment depends on the waves' arrival order, so the
tests compare multisets of records and sets of slots, slot by slot only where prosper_pt_set_particles placed the state.
Pools of 600 to 2048 slots: several blocks of 256, a partial last wave, slots above 255 (whose local id differs from the
slot, which the rng sees)."""
import ctypes
import math
import os

import numpy as np
import pytest

import particles_reference as P
from conftest import same_bits
from prosper_amd import gltf, scenes, structs as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
NO_RENDER = S.PARTICLES_DECAY | S.PARTICLES_INIT | S.PARTICLES_SIMULATE


def run(ctx, n, stages, reset=0, dt=0.0, sim_frame=1, render_frame=0, source=0, camera=None, w=0, h=0, depth_ptr=None):
    ctx.particles(S.ParticlesPC(n, source, reset, dt, sim_frame, render_frame), stages, camera, w, h, depth_ptr)


def place_fresh(ctx, n):
    ctx.set_particles(*P.fresh_pool(n))


def keys(records):
    """one hashable key per record: its 52 written bytes"""
    words = np.ascontiguousarray(records).view(np.uint32).reshape(len(records), 16)[:, :13]
    return [w.tobytes() for w in words]


def assert_pool_is_consistent(records, count, indices):
    """live slots and the free entries are a permutation of the pool"""
    n = len(records)
    live = np.nonzero(P.live(records))[0]
    free = indices[:count]
    assert len(set(free.tolist())) == count, "the freelist holds a slot twice"
    assert sorted(live.tolist() + free.tolist()) == list(range(n))


def synthetic_world():
    """draw instance 0: a displaced 30 x 30 grid (961 vertices) under a rotating, scaling transform; 1: a box (24)."""
    w = scenes.World()
    m = w.add_material(base_color=(0.8, 0.8, 0.8, 1.0))
    g = scenes._add(w, scenes.grid(30, 30, 2.0, 3.0, height_fn=lambda x, z: 0.25 * np.sin(3.0 * x) * np.cos(2.0 * z)), m)
    b = scenes._add(w, scenes.box(), m)
    a = 0.5
    t = np.array([[1.5 * math.cos(a), 0.0, math.sin(a), 0.25], [0.0, 0.75, 0.0, 1.0], [-1.5 * math.sin(a), 0.0, math.cos(a), -0.5],
                  [0.0, 0.0, 0.0, 1.0]])
    w.add_instance(w.add_model([(g, m)]), t)
    w.add_instance(w.add_model([(b, m)]))
    return w


# ---- init ----

@pytest.mark.parametrize("which", ("synthetic", "gltf"))
def test_init_makes_one_emitter_per_vertex(gpu_ctx, which):
    world = synthetic_world() if which == "synthetic" else gltf.load_gltf(os.path.join(HERE, "golden", "tiny_scene.gltf"))
    n = 2048
    want = P.init_records(world, 0)
    assert 0 < len(want) < n and (which == "gltf" or len(want) > 512)
    gpu_ctx.upload_scene(world)
    place_fresh(gpu_ctx, n)
    run(gpu_ctx, n, S.PARTICLES_DECAY | S.PARTICLES_INIT, reset=1)
    info = gpu_ctx.particles_info()
    rec, count, idx = gpu_ctx.read_particles()
    got = rec[P.live(rec)]
    assert info.initRecorded == 1 and info.maxParticleCount == n
    assert len(got) == len(want)  # every vertex got a slot of its own
    assert np.array_equal(P.multiset(got), P.multiset(want))
    assert count == n - len(want) == info.freelistCount and info.liveCount == len(want)
    assert_pool_is_consistent(rec, count, idx)
    dead = rec[~P.live(rec)]
    assert (dead["position_lifetime"] == -9999.0).all() and not dead["mask"].any()
    # a second reset frees them all and makes them again
    run(gpu_ctx, n, S.PARTICLES_DECAY | S.PARTICLES_INIT, reset=1)
    rec, count, idx = gpu_ctx.read_particles()
    assert np.array_equal(P.multiset(rec[P.live(rec)]), P.multiset(want)) and count == n - len(want)
    assert_pool_is_consistent(rec, count, idx)
    # without reset init does not run
    run(gpu_ctx, n, S.PARTICLES_DECAY | S.PARTICLES_INIT, reset=0)
    again = gpu_ctx.read_particles()
    assert gpu_ctx.particles_info().initRecorded == 0
    assert again[0].tobytes() == rec.tobytes() and again[1] == count and again[2].tobytes() == idx.tobytes()


def test_init_with_fewer_slots_than_vertices_fills_the_pool(gpu_ctx):
    world = synthetic_world()
    want = P.init_records(world, 0)
    n = 600
    assert len(want) > n
    gpu_ctx.upload_scene(world)
    place_fresh(gpu_ctx, n)
    run(gpu_ctx, n, S.PARTICLES_DECAY | S.PARTICLES_INIT, reset=1)
    info = gpu_ctx.particles_info()
    rec, count, idx = gpu_ctx.read_particles()
    assert P.live(rec).all() and count == 0 and info.initRecorded == 1 and info.freelistCount == 0 and info.liveCount == n
    predicted = {}
    for k in keys(want):
        predicted[k] = predicted.get(k, 0) + 1
    for k in keys(rec):  # each is one of the predicted records, none more often than predicted
        assert predicted.get(k, 0) > 0
        predicted[k] -= 1
    # a changed maxParticleCount reallocates a fresh pool
    run(gpu_ctx, 700, S.PARTICLES_DECAY)
    rec, count, idx = gpu_ctx.read_particles()
    fresh = P.fresh_pool(700)
    assert rec.tobytes() == fresh[0].tobytes() and count == 700 and idx.tolist() == list(range(700))


def test_an_unloaded_source_mesh_skips_init_and_reports_it(gpu_ctx):
    world = synthetic_world()
    gpu_ctx.upload_scene(world.with_meshes_loaded({1}))
    n = 640
    rec, count, idx = P.fresh_pool(n)
    rec["position_lifetime"][5] = (1.0, 2.0, 3.0, 0.5)
    rec["mask"][5] = S.PARTICLE_MASK_EMIT
    idx = np.concatenate([np.setdiff1d(idx, [5]), [5]]).astype(np.int32)  # slot 5 lies outside the n - 1 free entries
    gpu_ctx.set_particles(rec, n - 1, idx)
    run(gpu_ctx, n, S.PARTICLES_INIT, reset=1, source=0)
    assert gpu_ctx.particles_info().initRecorded == 0
    got = gpu_ctx.read_particles()
    assert got[0].tobytes() == rec.tobytes() and got[1] == n - 1 and got[2].tobytes() == idx.tobytes()
    # the loaded mesh of the same scene does record
    run(gpu_ctx, n, S.PARTICLES_INIT, reset=1, source=1)
    assert gpu_ctx.particles_info().initRecorded == 1
    assert gpu_ctx.read_particles()[1] == n - 1 - 24
    with pytest.raises(Exception, match="sourceDrawInstanceIndex"):
        run(gpu_ctx, n, S.PARTICLES_INIT, reset=1, source=2)


# ---- decay ----

def decay_state(n):
    """slot k % 6: 0 Decay just above 0, 1 Decay at 0, 2 Decay just below 0, 3 emitter at 0, 4 dead, 5 Decay | Gravity at -0."""
    rec, _, _ = P.fresh_pool(n)
    k = np.arange(n) % 6
    lifetime = np.array([np.nextafter(F(0), F(1)), 0.0, -np.nextafter(F(0), F(1)), 0.0, -9999.0, -0.0], F)[k]
    rec["position_lifetime"][:, :3] = np.arange(n * 3, dtype=F).reshape(n, 3)
    rec["position_lifetime"][:, 3] = lifetime
    rec["mask"] = np.array([2, 2, 2, 4, 0, 3], np.uint32)[k]
    rec["position_lifetime"][k == 4] = -9999.0
    rec["velocity_spawnTimerS"][:, 0] = 1.0
    dead = np.nonzero(k == 4)[0]
    rng = np.random.default_rng(3)
    idx = np.concatenate([rng.permutation(dead), rng.permutation(np.nonzero(k != 4)[0])]).astype(np.int32)
    return rec, len(dead), idx, k


def test_decay_frees_exactly_the_expired_decay_slots(gpu_ctx):
    n = 1500
    rec, count, idx, k = decay_state(n)
    gpu_ctx.set_particles(rec, count, idx)
    run(gpu_ctx, n, S.PARTICLES_DECAY)
    got, got_count, got_idx = gpu_ctx.read_particles()
    want, freed = P.decay(rec, 0)
    assert set(freed.tolist()) == set(np.nonzero((k == 1) | (k == 2) | (k == 5))[0].tolist())  # the design
    assert got.tobytes() == want.tobytes()
    assert (got["position_lifetime"][freed] == -9999.0).all()
    assert got_count == count + len(freed)
    assert got_idx[:count].tobytes() == idx[:count].tobytes()  # push appends
    pushed = got_idx[count:got_count]
    assert len(set(pushed.tolist())) == len(pushed) and set(pushed.tolist()) == set(freed.tolist())  # freed exactly once
    assert_pool_is_consistent(got, got_count, got_idx)
    info = gpu_ctx.particles_info()
    assert info.freelistCount == got_count and info.liveCount == n - got_count
    # again: nothing left to free, dead slots are not freed twice
    run(gpu_ctx, n, S.PARTICLES_DECAY)
    again = gpu_ctx.read_particles()
    assert again[0].tobytes() == got.tobytes() and again[1] == got_count and again[2].tobytes() == got_idx.tobytes()
    # reset: everything that was live is freed
    run(gpu_ctx, n, S.PARTICLES_DECAY, reset=1)
    got, got_count, got_idx = gpu_ctx.read_particles()
    assert got_count == n and sorted(got_idx.tolist()) == list(range(n))
    assert (got["position_lifetime"] == -9999.0).all()
    assert got.tobytes() == P.decay(rec, 1)[0].tobytes()


# ---- simulate ----

DT = F(1.0 / 64.0)
RATE = F(0.125)


def simulate_state(n):
    """Every third slot dead; among the others all eight masks, four lifetimes (two of them crossing or reaching 0), four
    spawn timers (0, just below the rate less dt, exactly at it, far above) and velocities on both sides of the clamp."""
    rec, _, _ = P.fresh_pool(n)
    i = np.arange(n)
    rng = np.random.default_rng(17)
    rec["position_lifetime"][:, :3] = rng.uniform(-2, 2, (n, 3)).astype(F)
    rec["position_lifetime"][:, 3] = np.array([0.0, DT / F(2), 1.0, DT], F)[(i // 32) % 4]
    normal = rng.standard_normal((n, 3)).astype(F)
    rec["normal_spawnRateS"][:, :3] = P.normalize3(normal)
    rec["normal_spawnRateS"][:, 3] = RATE
    at = F(RATE - DT)
    assert F(at + DT) == RATE and F(np.nextafter(at, F(0)) + DT) < RATE
    rec["velocity_spawnTimerS"][:, 3] = np.array([0.0, np.nextafter(at, F(0)), at, 0.5], F)[(i // 8) % 4]
    speed = np.array([0.0, 0.01, 0.2, 0.049], F)[(i // 128) % 4]
    rec["velocity_spawnTimerS"][:, :3] = P.normalize3(rng.standard_normal((n, 3)).astype(F)) * speed[:, None]
    rec["mask"] = (i % 8).astype(np.uint32)
    dead = i % 3 == 0
    rec["position_lifetime"][dead] = -9999.0
    for k in ("normal_spawnRateS", "velocity_spawnTimerS"):
        rec[k][dead] = 0
    rec["mask"][dead] = 0
    free = np.nonzero(dead)[0]
    idx = np.concatenate([rng.permutation(free), rng.permutation(np.nonzero(~dead)[0])]).astype(np.int32)
    return rec, len(free), idx


def test_simulate_matches_the_restatement_and_places_children_in_the_top_free_slots(gpu_ctx):
    n = 1500  # 5 blocks of 256 and one of 220: a partial last wave
    rec, count, idx = simulate_state(n)
    frame = 77
    want, children, parents = P.simulate(rec, DT, frame)
    live = P.live(rec)
    # the design: every mask occurs live, emitters spawn in every block, both timer sides and both clamp sides occur
    assert set(rec["mask"][live].tolist()) == set(range(8))
    assert set((parents // 256).tolist()) == set(range(6)) and 0 < len(children) < count
    emit = live & ((rec["mask"] & 4) != 0)
    timers = rec["velocity_spawnTimerS"][:, 3]
    assert not np.isin(np.nonzero(emit & (timers == np.nextafter(F(RATE - DT), F(0))))[0], parents).any()
    assert np.isin(np.nonzero(emit & (timers == F(RATE - DT)))[0], parents).all()
    speed_after = np.sqrt((want["velocity_spawnTimerS"][emit, :3].astype(np.float64) ** 2).sum(1))
    assert (speed_after < 0.0499).any() and (np.abs(speed_after - 0.05) < 1e-7).any()
    lifetimes = want["position_lifetime"][live & ((rec["mask"] & 2) != 0), 3]
    assert (lifetimes < 0).any() and (lifetimes == 0).any() and (lifetimes > 0).any()
    assert not np.isnan(want["position_lifetime"]).any()

    gpu_ctx.set_particles(rec, count, idx)
    run(gpu_ctx, n, S.PARTICLES_SIMULATE, dt=float(DT), sim_frame=frame)
    got, got_count, got_idx = gpu_ctx.read_particles()
    info = gpu_ctx.particles_info()
    g = len(children)
    assert got_count == count - g and got_idx.tobytes() == idx.tobytes()
    assert (info.grantedSpawns, info.refusedSpawns, info.freelistCount) == (g, 0, got_count)
    child_slots = idx[count - g:count]  # the top entries of the old freelist
    others = np.setdiff1d(np.arange(n), child_slots)
    assert got[others].tobytes() == want[others].tobytes()  # every pre-existing slot, slot by slot, padding included
    assert np.array_equal(P.multiset(got[child_slots]), P.multiset(children))
    # no child has moved: it sits where its parent was after the parent's own step, with its whole lifetime
    assert (got["position_lifetime"][child_slots, 3] == 4.0).all()
    parent_positions = {p.tobytes() for p in want["position_lifetime"][parents, :3]}
    assert all(p.tobytes() in parent_positions for p in got["position_lifetime"][child_slots, :3])


def test_simulate_on_a_dry_freelist_grants_what_is_left(gpu_ctx):
    n = 640
    rec, _, _ = P.fresh_pool(n)
    i = np.arange(n)
    rec["position_lifetime"][:, :3] = np.arange(n * 3, dtype=F).reshape(n, 3) / F(16)
    rec["position_lifetime"][:, 3] = 1.0
    rec["normal_spawnRateS"][:, :3] = (0.0, 1.0, 0.0)
    rec["normal_spawnRateS"][:, 3] = RATE
    due = np.arange(40) * 15 + 7  # 40 emitters whose timer is due, in nine of the ten waves
    rec["mask"][due] = S.PARTICLE_MASK_EMIT
    rec["velocity_spawnTimerS"][due, 3] = 0.5
    free = np.array([3, 250, 300, 511, 639])
    rec["position_lifetime"][free] = -9999.0
    rec["normal_spawnRateS"][free] = 0
    assert not np.isin(free, due).any() and len(set((due // 64).tolist())) >= 9
    idx = np.concatenate([free, np.setdiff1d(i, free)]).astype(np.int32)
    want, children, parents = P.simulate(rec, DT, 5)
    assert parents.tolist() == due.tolist() and P.pop_grants(len(children), 5) == 5
    gpu_ctx.set_particles(rec, 5, idx)
    run(gpu_ctx, n, S.PARTICLES_SIMULATE, dt=float(DT), sim_frame=5)
    got, got_count, got_idx = gpu_ctx.read_particles()
    info = gpu_ctx.particles_info()
    assert got_count == 0 and (info.grantedSpawns, info.refusedSpawns, info.freelistCount, info.liveCount) == (5, 35, 0, n)
    others = np.setdiff1d(i, free)
    assert got[others].tobytes() == want[others].tobytes()
    predicted = set(keys(children))
    made = keys(got[free])
    assert len(set(made)) == 5 and all(k in predicted for k in made)  # five of the forty, each once
    assert got_idx.tobytes() == idx.tobytes()  # no slot is lost: the entries are still there for the next push
    # the next launch starts from 0, not from a negative count: nothing is granted, nothing breaks
    run(gpu_ctx, n, S.PARTICLES_DECAY | S.PARTICLES_SIMULATE, dt=float(DT), sim_frame=6)
    assert gpu_ctx.read_particles()[1] == 0


def test_twenty_steps_after_a_reset_are_predicted_exactly(gpu_ctx):
    """The whole record, render aside.  The emitters' rng depends on their slots, which the model takes from the
    read-back of the reset step's init (one call: decay and init; simulate runs from the next call on, so that the first
    simulated step is checked too).  Children draw no random numbers, so the multiset of live records is exact."""
    world = synthetic_world()
    gpu_ctx.upload_scene(world)
    n, dt = 700, 1.0 / 60.0
    place_fresh(gpu_ctx, n)
    run(gpu_ctx, n, S.PARTICLES_DECAY | S.PARTICLES_INIT, reset=1, source=1)
    emitters, count, _ = gpu_ctx.read_particles()
    assert np.array_equal(P.multiset(emitters[P.live(emitters)]), P.multiset(P.init_records(world, 1))) and count == n - 24
    children = np.zeros(0, S.PARTICLE_DTYPE)
    for step in range(1, 21):
        run(gpu_ctx, n, NO_RENDER, reset=0, dt=dt, sim_frame=step, source=1)
        emitters, born, _ = P.simulate(emitters, dt, step)
        children = np.concatenate([P.simulate(children, dt, step)[0], born])  # the newborn are not simulated
        got, got_count, got_idx = gpu_ctx.read_particles()
        model = np.concatenate([emitters[P.live(emitters)], children])
        assert np.array_equal(P.multiset(got[P.live(got)]), P.multiset(model)), step
        assert got_count == n - len(model)
        assert_pool_is_consistent(got, got_count, got_idx)
    assert len(children) == 24 * 3  # a spawn every 0.1 s: steps 6, 12 and 18


# ---- render ----

W, H = 448, 512
EYE = np.array([0.0, 1.0, 3.0])
ZN = 0.02
N_RENDER = 1024


class DeviceArray:
    """device memory through the HIP runtime the library itself uses"""

    def __init__(self, nbytes):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.ptr = ctypes.c_void_p()
        self.nbytes = nbytes
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(nbytes)) == 0

    def upload(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.nbytes
        assert self.hip.hipMemcpy(self.ptr, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes), 1) == 0

    def download(self, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        assert out.nbytes == self.nbytes
        assert self.hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), self.ptr, ctypes.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.ptr)


def render_camera(oracle):
    return oracle.camera_uniforms(tuple(EYE), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), math.radians(59.0), ZN, 100.0, W, H)[0]


def render_design(camera):
    """-> (records, classes, depth image): hand-placed particles in front of a camera looking down -z, and a depth that is
    sky (0) on the left, a far wall on the right and a near strip of 30 columns in it."""
    focal = (H / 2) / math.tan(math.radians(59.0) / 2)  # pixels per unit of x / distance

    def at(px, py, d):  # the world position that projects to pixel coordinates (px, py) at distance d
        return EYE + np.array([(px - W / 2) * d / focal, -(py - H / 2) * d / focal, -d])

    rec, _, _ = P.fresh_pool(N_RENDER)
    classes = {}
    slot = [300]  # above 255, over two blocks

    def put(name, position, lifetime=4.0, emitter=False, at_slot=None):
        s = slot[0] if at_slot is None else at_slot
        if at_slot is None:
            slot[0] += 1
        rec["position_lifetime"][s, :3] = position
        rec["position_lifetime"][s, 3] = lifetime
        rec["mask"][s] = S.PARTICLE_MASK_EMIT if emitter else (S.PARTICLE_MASK_GRAVITY | S.PARTICLE_MASK_DECAY)
        classes.setdefault(name, []).append(s)
        return s

    big = 0.05  # 18 pixels a side
    put("front", at(60, 60, big), emitter=True)               # overlapping, different depths: the nearer one covers
    put("back", at(68, 66, 0.08))
    put("same_low_emitter", at(120, 60, 0.06), emitter=True)  # the same position twice: the lower slot wins
    put("same_high", at(120, 60, 0.06))
    put("same_low", at(180, 60, 0.06))
    put("same_high_emitter", at(180, 60, 0.06), emitter=True)
    put("over_wall", at(300, 60, big))                        # in front of the far wall
    put("behind_strip", at(415, 200, 0.08), emitter=True)     # behind the near strip
    for k in range(65):                                       # the fade: alpha = k / 64, over the sky
        put("fade", at(20 + 22 * (k % 10), 120 + 24 * (k // 10), big), lifetime=(k / 64.0) / 4.0)
    for name, px, py in (("edge_left", 0, 300), ("edge_right", W, 330), ("edge_top", 200, 0), ("edge_bottom", 230, H),
                         ("corner", W, H)):
        put(name, at(px, py, big), emitter=True)
    for k in range(12):                                       # under a pixel: 0.45 pixels a side at distance 2
        put("tiny", at(40 + 3 * k + k / 12.0, 420 + k / 7.0, 2.0), emitter=k % 2 == 0)
    put("medium", at(250.3, 420.6, 0.3))                      # three pixels
    put("behind_camera", EYE + np.array([0.0, 0.0, 0.5]))
    put("before_near_plane", at(224, 256, ZN / 2))
    put("outside", at(-200, 256, big))
    put("dead", at(224, 256, big), lifetime=-9999.0)
    put("negative_lifetime", at(224, 300, big), lifetime=-0.125)
    put("first_slot", at(350, 300, 0.1), at_slot=0)           # slot 0: ~slot is all ones
    put("last_slot", at(350, 340, 0.1), at_slot=N_RENDER - 1)

    def depth_of(d):
        return P.quad_corners(at(224, 256, d).astype(F), camera, W, H)[0]

    depth = np.zeros((H, W), F)
    depth[:, 260:] = depth_of(2.5)
    depth[:, 400:430] = depth_of(0.04)
    return rec, classes, depth


@pytest.fixture(scope="module")
def render_setup(gpu_ctx, oracle):
    """The HDR image is a caller-owned buffer, so that the test can put a designed image into it: one small render makes
    the context adopt it at this extent."""
    cam = render_camera(oracle)
    hdr = DeviceArray(W * H * 16)
    depth = DeviceArray(W * H * 4)
    world = scenes.cornell()
    gpu_ctx.upload_scene(world)
    gpu_ctx.set_output_buffer(hdr.ptr.value, hdr.nbytes)
    c = world.camera
    rcam, focal = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], W, H)
    pc = S.ReferencePC(0, S.PC_FLAG_SKIP_HISTORY, 1, 1e-5, 1.0, focal, 3, 1)
    gpu_ctx.render(pc, rcam, W, H)
    gpu_ctx.read_hdr()
    yield cam, hdr, depth
    # back to the context's own image before the buffer goes
    gpu_ctx.set_output_buffer(None, 0)
    gpu_ctx.render(pc, rcam, 8, 8)
    gpu_ctx.read_hdr()
    hdr.free()
    depth.free()


@pytest.mark.parametrize("frame", (0, 1, 9, 63))
def test_render_matches_the_restatement_bit_for_bit(gpu_ctx, render_setup, frame):
    cam, hdr, depth = render_setup
    rec, classes, depth_in = render_design(cam)
    hdr_in = np.random.default_rng(9).uniform(0.0, 4.0, (H, W, 4)).astype(F)
    want_hdr, want_depth, fragments = P.render(rec, cam, W, H, frame, hdr_in, depth_in)

    # ---- the design does what it was made for (on the restatement's output) ----
    def count(name):
        return int(sum(fragments[s] for s in classes[name]))

    def covered(name):
        d, X, Y = P.quad_corners(rec["position_lifetime"][classes[name][0], :3], cam, W, H)
        return len(P.quad_coverage(X, Y, 1 << 14, 1 << 14)[0]), max(X) - min(X)
    full, side = covered("front")
    assert side >= 8 * 256 and count("front") == full  # at least eight pixels a side, all of them in front
    assert 0 < count("back") < covered("back")[0]       # partly covered by the nearer quad
    assert count("same_low_emitter") > 0 and count("same_high") == 0
    assert count("same_low") > 0 and count("same_high_emitter") == 0
    assert count("over_wall") == covered("over_wall")[0] > 0 and count("behind_strip") == 0
    fade = [int(fragments[s]) for s in classes["fade"]]
    assert fade[64] == covered("fade")[0] and 0 < fade[0] < fade[16] < fade[32] < fade[48] < fade[64]
    for name in ("edge_left", "edge_right", "edge_top", "edge_bottom", "corner"):
        assert 0 < count(name) < full, name  # straddles the edge: some of it, not all
    tiny = [int(fragments[s]) for s in classes["tiny"]]
    assert max(tiny) == 1 and min(tiny) == 0 and covered("tiny")[1] < 256  # under a pixel: one pixel or none
    assert 4 <= count("medium") <= 16
    for name in ("behind_camera", "before_near_plane", "outside", "dead", "negative_lifetime"):
        assert count(name) == 0, name
        assert name in ("dead", "negative_lifetime", "outside") or P.quad_corners(
            rec["position_lifetime"][classes[name][0], :3], cam, W, H) is None
    assert count("first_slot") > 0 and count("last_slot") > 0
    changed = ~same_bits(want_depth, depth_in)
    assert changed.sum() == fragments.sum() > 2000
    yellow, magenta = np.array([1, 1, 0, 1], F), np.array([1, 0, 1, 1], F)
    assert ((want_hdr[changed] == yellow).all(1) | (want_hdr[changed] == magenta).all(1)).all()
    assert same_bits(want_hdr[~changed], hdr_in[~changed]).all()

    # ---- the pass ----
    gpu_ctx.set_particles(rec, 0, np.arange(N_RENDER, dtype=np.int32))
    results = []
    for _ in range(2):  # a second call with the same inputs gives the same bits (the keys were left zero)
        hdr.upload(hdr_in)
        depth.upload(depth_in)
        run(gpu_ctx, N_RENDER, S.PARTICLES_RENDER, render_frame=frame, camera=cam, w=W, h=H, depth_ptr=depth.ptr.value)
        info = gpu_ctx.particles_info()
        assert info.fragmentsWritten == fragments.sum()
        results.append((hdr.download((H, W, 4)), depth.download((H, W))))
    got_hdr, got_depth = results[0]
    bad = ~(same_bits(got_hdr, want_hdr).all(2) & same_bits(got_depth, want_depth))
    assert not bad.any(), "%d pixels differ, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    assert same_bits(results[1][0], got_hdr).all() and same_bits(results[1][1], got_depth).all()
    # the records and the freelist are read-only to render
    after = gpu_ctx.read_particles()
    assert after[0].tobytes() == rec.tobytes() and after[1] == 0


def test_render_refuses_what_it_cannot_write(gpu_ctx, render_setup):
    cam, hdr, depth = render_setup
    host = np.zeros((H, W), F)
    with pytest.raises(Exception, match="device memory"):
        run(gpu_ctx, N_RENDER, S.PARTICLES_RENDER, camera=cam, w=W, h=H, depth_ptr=host.ctypes.data)
    with pytest.raises(Exception, match="another extent"):
        run(gpu_ctx, N_RENDER, S.PARTICLES_RENDER, camera=cam, w=W - 1, h=H, depth_ptr=depth.ptr.value)
    with pytest.raises(Exception, match="unknown stage bits"):
        run(gpu_ctx, N_RENDER, 32)


def test_render_over_the_last_traced_depth_equals_the_same_depth_as_the_callers(gpu_ctx, render_setup, oracle):
    """No depth - the last traced G-buffer's, read and written where it lies - gives, bit for bit, the image and the depth
    that a device copy of that G-buffer's depth gives as the caller's."""
    w, h = 50, 35
    world = scenes.cornell()  # (what render_setup uploaded)
    c = world.camera
    cam, _ = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)
    # A quad is 2 mm across, far less than a pixel of this image: it draws only where it covers a pixel's centre.  So the
    # particles lie on the rays through the centres of random pixels, some in front of the room's surfaces, some behind.
    eye, target, up = (np.array(c[k], np.float64) for k in ("eye", "target", "up"))
    forward = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(forward, up) / np.linalg.norm(np.cross(forward, up))
    focal = (h / 2) / math.tan(c["fov"] / 2)  # pixels per unit of x / distance
    rng = np.random.default_rng(5)
    n = 600
    px, py, d = rng.integers(0, w, n), rng.integers(0, h, n), rng.uniform(0.5, 6.0, n)
    rays = forward * focal + right * (px + 0.5 - w / 2)[:, None] - np.cross(right, forward) * (py + 0.5 - h / 2)[:, None]
    rec, _, _ = P.fresh_pool(N_RENDER)
    rec["position_lifetime"][300:300 + n, :3] = eye + rays / focal * d[:, None]
    rec["position_lifetime"][300:300 + n, 3] = 4.0
    rec["mask"][300:300 + n] = S.PARTICLE_MASK_GRAVITY | S.PARTICLE_MASK_DECAY
    gpu_ctx.set_particles(rec, 0, np.arange(N_RENDER, dtype=np.int32))

    gpu_ctx.deferred_shading_traced(cam, w, h)
    hdr_in, depth_in = gpu_ctx.read_hdr(), gpu_ctx.read_gbuffer()[2]
    run(gpu_ctx, N_RENDER, S.PARTICLES_RENDER, camera=cam, w=w, h=h)
    written = gpu_ctx.particles_info().fragmentsWritten
    last_hdr, last_depth = gpu_ctx.read_hdr(), gpu_ctx.read_gbuffer()[2]
    assert written > 0 and not same_bits(last_depth, depth_in).all()  # (the pass drew, and into the G-buffer's own depth)

    gpu_ctx.deferred_shading_traced(cam, w, h)  # the same image and depth again
    assert gpu_ctx.read_hdr().tobytes() == hdr_in.tobytes() and gpu_ctx.read_gbuffer()[2].tobytes() == depth_in.tobytes()
    own = DeviceArray(w * h * 4)
    try:
        own.upload(depth_in)
        run(gpu_ctx, N_RENDER, S.PARTICLES_RENDER, camera=cam, w=w, h=h, depth_ptr=own.ptr.value)
        assert gpu_ctx.particles_info().fragmentsWritten == written
        assert gpu_ctx.read_hdr().tobytes() == last_hdr.tobytes()
        assert own.download((h, w)).tobytes() == last_depth.tobytes()
    finally:
        own.free()
