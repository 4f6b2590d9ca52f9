"""Meshlet culling on the GPU (prosper_pt_cull_meshlets_*, prosper_pt_cull_gbuffer; pt_culling.hip).

Sweep: a scene whose meshes are a few small triangles per meshlet but whose bounds words are written by the test
(tests/culling_scenes.py); the lists against tests/culling_reference.py as sorted sets, the counts, the argument triples and
DrawStats exactly.  Property: a wall, a tessellated plane behind it, hidden, outside and away-facing instances; the set of
meshlets that own a pixel, from a brute-force float64 coverage, must lie in the two phases' lists."""
import ctypes as C

import numpy as np
import pytest

import culling_reference as R
import culling_scenes as CS
from prosper_amd import capi, scenes, structs as S
from prosper_amd import world as W

pytestmark = pytest.mark.gpu

F = np.float32
W_, H_ = CS.WIDTH, CS.HEIGHT


def as_set(pairs):
    return sorted(map(tuple, np.asarray(pairs).reshape(-1, 2).tolist()))


def check_lists(ctx, world, view, mode, hiz=None, second_hiz=None, m2w=None):
    """the lists, counts, argument triples and DrawStats the context holds are the restatement's"""
    gen = R.generate(world, mode)
    vis, occ, tris = R.cull_list(world, gen, view, m2w, hiz)
    got_gen, a0 = ctx.read_draw_list(S.DRAW_LIST_GENERATED)
    assert as_set(got_gen) == as_set(gen) and list(a0) == [0, 0, 0]
    assert len(set(as_set(got_gen))) == len(got_gen)  # no entry twice
    got_vis, args = ctx.read_draw_list(S.DRAW_LIST_FIRST_PHASE)
    assert as_set(got_vis) == as_set(vis)
    assert list(args) == R.args_of(len(gen), len(vis))
    drawn = len(vis)
    if hiz is None:
        with pytest.raises(capi.ProsperPtError, match="did not produce"):
            ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE_INPUT)
    else:
        got_occ, _ = ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE_INPUT)
        assert as_set(got_occ) == as_set(occ)
    if second_hiz is not None:
        vis2, _, tris2 = R.cull_list(world, occ, view, m2w, second_hiz)
        got2, args2 = ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE)
        assert as_set(got2) == as_set(vis2)
        assert list(args2) == R.args_of(len(occ), len(vis2))
        drawn, tris = drawn + len(vis2), tris + tris2
    stats = ctx.draw_stats()
    want = R.totals(world, mode)
    assert {k: getattr(stats, k) for k in want} == want
    assert (stats.drawnMeshletCount, stats.rasterizedTriangleCount) == (drawn, tris)
    return gen, vis, occ


@pytest.fixture(scope="module")
def sweep(gpu_ctx):
    cam = CS.camera_at()
    full, info = CS.sweep_world(cam)
    loaded = [i for i in range(len(full.metadatas)) if i != info["missing_mesh"]]
    world = full.with_meshes_loaded(loaded)
    gpu_ctx.upload_scene(world)
    return gpu_ctx, world, cam, R.View(cam), info


def test_the_scales_are_the_rule_s_at_upload_and_after_an_update(sweep):
    ctx, world, cam, view, info = sweep
    n = len(world.model_instances)
    want = R.instance_scales(R.transforms_of(world))
    got = ctx.read_instance_scales(n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    inst = info["instances"]
    assert got[inst["scaled"]] == 2 and got[inst["negative"]] == F(1.5) and got[inst["non_uniform"]] == 0 and got[0] == 1
    with pytest.raises(capi.ProsperPtError, match="model instance count"):
        ctx.read_instance_scales(n + 1)


def test_without_a_pyramid_the_planes_and_the_cone_decide(sweep):
    ctx, world, cam, view, info = sweep
    ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE)
    gen, vis, occ = check_lists(ctx, world, view, R.MODE_OPAQUE)
    assert len(occ) == 0 and 0 < len(vis) < len(gen)
    # the cases are meaningful: each plane and the cone have entries on both sides in the restatement
    bounds, _, insts = R.meshlet_words(world, gen)
    m2w = R.transforms_of(world)
    r = R.cull(bounds, m2w[insts], R.instance_scales(m2w)[insts], view)
    labels = info["labels"]
    first = {l: k for k, l in enumerate(labels)}
    identity = np.array([k for k, (d, m) in enumerate(gen.tolist()) if d < info["labelled_meshes"]])  # the labelled bounds' meshes
    assert len(identity) == len(labels)
    for plane in ("nearPlane", "farPlane", "leftPlane", "rightPlane", "bottomPlane", "topPlane"):
        ks = [first[l] for l in labels if l.startswith("plane " + plane)]
        out = r["outside"][identity][ks]
        assert out.any() and not out.all(), plane
    ks = [first[l] for l in labels if l.startswith("cone")]
    hidden = r["cone_hidden"][identity][ks]
    assert hidden.any() and not hidden.all()
    assert not r["cone_hidden"][identity][first["cone cutoff 127"]] and r["cone_hidden"][identity][first["cone cutoff 120"]]
    assert r["cone_hidden"][identity][first["cone at +0"]] and not r["cone_hidden"][identity][first["cone at +1"]]
    assert r["outside"][identity][first["behind the eye"]] and r["visible"][identity][first["straddles near"]]


@pytest.mark.parametrize("columns", [W_, 40, 0])
def test_against_a_designed_pyramid_every_list_is_the_restatement_s(sweep, columns):
    ctx, world, cam, view, info = sweep
    depth = CS.wall_depth(cam, columns)
    rng = np.random.default_rng(columns)
    if columns == 40:
        depth[rng.integers(0, H_, 40), rng.integers(0, W_, 40)] = 0  # holes in the wall
    ctx.hiz_downsample(W_, H_, slot=0, depth=depth)
    hiz = R.hiz_pyramid(depth)
    ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE, hiz_slot=0)
    gen, vis, occ = check_lists(ctx, world, view, R.MODE_OPAQUE, hiz)
    if columns:
        assert len(occ) > 10
        # footprints land on every level and past the last: the restatement's own levels say so
        labels = info["labels"]
        assert any(l.startswith("behind r 0.0005") for l in labels) and any(l.startswith("behind r 8") for l in labels)
    else:
        assert len(occ) == 0  # a sky never occludes
    # the second phase against a pyramid with the wall pushed back: what hid behind the near wall shows in front of it
    far = CS.wall_depth(cam, columns, wall_z=-30.0)
    ctx.hiz_downsample(W_, H_, slot=1, depth=far)
    ctx.cull_second_phase(cam, 1)
    check_lists(ctx, world, view, R.MODE_OPAQUE, hiz, R.hiz_pyramid(far))
    got2, _ = ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE)
    assert (len(got2) > 0) == (columns != 0)
    # the transparent mode: BLEND only, against the current pyramid
    ctx.cull_first_phase(cam, S.CULL_MODE_TRANSPARENT, hiz_slot=0)
    gen_t, _, _ = check_lists(ctx, world, view, R.MODE_TRANSPARENT, hiz)
    assert 0 < len(gen_t) < len(gen) and not set(as_set(gen_t)) & set(as_set(gen))


def test_the_border_reads_the_far_plane(sweep):
    """a wall over the whole image: a sphere behind it whose centre lies off the screen gathers border texels, which are 0
    and never cull, whatever the shader's comment says about 1"""
    ctx, world, cam, view, info = sweep
    depth = CS.wall_depth(cam, W_)
    gen = R.generate(world, R.MODE_OPAQUE)
    bounds, _, insts = R.meshlet_words(world, gen)
    m2w = R.transforms_of(world)
    r = R.cull(bounds, m2w[insts], R.instance_scales(m2w)[insts], view, R.hiz_pyramid(depth))
    labels = info["labels"]
    off = [k for k, l in enumerate(labels) if l.startswith("off screen")]
    behind = [k for k, l in enumerate(labels) if l.startswith("behind r 0.25")]
    assert r["visible"][off].any() and not r["occluded"][off].all()
    assert r["occluded"][behind].all()


def test_a_moved_instance_is_culled_where_it_is_now(sweep, gpu_ctx):
    ctx, world, cam, view, info = sweep
    depth = CS.wall_depth(cam, 40)
    ctx.hiz_downsample(W_, H_, slot=0, depth=depth)
    hiz = R.hiz_pyramid(depth)
    moved = info["instances"]["moved"]
    model, before = world.model_instances[moved]
    try:
        ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE, hiz_slot=0)
        _, vis0, occ0 = check_lists(ctx, world, view, R.MODE_OPAQUE, hiz)
        world.model_instances[moved] = (model, W.translate((0.25, 0.0, 0.0)) @ W.scale(1.25))
        ctx.update_transforms(world)  # staged: the culling call flushes it
        ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE, hiz_slot=0)
        _, vis1, occ1 = check_lists(ctx, world, view, R.MODE_OPAQUE, hiz)
        di = [k for k, d in enumerate(R.draw_instances_of(world)) if d[0] == moved]
        count = lambda pairs: sum(1 for d, m in as_set(pairs) if d in di)
        assert count(vis0) == 0 and count(occ0) == 0 and count(vis1) > 0 and count(occ1) > 0
        scales = ctx.read_instance_scales(len(world.model_instances))
        assert np.array_equal(scales.view(np.uint32), R.instance_scales(R.transforms_of(world)).view(np.uint32))
        assert scales[moved] == F(1.25)
    finally:
        world.model_instances[moved] = (model, before)
        ctx.update_transforms(world)
        ctx.read_instance_scales(len(world.model_instances))


def test_refusals(sweep):
    ctx, world, cam, view, info = sweep
    lib = capi.lib()
    ctx.hiz_downsample(W_, H_, slot=0, depth=CS.wall_depth(cam))
    with pytest.raises(capi.ProsperPtError, match="unknown mode"):
        ctx.cull_first_phase(cam, 2)
    with pytest.raises(capi.ProsperPtError, match="hizSlot"):
        ctx.cull_first_phase(cam, 0, hiz_slot=2)
    ctx.hiz_downsample(8, 8, slot=1, depth=np.zeros((8, 8), F))
    with pytest.raises(capi.ProsperPtError, match="source extent"):
        ctx.cull_first_phase(cam, 0, hiz_slot=1)
    ctx.cull_first_phase(cam, 0)  # no pyramid: no second-phase input
    with pytest.raises(capi.ProsperPtError, match="second-phase input"):
        ctx.cull_second_phase(cam, 0)
    n = C.c_uint32()
    assert lib.prosper_pt_read_draw_list(ctx._h, 4, C.byref(n), None, 0, None, None) == -1
    assert lib.prosper_pt_cull_gbuffer(None, C.byref(cam), None) == -1
    fresh = capi.Context(device=0)
    try:
        assert lib.prosper_pt_cull_meshlets_first_phase(fresh._h, 0, C.byref(cam), S.NO_HIZ, None) == -4  # no scene
        assert lib.prosper_pt_cull_gbuffer(fresh._h, C.byref(cam), None) == -4
        assert lib.prosper_pt_read_draw_list(fresh._h, 1, C.byref(n), None, 0, None, None) == -4
        # meshlet ranges that leave the buffer are refused, once the culler is asked
        bad = scenes.World()
        m = bad.add_material()
        mesh = CS.add_designed_mesh(bad, [CS.bounds_word((0, 0, -5), 1.0)] * 3, m)
        bad.add_instance(bad.add_model([(mesh, m)]))
        bad.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 5.0, 0.0))
        bad.metadatas[mesh].meshletBoundsOffset = bad._buffer_words[0] - 10  # three bounds need fifteen words
        fresh.upload_scene(bad)  # the upload's rules have not changed
        with pytest.raises(capi.ProsperPtError, match="meshletBounds leave") as e:
            fresh.cull_first_phase(cam, 0)
        assert e.value.code == -5  # PROSPER_PT_ERR_SCENE
    finally:
        fresh.close()


def test_the_cpp_culler_records_what_the_direct_calls_record(sweep):
    from prosper_amd import rt_reference
    ctx, world, cam, view, info = sweep
    depth, far = CS.wall_depth(cam, 40), CS.wall_depth(cam, 40, wall_z=-30.0)
    ctx.hiz_downsample(W_, H_, slot=0, depth=depth)
    ctx.hiz_downsample(W_, H_, slot=1, depth=far)
    hcam = rt_reference.Camera()
    hcam.set_parameters(CS.FOV, CS.NEAR, CS.FAR)
    hcam.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    culler = rt_reference.MeshletCuller(ctx)
    try:
        out = culler.record_first_phase(hcam, W_, H_, culler.MODE_OPAQUE, hierarchical_depth=0)
        stats, landed = culler.read_draw_stats(wait=False)  # the totals at once, whether or not the counts have landed
        want = R.totals(world, R.MODE_OPAQUE)
        assert {k: getattr(stats, k) for k in want} == want
        lp, ap, cap = ctx.draw_list_device_ptr(S.DRAW_LIST_FIRST_PHASE)
        assert (out.dataBuffer, out.argumentBuffer, out.capacity) == (lp, ap, cap)
        assert out.secondPhaseInput == ctx.draw_list_device_ptr(S.DRAW_LIST_SECOND_PHASE_INPUT)[0]
        out2 = culler.record_second_phase(hcam, W_, H_, 1)
        assert (out2.dataBuffer, out2.argumentBuffer) == ctx.draw_list_device_ptr(S.DRAW_LIST_SECOND_PHASE)[:2] and not out2.secondPhaseInput
        check_lists(ctx, world, view, R.MODE_OPAQUE, R.hiz_pyramid(depth), R.hiz_pyramid(far))
        stats, landed = culler.read_draw_stats()
        direct = ctx.draw_stats()
        assert landed and bytes(stats) == bytes(direct) and stats.drawnMeshletCount > 0
        # the transparent mode without a pyramid: no second-phase input
        out = culler.record_first_phase(hcam, W_, H_, culler.MODE_TRANSPARENT)
        assert not out.secondPhaseInput
        check_lists(ctx, world, view, R.MODE_TRANSPARENT)
        # a refusal keeps the library's own code
        with pytest.raises(capi.ProsperPtError, match="second-phase input") as e:
            culler.record_second_phase(hcam, W_, H_, 1)
        assert e.value.code == -1
        with pytest.raises(capi.ProsperPtError, match="source extent"):
            culler.record_first_phase(hcam, W_ + 2, H_, hierarchical_depth=0)
    finally:
        culler.close()
        hcam.close()


def test_the_scales_follow_an_animated_update(gpu_ctx):
    """prosper_pt_animate is the third place a transform table is made: the scales beside it are the rule's over the table
    the device holds afterwards"""
    import os
    from prosper_amd import animation, gltf
    fixture = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "animated_scene.gltf")
    world = gltf.load_gltf(fixture)
    gpu_ctx.upload_scene(world)
    gpu_ctx.set_animations(animation.load_animations(fixture))
    n = len(world.model_instances)
    seen = []
    for t in (0.0, 0.55, 1.7):
        gpu_ctx.animate(t)  # staged: the read-back flushes it
        got = gpu_ctx.read_instance_scales(n)
        table = np.frombuffer(gpu_ctx.read_animated_transforms(), np.float32).reshape(-1, 2, 3, 4)[:n, 0]
        want = R.instance_scales(table)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), t
        seen.append(table.copy())
    assert not np.array_equal(seen[0], seen[1])  # the table did move


# (last: these upload scenes of their own into the session's context)
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_lists_of_every_length_around_a_wave(gpu_ctx, count):
    cam = CS.camera_at()
    view = R.View(cam)
    rng = np.random.default_rng(count)
    w = scenes.World()
    opaque = w.add_material(base_color=(0.8, 0.8, 0.8, 1.0))
    blend = w.add_material(base_color=(0.2, 0.2, 0.8, 0.5), alpha_mode=S.ALPHA_MODE_BLEND)
    n = max(count, 1)
    centres = np.stack([rng.uniform(-14, 14, n), rng.uniform(-9, 9, n), rng.uniform(-20, -4, n)], axis=1)
    bounds = [CS.bounds_word(c, r, (0, 0, int(a)), int(k)) for c, r, a, k in
              zip(centres, rng.uniform(0.05, 2.0, n), rng.choice([-127, 127], n), rng.integers(0, 128, n))]
    mesh = CS.add_designed_mesh(w, bounds, opaque if count else blend)
    w.add_instance(w.add_model([(mesh, opaque if count else blend)]))  # count 0: nothing opaque, an empty list
    w.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 5.0, 0.0))
    gpu_ctx.upload_scene(w)
    depth = CS.wall_depth(cam, 60, wall_z=-9.0)
    gpu_ctx.hiz_downsample(W_, H_, slot=1, depth=depth)
    gpu_ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE, hiz_slot=1)
    gen, vis, occ = check_lists(gpu_ctx, w, view, R.MODE_OPAQUE, R.hiz_pyramid(depth))
    assert len(gen) == count
    if count >= 63:
        assert 0 < len(vis) < count and len(occ) > 0
    far = CS.wall_depth(cam, 60, wall_z=-40.0)
    gpu_ctx.hiz_downsample(W_, H_, slot=0, depth=far)
    gpu_ctx.cull_second_phase(cam, 0)
    check_lists(gpu_ctx, w, view, R.MODE_OPAQUE, R.hiz_pyramid(depth), R.hiz_pyramid(far))
    lp, ap, cap = gpu_ctx.draw_list_device_ptr(S.DRAW_LIST_FIRST_PHASE)
    assert lp and ap and cap >= count


# ---- the property: no meshlet that owns a pixel is ever dropped ----

def test_no_meshlet_that_owns_a_pixel_is_dropped(gpu_ctx):
    world, inst = CS.property_world()
    gpu_ctx.upload_scene(world)
    di_of = {name: [k for k, d in enumerate(R.draw_instances_of(world)) if d[0] == i] for name, i in inst.items()}
    plane_meshlets = world.mesh_infos[world.models[world.model_instances[inst["plane"]][0]][0][0]].meshletCount
    assert 24 <= plane_meshlets <= 80
    frames = []
    for frame, eye_x in enumerate((0.0, 0.3)):
        cam = CS.camera_at((eye_x, 0.0, 0.0), (eye_x, 0.0, -1.0))
        gpu_ctx.trace_gbuffer(cam, W_, H_, jitter=False)
        gpu_ctx.cull_gbuffer(cam)
        first, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_FIRST_PHASE)
        generated, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_GENERATED)
        if frame == 0:
            # no previous pyramid: nothing is occluded, no second phase; what the planes and the cones leave is drawn
            with pytest.raises(capi.ProsperPtError, match="did not produce"):
                gpu_ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE)
            second = np.zeros((0, 2), np.uint32)
            vis, occ, _ = R.cull_list(world, R.generate(world, R.MODE_OPAQUE), R.View(cam))
            assert as_set(first) == as_set(vis) and len(occ) == 0
        else:
            second, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE)
        drawn = set(as_set(first)) | set(as_set(second))
        owning, depth = CS.owners(world, cam)
        traced = gpu_ctx.read_gbuffer()[2]
        assert np.abs(traced.astype(np.float64) - depth).max() < 1e-4  # the ground truth's depth is the traced one
        # 1. every meshlet that owns a pixel is in one of the two lists
        assert owning <= drawn, sorted(owning - drawn)[:5]
        assert len({o for o in owning if o[0] in di_of["plane"]}) >= 8 and any(o[0] in di_of["wall"] for o in owning)
        assert not any(o[0] in di_of["hidden"] + di_of["outside"] + di_of["away"] for o in owning)
        stats = gpu_ctx.draw_stats()
        assert stats.drawnMeshletCount == len(first) + len(second) and stats.totalMeshletCount == len(generated)
        frames.append((drawn, first, second))
    # 2. in the second frame the wholly hidden, the outside and the away-facing instances contribute nothing
    drawn, first, second = frames[1]
    for name in ("hidden", "outside", "away"):
        assert not any(d in di_of[name] for d, m in drawn), name
    # ... and the occlusion test did something: part of the plane lies behind the wall and is not drawn
    plane_drawn = {m for d, m in drawn if d in di_of["plane"]}
    assert 0 < len(plane_drawn) < plane_meshlets
    # 3. the first frame drew the hidden instance (nothing could say it was hidden yet), the second did not
    assert any(d in di_of["hidden"] for d, m in frames[0][0])
    # the pyramid the call kept is the traced depth's
    kept = [s for s in (0, 1) if gpu_ctx.hiz_info(s).valid]
    assert kept
