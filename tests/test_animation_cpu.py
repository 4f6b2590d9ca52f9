"""Keyframe animation without a GPU: known answers of the NumPy restatement the GPU tests compare the
kernels with (tests/animation_reference.py), the glTF parser (prosper_amd/animation.py) against `load_gltf`, the error of
float32 slerp over the GPU tests' case list, and the exported symbols."""
import math
import os
import re

import numpy as np
import pytest

import animation_reference as R
from prosper_amd import animation, capi, gltf, structs as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "animated_scene.gltf")
TINY = os.path.join(HERE, "golden", "tiny_scene.gltf")
NONE = S.ANIMATION_NONE
U = 2.0 ** -24  # unit roundoff of float32


def node(parent=NONE, flags=0, translation=(0, 0, 0), rotation=(0, 0, 0, 1), scale=(1, 1, 1), model_instance=NONE):
    n = S.AnimationNode()
    n.parent, n.modelInstance, n.pointLight, n.spotLight, n.flags = parent, model_instance, NONE, NONE, flags
    n.translation[:], n.rotation[:], n.scale[:] = translation, rotation, scale
    return n


def tables_of(nodes, channels):
    """channels: (node, path, interpolation, times, values[, start, end])"""
    out, times, values = [], [], []
    for spec in channels:
        nd, path, interpolation, t, v = spec[:5]
        t, v = np.asarray(t, np.float32), np.asarray(v, np.float32)
        c = S.AnimationChannel()
        c.node, c.path, c.interpolation = nd, path, interpolation
        c.timeOffset, c.keyCount = sum(x.size for x in times), t.size
        c.valueOffset, c.valueWidth = sum(x.size for x in values), v.shape[1]
        c.startTimeS, c.endTimeS = (spec[5], spec[6]) if len(spec) > 5 else (float(t.min()), float(t.max()))
        out.append(c)
        times.append(t)
        values.append(v.reshape(-1))
    return animation.AnimationTables(nodes, out, np.concatenate(times), np.concatenate(values))


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.float32(np.append(a * math.sin(angle / 2), math.cos(angle / 2)))


@pytest.fixture(scope="module")
def fixture_tables():
    return animation.load_animations(FIXTURE)


# ---- known answers ----

def test_linear_translation_at_the_midpoint():
    t = tables_of([node()], [(0, S.ANIMATION_PATH_TRANSLATION, S.ANIMATION_LINEAR, [0.0, 2.0], [[1, 2, 3], [3, 6, -1]])])
    trs = R.evaluate_trs(t, 1.0)
    assert trs.dtype == np.float32 and np.array_equal(trs[0, :3], np.float32([2, 4, 1]))
    # the early-outs: at or before the start the first key, at or past the end the last one
    assert np.array_equal(R.evaluate_trs(t, -1.0)[0, :3], np.float32([1, 2, 3]))
    assert np.array_equal(R.evaluate_trs(t, 0.0)[0, :3], np.float32([1, 2, 3]))
    assert np.array_equal(R.evaluate_trs(t, 2.0)[0, :3], np.float32([3, 6, -1]))
    assert np.array_equal(R.evaluate_trs(t, 9.0)[0, :3], np.float32([3, 6, -1]))


def test_half_of_a_quarter_turn_is_an_eighth_turn():
    t = tables_of([node()], [(0, S.ANIMATION_PATH_ROTATION, S.ANIMATION_LINEAR, [0.0, 1.0],
                              [[0, 0, 0, 1], quat([0, 0, 1], math.pi / 2)])])
    got = R.evaluate_trs(t, 0.5)[0, 3:7]
    want = np.array([0, 0, math.sin(math.pi / 8), math.cos(math.pi / 8)])
    # sin(theta / 2) / sin(theta) with theta = acos(cos(pi / 4)): three float32 transcendentals and a division, each
    # within an ulp or two of a value below 1
    assert np.max(np.abs(got - want)) <= 8 * U


def test_cubic_spline_with_zero_tangents_at_half_is_the_midpoint():
    t = tables_of([node()], [(0, S.ANIMATION_PATH_SCALE, S.ANIMATION_CUBICSPLINE, [0.0, 4.0],
                              [[0, 0, 0], [1, 2, 3], [0, 0, 0], [0, 0, 0], [3, 4, 9], [0, 0, 0]])])
    assert np.array_equal(R.evaluate_trs(t, 2.0)[0, 7:10], np.float32([2, 3, 6]))
    # exactly on a key: the value in the middle of the key's three
    assert np.array_equal(R.evaluate_trs(t, 4.0)[0, 7:10], np.float32([3, 4, 9]))


def test_cubic_spline_tangents_are_scaled_by_the_elapsed_time():
    """stepDuration = timeS - firstTime (Accessors.cpp:67), not the key interval.  Keys at 0 and 2, sampled at 0.5:
    t = 0.25, td = 0.5; with vk = 1, bk = 4, vk1 = 3, ak1 = 8 the weights 0.84375, 0.0703125, 0.15625, -0.0234375 give
    1.40625 (the key interval, td = 2, would give 1.6875).  Every term is exact in binary."""
    k = lambda x: [x, x, x]  # noqa: E731
    t = tables_of([node()], [(0, S.ANIMATION_PATH_TRANSLATION, S.ANIMATION_CUBICSPLINE, [0.0, 2.0],
                              [k(0), k(1), k(4), k(8), k(3), k(0)])])
    assert np.array_equal(R.evaluate_trs(t, 0.5)[0, :3], np.float32(k(1.40625)))


def test_binary_search_returns_the_frame_of_the_linear_scan():
    rng = np.random.default_rng(2024)
    for keys in (2, 3, 7, 64):
        times = np.sort(rng.uniform(0.0, 4.0, keys).astype(np.float32))
        if keys > 3:
            times[keys // 2] = times[keys // 2 - 1]      # repeated key times
            times[-1] = times[-2] = times[-3]
        queries = np.concatenate([rng.uniform(float(times[0]), float(times[-1]), 2500 - keys).astype(np.float32), times])
        for q in queries:
            if q < times[0]:
                continue
            assert R.first_frame_binary(times, q) == R.first_frame_linear(times, q), (keys, q)
            a = R.key_frame(times, times[0], times[-1], q, search=R.first_frame_linear)
            b = R.key_frame(times, times[0], times[-1], q, search=R.first_frame_binary)
            assert a[2] == b[2] and (a[0] == b[0] or (np.isnan(a[0]) and np.isnan(b[0])))


def test_the_last_channel_on_a_target_wins(fixture_tables):
    t = fixture_tables
    bob = t.gltf_nodes.index(8)
    on_bob = [c for c in t.channels if c.node == bob and c.path == S.ANIMATION_PATH_TRANSLATION]
    assert len(on_bob) == 2 and R.resolve_targets(t)[(bob, S.ANIMATION_PATH_TRANSLATION)] is on_bob[1]
    lamp = t.gltf_nodes.index(6)
    assert (lamp, S.ANIMATION_PATH_TRANSLATION) in R.resolve_targets(t)  # (the same glTF sampler as bob's winning channel)
    for time_s in (0.0, 0.75, 1.7, 3.0):
        trs = R.evaluate_trs(t, time_s)
        assert np.array_equal(trs[bob, :3], trs[lamp, :3]) and np.all(np.abs(trs[bob, :3]) < 4.0)


def test_dynamic_flags_reach_the_descendants(fixture_tables):
    t = fixture_tables
    names = ["carousel", "arm", "wrist", "blade", "floor", "rig", "lamp", "spot", "bob", "sun", "camera", "mast"]
    dynamic = {names[t.gltf_nodes[i]] for i, d in enumerate(R.dynamic_nodes(t)) if d}
    assert dynamic == set(names) - {"floor"}  # arm, blade, camera and mast through their ancestors only
    targeted = {names[t.gltf_nodes[n]] for (n, _) in R.resolve_targets(t)}
    assert targeted == {"carousel", "wrist", "rig", "lamp", "spot", "bob", "sun"}


def test_a_targeted_component_exists_and_starts_at_the_identity(fixture_tables):
    t = fixture_tables
    wrist = t.gltf_nodes.index(2)
    assert not t.nodes[wrist].flags & S.NODE_HAS_ROTATION  # inside the 1e-3 threshold: dropped as a static component
    flags, trs = R.static_pose(t)
    assert flags[wrist] & S.NODE_HAS_ROTATION and np.array_equal(trs[wrist, 3:7], np.float32([0, 0, 0, 1]))
    assert flags[wrist] & S.NODE_HAS_SCALE and np.array_equal(trs[wrist, 7:10], np.float32([1, 1, 1]))


# ---- the parser against load_gltf ----

def _chain_depth(t, i):
    d = 1
    while t.nodes[i].parent != NONE:
        i, d = t.nodes[i].parent, d + 1
    return d


def _abs_chain(t, flags, trs, i):
    """Product of the absolute values of the chain's factors: what a rounding error of a factor is multiplied by."""
    chain = []
    while i != NONE:
        chain.insert(0, i)
        i = t.nodes[i].parent
    m = np.eye(4)
    for n in chain:
        if flags[n] & S.NODE_HAS_TRANSLATION:
            m = np.abs(m) @ np.abs(R.translate(np.eye(4), trs[n, 0:3].astype(np.float64)).T)
        if flags[n] & S.NODE_HAS_ROTATION:
            # (an entry's roundings are relative to its terms, 1 and 2 (yy + zz) or 2 xy and 2 wz, not to their difference)
            x, y, z, w = np.abs(trs[n, 3:7].astype(np.float64))
            m = np.abs(m) @ np.array([[1 + 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z + w * y), 0],
                                      [2 * (x * y + w * z), 1 + 2 * (x * x + z * z), 2 * (y * z + w * x), 0],
                                      [2 * (x * z + w * y), 2 * (y * z + w * x), 1 + 2 * (x * x + y * y), 0],
                                      [0, 0, 0, 1]])
        if flags[n] & S.NODE_HAS_SCALE:
            m = np.abs(m) @ np.diag(list(np.abs(trs[n, 7:10].astype(np.float64))) + [1.0])
    return m  # row-major


@pytest.mark.parametrize("path", [TINY, FIXTURE], ids=["tiny", "animated"])
def test_parser_binds_what_load_gltf_assigned(path):
    world = gltf.load_gltf(path)
    t = animation.load_animations(path)
    doc = gltf._Document(path).doc
    bound = sorted(n.modelInstance for n in t.nodes if n.modelInstance != NONE)
    assert bound == list(range(len(world.model_instances)))
    assert sorted(n.pointLight for n in t.nodes if n.pointLight != NONE) == list(range(world.point_lights.count))
    assert sorted(n.spotLight for n in t.nodes if n.spotLight != NONE) == list(range(world.spot_lights.count))
    assert sum(1 for n in t.nodes if n.flags & S.NODE_CAMERA) == 1 and sum(1 for n in t.nodes if n.flags & S.NODE_DIRECTIONAL_LIGHT) == 1
    assert all(n.parent == NONE or n.parent < i for i, n in enumerate(t.nodes))
    for i, n in enumerate(t.nodes):
        if n.modelInstance != NONE:
            assert world.model_instances[n.modelInstance][0] == doc["nodes"][t.gltf_nodes[i]]["mesh"]

    # The static pose through the restatement of kernel B against the table load_gltf made.  Both are float32 chains over
    # the same float32 components in different operation orders.  A factor's entries carry at most 4 roundings
    # (mat4_cast: product, sum, doubling, 1 -), a product of two 4 x 4 matrices at most 4 more per entry (three sums and
    # the product), a chain of depth d has at most 3 d factors, and an error made at one factor is multiplied by the
    # absolute values of the others: |difference| <= 2 sides * 3 d * 8 u * (product of the |factors|), u = 2^-24.
    flags, trs = R.static_pose(t)
    world_matrices = R.hierarchy(t, trs)
    f = world.freeze()
    table = np.frombuffer(f["transforms"], np.float32).reshape(-1, 2, 3, 4)[:len(world.model_instances)]
    d, p, s = world.directional, world.point_lights, world.spot_lights
    got = R.outputs(t, world_matrices, table, np.frombuffer(d, np.float32)[4:8],
                    np.frombuffer(p, np.float32, 4 * 1024 * 2).reshape(-1, 2, 4)[:, 1],
                    np.frombuffer(s, np.float32, 4 * 1024 * 3).reshape(-1, 3, 4)[:, 1:3])
    for i, n in enumerate(t.nodes):
        depth = _chain_depth(t, i)
        magnitude = _abs_chain(t, flags, trs, i)
        eps = 2 * 3 * depth * 8 * U
        if n.modelInstance != NONE:
            m_bound = eps * magnitude[:3]
            assert np.all(np.abs(got[0][n.modelInstance, 0].astype(np.float64) - table[n.modelInstance, 0]) <= m_bound + 1e-30), i
            # the inverse: first order |d(inv)| <= |inv| |dM| |inv|, plus the float32 cofactor evaluation itself - 3-factor
            # products summed in fours and one division, 12 roundings against the same magnitude
            m64 = world_matrices[i].astype(np.float64).T
            inv = np.abs(np.linalg.inv(m64))
            n_bound = (inv @ (eps * magnitude + 12 * U * np.abs(m64)) @ inv).T[:3]
            assert np.all(np.abs(got[0][n.modelInstance, 1].astype(np.float64) - table[n.modelInstance, 1]) <= n_bound + 1e-30), i
        if n.pointLight != NONE:
            want = np.frombuffer(p, np.float32, 4 * 1024 * 2).reshape(-1, 2, 4)[n.pointLight, 1]
            assert np.all(np.abs(got[2][n.pointLight].astype(np.float64) - want) <= eps * magnitude[:, 3] + 1e-30)
        if n.spotLight != NONE:
            want = np.frombuffer(s, np.float32, 4 * 1024 * 3).reshape(-1, 3, 4)[n.spotLight, 1:3]
            assert np.all(np.abs(got[3][n.spotLight, 0, :3].astype(np.float64) - want[0, :3]) <= eps * magnitude[:3, 3] + 1e-30)
            assert np.all(np.abs(got[3][n.spotLight, 1, :3].astype(np.float64) - want[1, :3]) <= eps * magnitude[:3, 2] + 1e-30)
        if n.flags & S.NODE_DIRECTIONAL_LIGHT:
            want = np.frombuffer(d, np.float32)[4:7]
            assert np.all(np.abs(got[1][:3].astype(np.float64) - want) <= eps * magnitude[:3, 2] + 1e-30)
        if n.flags & S.NODE_CAMERA:
            assert np.all(np.abs(got[4][:3].astype(np.float64) - np.float32(world.camera["eye"])) <= eps * magnitude[:3, 3] + 4 * U)


def test_a_scene_without_animations_has_no_channels():
    t = animation.load_animations(TINY)
    assert len(t.channels) == 0 and t.times.size == 0 and t.values.size == 0 and t.end_time == 0.0
    assert len(t.nodes) == 8 and not any(R.dynamic_nodes(t))


def test_the_fixture_holds_what_it_was_designed_to_hold(fixture_tables):
    t = fixture_tables
    assert len(t.nodes) == 12 and t.end_time == 2.5
    kinds = {(c.path, c.interpolation) for c in R.resolve_targets(t).values()}
    assert kinds == {(p, i) for p in range(3) for i in range(3)}  # Step / Linear / CubicSpline on each of T, R, S
    assert any(c.keyCount == 1 for c in t.channels)
    assert any(R.channel_times(t, c)[0] == 0.5 for c in t.channels)
    assert any(np.any(np.diff(R.channel_times(t, c)) == 0) for c in t.channels)
    blade = t.gltf_nodes.index(3)
    assert _chain_depth(t, blade) == 4 and t.nodes[blade].modelInstance != NONE
    dyn = R.dynamic_nodes(t)
    assert all(dyn[i] for i, n in enumerate(t.nodes)
               if n.pointLight != NONE or n.spotLight != NONE or n.flags & (S.NODE_DIRECTIONAL_LIGHT | S.NODE_CAMERA))
    assert sum(1 for i, n in enumerate(t.nodes) if n.modelInstance != NONE and not dyn[i]) == 1
    assert os.path.getsize(FIXTURE) < 32 * 1024


# ---- slerp ----

def test_slerp_error_and_the_conditions_of_the_case_list(fixture_tables):
    """E_ref, the float32 restatement's distance from the float64 one over every slerp sample of the GPU test, is what
    that test's tolerance rests on (4 * max(E_ref, 2^-22)); DESIGN.md (f15) quotes it.  The key pairs keep the branch away
    from a transcendental: one pair with a negative dot, one of two identical quaternions (the mix branch), the rest at
    least 0.1 rad apart with a dot at least 1e-3 below 1 - FLT_EPSILON."""
    t = fixture_tables
    times = R.sample_times(t)
    assert len(times) >= 64 + 20 and times[0] < 0.0 and times[-1] > t.end_time and t.end_time in times
    samples = R.slerp_samples(t, times)
    assert {b for *_, b in samples} == {"mix", "slerp"} and len(samples) >= 50
    e_ref = R.slerp_error(t, times)
    assert 0.0 < e_ref < 2.0 ** -20
    print("E_ref = %.3e" % e_ref)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert ("E_ref = %.3e" % e_ref) in design[design.index("## (f15)"):]

    negative = identical = 0
    for ch in R.resolve_targets(t).values():
        if ch.path != S.ANIMATION_PATH_ROTATION or ch.interpolation != S.ANIMATION_LINEAR:
            continue
        v = R.channel_values(t, ch)
        for x, y in zip(v[:-1], v[1:]):
            dot = R.quat_dot(x, y)
            negative += dot < 0
            if np.array_equal(x, y):
                identical += 1
                assert dot > np.float32(1.0) - R.FLT_EPSILON
            else:
                assert abs(dot) <= float(np.float32(1.0) - R.FLT_EPSILON) - 1e-3
                assert 2.0 * math.acos(min(1.0, abs(float(dot)))) >= 0.1
    assert negative >= 1 and identical == 1


# ---- exports ----

def test_the_animation_symbols_are_exported():
    lib = capi.lib()
    for name in ("prosper_pt_set_animations", "prosper_pt_animate", "prosper_pt_get_animation_state",
                 "prosper_pt_read_animated_transforms", "prosper_pt_read_lights", "prosper_pt_debug_read_animation_nodes",
                 "prosper_host_animations_create", "prosper_host_animations_destroy", "prosper_host_animations_update",
                 "prosper_host_animations_end_time"):
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()
    body = header[header.index("typedef struct prosper_pt_animation_channel"):header.index("} prosper_pt_animation_channel;")]
    assert re.findall(r"\b(?:uint32_t|float)\s+([A-Za-z]+);", body) == [n for n, _ in S.AnimationChannel._fields_]
    body = header[header.index("typedef struct prosper_pt_animation_node"):header.index("} prosper_pt_animation_node;")]
    assert re.findall(r"\b(?:uint32_t|float)\s+([A-Za-z]+)(?:\[\d\])?;", body) == [n for n, _ in S.AnimationNode._fields_]
    # refused without touching a device
    assert lib.prosper_pt_set_animations(None, None) == -1
    assert lib.prosper_pt_animate(None, 0.0, 2, None) == -1 and b"unknown flag" in lib.prosper_pt_last_error()
