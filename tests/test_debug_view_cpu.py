"""The debug lines without a GPU: the entry points exist and refuse bad arguments before they touch the
device, tests/debug_view_reference.py gives the answers worked by hand for the line rule on a 16 x 12 image, and
prosper_amd/debug_geometry.py restates App::updateDebugLines and the click-to-focus distance."""
import ctypes as C
import math

import numpy as np
import pytest

import debug_view_reference as R
from prosper_amd import capi, debug_geometry as G, structs as S

F = np.float32
W, H = 16, 12
FOV = math.radians(59.0)
ZN, ZF = 0.1, 100.0
FOCAL = (H / 2) / math.tan(FOV / 2)  # pixels per unit of x / distance


def camera(oracle, w=W, h=H):
    return oracle.camera_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), FOV, ZN, ZF, w, h)[0]


def at(px, py, d):
    """the world position that projects to framebuffer coordinates (px, py) at distance d"""
    return np.array([(px - W / 2) * d / FOCAL, -(py - H / 2) * d / FOCAL, -d])


def line(p0, p1, colour=(1.0, 0.0, 0.0)):
    return np.concatenate([p0, p1, colour]).astype(F)


def pixels(x, y):
    return list(zip(x.tolist(), y.tolist()))


def seg(a, b, za=0.5, zb=0.5):
    return (F(a[0]), F(a[1]), F(za)), (F(b[0]), F(b[1]), F(zb))


# ---- the C interface ----

def test_the_symbols_exist_and_bad_arguments_are_rejected_before_touching_the_gpu(oracle):
    lib = capi.lib()
    for name in ("prosper_pt_debug_lines", "prosper_pt_get_debug_lines_info", "prosper_host_debug_lines_create",
                 "prosper_host_debug_lines_destroy", "prosper_host_debug_lines_reset", "prosper_host_debug_lines_add_line",
                 "prosper_host_debug_lines_count", "prosper_host_debug_lines_data", "prosper_host_debug_renderer_create",
                 "prosper_host_debug_renderer_destroy", "prosper_host_debug_renderer_record"):
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    cam = camera(oracle)
    lines = np.zeros((2, 9), F)

    def call(ptr, count, cam_ref, w, h):
        return lib.prosper_pt_debug_lines(None, ptr, count, cam_ref, w, h, None)

    assert call(lines.ctypes.data, S.MAX_DEBUG_LINE_COUNT + 1, C.byref(cam), W, H) == -1
    assert b"100 000" in lib.prosper_pt_last_error()
    assert call(None, 2, C.byref(cam), W, H) == -1
    assert call(lines.ctypes.data, 2, None, W, H) == -1
    assert call(lines.ctypes.data, 2, C.byref(cam), 0, H) == -1
    assert b"empty extent" in lib.prosper_pt_last_error()
    assert call(lines.ctypes.data, 2, C.byref(cam), 32769, H) == -1
    assert b"32768" in lib.prosper_pt_last_error()
    assert call(lines.ctypes.data, 2, C.byref(cam), W, H) == -1  # everything else is fine: the null context
    assert b"null argument" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_get_debug_lines_info(None, None) == -1
    h = C.c_void_p()
    assert lib.prosper_host_debug_renderer_create(None, C.byref(h)) == -1
    assert lib.prosper_host_debug_renderer_record(None, None, None, W, H, None) == -1


def test_the_info_struct_mirrors_the_header():
    assert C.sizeof(S.DebugLinesInfo) == 20
    assert [f[0] for f in S.DebugLinesInfo._fields_] == ["valid", "lineCount", "fragmentsWritten", "linesClippedAway", "ms"]


def test_the_cpp_debug_lines_keep_what_was_added_and_refuse_the_line_past_the_maximum():
    lib = capi.lib()
    h = C.c_void_p()
    assert lib.prosper_host_debug_lines_create(C.byref(h)) == 0
    try:
        assert lib.prosper_host_debug_lines_count(h) == 0 and lib.prosper_host_debug_lines_data(h) is None
        add = lib.prosper_host_debug_lines_add_line
        p = np.arange(9, dtype=F)
        a, b, c = (C.c_void_p(p[k:].ctypes.data) for k in (0, 3, 6))
        assert add(h, a, b, None) == -1 and lib.prosper_host_debug_lines_count(h) == 0
        for _ in range(S.MAX_DEBUG_LINE_COUNT):
            assert add(h, a, b, c) == 0
        assert lib.prosper_host_debug_lines_count(h) == S.MAX_DEBUG_LINE_COUNT == 100000
        assert add(h, a, b, c) == -1  # full: dropped, where the reference would write past its buffer
        assert lib.prosper_host_debug_lines_count(h) == S.MAX_DEBUG_LINE_COUNT
        data = np.ctypeslib.as_array(C.cast(lib.prosper_host_debug_lines_data(h), C.POINTER(C.c_float)),
                                     (S.MAX_DEBUG_LINE_COUNT, 9))
        assert (data[0] == p).all() and (data[-1] == p).all()
        lib.prosper_host_debug_lines_reset(h)
        assert lib.prosper_host_debug_lines_count(h) == 0
        assert add(h, b, a, c) == 0 and lib.prosper_host_debug_lines_count(h) == 1
        data = np.ctypeslib.as_array(C.cast(lib.prosper_host_debug_lines_data(h), C.POINTER(C.c_float)), (1, 9))
        assert data[0].tolist() == [3, 4, 5, 0, 1, 2, 6, 7, 8]
    finally:
        lib.prosper_host_debug_lines_destroy(h)


# ---- the line rule, on screen segments (answers by hand) ----

def test_a_horizontal_line_between_pixel_centres_is_half_open_from_start_to_end():
    x, y, d = R.walk(*seg((2.5, 5.5), (9.5, 5.5)), W, H)
    assert pixels(x, y) == [(k, 5) for k in range(2, 9)]  # the centre 9.5 is the end: left out
    x, y, d = R.walk(*seg((9.5, 5.5), (2.5, 5.5)), W, H)
    assert pixels(x, y) == [(k, 5) for k in range(9, 2, -1)]  # now 2.5 is the end
    assert (d == F(0.5)).all()


def test_a_vertical_line_walks_rows():
    x, y, _ = R.walk(*seg((4.5, 1.5), (4.5, 7.5)), W, H)
    assert pixels(x, y) == [(4, k) for k in range(1, 7)]
    x, y, _ = R.walk(*seg((4.5, 7.5), (4.5, 1.5)), W, H)
    assert pixels(x, y) == [(4, k) for k in range(7, 1, -1)]


def test_a_diagonal_is_x_major_and_steps_both_coordinates():
    x, y, _ = R.walk(*seg((1.5, 1.5), (6.5, 6.5)), W, H)
    assert pixels(x, y) == [(k, k) for k in range(1, 6)]
    x, y, _ = R.walk(*seg((6.5, 6.5), (1.5, 1.5)), W, H)
    assert pixels(x, y) == [(k, k) for k in range(6, 1, -1)]


def test_a_steep_line_is_y_major_with_one_fragment_per_row():
    x, y, _ = R.walk(*seg((3.5, 0.5), (5.5, 8.5)), W, H)
    assert pixels(x, y) == [(3, 0), (3, 1), (4, 2), (4, 3), (4, 4), (4, 5), (5, 6), (5, 7)]
    x, y, _ = R.walk(*seg((5.5, 8.5), (3.5, 0.5)), W, H)
    assert pixels(x, y) == [(5, 8), (5, 7), (5, 6), (4, 5), (4, 4), (4, 3), (4, 2), (3, 1)]


def test_a_shallow_line_is_x_major_with_one_fragment_per_column_and_interpolates_depth_linearly():
    x, y, d = R.walk(*seg((0.5, 2.5), (8.5, 4.5), 0.25, 0.75), W, H)
    assert pixels(x, y) == [(0, 2), (1, 2), (2, 3), (3, 3), (4, 3), (5, 3), (6, 4), (7, 4)]
    assert d.tolist() == [0.25 + 0.5 * k / 8 for k in range(8)]  # exact in float32
    x, y, d = R.walk(*seg((8.5, 4.5), (0.5, 2.5), 0.75, 0.25), W, H)
    assert pixels(x, y) == [(8, 4), (7, 4), (6, 4), (5, 3), (4, 3), (3, 3), (2, 3), (1, 2)]
    assert d.tolist() == [0.75 - 0.5 * k / 8 for k in range(8)]


def test_a_zero_length_line_writes_nothing():
    for p in ((4.5, 4.5), (4.2, 7.9), (0.0, 0.0), (16.0, 12.0)):
        x, y, d = R.walk(*seg(p, p, 0.2, 0.9), W, H)  # also: seen end-on, two depths at one point
        assert len(x) == len(y) == len(d) == 0


def test_a_line_shorter_than_a_pixel_writes_one_fragment_or_none():
    x, y, _ = R.walk(*seg((4.3, 4.2), (4.7, 4.4)), W, H)  # crosses the centre 4.5
    assert pixels(x, y) == [(4, 4)]
    x, y, _ = R.walk(*seg((4.6, 4.2), (4.9, 4.4)), W, H)  # crosses none
    assert pixels(x, y) == []


def test_a_polyline_writes_no_pixel_twice_and_leaves_no_gap_at_the_joint():
    a, b, c = (1.2, 3.3), (6.5, 5.1), (13.9, 4.2)  # the joint lies exactly on a centre: it belongs to the second segment
    x0, y0, _ = R.walk(*seg(a, b), W, H)
    x1, y1, _ = R.walk(*seg(b, c), W, H)
    assert x0.tolist() == [1, 2, 3, 4, 5] and x1.tolist() == list(range(6, 14))
    both = pixels(x0, y0) + pixels(x1, y1)
    assert len(set(both)) == len(both)
    # and walked the other way round the joint belongs to the first
    x1, y1, _ = R.walk(*seg(c, b), W, H)
    x0, y0, _ = R.walk(*seg(b, a), W, H)
    assert x1.tolist() == list(range(13, 6, -1)) and x0.tolist() == [6, 5, 4, 3, 2, 1]
    # a joint off the centres: the same columns, each once
    b = (6.8, 5.1)
    xs = R.walk(*seg(a, b), W, H)[0].tolist() + R.walk(*seg(b, c), W, H)[0].tolist()
    assert xs == list(range(1, 14))


def test_the_walk_stays_in_the_image_up_to_the_viewport_edges():
    x, y, _ = R.walk(*seg((10.0, 2.5), (16.0, 2.5)), W, H)
    assert pixels(x, y) == [(k, 2) for k in range(10, 16)]
    x, y, _ = R.walk(*seg((16.0, 12.0), (0.0, 0.0)), W, H)  # corner to corner; the minor coordinate 12.0 clamps to row 11
    assert x.tolist() == list(range(15, -1, -1)) and y.max() == 11 and y.min() == 0
    x, y, _ = R.walk(*seg((3.0, 12.0), (3.0, 0.0)), W, H)
    assert pixels(x, y) == [(3, k) for k in range(11, -1, -1)]


# ---- projection and clipping ----

def test_the_projection_puts_a_point_where_it_was_aimed(oracle):
    cam = camera(oracle)
    a, b = R.screen_segment(line(at(3.25, 4.5, 1.0), at(12.75, 9.0, 2.0)), R.mat4(cam.worldToCamera), R.mat4(cam.cameraToClip), W, H)
    assert np.allclose(a[:2], (3.25, 4.5), atol=1e-4) and np.allclose(b[:2], (12.75, 9.0), atol=1e-4)
    assert 0.0 < b[2] < a[2] < 1.0  # reverse Z: nearer is greater
    c2c = R.mat4(cam.cameraToClip).astype(np.float64)
    assert abs(a[2] - (c2c[2, 2] * -1.0 + c2c[2, 3]) / 1.0) < 1e-6


def test_a_line_through_the_near_plane_is_cut_there(oracle):
    cam = camera(oracle)
    behind = np.array([0.3, 0.0, 1.0])  # behind the eye
    for l in (line(at(4.0, 6.0, 1.0), behind), line(behind, at(4.0, 6.0, 1.0))):
        a, b = R.screen_segment(l, R.mat4(cam.worldToCamera), R.mat4(cam.cameraToClip), W, H)
        cut = b if (l[3:6] == behind.astype(F)).all() else a
        assert abs(float(cut[2]) - 1.0) < 1e-5  # on the near plane (z / w of a point with z = w up to rounding)
        x, y, d = R.line_fragments(l, cam, W, H)
        assert 0 < len(x) <= W and x.min() >= 0 and x.max() < W and y.min() >= 0 and y.max() < H
        assert (d <= F(1.0)).all() and (d > F(0.0)).all()


def test_a_line_behind_the_eye_or_with_a_non_finite_endpoint_is_clipped_away(oracle):
    cam = camera(oracle)
    good = at(8.0, 6.0, 1.0)
    gone = [line(np.array([0.3, 0.0, 1.0]), np.array([-0.2, 0.1, 2.0])),  # both ends behind the eye
            line(at(-9.0, 6.0, 1.0), at(-3.0, 2.0, 2.0)),                 # both left of the viewport
            line(at(4.0, 6.0, 0.01), at(9.0, 6.0, 0.05)),                 # both before the near plane
            line(at(4.0, 6.0, 200.0), at(9.0, 6.0, 300.0)),               # both beyond the far plane
            line(np.array([1e30, 0.0, -1.0]), np.array([1e30, 1.0, -1.0]))]
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            l = line(good, at(3.0, 3.0, 1.0))
            l[k] = bad
            gone.append(l)
    for l in gone:
        assert R.line_fragments(l, cam, W, H) is None, l
    hdr, depth = np.zeros((H, W, 4), F), np.zeros((H, W), F)
    out_hdr, out_depth, info = R.debug_lines(np.stack(gone), cam, W, H, hdr, depth)
    assert info["linesClippedAway"] == len(gone) and info["fragmentsWritten"] == 0
    assert (out_hdr == hdr).all() and (out_depth == depth).all()


def test_a_far_away_endpoint_is_walked_in_bounded_steps(oracle):
    cam = camera(oracle)
    for far in (np.array([1e30, 0.0, -1.0]), np.array([1e30, 1e30, -1e30]), np.array([0.0, -3e38, -1.0])):
        frags = R.line_fragments(line(at(8.0, 6.0, 1.0), far), cam, W, H)
        if frags is not None:
            assert len(frags[0]) <= max(W, H)


def test_a_segment_leaves_through_each_viewport_edge_and_ends_on_it(oracle):
    cam = camera(oracle)
    centre = at(8.0, 6.0, 1.0)
    cases = {"left": (at(-20.0, 6.0, 1.0), [(k, 6) for k in range(7, -1, -1)]),
             "right": (at(40.0, 6.0, 1.0), [(k, 6) for k in range(8, 16)]),
             "top": (at(8.0, -20.0, 1.0), [(8, k) for k in range(5, -1, -1)]),
             "bottom": (at(8.0, 40.0, 1.0), [(8, k) for k in range(6, 12)])}
    for name, (far, want) in cases.items():
        a, b = R.screen_segment(line(centre, far), R.mat4(cam.worldToCamera), R.mat4(cam.cameraToClip), W, H)
        edge = {"left": (b[0], 0.0), "right": (b[0], W), "top": (b[1], 0.0), "bottom": (b[1], H)}[name]
        assert abs(edge[0] - edge[1]) < 1e-3, name
        x, y, _ = R.line_fragments(line(centre, far), cam, W, H)
        assert pixels(x, y) == want, name
        # from outside in: the same pixels but the half-open end moves to the centre's side
        x, y, _ = R.line_fragments(line(far, centre), cam, W, H)
        assert sorted(pixels(x, y)) == sorted(want), name


def test_depth_test_nearest_wins_and_equal_depth_goes_to_the_higher_index(oracle):
    cam = camera(oracle)
    hdr = np.full((H, W, 4), 0.25, F)
    depth = np.zeros((H, W), F)
    near, far = 1.0, 2.0
    red, green, blue = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    lines = np.stack([line(at(2.0, 6.5, near), at(14.0, 6.5, near), red),      # 0: horizontal, near
                      line(at(8.5, 1.0, far), at(8.5, 11.0, far), green),      # 1: vertical, far: loses at the crossing
                      line(at(2.0, 3.5, near), at(14.0, 3.5, near), green),    # 2 and 3: the same line twice
                      line(at(2.0, 3.5, near), at(14.0, 3.5, near), blue)])
    out_hdr, out_depth, info = R.debug_lines(lines, cam, W, H, hdr, depth)
    assert info["winner"][6, 8] == 0 and (out_hdr[6, 8] == (1, 0, 0, 1)).all()
    assert info["winner"][5, 8] == 1 and info["winner"][7, 8] == 1
    assert (info["winner"][3, 2:14] == 3).all()  # the higher index
    assert info["fragmentsWritten"] == (info["winner"] >= 0).sum() == 12 + 12 + 10 - 2  # the verticals at rows 3 and 6 lose
    # a stored depth in front of everything: nothing passes; equal to the line's: equal loses
    d_near = out_depth[6, 8]
    for stored in (F(1.0), d_near):
        depth2 = np.full((H, W), stored, F)
        assert R.debug_lines(lines[:1], cam, W, H, hdr, depth2)[2]["fragmentsWritten"] == 0
    assert R.debug_lines(lines[:1], cam, W, H, hdr, np.full((H, W), np.nextafter(d_near, F(0.0)), F))[2]["fragmentsWritten"] == 12
    # order independence once the indices are accounted for
    perm = [3, 1, 0, 2]
    hdr_p, depth_p, info_p = R.debug_lines(lines[perm], cam, W, H, hdr, depth)
    assert (depth_p == out_depth).all() and info_p["fragmentsWritten"] == info["fragmentsWritten"]
    differs = (hdr_p != out_hdr).any(2)
    assert differs[3, 2:14].all() and differs.sum() == 12  # only the tie changes hands: index 3 is now the green copy


# ---- debug_geometry.py ----

def test_debug_lines_holds_lines_in_order_and_overflows_at_the_maximum():
    lines = G.DebugLines()
    assert lines.count == 0 and lines.array().shape == (0, 9) and G.DebugLines.sMaxLineCount == 100000
    lines.addLine((1, 2, 3), (4, 5, 6), (7, 8, 9))
    lines.addLine((0, 0, 0), (1, 1, 1), (0.5, 0.5, 0.5))
    assert lines.count == 2 and lines.array().dtype == F
    assert lines.array().tolist() == [[1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 0, 0, 1, 1, 1, 0.5, 0.5, 0.5]]
    lines.reset()
    assert lines.count == 0
    lines._lines = [np.zeros(9, F)] * G.DebugLines.sMaxLineCount
    with pytest.raises(OverflowError):
        lines.addLine((0, 0, 0), (1, 1, 1), (1, 1, 1))


def test_light_axes_against_literal_arrays():
    r, g, b = [1.0, 0.05, 0.05], [0.05, 1.0, 0.05], [0.05, 0.05, 1.0]
    got = G.light_axes([(1.0, 2.0, 3.0, 1.0)], [((0.0, 1.0, 0.0), (0.0, 0.0, -1.0)), ((2.0, 0.0, 0.0), (0.0, 1.0, 0.0))])
    want = np.array([
        [1, 2, 3, 1.2, 2, 3] + r, [1, 2, 3, 1, 2.2, 3] + g, [1, 2, 3, 1, 2, 3.2] + b,
        # looking down -z: right = +x, up = +y
        [0, 1, 0, 0.2, 1, 0] + r, [0, 1, 0, 0, 1.2, 0] + g, [0, 1, 0, 0, 1, -0.2] + b,
        # looking up (|1 - direction.y| < 0.1): right = cross(fwd, (0, 0, -1)) = -x, up = cross(right, fwd) = -z
        [2, 0, 0, 1.8, 0, 0] + r, [2, 0, 0, 2, 0, -0.2] + g, [2, 0, 0, 2, 0.2, 0] + b], np.float64)
    assert got.dtype == F and got.shape == (9, 9)
    assert np.abs(got - want).max() < 1e-6  # the sums are float32
    assert G.light_axes([], []).shape == (0, 9)
    # the records of the scene's light buffers
    points, spots = S.PointLightsBuffer(), S.SpotLightsBuffer()
    points.count, spots.count = 1, 1
    points.lights[0].position = S.Vec4(1.0, 2.0, 3.0, 1.0)
    spots.lights[0].positionAndAngleOffset = S.Vec4(0.0, 1.0, 0.0, 0.3)
    spots.lights[0].direction = S.Vec4(0.0, 0.0, -1.0, 0.0)
    assert (G.light_axes_from_buffers(points, spots) == got[:6]).all()


def test_frustum_lines_against_a_literal_array():
    names = G.FRUSTUM_CORNER_NAMES
    corners = {name: (float(k), float(10 + k), float(20 + k)) for k, name in enumerate(names)}
    got = G.frustum_lines(corners, (1.0, 1.0, 0.0))
    order = [(0, 2), (0, 1), (3, 2), (3, 1), (4, 6), (4, 5), (7, 6), (7, 5), (0, 4), (1, 5), (2, 6), (3, 7)]
    want = [[a, 10 + a, 20 + a, b, 10 + b, 20 + b, 1, 1, 0] for a, b in order]
    assert got.dtype == F and got.tolist() == want


def test_frustum_corners_lie_on_the_near_and_far_planes(oracle):
    cam = camera(oracle)
    c = G.frustum_corners(cam)
    for name, p in c.items():
        assert abs(-p[2] - (ZN if name.endswith("Near") else ZF)) < 1e-3 * (ZN if name.endswith("Near") else ZF), name
        assert (p[0] < 0) == ("Left" in name) and (p[1] < 0) == name.startswith("bottom"), name


@pytest.mark.parametrize("distance", (2.0, 7.5))
def test_focus_distance_of_a_plane_perpendicular_to_the_view_axis_is_its_distance_at_every_pixel(oracle, distance):
    cam = camera(oracle)
    c2c = R.mat4(cam.cameraToClip).astype(np.float64)
    for py in range(H):
        for px in range(W):
            p = np.append(at(px + 0.5, py + 0.5, distance), 1.0)  # the plane's point under the pixel centre (camera = world)
            clip = c2c @ p
            depth = clip[2] / clip[3]
            d64 = G.focus_distance_from_depth(cam, (px, py), (W, H), depth, dtype=np.float64)
            assert abs(d64 - distance) <= 1e-9 * distance, (px, py)
            d32 = G.focus_distance_from_depth(cam, (px, py), (W, H), F(depth))
            assert d32.dtype == F and abs(float(d32) - distance) <= 1e-5 * distance, (px, py)


# ---- the registry and the one-texel readback ----

def test_the_registry_and_readback_symbols_exist_and_refuse_without_a_context():
    lib = capi.lib()
    for name in ("prosper_pt_debug_resource_count", "prosper_pt_get_debug_resource", "prosper_pt_texture_readback",
                 "prosper_pt_try_texture_readback", "prosper_host_texture_readback_create", "prosper_host_texture_readback_destroy",
                 "prosper_host_texture_readback_start_frame", "prosper_host_texture_readback_record",
                 "prosper_host_texture_readback_readback", "prosper_host_texture_readback_frames_until_ready"):
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4 and S.NOT_READY == -7
    assert lib.prosper_pt_debug_resource_count(None) == 0
    assert lib.prosper_pt_get_debug_resource(None, 0, C.byref(S.DebugResource())) == -1
    assert lib.prosper_pt_texture_readback(None, 0, float("nan"), 0.0, None) == -1
    assert b"non-finite" in lib.prosper_pt_last_error()
    assert lib.prosper_pt_texture_readback(None, 0, 1.0, 1.0, None) == -1
    assert lib.prosper_pt_try_texture_readback(None, None) == -1
    h = C.c_void_p()
    assert lib.prosper_host_texture_readback_create(None, C.byref(h)) == -1
    assert lib.prosper_host_texture_readback_frames_until_ready(None) == -1
    assert C.sizeof(S.DebugResource) == 64 + 5 * 4


def test_the_readback_restatement_by_hand():
    # uv = px / extent, then clamp(floor(u * extent), 0, extent - 1)
    assert [R.nearest_texel(px, 5) for px in (-3.0, -0.25, 0.0, 0.99, 1.0, 4.5, 5.0, 7.0, 1e30, -1e30)] == [0, 0, 0, 0, 1, 4, 4, 4, 4, 0]
    r = np.arange(6, dtype=F).reshape(2, 3)  # R32F
    assert R.texture_readback(r, 2.0, 1.0).tolist() == [5.0, 0.0, 0.0, 1.0]
    rg = np.arange(12, dtype=np.float16).reshape(2, 3, 2)  # RG16F
    assert R.texture_readback(rg, 1.5, 0.0).tolist() == [2.0, 3.0, 0.0, 1.0]
    unorm = np.array([[[65535, 0], [13107, 65535]]], np.uint16)  # RG16_UNORM
    assert R.texture_readback(unorm, 1.0, 0.0).tolist() == [float(F(13107) / F(65535)), 1.0, 0.0, 1.0]
    rgba8 = np.array([[[255, 0, 51, 255]]], np.uint8)
    assert R.texture_readback(rgba8, 0.0, 0.0).tolist() == [1.0, 0.0, float(F(51) / F(255)), 1.0]
    assert R.FORMAT_BYTES == (16, 8, 4, 8, 4, 2, 4, 4)


# ---- the C++ TextureReadback's frame counting, against fakes of the library calls below it ----

def test_cpp_texture_readback_counts_frames_as_the_reference_does(tmp_path):
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "the host C++ compiler (g++) is needed"
    exe = str(tmp_path / "texture_readback_main")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", os.path.join(root, "tests", "texture_readback_main.cpp"),
                           os.path.join(root, "prosper_amd", "csrc", "host", "texture_readback.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


# ---- the texture viewer's restatement, by hand ----

def test_in_res_at_lod_for_5x3_down_to_1x1():
    assert [R.in_res((5, 3), lod) for lod in range(5)] == [(5, 3), (2, 1), (1, 1), (1, 1), (1, 1)]


def test_the_aspect_branches():
    # 16x16 into 37x23: in 1 < out 37/23 -> x is scaled by (37/23) / 1 about its centre
    s = F(37) / F(23) / (F(16) / F(16))
    u, v = R.aspect_corrected_uv(F(0.5), F(0.25), (16, 16), (37, 23))
    assert v == F(0.25) and u == F(0.5) * s - (s - F(1)) * F(0.5) and abs(float(u) - 0.5) < 1e-6  # the centre stays
    u, v = R.aspect_corrected_uv(F(0.0), F(0.0), (16, 16), (37, 23))
    assert abs(float(u) - (-(37 / 23 - 1) / 2)) < 1e-6 and v == 0  # the left edge lies in the bar: uv.x < 0, black
    # 8x24 into 37x23: the same branch (1/3 < 37/23), scale (37/23) / (1/3)
    u, v = R.aspect_corrected_uv(F(1.0), F(0.7), (8, 24), (37, 23))
    scale = (37 / 23) / (8 / 24)
    assert v == F(0.7) and abs(float(u) - (scale - (scale - 1) / 2)) < 1e-5
    # the other branch: 24x8 into 37x23 (3 > 37/23): y is scaled by 3 / (37/23)
    u, v = R.aspect_corrected_uv(F(0.3), F(0.0), (24, 8), (37, 23))
    scale = 3 / (37 / 23)
    assert u == F(0.3) and abs(float(v) - (-(scale - 1) / 2)) < 1e-6
    # equal extents: untouched, whatever the aspect
    assert R.aspect_corrected_uv(F(0.3), F(0.9), (37, 23), (37, 23)) == (F(0.3), F(0.9))
    # and undone
    for wh in ((16, 16), (8, 24), (24, 8)):
        u, v = R.aspect_corrected_uv(*R.aspect_corrected_uv(F(0.3), F(0.8), wh, (37, 23)), wh, (37, 23), undo=True)
        assert abs(float(u) - 0.3) < 1e-6 and abs(float(v) - 0.8) < 1e-6


def test_zoom_uv_maps_the_view_onto_the_middle_quarter():
    assert R.zoom4x_uv(F(0.0), F(1.0)) == (F(0.375), F(0.625)) and R.zoom4x_uv(F(0.5), F(0.5)) == (F(0.5), F(0.5))
    assert R.unzoom4x_uv(F(0.375), F(0.625)) == (F(0.0), F(1.0))


def test_the_view_of_a_small_image_by_hand():
    image = np.zeros((2, 4, 4), F)  # 4 x 2, red = column / 4, green = row, blue = -1, alpha = 0.5
    image[..., 0] = np.arange(4)[None, :] / 4.0
    image[..., 1] = np.arange(2)[:, None]
    image[..., 2], image[..., 3] = -1.0, 0.5
    out, peek = R.texture_debug(image, (4, 2))
    assert peek is None and out[..., 0].tolist() == [[0, 64, 128, 191]] * 2  # rint(0.25 * 255) = 64, rint(191.25) = 191
    assert out[..., 1].tolist() == [[0] * 4, [255] * 4] and (out[..., 2] == 0).all() and (out[..., 3] == 255).all()
    assert (R.texture_debug(image, (4, 2), flags=2 | R.ABS_BEFORE_RANGE)[0][..., :3] == 255).all()  # |blue| in all three
    assert (R.texture_debug(image, (4, 2), flags=3)[0][..., :3] == 128).all()  # alpha: rint(127.5) = 128, half to even
    assert (R.texture_debug(image, (4, 2), (1.0, 0.0), flags=1)[0][0, :, :3] == 255).all()  # the range upside down
    flat = R.texture_debug(image, (4, 2), (0.5, 0.5), flags=0)[0][0, :, 0]  # (c - 0.5) / 0: -inf, -inf, NaN, +inf
    assert flat.tolist() == [0, 0, 0, 255]
    # bilinear between the columns' centres: at u = 0.5 of 4 columns, halfway between columns 1 and 2
    s = R.sample_level(R.expand_texels(image), np.array([0.5], F), np.array([0.25], F), True)
    assert s[0].tolist() == [0.375, 0.0, -1.0, 0.5]
    # zoomed, the 4 x 2 output shows uv 0.40625 .. 0.59375: columns 1, 1, 2, 2
    assert R.texture_debug(image, (4, 2), flags=0 | R.ZOOM)[0][0, :, 0].tolist() == [64, 64, 128, 128]
    # into a square the wide image keeps its aspect: black bars above and below (uv.y outside [0, 1])
    out, _ = R.texture_debug(image, (4, 4), flags=3)
    assert (out[0, :, :3] == 0).all() and (out[3, :, :3] == 0).all() and (out[1:3, :, :3] == 128).all()


def test_the_marker_squares_and_the_peek():
    image = np.zeros((8, 8, 4), F)
    image[..., 0] = np.arange(64).reshape(8, 8)
    out, peek = R.texture_debug(image, (16, 16), (0.0, 64.0), R.MAGNIFIER | 0, cursor_uv=(0.3, 0.6))
    # the cursor's texel: floor(0.3 * 8) = 2, floor(0.6 * 8) = 4: value 34; snapped uv (2.5, 4.5) / 8 -> output (5, 9)
    assert peek.tolist() == [34.0, 0.0, 0.0, 0.0]
    assert R.snapped_cursor((0.3, 0.6), (8, 8), (16, 16), False) == (F(2.5) / F(8), F(4.5) / F(8))
    white = (out[..., :3] == 255).all(2)
    ys, xs = np.nonzero(white)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (4, 6, 8, 10)  # |5 - x| < 2, |9 - y| < 2
    ring = (out[..., :3] == 0).all(2)
    assert ring[7, 3] and ring[11, 7] and ring[7, 7] and not ring[6, 5] and not ring[12, 5] and ring[9, 3] and not ring[9, 2]
    # outside [0, 1): +inf in all four, and no marker in the image
    for cursor in ((1.0, 0.5), (0.5, -0.1), (2.0, 2.0)):
        out, peek = R.texture_debug(image, (16, 16), (0.0, 64.0), R.MAGNIFIER, cursor_uv=cursor)
        assert np.isposinf(peek).all() and peek.dtype == F
    assert not np.isposinf(R.texture_debug(image, (16, 16), (0.0, 64.0), R.MAGNIFIER, cursor_uv=(0.999, 0.0))[1]).any()


def test_the_viewer_symbols_exist_and_refuse_without_a_context():
    lib = capi.lib()
    assert hasattr(lib, "prosper_pt_texture_debug") and hasattr(lib, "prosper_pt_get_texture_debug_peek")
    assert C.sizeof(S.TextureDebugPC) == 40 and lib.prosper_pt_abi_version() == 4
    out = np.zeros(16 * 16 * 4, np.uint8)

    def call(pc, bilinear=0, size=out.nbytes, host=out.ctypes.data):
        return lib.prosper_pt_texture_debug(None, 0, pc, bilinear, None, host, size, None)

    def pc(out_res=(16, 16), flags=4):
        return C.byref(S.TextureDebugPC((C.c_int32 * 2)(8, 8), (C.c_int32 * 2)(*out_res), (C.c_float * 2)(0.0, 1.0), 0, flags,
                                        (C.c_float * 2)(0.0, 0.0)))
    assert call(None) == -1 and call(pc(), host=None) == -1
    assert call(pc(), bilinear=2) == -1 and b"useBilinearSampler" in lib.prosper_pt_last_error()
    assert call(pc(flags=64)) == -1 and b"flag bits" in lib.prosper_pt_last_error()
    assert call(pc((0, 16))) == -1 and b"empty outRes" in lib.prosper_pt_last_error()
    assert call(pc((32769, 1))) == -1 and b"32768" in lib.prosper_pt_last_error()
    assert call(pc(), size=16 * 16 * 4 - 1) == -1 and b"too small" in lib.prosper_pt_last_error()
    assert call(pc()) == -1 and b"null argument" in lib.prosper_pt_last_error()  # everything else is fine: the null context
    assert lib.prosper_pt_get_texture_debug_peek(None, None) == -1
