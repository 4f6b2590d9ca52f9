"""The debug lines on the GPU (prosper_pt_debug_lines; pt_debug_view.hip): a designed scene - one large
quad at distance 2 facing the camera, sky to its right - at 48 x 32, and every line set against
tests/debug_view_reference.py over the GPU's own read-back of the HDR image, the depth and the camera, bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import debug_view_reference as R
from conftest import same_bits
from debug_view_scene import FOCAL, FOV, H, QUAD_DISTANCE, W, quad_world
from prosper_amd import structs as S

pytestmark = pytest.mark.gpu

F = np.float32


def at(px, py, d):
    """the world position that projects to framebuffer coordinates (px, py) at distance d (the camera sits at the origin)"""
    return np.array([(px - W / 2) * d / FOCAL, -(py - H / 2) * d / FOCAL, -d])


def line(p0, p1, colour):
    return np.concatenate([p0, p1, colour]).astype(F)


def colour_of(k):
    """a colour of its own for every line"""
    return (1.0 + k, 0.25 + 0.5 * (k % 7), 3.0 - 0.125 * (k % 13))


@pytest.fixture(scope="module")
def setup(gpu_ctx, oracle):
    gpu_ctx.upload_scene(quad_world())
    cam = oracle.camera_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), FOV, 0.1, 100.0, W, H)[0]
    return gpu_ctx, cam


def baseline(ctx, cam):
    """a fresh HDR image and depth of the scene, read back"""
    ctx.deferred_shading_traced(cam, W, H)
    return ctx.read_hdr(), ctx.read_gbuffer()[2]


def draw(ctx, cam, lines):
    """-> (hdr before, depth before, hdr after, depth after, info)"""
    hdr0, depth0 = baseline(ctx, cam)
    ctx.debug_lines(lines, cam, W, H)
    info = ctx.debug_lines_info()
    return hdr0, depth0, ctx.read_hdr(), ctx.read_gbuffer()[2], info


def check(ctx, cam, lines):
    """the pass equals the restatement over the read-back; -> (restatement's info, before, after)"""
    hdr0, depth0, hdr1, depth1, info = draw(ctx, cam, lines)
    want_hdr, want_depth, want = R.debug_lines(lines, cam, W, H, hdr0, depth0)
    bad = ~(same_bits(hdr1, want_hdr).all(2) & same_bits(depth1, want_depth))
    assert not bad.any(), "%d pixels differ, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    assert info.valid == 1 and info.lineCount == len(lines)
    assert info.fragmentsWritten == want["fragmentsWritten"]
    assert info.linesClippedAway == want["linesClippedAway"]
    return want, (hdr0, depth0), (hdr1, depth1)


def geometric_cases(d, confined):
    """The CPU test's cases at distance d, scaled to this image; `confined`: only those that stay over the quad - the set
    behind the quad leaves out the lines that leave the viewport or cross the near plane, which would cross the sky columns
    (stored depth 0) and draw there."""
    pts = [((2.5, 5.5), (19.5, 5.5)), ((19.5, 7.5), (2.5, 7.5)),      # horizontal, both directions
           ((4.5, 10.5), (4.5, 27.5)), ((6.5, 27.5), (6.5, 10.5)),    # vertical
           ((9.5, 10.5), (22.5, 23.5)), ((24.5, 23.5), (11.5, 10.5)),  # 45 degrees
           ((26.5, 2.5), (29.5, 28.5)), ((32.5, 28.5), (29.5, 2.5)),  # steep
           ((1.5, 29.5), (30.5, 25.5)), ((30.5, 27.5), (1.5, 31.5)),  # shallow
           ((8.2, 1.3), (15.5, 3.1)), ((15.5, 3.1), (27.9, 2.2)),     # a polyline, its joint on a pixel centre
           ((20.5, 15.5), (20.5, 15.5)),                               # zero length
           ((12.3, 12.2), (12.7, 12.4)), ((12.6, 14.2), (12.9, 14.4))]  # under a pixel: across a centre, across none
    lines = [line(at(*a, d), at(*b, d), colour_of(k)) for k, (a, b) in enumerate(pts)]
    if not confined:
        k = len(lines)
        centre = at(24.0, 16.0, d)
        for far in (at(-40.0, 16.0, d), at(100.0, 17.0, d), at(23.0, -50.0, d), at(25.0, 90.0, d)):  # through each edge
            lines.append(line(centre, far, colour_of(len(lines))))
            lines.append(line(far, centre + np.array([0.0, 0.1, 0.0]), colour_of(len(lines))))
        lines.append(line(at(10.0, 20.0, d), np.array([0.3, 0.0, 1.0]), colour_of(len(lines))))   # through the near plane
        lines.append(line(np.array([0.3, 0.0, 1.0]), np.array([-0.2, 0.1, 2.0]), colour_of(len(lines))))  # behind the eye
        assert len(lines) == k + 10
    return np.stack(lines)


def test_the_scene_is_what_the_design_says(setup):
    ctx, cam = setup
    _, depth = baseline(ctx, cam)
    assert (depth[:, :35] > 0).all() and (depth[:, 37:] == 0).all()  # the quad, then the sky
    want = R.screen_segment(line(at(10.0, 10.0, QUAD_DISTANCE), at(20.0, 10.0, QUAD_DISTANCE), (1, 1, 1)),
                            R.mat4(cam.worldToCamera), R.mat4(cam.cameraToClip), W, H)[0][2]
    assert np.abs(depth[:, :35] - want).max() < 1e-5


def test_lines_in_front_of_the_quad_match_the_restatement_bit_for_bit(setup):
    ctx, cam = setup
    lines = geometric_cases(1.0, confined=False)
    want, (hdr0, depth0), (hdr1, depth1) = check(ctx, cam, lines)
    assert want["linesClippedAway"] == 1 and want["fragmentsWritten"] > 200
    wrote = want["winner"] >= 0
    assert same_bits(hdr1[~wrote], hdr0[~wrote]).all() and same_bits(depth1[~wrote], depth0[~wrote]).all()
    assert (hdr1[wrote][:, 3] == 1).all() and (depth1[wrote] > depth0[wrote]).all()
    # every fragment of a line in front of everything was written, unless a later line took the pixel
    fragments = sum(len(R.line_fragments(l, cam, W, H)[0]) for l in lines[:-1])
    assert want["fragmentsWritten"] <= fragments
    for k in (12, 14):  # the zero-length line and the one across no centre
        assert not (want["winner"] == k).any()
    assert (want["winner"] == 13).sum() == 1


def test_lines_behind_the_quad_change_nothing(setup):
    ctx, cam = setup
    want, (hdr0, depth0), (hdr1, depth1) = check(ctx, cam, geometric_cases(3.0, confined=True))
    assert want["fragmentsWritten"] == 0 and want["linesClippedAway"] == 0
    assert same_bits(hdr1, hdr0).all() and same_bits(depth1, depth0).all()


def test_a_line_in_the_quads_plane_is_decided_by_the_strict_test(setup):
    ctx, cam = setup
    d = QUAD_DISTANCE
    lines = np.stack([line(at(3.5, 9.5, d), at(30.5, 9.5, d), colour_of(0)), line(at(5.5, 3.5, d), at(25.5, 28.5, d), colour_of(1))])
    want, (hdr0, depth0), _ = check(ctx, cam, lines)
    # where the line's interpolated depth has the stored depth's bits, equal loses
    x, y, z = R.line_fragments(lines[0], cam, W, H)
    equal = same_bits(z, depth0[y, x])
    assert (want["winner"][y[equal], x[equal]] != 0).all()
    assert (want["winner"][y, x] == 0).sum() == (z > depth0[y, x]).sum()


def test_crossing_lines_nearest_wins_and_at_equal_depth_the_higher_index(setup):
    ctx, cam = setup
    lines = np.stack([line(at(4.5, 16.5, 1.0), at(30.5, 16.5, 1.0), colour_of(0)),    # 0 near, horizontal
                      line(at(16.5, 4.5, 1.5), at(16.5, 28.5, 1.5), colour_of(1)),    # 1 farther, vertical: loses at (16, 16)
                      line(at(4.5, 20.5, 1.0), at(30.5, 20.5, 1.0), colour_of(2)),    # 2 and 3: the same line twice
                      line(at(4.5, 20.5, 1.0), at(30.5, 20.5, 1.0), colour_of(3)),
                      line(at(20.5, 4.5, 1.0), at(20.5, 28.5, 1.0), colour_of(4))])   # 4: the same depth as 0, 2 and 3
    want, _, (hdr1, _) = check(ctx, cam, lines)
    winner = want["winner"]
    assert winner[16, 16] == 0 and winner[15, 16] == 1 and winner[17, 16] == 1 and winner[20, 16] == 3
    assert (winner[20, 4:30] != 2).all() and (winner[20, 4:20] == 3).all()
    assert winner[16, 20] == 4 and winner[20, 20] == 4
    assert tuple(hdr1[16, 20]) == tuple(F(c) for c in colour_of(4)) + (F(1.0),)


def test_a_line_through_the_sky_is_drawn_over_depth_zero(setup):
    ctx, cam = setup
    lines = np.stack([line(at(30.5, 10.5, 5.0), at(46.5, 12.5, 5.0), colour_of(0)),   # behind the quad, then over the sky
                      line(at(40.5, 2.5, 90.0), at(44.5, 30.5, 90.0), colour_of(1))])  # nearly at the far plane
    want, (_, depth0), _ = check(ctx, cam, lines)
    winner = want["winner"]
    assert (winner[:, :35] == -1).all() and (winner[:, 37:] == 0).sum() >= 9 and (winner == 1).sum() >= 26
    assert (depth0[winner >= 0] == 0).all()


def test_non_finite_and_far_away_endpoints_write_nothing_and_are_counted(setup):
    ctx, cam = setup
    good = at(24.0, 16.0, 1.0)
    lines = [line(np.array([1e30, 0.0, -1.0]), np.array([1e30, 1.0, -1.0]), colour_of(0)),
             line(np.array([1e30, 1e30, 1e30]), np.array([-1e30, 1e30, 1e30]), colour_of(1))]
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            l = line(good, at(10.0, 10.0, 1.0), colour_of(len(lines)))
            l[k] = bad
            lines.append(l)
    lines = np.stack(lines)
    want, (hdr0, depth0), (hdr1, depth1) = check(ctx, cam, lines)
    assert want["linesClippedAway"] == len(lines) == 20 and want["fragmentsWritten"] == 0
    assert same_bits(hdr1, hdr0).all() and same_bits(depth1, depth0).all()
    # one end in view and the other 1e30 away: walked in bounded steps to the viewport's edge
    lines = np.stack([line(good, np.array([1e30, 0.0, -1.0]), colour_of(0)), line(np.array([0.0, -3e38, -1.0]), good, colour_of(1)),
                      line(good, np.array([1e30, 1e30, -1e30]), colour_of(2))])
    want, _, _ = check(ctx, cam, lines)
    assert 0 < want["fragmentsWritten"] <= 3 * W


def random_lines(n, seed):
    rng = np.random.default_rng(seed)
    lines = []
    for k in range(n):
        a = at(rng.uniform(-8, W + 8), rng.uniform(-8, H + 8), rng.uniform(0.5, 3.5))
        b = at(rng.uniform(-8, W + 8), rng.uniform(-8, H + 8), rng.uniform(0.5, 3.5))
        lines.append(line(a, b, colour_of(k)))
    return np.stack(lines)


@pytest.mark.parametrize("n", (65, 257))
def test_more_lines_than_a_wave_and_a_workgroup_hold_in_any_order(setup, n):
    ctx, cam = setup
    lines = random_lines(n, n)
    want, _, (hdr1, depth1) = check(ctx, cam, lines)
    assert want["fragmentsWritten"] > 400 and len(np.unique(want["winner"])) > n // 4
    perm = np.random.default_rng(1).permutation(n)
    want_p, _, (hdr_p, depth_p) = check(ctx, cam, lines[perm])
    assert same_bits(depth_p, depth1).all() and want_p["fragmentsWritten"] == want["fragmentsWritten"]
    # the same line wins every pixel (no two lines tie in these sets), whatever its index
    wrote = want["winner"] >= 0
    assert (perm[want_p["winner"][wrote]] == want["winner"][wrote]).all()
    assert same_bits(hdr_p, hdr1).all()


def test_a_second_identical_call_gives_the_identical_image_and_count(setup):
    ctx, cam = setup
    lines = random_lines(65, 3)
    results = []
    for _ in range(2):  # the keys were left zero
        _, _, hdr1, depth1, info = draw(ctx, cam, lines)
        results.append((hdr1, depth1, info.fragmentsWritten))
    assert results[0][2] == results[1][2] > 0
    assert same_bits(results[0][0], results[1][0]).all() and same_bits(results[0][1], results[1][1]).all()
    # and drawn again over their own result nothing passes the strict test
    ctx.debug_lines(lines, cam, W, H)
    assert ctx.debug_lines_info().fragmentsWritten == 0
    assert same_bits(ctx.read_hdr(), results[1][0]).all()


def test_no_lines_is_a_no_op_and_too_many_are_refused(setup):
    ctx, cam = setup
    hdr0, depth0 = baseline(ctx, cam)
    ctx.debug_lines(np.zeros((0, 9), F), cam, W, H)
    info = ctx.debug_lines_info()
    assert info.valid == 1 and info.lineCount == 0 and info.fragmentsWritten == 0 and info.ms == 0.0
    assert same_bits(ctx.read_hdr(), hdr0).all() and same_bits(ctx.read_gbuffer()[2], depth0).all()
    with pytest.raises(Exception, match="100 000"):
        ctx.debug_lines(np.zeros((100001, 9), F), cam, W, H)
    with pytest.raises(Exception, match="another extent"):
        ctx.debug_lines(np.zeros((1, 9), F), cam, W + 1, H)
    assert same_bits(ctx.read_hdr(), hdr0).all()


def test_the_maximum_of_lines_is_drawn(setup):
    ctx, cam = setup
    # 100 000 short lines over the whole image at distance 1: every pixel centre is crossed by some line
    n = S.MAX_DEBUG_LINE_COUNT
    k = np.arange(n)
    px, py = (k % 480) * 0.1, (k // 480) * (H / (n / 480.0))
    lines = np.stack([line(at(x, y, 1.0), at(x + 0.7, y + 0.05, 1.0), (1.0, 2.0, 3.0)) for x, y in zip(px[::1000], py[::1000])])
    full = np.zeros((n, 9), F)
    full[:] = line(at(-5.0, -5.0, 1.0), at(-4.0, -5.0, 1.0), (0.0, 0.0, 0.0))  # the rest: outside, clipped away
    full[::1000] = lines
    hdr0, depth0, hdr1, depth1, info = draw(ctx, cam, full)
    want_hdr, want_depth, want = R.debug_lines(lines, cam, W, H, hdr0, depth0)
    assert info.lineCount == n and info.linesClippedAway == n - len(lines) + want["linesClippedAway"]
    assert info.fragmentsWritten == want["fragmentsWritten"] > 0
    assert same_bits(hdr1, want_hdr).all() and same_bits(depth1, want_depth).all()


def test_before_any_gbuffer_the_call_returns_no_scene(oracle):
    from prosper_amd import capi
    cam = oracle.camera_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), FOV, 0.1, 100.0, W, H)[0]
    ctx = capi.Context(device=0)
    try:
        lines = np.zeros((1, 9), F)
        rc = capi.lib().prosper_pt_debug_lines(ctx._h, C.c_void_p(lines.ctypes.data), 1, C.byref(cam), W, H, None)
        assert rc == -4  # PROSPER_PT_ERR_NO_SCENE
        assert ctx.debug_lines_info().valid == 0
    finally:
        ctx.close()


def test_the_focus_distance_of_the_traced_quad_is_its_distance(setup):
    """render_gltf.py --focus-at: focus_distance_from_depth over read-back texels of the quad, perpendicular to the view
    at distance 2.  Against the float64 restatement over the same texel: 1e-5 relative (about ten float32 operations at
    6e-8 each, tenfold margin).  Against the distance itself the same bound holds: the traced depth is z / w of two fused
    rows, a few float32 roundings more, and d(distance) / distance <= d(depth) / depth for this projection."""
    from prosper_amd import debug_geometry as G
    ctx, cam = setup
    _, depth = baseline(ctx, cam)
    for px, py in ((0, 0), (34, 31), (17, 16), (5, 27), (30, 3)):
        texel = depth[py, px]
        assert texel > 0
        d32 = G.focus_distance_from_depth(cam, (px, py), (W, H), texel)
        d64 = G.focus_distance_from_depth(cam, (px, py), (W, H), texel, dtype=np.float64)
        assert d32.dtype == F and abs(float(d32) - d64) <= 1e-5 * d64, (px, py)
        assert abs(float(d32) - QUAD_DISTANCE) <= 1e-5 * QUAD_DISTANCE, (px, py, float(d32))


def test_the_cpp_debug_renderer_draws_what_the_direct_call_draws(setup):
    from prosper_amd.rt_reference import Camera, DebugRenderer, HostDebugLines
    ctx, _ = setup
    lines = geometric_cases(1.0, confined=False)
    hcam = Camera()
    hcam.set_parameters(FOV, 0.1, 100.0)
    hcam.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))
    hcam.update_resolution(W, H)
    cam = hcam.update_buffer()[0]  # what record will hand to the pass
    _, _, hdr1, depth1, info = draw(ctx, cam, lines)
    host_lines, renderer = HostDebugLines(), DebugRenderer(ctx)
    try:
        host_lines.add_line((9, 9, 9), (8, 8, 8), (7, 7, 7))
        host_lines.reset()
        for l in lines:
            host_lines.add_line(l[0:3], l[3:6], l[6:9])
        assert host_lines.count == len(lines)
        baseline(ctx, cam)
        renderer.record(hcam, host_lines, W, H)
        assert ctx.debug_lines_info().fragmentsWritten == info.fragmentsWritten > 0
        assert same_bits(ctx.read_hdr(), hdr1).all() and same_bits(ctx.read_gbuffer()[2], depth1).all()
        host_lines.reset()  # an empty list records a call that draws nothing
        renderer.record(hcam, host_lines, W, H)
        assert ctx.debug_lines_info().lineCount == 0
        with pytest.raises(Exception, match="another extent"):
            renderer.record(hcam, host_lines, W + 2, H)
    finally:
        renderer.close()
        host_lines.close()
        hcam.close()


CW, CH = 384, 256  # the chain's image: large enough for the passes' footprints to leave most of it out of reach
CHAIN_DOF = (QUAD_DISTANCE, 1.0, 2.0, 1)  # focus, maxBackgroundCoC, maxCoC (half-resolution texels), gatherRadius (tiles)


def chain_reach(wrote, bloom_reaches):
    """Where lines that wrote the pixels `wrote` can change the image behind bloom, TAA and depth of field: the bounding
    box of `wrote`, grown by each pass's footprint as its restatement (bloom_reference.py, taa_reference.py,
    dof_reference.py) is built.  Conservative: a box, every footprint rounded up.

    bloom (HALF, four levels, compose reads 0-2), only when a line is above the threshold (otherwise every highlight is 0
      in both chains and compose adds 0): rows - a level-2 texel is 8 pixels; block alignment 1 texel, vertical taps
      within [-2.09, 3] plus the bilinear neighbour 4, the horizontal pass's neighbour row 1, compose's biquadratic
      lookup 2: 8 texels = 64 pixels, and separate's bilinear 2 -> 66.  Columns - level 1's streak reads width / 8 of its
      texels (4 pixels each) to either side, width / 2 pixels, then the same 66.
    TAA with the history ignored: the 3 x 3 neighbourhood of illumination and depth -> 1, taken as 2.
    depth of field with CHAIN_DOF, in half-resolution texels: |CoC| <= 2; dilate looks gatherRadius = 1 tile of 8 to
      either side of the texel's own tile 8 + 7 = 15; gather's taps lie within the kernel radius 2 and read mips
      <= log2(2) - 1 + 1 = 1 trilinearly, a texel of 2 and its neighbour 4; the median 1; combine's upsampling 1:
      23 texels = 46 pixels, and setup's 2 x 2 footprint 2 -> 48."""
    ys, xs = np.nonzero(wrote)
    y0, y1, x0, x1 = ys.min(), ys.max(), xs.min(), xs.max()
    if bloom_reaches:
        y0, y1, x0, x1 = y0 - 66, y1 + 66, x0 - CW // 2 - 66, x1 + CW // 2 + 66
    grow = 2 + 48
    y0, y1, x0, x1 = max(y0 - grow, 0), min(y1 + grow, CH - 1), max(x0 - grow, 0), min(x1 + grow, CW - 1)
    reach = np.zeros((CH, CW), bool)
    reach[y0:y1 + 1, x0:x1 + 1] = True
    return reach


def test_the_pass_composes_with_bloom_taa_and_depth_of_field(setup, oracle):
    """lines -> bloom -> TAA -> depth of field against the same chain without lines: bit-identical wherever chain_reach says
    the lines, or their bloom, cannot reach; changed where the lines were drawn."""
    ctx, _ = setup
    cam = oracle.camera_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), FOV, 0.1, 100.0, CW, CH)[0]
    focal = (CH / 2) / math.tan(FOV / 2)

    def at_chain(px, py, d):
        return np.array([(px - CW / 2) * d / focal, -(py - CH / 2) * d / focal, -d])

    def lines_of(d, colour):
        # a few lines in the top left corner, over the quad: the box of columns 8-60 and rows 8-40
        pts = [((8.5, 8.5), (60.5, 12.5)), ((60.5, 40.5), (8.5, 30.5)), ((20.5, 8.5), (24.5, 40.5)), ((10.5, 10.5), (40.5, 40.5)),
               ((30.2, 20.3), (30.7, 20.4))]
        return np.stack([line(at_chain(*a, d), at_chain(*b, d), colour) for a, b in pts])

    def chain(lines, threshold):
        ctx.trace_gbuffer_velocity(cam, CW, CH)
        g, _, _ = ctx.gbuffer_device_ptrs()
        ctx.deferred_shading_device(cam, CW, CH, g.albedoRoughness, g.normalMetallic, g.nonLinearDepth)
        ctx.skybox_fill(cam, CW, CH)
        before = ctx.read_hdr(), ctx.read_gbuffer()[2]
        if lines is not None:
            ctx.debug_lines(lines, cam, CW, CH)
        ctx.bloom(S.BloomPC.default(threshold=threshold), CW, CH)
        ctx.taa_resolve(S.TaaPC.default(reset_history=1), CW, CH)
        ctx.depth_of_field(S.DofPC(*CHAIN_DOF), cam, CW, CH)
        return ctx.read_hdr(), before

    def wrote_by(lines, before):
        return R.debug_lines(lines, cam, CW, CH, *before)[2]["winner"] >= 0

    # ---- bloom's threshold above everything: no highlight in either chain, the lines reach through TAA and the lens only
    high = 1.0e6
    plain, before = chain(None, high)
    assert np.isfinite(plain).all() and before[0][..., :3].max() < high
    # lines that lose every depth test reach nothing
    behind = lines_of(3.0, (0.5, 0.4, 0.3))
    assert not wrote_by(behind, before).any()
    assert same_bits(chain(behind, high)[0], plain).all()
    dim = lines_of(1.0, (0.5, 0.4, 0.3))
    lit, before_lit = chain(dim, high)
    assert same_bits(before_lit[0], before[0]).all() and same_bits(before_lit[1], before[1]).all()
    wrote = wrote_by(dim, before)
    assert wrote.sum() > 100 and wrote[:8].sum() == 0 and wrote[42:].sum() == 0 and wrote[:, 62:].sum() == 0
    reach = chain_reach(wrote, bloom_reaches=False)
    assert reach.mean() < 0.15
    changed = ~same_bits(lit, plain).all(2)
    assert not (changed & ~reach).any(), "%d pixels changed out of the lines' reach" % (changed & ~reach).sum()
    assert changed[wrote].mean() > 0.9  # ... and the lines are there

    # ---- prosper's threshold, lines above it: their bloom reaches along the rows, not down the image
    plain, before = chain(None, 1.0)
    bright = lines_of(1.0, (8.0, 6.0, 4.0))
    lit, _ = chain(bright, 1.0)
    assert np.isfinite(lit).all()
    wrote = wrote_by(bright, before)
    reach = chain_reach(wrote, bloom_reaches=True)
    assert reach.mean() < 0.65 and not reach[170:].any() and not reach[:, 372:].any()
    changed = ~same_bits(lit, plain).all(2)
    assert not (changed & ~reach).any(), "%d pixels changed out of the reach of the lines and their bloom" % (changed & ~reach).sum()
    assert changed[wrote].mean() > 0.9
    assert (changed & ~chain_reach(wrote, bloom_reaches=False)).any()  # the bloom does spread beyond the lens's reach
