"""The forward transparent pass without a GPU: the C-ABI surface and its refusals, the restatement's two arrangements of
the blend state, the designed scene of tests/test_transparent.py (its expected layers, the share of edge pixels) and the
front-face rule's sign against the camera's projection."""
import ctypes as C

import numpy as np

import deferred_shading_reference as D
import transparent_reference as T
from prosper_amd import capi, scenes, structs as S
from test_transparent import DESIGN, EXTENTS, designed_scene, expected_layers, pixel_coordinates

NEW_SYMBOLS = ("prosper_pt_forward_transparent", "prosper_pt_get_transparent_info", "prosper_pt_set_transparent_debug_layers",
               "prosper_pt_read_transparent_layers", "prosper_host_forward_renderer_create",
               "prosper_host_forward_renderer_destroy", "prosper_host_forward_renderer_record_transparent",
               "prosper_host_gbuffer_tracer_set_opaque_only")


def camera(oracle, world, w, h):
    c = world.camera
    return oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)[0]


def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4
    assert (S.GBUFFER_JITTER, S.GBUFFER_OPAQUE_ONLY) == (1, 4)
    assert (S.TRANSPARENT_JITTER, S.TRANSPARENT_CAMERA_JITTER) == (1, 2)
    assert C.sizeof(S.ForwardPC) == 12 and C.sizeof(S.TransparentLayer) == 64 and C.sizeof(S.TransparentInfo) == 24
    assert np.dtype(S.TransparentLayer).itemsize == 64


def test_bad_arguments_are_rejected_before_touching_the_gpu(oracle):
    lib = capi.lib()
    cam = camera(oracle, scenes.cornell(), 4, 4)
    pc = S.ForwardPC(0, 0, 0)

    def refused(rc, words, code=-1):
        return rc == code and words in lib.prosper_pt_last_error().decode()

    def run(pc_=C.byref(pc), flags=0, cam_=C.byref(cam), w=4, h=4):
        return lib.prosper_pt_forward_transparent(None, pc_, flags, 0, cam_, w, h, None, 0, None)

    assert refused(run(), "null argument")  # only the context is missing
    assert refused(run(pc_=None), "null argument")
    assert refused(run(cam_=None), "null argument")
    assert refused(run(w=0), "empty extent")
    assert refused(run(h=0), "empty extent")
    assert refused(run(flags=S.TRANSPARENT_JITTER | S.TRANSPARENT_CAMERA_JITTER), "exclude each other")
    assert refused(run(flags=4), "unknown flags")
    assert refused(run(flags=S.TRANSPARENT_JITTER | 8), "unknown flags")
    assert refused(run(pc_=C.byref(S.ForwardPC(len(S.DRAW_TYPES), 0, 0))), "drawType out of range")
    assert refused(run(pc_=C.byref(S.ForwardPC(0, 2, 0))), "ibl is 0 or 1")
    assert refused(run(pc_=C.byref(S.ForwardPC(0, 1, 0))), "ImageBasedLighting", code=-6)  # UNSUPPORTED
    bad = S.CameraUniforms.from_buffer_copy(bytes(cam))
    bad.far_ = bad.near_
    assert refused(run(cam_=C.byref(bad)), "near_ < far_")
    info = S.TransparentInfo()
    assert refused(lib.prosper_pt_get_transparent_info(None, C.byref(info)), "null argument")
    assert refused(lib.prosper_pt_set_transparent_debug_layers(None, 4), "null argument")
    assert refused(lib.prosper_pt_read_transparent_layers(None, None, None, 16, 4, None), "null argument")
    assert lib.prosper_host_forward_renderer_record_transparent(None, None, 4, 4, None, 1, 0, 0, 0, 0, None, None) == -1
    h = C.c_void_p()
    assert lib.prosper_host_forward_renderer_create(None, C.byref(h)) == -1 and not h.value
    assert lib.prosper_host_gbuffer_tracer_set_opaque_only(None, 1) == -1


def test_the_gbuffer_entries_accept_the_opaque_only_flag_and_nothing_else_new():
    """Bit 2 passes the flag check of both entries (the refusal is then the missing camera or context); bit 1 stays an
    unknown flag of both, bit 0 of the velocity entry."""
    lib = capi.lib()
    cam = S.CameraUniforms()
    desc = S.VelocityGBufferDesc()

    def message(rc):
        assert rc == -1
        return lib.prosper_pt_last_error().decode()

    for flags in (S.GBUFFER_OPAQUE_ONLY, S.GBUFFER_OPAQUE_ONLY | S.GBUFFER_JITTER):
        assert "null argument" in message(lib.prosper_pt_trace_gbuffer(None, 0, 1, flags, C.byref(cam), 4, 4, None, None))
    assert "null argument" in message(lib.prosper_pt_trace_gbuffer_velocity(None, 0, 1, S.GBUFFER_OPAQUE_ONLY, C.byref(cam), 4, 4,
                                                                            C.byref(desc), None))
    for flags in (2, 6, 8):
        assert "unknown flags" in message(lib.prosper_pt_trace_gbuffer(None, 0, 1, flags, C.byref(cam), 4, 4, None, None))
    for flags in (1, 2, 5, 8):
        assert "unknown flags" in message(lib.prosper_pt_trace_gbuffer_velocity(None, 0, 1, flags, C.byref(cam), 4, 4,
                                                                                C.byref(desc), None))


def test_front_to_back_equals_back_to_front():
    """Random stacks of 0 to 12 layers, alphas 0 and 1 among them: the two arrangements agree to float64 rounding (a
    layer of alpha 1 ends the front-to-back loop: what lies behind it has weight 0 in the other arrangement too)."""
    rng = np.random.default_rng(12)
    for trial in range(2000):
        k = int(rng.integers(0, 13))
        src = rng.uniform(0.0, 20.0, (k, 3))
        a = rng.uniform(0.0, 1.0, k)
        special = rng.uniform(0.0, 1.0, k)
        a = np.where(special < 0.15, 0.0, np.where(special > 0.85, 1.0, a))
        dst = rng.uniform(0.0, 20.0, 4)
        f, fa = T.composite_front_to_back(src, a, dst)
        b, ba = T.composite_back_to_front(src, a, dst)
        assert np.allclose(f, b, rtol=1e-13, atol=1e-13), (trial, a)
        assert fa == ba and (fa is None) == (k == 0)
        if k and a[0] == 1.0:
            assert np.array_equal(f, src[0]) and fa == 0.0
        if k and (a == 0.0).all():
            assert np.allclose(f, dst[:3], rtol=0, atol=0)
    # one layer: prosper's blend state itself
    f, fa = T.composite_front_to_back(np.array([[1.0, 2.0, 3.0]]), np.array([0.25]), np.array([4.0, 4.0, 4.0, 1.0]))
    assert np.allclose(f, [3.25, 3.5, 3.75]) and fa == 0.25 * 0.75


def test_the_designed_scene_has_the_expected_layers(oracle):
    world = designed_scene()
    f = world.freeze()
    assert f["draw_instance_count"] == len(DESIGN)
    assert [d.materialIndex for d in f["draw_instances"]] == list(range(1, len(DESIGN) + 1))  # draw instance k is DESIGN[k]
    names = [d[0] for d in DESIGN]
    w, h = EXTENTS[0]
    cam = camera(oracle, world, w, h)
    seq, undecided = expected_layers(cam, w, h)
    # a condition on the design: at most 10 % of the pixels lie within one pixel of a projected edge
    assert undecided.mean() <= 0.10, undecided.mean()
    # the four regions between the three edge lines, left to right, front to back
    want = [("L1", "L3"),
            ("L1", "L2", "D1", "D2", "L3"),
            ("texture", "L2", "D1", "D2", "L3", "L4"),
            ("texture", "L2", "L3", "L4", "behind")]
    row = h // 2
    found = []
    for x in range(w):
        if undecided[row, x]:
            continue
        s = tuple(names[k] for k in seq[row, x])
        if not found or found[-1] != s:
            found.append(s)
    assert found == want, found
    # no horizontal edge shows: every decided column is the same from top to bottom
    for x in np.nonzero(~undecided[row])[0]:
        assert all(seq[y, x] == seq[row, x] for y in range(h) if not undecided[y, x])
    assert (~undecided).all(axis=0).sum() == (~undecided[row]).sum()
    # the other ray modes move the samples by less than a pixel: the same sequences on the pixels decided in both
    seq2, undecided2 = expected_layers(cam, w, h, (0.2, 0.7))
    both = ~undecided & ~undecided2
    assert all(seq[y, x] == seq2[y, x] for y, x in zip(*np.nonzero(both)))


def test_front_faces_are_counter_clockwise_under_the_cameras_projection(oracle):
    """The pass calls a triangle front-facing when cross(p1 - p0, p2 - p0) . d < 0.  prosper's pipeline culls by the
    winding in framebuffer coordinates (VkUtils.hpp:67, counter-clockwise front): Vulkan's signed area
    a = -1/2 sum(x_i y_i+1 - x_i+1 y_i) over the projected corners, y down, positive = counter-clockwise.  Over random
    triangles in front of the camera the two signs agree, through the camera's own cameraToClip (whose y is flipped)."""
    world = scenes.cornell()
    cam = camera(oracle, world, 96, 64)
    eye = np.array(world.camera["eye"], np.float64)
    rng = np.random.default_rng(5)
    tri = rng.uniform(-1.0, 1.0, (500, 3, 3)) + [0.0, 1.0, 0.0]  # inside the room, in front of the camera at z = 3.4
    p = pixel_coordinates(cam, tri.reshape(-1, 3), 96, 64).reshape(500, 3, 2)
    x, y = p[..., 0], p[..., 1]
    area = -0.5 * sum(x[:, i] * y[:, (i + 1) % 3] - x[:, (i + 1) % 3] * y[:, i] for i in range(3))
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    d = tri.mean(axis=1) - eye
    facing = (n * d).sum(-1) < 0.0
    decided = np.abs(area) > 1e-3
    assert decided.sum() > 400 and ((area > 0.0) == facing)[decided].all()
    # and the pixel coordinates are the primary ray's: y grows downwards in the image (the projection flips world y)
    top = pixel_coordinates(cam, np.array([[0.0, 1.9, 0.0], [0.0, 0.1, 0.0]]), 96, 64)
    assert top[0, 1] < top[1, 1]
    # scenes.quad documents its winding as counter-clockwise seen from its normal's side: the designed quads face +z
    for k, (name, z, t, kind, rgba) in enumerate(DESIGN):
        pos = designed_scene_quads()[k]
        nq = np.cross(pos[1] - pos[0], pos[2] - pos[0])
        assert (nq[2] > 0) == (kind != "away"), name


def designed_scene_quads():
    """The corner positions of every designed quad, as scenes.quad orders them."""
    from test_transparent import EYE_Z
    out = []
    for name, z, (t0, t1), kind, rgba in DESIGN:
        dist = EYE_Z - z
        corners = [(t0 * dist, -0.5 * dist, z), (t1 * dist, -0.5 * dist, z), (t1 * dist, 0.5 * dist, z), (t0 * dist, 0.5 * dist, z)]
        if kind == "away":
            corners.reverse()
        out.append(scenes.quad(*corners)[0])
    return out


def test_the_restatement_shades_a_layer_like_the_deferred_restatement(oracle):
    """A layer record built from a G-buffer texel's surface shades to deferred_shading_reference.shade's value for that
    texel (brute force over every light): the two restatements share their lighting."""
    import restir_resampling_reference as R
    world = scenes.cornell()
    w, h = 24, 16
    cam, fl, osc, ar, nm, depth, _ = R.make_gbuffer(oracle, world, w, h)
    want, total, _ = D.shade(world, cam, ar, nm, depth)
    sf = R.Surfaces(cam, ar, nm, depth)
    hit = depth.ravel() != 0.0
    layers = np.zeros(hit.sum(), np.dtype(S.TransparentLayer))
    layers["positionWS"], layers["normal"] = sf.pos[hit], sf.n[hit]
    layers["albedo"], layers["roughness"], layers["metallic"] = sf.albedo[hit], sf.rough[hit], sf.metal[hit]
    lsf = T.LayerSurfaces(cam, layers, sf.px[hit], sf.py[hit])
    got, gtotal, _ = T.shade(world, cam, lsf)
    assert np.allclose(got, want.reshape(-1, 3)[hit], rtol=1e-5, atol=1e-7)
    assert np.allclose(lsf.z_cam, sf.lin_depth[hit], rtol=1e-4)
