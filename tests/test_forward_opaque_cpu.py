"""The forward opaque pass without a GPU: the C-ABI surface and its refusals, the restatement
(tests/forward_reference.py) against the two restatements it stands between - transparent_reference.shade on the same
records, deferred_shading_reference.shade on a surface rebuilt from a G-buffer - the alpha rule, the clear values and the
three draw-type branches, and the condition on the twin scene of tests/test_forward_opaque.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import culling_reference as CR
import deferred_shading_reference as D
import forward_reference as FR
import raster_reference as RR
import raster_scenes as RS
import restir_resampling_reference as R
import transparent_reference as T
from prosper_amd import capi, scenes, structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# test_deferred_shading.py's shading tolerance, relative to the pixel's sum of absolute terms
REL = 2e-4
ABS = 1e-6

NEW_SYMBOLS = ("prosper_pt_raster_forward_shade", "prosper_pt_raster_forward", "prosper_pt_set_forward_debug_surfaces",
               "prosper_pt_read_forward_surfaces", "prosper_pt_get_forward_opaque_info", "prosper_pt_get_forward_depth_device_ptr",
               "prosper_pt_read_forward_depth", "prosper_host_forward_renderer_record_opaque", "prosper_host_forward_renderer_release_preserved")


def header_struct_size(header, name):
    """The size of a header struct of 4-byte scalars, arrays of them and pointers, laid out as the C ABI lays it out."""
    text = open(os.path.join(ROOT, "include", "prosper_pt", header)).read()
    body = text[text.index("typedef struct " + name + "\n"):text.index("} " + name + ";")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    offset, align = 0, 4
    for decl in re.findall(r"([^;{}]+);", body[body.index("{") + 1:]):
        decl = decl.strip()
        if "*" in decl:
            offset = (offset + 7) & ~7
            offset += 8 * len(decl.split(","))
            align = 8
            continue
        assert re.match(r"(uint32_t|int32_t|float)\s", decl), decl
        for field in decl.split(","):
            m = re.search(r"\[(\d+)\]", field)
            offset += 4 * (int(m.group(1)) if m else 1)
    return (offset + align - 1) & ~(align - 1)


def camera(oracle, world, w, h):
    c = world.camera
    return oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)[0]


def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4


def test_struct_sizes_equal_the_headers():
    assert C.sizeof(S.ForwardOpaqueDesc) == header_struct_size("prosper_pt.h", "prosper_pt_forward_opaque_desc") == 32
    assert C.sizeof(S.ForwardOpaqueInfo) == header_struct_size("prosper_pt.h", "prosper_pt_forward_opaque_info") == 16
    assert C.sizeof(S.ForwardRendererOutput) == header_struct_size("prosper_host.h", "prosper_host_forward_renderer_output") == 24
    assert C.sizeof(S.TransparentLayer) == header_struct_size("prosper_pt.h", "prosper_pt_transparent_layer") == 64
    assert [f[0] for f in S.ForwardOpaqueDesc._fields_] == ["nonLinearDepth", "velocity", "previousTransforms", "previousTransformCount"]
    assert [f[0] for f in S.ForwardOpaqueInfo._fields_] == ["shadedPixels", "reclustered", "ms", "shadeMs"]


def test_bad_arguments_are_rejected_before_touching_the_gpu(oracle):
    lib = capi.lib()
    cam = camera(oracle, scenes.cornell(), 4, 4)
    pc, desc = S.ForwardPC(0, 0, 0), S.ForwardOpaqueDesc()

    def refused(rc, words, code=-1):
        return rc == code and words in lib.prosper_pt_last_error().decode()

    for entry in (lib.prosper_pt_raster_forward_shade, lib.prosper_pt_raster_forward):
        def run(pc_=C.byref(pc), cam_=C.byref(cam), desc_=C.byref(desc)):
            return entry(None, pc_, cam_, desc_, None)

        assert refused(run(), "null argument")  # only the context is missing
        assert refused(run(pc_=None), "null argument")
        assert refused(run(cam_=None), "null argument")
        assert refused(run(desc_=None), "null argument")
        assert refused(run(pc_=C.byref(S.ForwardPC(len(S.DRAW_TYPES), 0, 0))), "drawType out of range")
        assert refused(run(pc_=C.byref(S.ForwardPC(0, 2, 0))), "ibl is 0 or 1")
        assert refused(run(pc_=C.byref(S.ForwardPC(0, 1, 0))), "ImageBasedLighting", code=-6)  # UNSUPPORTED
        bad = S.CameraUniforms.from_buffer_copy(bytes(cam))
        bad.far_ = bad.near_
        assert refused(run(cam_=C.byref(bad)), "near_ < far_")
        odd = S.ForwardOpaqueDesc()
        odd.nonLinearDepth = 258
        assert refused(run(desc_=C.byref(odd)), "4-byte aligned")
        odd = S.ForwardOpaqueDesc()
        odd.velocity = 260
        assert refused(run(desc_=C.byref(odd)), "8-byte aligned")
        count = S.ForwardOpaqueDesc()
        count.previousTransformCount = 3
        assert refused(run(desc_=C.byref(count)), "previousTransformCount without previousTransforms")
    info = S.ForwardOpaqueInfo()
    assert refused(lib.prosper_pt_get_forward_opaque_info(None, C.byref(info)), "null argument")
    assert refused(lib.prosper_pt_set_forward_debug_surfaces(None, 1), "null argument")
    assert refused(lib.prosper_pt_read_forward_surfaces(None, None, 16, None), "null argument")
    assert refused(lib.prosper_pt_read_forward_depth(None, None, 16, None), "null argument")
    out = S.ForwardRendererOutput()
    assert lib.prosper_host_forward_renderer_record_opaque(None, None, 4, 4, 0, 0, None, 0, None, C.byref(out)) == -1
    assert lib.prosper_host_forward_renderer_release_preserved(None) == -1


def hand_made_records(rng, h, w, uncovered=0.25):
    """records of random surfaces in front of the cornell camera, a share of them uncovered, alphas of every kind"""
    rec = np.zeros((h, w), np.dtype(S.TransparentLayer))
    rec["positionWS"] = rng.uniform(-0.9, 0.9, (h, w, 3)) + [0.0, 1.0, 0.0]
    n = rng.normal(size=(h, w, 3))
    rec["normal"] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    rec["albedo"] = rng.uniform(0.0, 1.0, (h, w, 3))
    rec["roughness"] = rng.uniform(0.05, 1.0, (h, w))
    rec["metallic"] = rng.uniform(0.0, 1.0, (h, w))
    kind = rng.uniform(0.0, 1.0, (h, w))
    rec["alpha"] = np.where(kind < 0.4, -1.0, np.where(kind < 0.5, 1.0, rng.uniform(0.01, 1.0, (h, w))))
    rec["drawInstance"] = np.where(rng.uniform(0.0, 1.0, (h, w)) < uncovered, FR.NO_SURFACE, rng.integers(0, 5, (h, w)))
    rec["primitive"] = rng.integers(0, 100, (h, w))
    return rec


def test_the_restatement_is_the_transparent_restatement_on_the_same_records(oracle):
    world = scenes.cornell()
    w, h = 24, 16
    cam = camera(oracle, world, w, h)
    rec = hand_made_records(np.random.default_rng(19), h, w)
    covered = FR.covered_of(rec)
    assert covered.any() and not covered.all()
    rgba, total, margin = FR.shade(world, cam, rec)
    py, px = np.mgrid[0:h, 0:w]
    want, wtotal, wmargin = T.shade(world, cam, T.LayerSurfaces(cam, rec[covered], px[covered], py[covered]))
    assert np.array_equal(rgba[covered][:, :3], want) and np.array_equal(total[covered], wtotal) and np.array_equal(margin[covered], wmargin)
    assert (want != 0.0).any()
    # the clear values (ForwardRenderer.cpp:574-604) and the alpha rule (forward.frag:83,118)
    assert not rgba[~covered].any() and not total[~covered].any() and np.isinf(margin[~covered]).all()
    a = rec["alpha"][covered].astype(np.float64)
    assert np.array_equal(rgba[covered][:, 3], np.where(a > 0.0, a, 1.0))
    assert FR.alpha_of(-1.0) == 1.0 and FR.alpha_of(0.0) == 1.0 and FR.alpha_of(0.25) == 0.25 and FR.alpha_of(1.0) == 1.0
    assert FR.CLEAR == (0.0, 0.0, 0.0, 0.0)


def test_the_restatement_over_a_rebuilt_surface_is_the_deferred_restatement(oracle):
    """Records built from a G-buffer the way deferred shading rebuilds its surface shade to deferred_shading_reference's
    image, within the shading tolerance (the records hold float32; zCam comes from worldToCamera, not the depth), with
    alpha 1 where deferred shading writes alpha 1; and the cluster lookup is the same one, over given lists."""
    world = scenes.cornell()
    w, h = 24, 16
    cam, fl, osc, ar, nm, depth, _ = R.make_gbuffer(oracle, world, w, h)
    rec = FR.records_of_gbuffer(cam, ar, nm, depth)
    hit = depth != 0.0
    assert hit.any() and np.array_equal(FR.covered_of(rec), hit)
    visible, _ = D.clusters(world, cam, w, h)
    spots = np.ones(visible.shape[:3] + (world.spot_lights.count,), bool)
    for lists in (None, (visible, spots)):
        want, total, _ = D.shade(world, cam, ar, nm, depth, lists=lists)
        got, gtotal, _ = FR.shade(world, cam, rec, lists=lists)
        err = np.abs(got[..., :3] - want).max(-1)
        assert (err[hit] <= REL * total[hit] + ABS).all(), err[hit].max()
        assert (got[..., 3][hit] == 1.0).all() and not got[~hit].any()


def test_the_three_draw_type_branches():
    rng = np.random.default_rng(3)
    h, w = 6, 9
    rec = hand_made_records(rng, h, w)
    covered = FR.covered_of(rec)
    meshlet, local = rng.integers(0, 4000, (h, w)), rng.integers(0, 124, (h, w))
    dbg = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    m = FR.debug_image(S.DrawType["MeshletID"], rec, meshlet=meshlet, local=local, debug_color=dbg)
    p = FR.debug_image(S.DrawType["PrimitiveID"], rec, meshlet=meshlet, local=local, debug_color=dbg)
    assert np.array_equal(m[covered][:, :3], FR.uint_to_color(meshlet[covered])) and np.array_equal(p[covered][:, :3], FR.uint_to_color(local[covered]))
    assert not np.array_equal(m, p)
    for dt in range(1, len(S.DRAW_TYPES)):
        if dt in (S.DrawType["MeshletID"], S.DrawType["PrimitiveID"]):
            continue
        o = FR.debug_image(dt, rec, meshlet=meshlet, local=local, debug_color=dbg)
        assert np.array_equal(o[covered][:, :3], dbg[covered]), S.DRAW_TYPES[dt]
    for o in (m, p, o):
        assert (o[covered][:, 3] == 1.0).all() and not o[~covered].any()
    with pytest.raises(AssertionError):
        FR.debug_image(S.DrawType["Default"], rec)
    # uintToColor is the one tests/test_raster_resolve.py checks the resolve against: spot values of the hash
    assert FR.uint_to_color(np.array([0, 1])).shape == (2, 3) and (FR.uint_to_color(np.arange(64)) <= 1.0).all()
    assert len(np.unique(FR.uint_to_color(np.arange(64)).view(np.uint32), axis=0)) == 64


def blend_twin(world):
    """the same world with every material BLEND with alpha factor 1: what the transparent pass draws in place of the opaque one"""
    for m in world.materials:
        m.alphaMode = S.ALPHA_MODE_BLEND
        m.baseColorFactor.w = 1.0
    world._frozen = None
    return world


def test_the_twin_scene_stays_within_the_raster_against_traced_cap(oracle):
    """The condition the bit-exact twin test of tests/test_forward_opaque.py inherits: on the closed scene at 96 x 64 under
    the jittered camera of that test, the rasteriser's restatement and the oracle's traversal of the pixels' own rays
    (centre minus currentJitter / 2) name another triangle on at most 2 % of the pixels (tests/test_raster_cpu.py's cap);
    and the twin has the same geometry, so the same ids."""
    from test_raster_resolve import jittered_camera
    width, height = 96, 64
    world = RS.closed_world()
    cam = jittered_camera()
    ids, _ = RR.decode(world, RR.rasterise(world, cam, CR.generate(world, CR.MODE_OPAQUE))["keys"])
    got = RR.geometry_ids(world, ids)
    w2c, c2c = CR.mat4_of(cam.worldToCamera).astype(np.float64), CR.mat4_of(cam.cameraToClip).astype(np.float64)
    eye = np.array([cam.eye.x, cam.eye.y, cam.eye.z], np.float64)
    right, up, fwd = w2c[0, :3], w2c[1, :3], -w2c[2, :3]
    py, px = np.mgrid[0:height, 0:width]
    ndx = (px + 0.5) / width * 2.0 - 1.0 - cam.currentJitter[0]
    ndy = (py + 0.5) / height * 2.0 - 1.0 - cam.currentJitter[1]
    d = ndx[..., None] * (right / c2c[0, 0]) + ndy[..., None] * (up / c2c[1, 1]) + fwd
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    want = np.full((height, width, 2), -1, np.int64)
    osc = oracle.OracleScene(world, brute_force=True)
    try:
        for y in range(height):
            for x in range(width):
                hit, di, prim, _ = osc.trace_closest(eye, d[y, x])
                if hit:
                    want[y, x] = (di, prim)
    finally:
        osc.close()
    covered = got[..., 0] >= 0
    differ = (got != want).any(axis=2)
    print("closed scene, jittered: %d of %d pixels differ, %d covered" % (differ.sum(), differ.size, covered.sum()))
    assert covered.mean() > 0.15 and differ.mean() <= 0.02
    twin = blend_twin(RS.closed_world())
    assert all(m.alphaMode == S.ALPHA_MODE_BLEND for m in twin.materials)
    assert np.array_equal(np.concatenate(twin.freeze()["geometry_buffers"][0:1]), np.concatenate(world.freeze()["geometry_buffers"][0:1]))
