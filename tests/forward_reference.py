"""NumPy restatement of the forward opaque pass (not a test module), for tests/test_forward_opaque.py and
tests/test_forward_opaque_cpu.py: forward.frag over the surface records the GPU's own debug read-back
reports (prosper_pt_read_forward_surfaces), in float64, as transparent_reference.py works over the layer records.

  shade(world, cam, surfaces, lists, maps)   the illumination of a [h, w] record image: forward.frag:69-83 on covered
                                             pixels, the clear value on the others
  alpha_of(material_alpha)                   forward.frag:83,118
  debug_image(draw_type, ...)                forward.frag:99-116: what the three draw-type branches write
  records_of_gbuffer(cam, ar, nm, depth)     records built from a G-buffer the way deferred shading rebuilds its surface

The lighting is transparent_reference.shade's (and with it deferred_shading_reference's cluster lookup): neither is edited.
"""
import numpy as np

import deferred_shading_reference as D
import restir_resampling_reference as R
import transparent_reference as T
from prosper_amd import structs as S

NO_SURFACE = 0xFFFFFFFF  # drawInstance of an uncovered pixel's record
CLEAR = (0.0, 0.0, 0.0, 0.0)  # ForwardRenderer.cpp:574-604: loadOp eClear, zero clear values (the depth's is 0 as well)
MESHLET_ID, PRIMITIVE_ID = S.DrawType["MeshletID"], S.DrawType["PrimitiveID"]


def uint_to_color(v):
    """common/random.glsl uintToColor: pcg, xor-shifted, three 10-bit fields"""
    v = np.asarray(v, np.uint64)
    state = (v * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    xr = (word >> np.uint64(22)) ^ word
    k = np.float32(1.0) / np.float32(1023.0)
    return np.stack([((xr >> np.uint64(20)) & np.uint64(0x3FF)).astype(np.float32) * k, ((xr >> np.uint64(10)) & np.uint64(0x3FF)).astype(np.float32) * k,
                     (xr & np.uint64(0x3FF)).astype(np.float32) * k], axis=-1)


def alpha_of(material_alpha):
    """forward.frag:83,118: the material's alpha where it is above 0 (BLEND and MASK surfaces carry theirs), else 1 (an
    opaque surface's alpha is -1)"""
    a = np.asarray(material_alpha, np.float64)
    return np.where(a > 0.0, a, 1.0)


def covered_of(surfaces):
    return surfaces["drawInstance"] != NO_SURFACE


def shade(world, cam, surfaces, lists=None, maps=None):
    """The Default draw type over a record image [h, w] (the dtype of structs.TransparentLayer).  Returns (rgba [h, w, 4]
    float64, the sum of the absolute terms [h, w], slice margin [h, w] - inf on uncovered pixels)."""
    h, w = surfaces.shape
    covered = covered_of(surfaces)
    py, px = np.mgrid[0:h, 0:w]
    rgba = np.empty((h, w, 4))
    rgba[...] = CLEAR
    total, margin = np.zeros((h, w)), np.full((h, w), np.inf)
    if covered.any():
        flat = surfaces[covered]
        sf = T.LayerSurfaces(cam, flat, px[covered], py[covered])
        color, tot, mar = T.shade(world, cam, sf, lists, maps)
        rgba[covered, :3] = color
        rgba[covered, 3] = alpha_of(flat["alpha"])
        total[covered], margin[covered] = tot, mar
    return rgba, total, margin


def debug_image(draw_type, surfaces, meshlet=None, local=None, debug_color=None):
    """forward.frag:99-116 for a draw type other than Default, float32 [h, w, 4]: MeshletID uintToColor(meshletIndex)
    (`meshlet` [h, w]), PrimitiveID the meshlet-local triangle (`local` [h, w]), every other type `debug_color` [h, w, 3]
    as given; alpha 1 on covered pixels, the clear value elsewhere."""
    assert draw_type != S.DrawType["Default"]
    covered = covered_of(surfaces)
    out = np.zeros(surfaces.shape + (4,), np.float32)
    if draw_type == MESHLET_ID:
        rgb = uint_to_color(np.where(covered, meshlet, 0))
    elif draw_type == PRIMITIVE_ID:
        rgb = uint_to_color(np.where(covered, local, 0))
    else:
        rgb = np.asarray(debug_color, np.float32)
    out[covered, :3] = rgb[covered]
    out[covered, 3] = 1.0
    return out


def records_of_gbuffer(cam, ar, nm, depth, alpha=-1.0):
    """Surface records [h, w] of a G-buffer, the surface rebuilt as deferred shading rebuilds it
    (restir_resampling_reference.Surfaces: the position from the depth through clipToWorld, the normal decoded from its
    octahedral encoding); a texel of depth 0 is uncovered."""
    h, w = depth.shape
    sf = R.Surfaces(cam, ar, nm, depth)
    out = np.zeros((h, w), np.dtype(S.TransparentLayer))
    out["positionWS"] = sf.pos.reshape(h, w, 3)
    out["normal"] = sf.n.reshape(h, w, 3)
    out["albedo"] = sf.albedo.reshape(h, w, 3)
    out["roughness"] = sf.rough.reshape(h, w)
    out["metallic"] = sf.metal.reshape(h, w)
    out["nonLinearDepth"] = depth
    out["alpha"] = alpha
    out["drawInstance"] = np.where(depth != 0.0, 0, NO_SURFACE)
    return out
