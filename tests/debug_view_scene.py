"""The designed scene the inspection passes' GPU tests share (a helper, like the *_reference.py files): one large quad at
distance 2 facing a camera at the origin, sky to its right, at 48 x 32, and one frame of the chain over it."""
import math

import numpy as np

from prosper_amd import scenes, structs as S

F = np.float32
W, H = 48, 32
FOV = math.radians(59.0)
FOCAL = (H / 2) / math.tan(FOV / 2)
QUAD_DISTANCE = 2.0
QUAD_RIGHT_EDGE = 0.8  # world x: about column 35; the columns right of it are sky


def quad_world():
    w = scenes.World()
    m = w.add_material(base_color=(0.8, 0.6, 0.4, 1.0), metallic=0.0, roughness=0.7)
    z = -QUAD_DISTANCE
    q = scenes._add(w, scenes.quad((-4.0, -4.0, z), (QUAD_RIGHT_EDGE, -4.0, z), (QUAD_RIGHT_EDGE, 4.0, z), (-4.0, 4.0, z)), m)
    w.add_instance(w.add_model([(q, m)]))
    w.add_point_light((1.0, 1.0, 1.0), 200.0, (0.5, 0.5, 0.0))
    return w


def camera(oracle, w=W, h=H):
    return oracle.camera_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), FOV, 0.1, 100.0, w, h)[0]


def frame(ctx, cam):
    """traced velocity G-buffer, deferred shading, sky, bloom (half), TAA, depth of field: once"""
    ctx.trace_gbuffer_velocity(cam, W, H)
    g, _, _ = ctx.gbuffer_device_ptrs()
    ctx.deferred_shading_device(cam, W, H, g.albedoRoughness, g.normalMetallic, g.nonLinearDepth)
    ctx.skybox_fill(cam, W, H)
    ctx.bloom(S.BloomPC.default(), W, H)
    ctx.taa_resolve(S.TaaPC.default(reset_history=1), W, H)
    ctx.depth_of_field(S.DofPC(QUAD_DISTANCE, 2.0, 4.0, 2), cam, W, H)


# the registry, in its order
NAMES = ["illumination", "albedoRoughness", "normalMetalness", "depth", "velocity", "SpecularBrdfLut",
         "HalfResIllumination", "HalfResCircleOfConfusion", "tileMinMaxCircleOfConfusion", "dilatedTileMinMaxCoC",
         "halfResFgBokehColorWeight", "halfResBgBokehColorWeight", "halfResFgBokehColorWeightFiltered",
         "halfResBgBokehColorWeightFiltered", "BloomWorkingImage", "BloomBlurPong", "BloomBlurred", "BloomFftHighlights",
         "BloomKernelImageCentered", "BloomKernelDft", "BloomFftConvolved", "previousResolvedIllumination", "toneMapped"]


def by_name(ctx):
    return {r.name.decode(): (i, r) for i, r in enumerate(ctx.debug_resources())}


def read_back(ctx, name, level=0):
    """the existing read-back call for the image the registry calls `name`"""
    gb = ("albedoRoughness", "normalMetalness", "depth")
    dof, bloom, fft = NAMES[6:14], NAMES[14:17], NAMES[17:21]
    if name == "illumination":
        return ctx.read_hdr()
    if name in gb:
        return ctx.read_gbuffer()[gb.index(name)]
    if name == "velocity":
        return ctx.read_velocity()
    if name == "SpecularBrdfLut":
        return ctx.read_ibl()["lut"]
    if name in dof:
        return ctx.read_dof_stage(dof.index(name), level)
    if name in bloom:
        first = 0 if name == "BloomWorkingImage" else ctx.bloom_info().firstLevel
        return ctx.read_bloom_stage(bloom.index(name), first + level)
    if name in fft:
        return ctx.read_bloom_fft_stage(fft.index(name))
    if name == "previousResolvedIllumination":
        return ctx.read_taa_history()
    raise KeyError(name)
