#!/usr/bin/env python3
"""glTF/GLB -> path-traced PNG on one MI355X, end to end through the C-ABI:

    python scripts/render_gltf.py scene.gltf --spp 64 --size 1280x720 --out out.png \\
        [--lut res/texture/tony_mc_mapface.dds] [--env env/sky.ktx] [--eye x,y,z --target x,y,z]

glTF ingest (prosper_amd/gltf.py) -> prosper_pt_upload_scene -> prosper_pt_render_frames -> prosper_pt_tone_map
(Tony McMapface LUT when given, otherwise an identity LUT, i.e. plain x/(x+1) + gamma) -> PNG.

    --restir-di [--no-spatial]   direct illumination instead: --spp accumulated frames of prosper_pt_restir_di_record
                                 over the jittered ray-traced G-buffer it traces first (PROSPER_PT_RESTIR_TRACE_GBUFFER)
    --deferred                   prosper's default lighting instead: the pixel-centre ray-traced G-buffer, light
                                 clustering and deferred shading (prosper_pt_deferred_shading with
                                 PROSPER_PT_DEFERRED_TRACE_GBUFFER), unshadowed, one frame
    --deferred --ibl             with the image-based lighting term: the irradiance / radiance maps and the BRDF LUT
                                 are generated once from the sky (prosper_pt_generate_ibl), then the frame is shaded
    --deferred --sky             prosper_pt_skybox_fill after the shading: the sky wherever the G-buffer's ray missed
    --deferred --transparents    prosper's transparent pass: the G-buffer leaves BLEND surfaces out
                                 (PROSPER_PT_GBUFFER_OPAQUE_ONLY) and prosper_pt_forward_transparent blends them, lit
                                 forward over the light clusters, over the shaded image after --sky and before --bloom
                                 (Renderer.cpp:493-500), through the host layer's ForwardRenderer; under --taa along the
                                 camera-jittered ray.  With --forward or --deferred --raster the transparents are
                                 rasterised too (prosper_pt_raster_forward_transparent): the TRANSPARENT
                                 draw list, per-pixel fragment lists, sorted and blended against the rasteriser's depth
    --deferred --debug-lines [--debug-frustum]
                                 prosper's DebugRenderer (prosper_pt_debug_lines) between the transparents and bloom
                                 (Renderer.cpp:502): the axes of the point and spot lights as the device holds them
                                 (prosper_pt_read_lights, so lights moved by --time show where they are), 0.2 long in
                                 red / green / blue, depth-tested against the traced G-buffer; --debug-frustum adds the
                                 glTF camera's own frustum in white, to look at from an --eye / --target elsewhere
    --deferred --bloom [--bloom-threshold T] [--bloom-quarter] [--bloom-fft]
                                 prosper_pt_bloom over the (filled) image, through the host layer's Bloom with prosper's
                                 defaults: after --sky and before --dof, which is prosper's order (Renderer.cpp:516-573);
                                 --bloom-fft: the FFT technique (prosper_pt_bloom_fft) instead of the multi-resolution blur
    --deferred --particles [--particle-source N] [--particle-steps K]
                                 prosper's particle system (prosper_pt_particles) between bloom and TAA
                                 (Renderer.cpp:530-538): one emitter per vertex of draw instance N's mesh (default 0), K
                                 steps (default 120) at 1/60 s of decay / simulate before the first frame, then every
                                 frame one more step and the quads drawn into the image and the depth, which TAA and
                                 depth of field then read
    --deferred --taa [--frames N]
                                 temporal anti-aliasing: N frames (8, one Halton cycle) of jittered camera -> velocity
                                 G-buffer -> shading -> sky -> bloom -> prosper_pt_taa_resolve -> Camera::endFrame, through
                                 the host layer's GBufferTracer and TemporalAntiAliasing; depth of field and the tone map
                                 run after the last frame (Renderer.cpp:516-573's order)
    --time T [--time-step DT]    an animated glTF at T seconds: its nodes and channels go to the library
                                 (prosper_amd/animation.py -> prosper_pt_set_animations) and prosper_pt_animate(T) runs on
                                 the GPU ahead of the refit, before anything is rendered; the camera node's animated pose is
                                 the camera unless --eye / --target are given.  Under --taa every jittered frame advances
                                 the time by DT (default 1/60 s) and hands its table to the velocity target
    --denoise [--denoise-frames N] [--spp 1] [--time T [--time-step DT]]
                                 the path-traced mode for a moving scene: N frames (8) of --spp samples, each rendered afresh
                                 (PROSPER_PC_FLAG_SKIP_HISTORY), preceded by prosper_pt_trace_gbuffer_velocity with the previous
                                 frame's transforms (prosper_pt_read_animated_transforms, which = 1) and followed by
                                 prosper_pt_denoise; with --time every frame advances the animation by DT.  The PNG is the
                                 last frame through the tone map
    --deferred --sky --dof --aperture A --focus D
                                 prosper_pt_depth_of_field over the filled image, through the host layer's DepthOfField:
                                 aperture diameter A and focus distance D in scene units drive the push constants
    --deferred --sky --dof --focus-at X,Y
                                 prosper's click-to-focus (App.cpp:583-631): the focus distance is that of the surface
                                 under pixel (X, Y), from the depth texel prosper_pt_texture_readback hands back
                                 (prosper_amd/debug_geometry.py focus_distance_from_depth)
    --deferred ... --debug-view NAME[:LOD] [--debug-channel r|g|b|a|rgb] [--debug-range LO,HI] [--debug-abs]
                   [--debug-bilinear] [--debug-zoom]
                                 prosper's texture viewer (prosper_pt_texture_debug): the PNG is level LOD of the registry
                                 image NAME through these settings instead of the tone map's output, as Renderer.cpp:621-640
                                 replaces the final composite
    --deferred --raster          the G-buffer by prosper_pt_raster_gbuffer in place of the traced one: meshlets
                                 are built for the loaded scene, both culling phases run on the rasteriser's own depth, the
                                 resolve fills the context's targets; composes with --sky --ibl --bloom --taa --dof
                                 --texture-lod --cull-stats; --draw-type MeshletID / PrimitiveID show the mesh shader's ids.
    --forward                    prosper's forward path in place of --deferred's G-buffer and shading:
                                 prosper_pt_raster_forward - meshlets are built for the loaded scene, both culling phases run
                                 on the rasteriser's own depth, and every pixel's winning triangle is shaded directly over
                                 the light clusters into the image, with the depth and the velocity the later passes read;
                                 composes with --ibl --sky --bloom --particles --taa --dof --texture-lod --draw-type
                                 --cull-stats --debug-lines exactly as --deferred --raster does; not with --deferred or
                                 --restir-di
    --deferred --cull-stats      prosper's visibility system: meshlets are built for the loaded scene
                                 (World.add_meshlets), prosper_pt_cull_gbuffer runs after the G-buffer of each frame - first
                                 phase against the previous frame's depth pyramid, the pyramid of this frame's depth, second
                                 phase - and the frame's DrawStats are printed
    --deferred ... --list-debug-views
                                 after the frame, the registry of the context's 2-D images (prosper_pt_get_debug_resource):
                                 index, name, format, extent and levels of what each pass left
"""
import argparse
import math
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def write_png(path, rgba):
    h, w, _ = rgba.shape
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("gltf")
    ap.add_argument("--out", default="out.png")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--lut", default=None, help="tony_mc_mapface.dds (3-D R9G9B9E5 DDS)")
    ap.add_argument("--env", default=None, help="RGBA16F cube map (.ktx, KTX 1.1): enables IBL")
    ap.add_argument("--eye", default=None)
    ap.add_argument("--target", default=None)
    ap.add_argument("--exposure", type=float, default=1.0)
    ap.add_argument("--restir-di", action="store_true", help="ReSTIR-DI direct illumination from a traced G-buffer")
    ap.add_argument("--no-spatial", action="store_true", help="with --restir-di: no spatial reuse")
    ap.add_argument("--deferred", action="store_true", help="clustered deferred shading of a traced G-buffer")
    ap.add_argument("--ibl", action="store_true", help="with --deferred: add image-based lighting from the sky")
    ap.add_argument("--sky", action="store_true", help="with --deferred: fill the sky where the G-buffer's ray missed")
    ap.add_argument("--transparents", action="store_true", help="with --deferred: BLEND surfaces through the forward transparent pass")
    ap.add_argument("--debug-lines", action="store_true", help="with --deferred: the lights' axes as depth-tested debug lines")
    ap.add_argument("--debug-frustum", action="store_true", help="with --deferred: the glTF camera's frustum as debug lines")
    ap.add_argument("--bloom", action="store_true", help="with --deferred: bloom (multi-resolution blur) over the shaded image")
    ap.add_argument("--bloom-threshold", type=float, default=1.0, help="with --bloom: what is subtracted from the highlights")
    ap.add_argument("--bloom-quarter", action="store_true", help="with --bloom: quarter resolution instead of half")
    ap.add_argument("--bloom-fft", action="store_true", help="with --bloom: the FFT technique instead of the multi-resolution blur")
    ap.add_argument("--particles", action="store_true", help="with --deferred: the particle system, between bloom and TAA")
    ap.add_argument("--particle-source", type=int, default=0, help="with --particles: the draw instance whose vertices emit")
    ap.add_argument("--particle-steps", type=int, default=120, help="with --particles: steps of 1/60 s before the first frame")
    ap.add_argument("--taa", action="store_true", help="with --deferred: temporal anti-aliasing over jittered frames")
    ap.add_argument("--texture-lod", action="store_true",
                    help="with --deferred: the G-buffer samples material textures through mip chains (bias -1 under --taa)")
    ap.add_argument("--frames", type=int, default=8, help="with --taa: frames to resolve (8 is one Halton cycle)")
    ap.add_argument("--dof", action="store_true", help="with --deferred: depth of field over the shaded image")
    ap.add_argument("--aperture", type=float, default=0.02, help="with --dof: aperture diameter in scene units")
    ap.add_argument("--focus", type=float, default=None, help="with --dof: focus distance (default: eye to target)")
    ap.add_argument("--focus-at", default=None, metavar="X,Y",
                    help="with --dof: focus on the surface under this pixel instead of --focus (prosper's click-to-focus)")
    ap.add_argument("--list-debug-views", action="store_true",
                    help="with --deferred: print the registry of the context's images after the frame")
    ap.add_argument("--debug-view", default=None, metavar="NAME[:LOD]",
                    help="with --deferred: the PNG is the texture viewer's output over this registry image instead of the tone map's")
    ap.add_argument("--debug-channel", default="rgb", choices=("r", "g", "b", "a", "rgb"), help="with --debug-view: the channel shown")
    ap.add_argument("--debug-range", default="0,1", metavar="LO,HI", help="with --debug-view: the values mapped to black and white")
    ap.add_argument("--debug-abs", action="store_true", help="with --debug-view: the absolute value before the range")
    ap.add_argument("--debug-bilinear", action="store_true", help="with --debug-view: the bilinear sampler instead of nearest")
    ap.add_argument("--debug-zoom", action="store_true", help="with --debug-view: the middle of the image four times larger")
    ap.add_argument("--raster", action="store_true", help="with --deferred: the G-buffer by prosper_pt_raster_gbuffer (meshlets, both culling phases, "
                    "the compute rasteriser and its resolve) in place of the traced one")
    ap.add_argument("--forward", action="store_true", help="the forward path (prosper_pt_raster_forward) in place of --deferred's G-buffer and shading; "
                    "implies the rasteriser and meshlets")
    ap.add_argument("--draw-type", default="Default", choices=["Default", "PrimitiveID", "MeshletID", "MeshID", "MaterialID", "Position", "ShadingNormal", "TexCoord0", "Albedo",
                             "Roughness", "Metallic"],
                    help="with --raster: the G-buffer's draw type (MeshletID and PrimitiveID are the mesh shader's), shaded as that debug view")
    ap.add_argument("--cull-stats", action="store_true", help="with --deferred: meshlet culling after each frame's G-buffer, DrawStats printed")
    ap.add_argument("--denoise", action="store_true", help="the path-traced mode: --spp samples per frame (think 1), each frame through "
                    "prosper_pt_denoise over a traced velocity G-buffer; with --time every frame advances the animation by --time-step")
    ap.add_argument("--denoise-frames", type=int, default=8, help="with --denoise: frames to render; the PNG is the last one")
    ap.add_argument("--time", type=float, default=None, help="evaluate the glTF's animations at this time (seconds) before rendering")
    ap.add_argument("--gpu-hierarchy", nargs="?", const="linear", default=None, metavar="linear|ploc[:radius]",
                    help="build the hierarchy once more on the GPU after the upload (and after --time's pose), the same image: "
                         "a linear BVH (the default), or ploc[:radius] for the PLOC method with a search radius of 1 .. 32")
    ap.add_argument("--gpu-first-tree", nargs="?", const="linear", default=None, metavar="linear|ploc[:radius]",
                    help="build the scene's first tree on the GPU, inside the upload (site UPLOAD of "
                         "prosper_pt_set_gpu_hierarchy_sites): no host build, the same image")
    ap.add_argument("--time-step", type=float, default=1.0 / 60.0, help="with --time and --taa: seconds per jittered frame")
    ap.add_argument("--build-texture-cache", action="store_true",
                    help="compress every image whose prosper_cache file is missing or stale (GPU BC7 encoder) before loading")
    ap.add_argument("--build-mesh-cache", action="store_true",
                    help="prepare every primitive whose prosper_cache mesh file is missing or stale (tangents, meshlets and packing "
                         "on the GPU), then load the meshes from those files")
    args = ap.parse_args()
    if args.forward and (args.deferred or args.restir_di):
        ap.error("--forward is the forward path: it does not go with --deferred or --restir-di")
    if args.forward:
        # what follows the opaque image is --deferred --raster's: the same passes over the same "last" depth and velocity
        args.deferred = args.raster = True
    if args.bloom_fft and not args.bloom:
        ap.error("--bloom-fft belongs to --bloom")
    if (args.sky or args.dof or args.bloom or args.taa or args.transparents or args.particles or args.debug_lines
            or args.debug_frustum or args.debug_view or args.list_debug_views or args.cull_stats or args.raster) and not args.deferred:
        ap.error("--sky, --transparents, --debug-lines, --debug-frustum, --bloom, --particles, --taa, --cull-stats and --dof belong to --deferred")
    if args.focus_at and not args.dof:
        ap.error("--focus-at belongs to --dof")
    if args.frames < 1:
        ap.error("--frames must be at least 1")
    from prosper_amd import capi, dds, gltf, ktx, structs as S
    from prosper_amd.rt_reference import Bloom, Camera, DepthOfField, ForwardRenderer, GBufferTracer, TemporalAntiAliasing
    w, h = (int(v) for v in args.size.lower().split("x"))
    if args.build_texture_cache:
        from prosper_amd import texture_cache
        builder = capi.Context(0)
        for cached in texture_cache.build_for_gltf(args.gltf, builder):
            print("texture cache: wrote %s" % cached)
        builder.close()
    if args.build_mesh_cache:
        from prosper_amd import mesh_cache
        builder = capi.Context(0)
        for cached in mesh_cache.build_for_gltf(builder, args.gltf):
            print("mesh cache: wrote %s" % cached)
        builder.close()
    # prosper_cache BC7 files are decoded by the library at upload; with --texture-lod their mip levels go along
    world = gltf.load_gltf(args.gltf, bc7_on_gpu=True, mip_chains=args.texture_lod, use_mesh_cache=args.build_mesh_cache)
    if world.missing_images:
        print("missing images replaced by white: %s" % ", ".join(world.missing_images), file=sys.stderr)
    if args.env:
        world.skybox = ktx.read_cube(args.env)
    gltf_camera = dict(world.camera)  # before --eye / --target: what --debug-frustum draws
    if args.eye:
        world.camera["eye"] = tuple(float(v) for v in args.eye.split(","))
    if args.target:
        world.camera["target"] = tuple(float(v) for v in args.target.split(","))
    if args.raster and args.time is not None:
        ap.error("--raster does not take --time yet (the animated tables' previous frame is the tracer's to keep)")
    if args.draw_type != "Default" and not args.raster:
        ap.error("--draw-type belongs to --raster")
    if args.cull_stats or args.raster:
        print("meshlets: %d over %d meshes" % (world.add_meshlets(), len(world.metadatas)))
    ctx = capi.Context(0, flags=S.CREATE_TEXTURE_MIPS if args.texture_lod else 0)

    def gpu_method(option, text):
        method, _, radius = text.partition(":")
        if method not in ("linear", "ploc") or (radius and (method != "ploc" or not radius.isdigit())):
            ap.error("%s takes linear or ploc[:radius]" % option)
        ctx.set_gpu_hierarchy_method(S.GPU_HIERARCHY_PLOC if method == "ploc" else S.GPU_HIERARCHY_LINEAR, int(radius or 0))

    def print_gpu_build(what):
        info, how = ctx.hierarchy_build_info(), ctx.gpu_hierarchy_method_info()
        if how.method == S.GPU_HIERARCHY_PLOC:
            print("%s: PLOC, radius %d, %d rounds (%d of them in one workgroup)" % (what, how.radius, how.rounds, how.finishRounds),
                  file=sys.stderr)
        print("%s: %d nodes, %d levels, stack bound %d, leaves of at most %d, %.3f ms on the device (%s)" % (
            what, info.nodeCount, info.levels, info.stackBound, info.leafSize, info.totalMs,
            ", ".join("%s %.3f" % (n, ms) for n, ms in zip(S.HIERARCHY_BUILD_STAGE_NAMES, info.stageMs))), file=sys.stderr)

    if args.gpu_first_tree:
        gpu_method("--gpu-first-tree", args.gpu_first_tree)
        ctx.set_gpu_hierarchy_sites(S.GPU_BUILD_SITE_UPLOAD)
    ctx.upload_scene(world)
    st = ctx.scene_stats()
    if args.gpu_first_tree and ctx.hierarchy_build_info().builder == S.BUILDER_GPU:  # (a scene without triangles: the host's root)
        print_gpu_build("GPU first tree (stage 'bounds' is the one pass over the geometry)")
    if args.time is not None:
        from prosper_amd import animation
        ctx.set_animations(animation.load_animations(args.gltf))
        ctx.animate(args.time)
        pose = ctx.animation_state()
        print("animation: %d of %d nodes animated, end time %.3f s, evaluated at %.3f s" % (
            pose.animatedNodeCount, pose.nodeCount, pose.endTimeS, args.time), file=sys.stderr)
        if pose.cameraValid and not args.eye and not args.target:
            world.camera.update(eye=tuple(pose.eye), target=tuple(pose.target), up=tuple(pose.up))
    if args.gpu_hierarchy:
        gpu_method("--gpu-hierarchy", args.gpu_hierarchy)
        ctx.build_hierarchy_gpu()  # (flushes the pose --time staged first)
        print_gpu_build("GPU hierarchy")
    hcam = Camera.from_world(world, w, h)
    if args.dof:
        c = world.camera
        focus = args.focus or math.dist(c["eye"], c["target"])
        hcam.set_parameters(c["fov"], c["zN"], c["zF"], args.aperture, focus)
    cam, focal = hcam.update_buffer()
    flags = S.PC_FLAG_ACCUMULATE | S.PC_FLAG_CLAMP_INDIRECT | S.PC_FLAG_SKIP_HISTORY | (S.PC_FLAG_IBL if args.env else 0)
    samples = None  # (--denoise renders more than --spp)
    if args.deferred:
        import time
        if args.ibl:
            ctx.generate_ibl()  # once per sky, before the first frame that applies IBL (Renderer.cpp:380-382)
        t0 = time.perf_counter()
        bloom = Bloom(ctx, technique=S.BLOOM_FFT if args.bloom_fft else S.BLOOM_MULTI_RESOLUTION_BLUR) if args.bloom else None
        if bloom:
            bloom.draw_ui(threshold=args.bloom_threshold, resolution_scale=S.BLOOM_QUARTER if args.bloom_quarter else S.BLOOM_HALF)
        forward = ForwardRenderer(ctx) if args.transparents else None
        tracer = GBufferTracer(ctx)
        tracer.set_opaque_only(args.transparents)  # the BLEND surfaces are the transparent pass's
        if args.texture_lod:
            from prosper_amd.rt_reference import renderer_lod_bias
            tracer.set_texture_lod(True, renderer_lod_bias(args.taa))  # Renderer::lodBias(): -1 while TAA is on
            if forward:
                forward.set_texture_lod(True, renderer_lod_bias(args.taa))
            if args.forward:
                ctx.set_texture_lod(True, renderer_lod_bias(args.taa))  # the rasteriser's discard and the shade read the context's state
        if args.taa:
            hcam.set_jitter(True)
            taa = TemporalAntiAliasing(ctx)
            transforms = world.freeze()["transforms"]
        frustum = None
        if args.debug_frustum:
            from prosper_amd import debug_geometry
            own = Camera()
            own.set_parameters(gltf_camera["fov"], gltf_camera["zN"], gltf_camera["zF"])
            own.look_at(gltf_camera["eye"], gltf_camera["target"], gltf_camera["up"])
            own.update_resolution(w, h)
            frustum = debug_geometry.frustum_lines(debug_geometry.frustum_corners(own.update_buffer()[0]), (1.0, 1.0, 1.0))
        particle_step = 0
        if args.particles:
            # Particles::record without its render, K times: the reset step makes the emitters, the rest ages them
            for particle_step in range(1, args.particle_steps + 1):
                ppc = S.ParticlesPC(0, args.particle_source, 1 if particle_step == 1 else 0, 1.0 / 60.0, particle_step, 0)
                ctx.particles(ppc, S.PARTICLES_DECAY | S.PARTICLES_INIT | S.PARTICLES_SIMULATE)
        for frame in range(args.frames if args.taa else 1):
            if args.raster:
                # GBufferRenderer::record: the culled lists drawn by the compute rasteriser, resolved into the context's
                # own targets, which every pass below then reads as the last G-buffer (and TAA its velocity)
                if args.taa:
                    cam, focal = hcam.update_buffer()
                # (this frame's table is the next frame's previous one; the first frame sees unmoved instances)
                if args.forward:
                    # ForwardRenderer::recordOpaque: the same lists and draws, shaded without a G-buffer in between
                    ctx.raster_forward(cam, draw_type=S.DrawType[args.draw_type], ibl=1 if args.ibl else 0,
                                       previous_transforms=transforms if args.taa and frame else None)
                else:
                    ctx.raster_gbuffer(cam, draw_type=S.DrawType[args.draw_type], previous_transforms=transforms if args.taa and frame else None)
                    g, _, _ = ctx.gbuffer_device_ptrs()
                    ctx.deferred_shading_device(cam, w, h, g.albedoRoughness, g.normalMetallic, g.nonLinearDepth,
                                                draw_type=S.DrawType[args.draw_type], ibl=1 if args.ibl else 0)
                if args.cull_stats:
                    ds = ctx.draw_stats()
                    print("frame %d DrawStats: drawn meshlets %d of %d, rasterized triangles %d of %d, meshes %d, models %d" % (
                        frame, ds.drawnMeshletCount, ds.totalMeshletCount, ds.rasterizedTriangleCount, ds.totalTriangleCount,
                        ds.totalMeshCount, ds.totalModelCount))
            elif args.taa:
                if args.time is not None and frame:
                    # the scene moves on; this frame's table is the next frame's previous one (the tracer keeps it)
                    ctx.animate(args.time + frame * args.time_step)
                    pose = ctx.animation_state()
                    if pose.cameraValid and not args.eye and not args.target:
                        hcam.look_at(tuple(pose.eye), tuple(pose.target), tuple(pose.up))
                if args.time is not None:
                    transforms = ctx.read_animated_transforms()
                # the G-buffer through the jittered projection's pixel centres, with the velocity the resolve reads
                cam, focal = hcam.update_buffer()
                g, _ = tracer.record_velocity(hcam, w, h, frame_index=frame, transforms=transforms)
                ctx.deferred_shading_device(cam, w, h, g.albedoRoughness, g.normalMetallic, g.nonLinearDepth, ibl=1 if args.ibl else 0)
            elif args.transparents:
                g = tracer.record(hcam, w, h, jitter=False)
                ctx.deferred_shading_device(cam, w, h, g.albedoRoughness, g.normalMetallic, g.nonLinearDepth, ibl=1 if args.ibl else 0)
            else:
                ctx.deferred_shading_traced(cam, w, h, ibl=1 if args.ibl else 0)
            if args.cull_stats and not args.raster:
                # GBufferRenderer::record's culling around this frame's depth (the previous frame's pyramid is kept)
                ctx.cull_gbuffer(cam)
                ds = ctx.draw_stats()
                print("frame %d DrawStats: drawn meshlets %d of %d, rasterized triangles %d of %d, meshes %d, models %d" % (
                    frame, ds.drawnMeshletCount, ds.totalMeshletCount, ds.rasterizedTriangleCount, ds.totalTriangleCount,
                    ds.totalMeshCount, ds.totalModelCount))
            if args.sky:
                ctx.skybox_fill(cam, w, h)  # before the lens: a silhouette against an empty background blurs towards black
            if forward and args.raster:
                # the raster frame's transparents: the TRANSPARENT draw list culled once, listed per pixel and
                # resolved over the sky-filled image against the rasteriser's own depth; ibl = 0, as prosper draws them
                forward.record_transparent_raster(hcam, w, h)
            elif forward:
                # over the sky-filled image, along the ray the G-buffer was traced with; ibl = 0, as prosper draws them
                forward.record_transparent(hcam, w, h, ray_flags=S.TRANSPARENT_CAMERA_JITTER if args.taa else 0, frame_index=frame)
            if args.debug_lines or frustum is not None:
                # App::updateDebugLines, then DebugRenderer::record in place over the illumination and the depth
                from prosper_amd import debug_geometry
                debug = debug_geometry.DebugLines()
                if args.debug_lines:
                    _, points, spots = ctx.read_lights()
                    debug.extend(debug_geometry.light_axes_from_buffers(points, spots))
                if frustum is not None:
                    debug.extend(frustum)
                ctx.debug_lines(debug.array(), cam, w, h)
            if bloom:
                bloom.record(w, h)  # in place
            if args.particles:
                # in place over the illumination and the traced G-buffer's depth (Renderer.cpp:530-538)
                particle_step += 1
                ppc = S.ParticlesPC(0, args.particle_source, 1 if particle_step == 1 else 0, 1.0 / 60.0, particle_step, particle_step % 64)
                ctx.particles(ppc, S.PARTICLES_ALL, cam, w, h)
            if args.taa:
                taa.record(w, h)  # in place, over the traced velocity and depth
                hcam.end_frame()
        if bloom and args.bloom_fft:
            info = ctx.bloom_fft_info()
            print("bloom (FFT): threshold %.3f, transform %dx%d, kernel image %dx%d" % (
                args.bloom_threshold, info.dim, info.dim, info.kernelDim, info.kernelDim), file=sys.stderr)
        elif bloom:
            info = ctx.bloom_info()
            print("bloom: threshold %.3f, working extent %dx%d, streak half-width %d" % (
                args.bloom_threshold, info.workingWidth, info.workingHeight, info.streakHalfWidth), file=sys.stderr)
        if args.forward:
            ctx.read_hdr()  # (synchronises: the info never waits)
            info = ctx.forward_opaque_info() or S.ForwardOpaqueInfo()
            print("forward opaque: %d pixels shaded, last shade %.3f ms (kernel %.3f ms)" % (info.shadedPixels, info.ms, info.shadeMs), file=sys.stderr)
        if forward and args.raster:
            ctx.read_hdr()  # (synchronises: the info never waits)
            info = ctx.raster_transparent_info() or S.RasterTransparentInfo()
            print("transparents (rasterised): %d fragments in %d pixels, %d layers shaded, deepest %d; count %.3f + scan %.3f + fill %.3f + resolve %.3f ms" % (
                info.fragments, info.coveredPixels, info.shadedLayers, info.maxLayers, info.countMs, info.scanMs, info.fillMs, info.resolveMs), file=sys.stderr)
        elif forward:
            info = ctx.transparent_info()
            print("transparents: %d pixels with layers, %d layers, deepest %d, last pass %.3f ms" % (
                info.coveredPixels, info.totalLayers, info.maxLayers, info.ms), file=sys.stderr)
        if args.debug_lines or frustum is not None:
            info = ctx.debug_lines_info()
            print("debug lines: %d lines, %d clipped away, %d fragments written, %.3f ms" % (
                info.lineCount, info.linesClippedAway, info.fragmentsWritten, info.ms), file=sys.stderr)
        if args.particles:
            info = ctx.particles_info()
            print("particles: %d live of %d, %d fragments written, last step decay %.3f + simulate %.3f + render %.3f ms" % (
                info.liveCount, info.maxParticleCount, info.fragmentsWritten, info.decayMs, info.simulateMs, info.renderMs), file=sys.stderr)
        if args.taa:
            info = ctx.taa_info()
            print("taa: %d frames, last resolve %.3f ms + expand %.3f ms" % (args.frames, info.resolveMs, info.expandMs), file=sys.stderr)
        if args.focus_at:
            # prosper's click-to-focus (App.cpp:583-631): TextureReadback of the depth as it stands here, debug lines and
            # particles included, as Renderer.cpp:510 records it; prosper polls the value over the next frames, this waits
            from prosper_amd import debug_geometry
            px, py = (float(v) for v in args.focus_at.split(","))
            ctx.texture_readback("depth", px, py)
            ctx.read_hdr()  # (synchronises)
            texel = ctx.try_texture_readback()
            if texel is None or not texel[0] > 0.0:
                sys.exit("--focus-at %s: nothing but sky under that pixel" % args.focus_at)
            focus = float(debug_geometry.focus_distance_from_depth(cam, (px, py), (w, h), texel[0]))
            c = world.camera
            hcam.set_parameters(c["fov"], c["zN"], c["zF"], args.aperture, focus)
            print("focus at (%g, %g): depth %.6f, focus distance %.4f" % (px, py, texel[0], focus), file=sys.stderr)
        if args.dof:
            dpc = DepthOfField(ctx).record(hcam, w, h)  # in place over the traced G-buffer's depth
            print("depth of field: focus %.3f, maxBackgroundCoC %.2f half-resolution texels, gatherRadius %d tiles" % (
                dpc.focusDistance, dpc.maxBackgroundCoC, dpc.gatherRadius), file=sys.stderr)
        ctx.read_hdr()  # (synchronises)
        ms = (time.perf_counter() - t0) * 1e3
        args.spp = 1
        if args.list_debug_views:
            formats = ("RGBA32F", "RG32F", "R32F", "RGBA16F", "RG16F", "R16F", "RG16_UNORM", "RGBA8_UNORM")
            for i, r in enumerate(ctx.debug_resources()):
                print("%2d %-36s %-11s %s" % (i, r.name.decode(), formats[r.format], "%dx%d, %d level%s" % (
                    r.width, r.height, r.levelCount, "" if r.levelCount == 1 else "s") if r.valid else "(not valid: its pass has not run)"))
    elif args.restir_di:
        import time
        t0 = time.perf_counter()
        for frame in range(1, args.spp + 1):
            rpc = S.RestirTracePC(0, frame, (1 if frame == 1 else 0) | 2)  # skipHistory on the first, accumulate
            ctx.restir_di_record_traced(rpc, cam, w, h, spatial_reuse=not args.no_spatial)
        ctx.read_hdr()  # (synchronises)
        ms = (time.perf_counter() - t0) * 1e3
    elif args.denoise:
        # every frame: the scene moves on, the velocity G-buffer is traced against the previous frame's transforms, the frame is
        # rendered afresh (SKIP_HISTORY: no running mean over a moving scene) and denoised into the HDR image
        import time
        t0 = time.perf_counter()
        dpc = S.DenoisePC.default()
        for frame in range(args.denoise_frames):
            transforms = None
            if args.time is not None:
                if frame:
                    ctx.animate(args.time + frame * args.time_step)
                    pose = ctx.animation_state()
                    if pose.cameraValid and not args.eye and not args.target:
                        hcam.look_at(tuple(pose.eye), tuple(pose.target), tuple(pose.up))
                transforms = ctx.read_animated_transforms(previous=True)
            cam, focal = hcam.update_buffer()
            ctx.trace_gbuffer_velocity(cam, w, h, frame_index=frame, previous_transforms=transforms)
            pc = S.ReferencePC(0, flags, 1 + frame * args.spp, 1e-5, 1.0, focal, 3, min(args.bounces, 6))
            ctx.render(pc, cam, w, h, frames=args.spp)
            ctx.denoise(dpc, cam, w, h)
            hcam.end_frame()
        info = ctx.denoise_info()  # (synchronises)
        ms = (time.perf_counter() - t0) * 1e3
        samples = args.spp * args.denoise_frames  # per pixel, over every frame: what the closing line reports
        print("denoise: %d frames of %d spp; the last: %d pixels with a history, %d without, %.3f ms on the device" % (
            args.denoise_frames, args.spp, info.historyPixels, info.noHistoryPixels, info.totalMs), file=sys.stderr)
    else:
        pc = S.ReferencePC(0, flags, 1, 1e-5, 1.0, focal, 3, min(args.bounces, 6))
        ctx.set_kernel_timing(True)
        ctx.render(pc, cam, w, h, frames=args.spp)
        ms, _ = ctx.last_render_timing()
    if args.lut:
        lut = dds.read_lut(args.lut)
    else:
        g = np.linspace(0.0, 1.0, 48)
        b, gg, r = np.meshgrid(g, g, g, indexing="ij")
        lut = dds.encode_r9g9b9e5(np.stack([r, gg, b], axis=-1))
    ctx.set_tone_map_lut(lut)
    image = ctx.tone_map(args.exposure, 1.0)
    if args.debug_view:
        # TextureDebug::record, whose output replaces the final composite (Renderer.cpp:621-640)
        name, _, lod = args.debug_view.partition(":")
        lo, hi = (float(v) for v in args.debug_range.split(","))
        flags = ("r", "g", "b", "a", "rgb").index(args.debug_channel) | (S.TEXTURE_DEBUG_ABS_BEFORE_RANGE if args.debug_abs else 0) | (
            S.TEXTURE_DEBUG_ZOOM if args.debug_zoom else 0)
        image = ctx.texture_debug(name, (w, h), (lo, hi), int(lod or 0), flags, bilinear=args.debug_bilinear)
        print("debug view: %s, level %d, range %g..%g, channel %s" % (name, int(lod or 0), lo, hi, args.debug_channel), file=sys.stderr)
    write_png(args.out, image)
    print("%s: %d triangles, %dx%d x %d spp in %.1f ms (%.0f Mpaths/s) -> %s" % (
        os.path.basename(args.gltf), st.triangleCount, w, h, samples or args.spp, ms, w * h * (samples or args.spp) / ms / 1e3, args.out))
    ctx.close()


if __name__ == "__main__":
    main()
