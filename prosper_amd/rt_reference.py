"""Python handles onto the C++ host layer (prosper_amd/csrc/host): `Camera`, `RtReference` and the passes beside it.

Same names, argument meaning and error behaviour as prosper's `scene::Camera`
(src/scene/Camera.hpp) and `render::RtReference` (src/render/RtReference.hpp:32-60); every call
goes through libprosper_pt.so (no Python re-implementation of the pass).
"""
import ctypes as C
import os

import numpy as np

from . import structs as S
from .capi import Context, ProsperPtError, RecordOptions, lib


class Camera:
    def __init__(self):
        self._h = C.c_void_p(lib().prosper_host_camera_create())
        if not self._h:
            raise MemoryError("prosper_host_camera_create failed")

    def close(self):
        if getattr(self, "_h", None):
            lib().prosper_host_camera_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def look_at(self, eye, target, up=(0.0, 1.0, 0.0)):
        f3 = C.c_float * 3
        lib().prosper_host_camera_look_at(self._h, f3(*eye), f3(*target), f3(*up))

    def set_parameters(self, fov, zN=0.1, zF=100.0, aperture_diameter=0.00001, focus_distance=1.0):
        lib().prosper_host_camera_set_parameters(self._h, fov, zN, zF, aperture_diameter, focus_distance)

    def update_resolution(self, width, height):
        lib().prosper_host_camera_update_resolution(self._h, width, height)

    def update_buffer(self):
        """Camera::updateBuffer -> (CameraUniforms, focalLength)"""
        u = S.CameraUniforms()
        fl = C.c_float()
        lib().prosper_host_camera_update_buffer(self._h, C.byref(u), C.byref(fl))
        return u, fl.value

    def changed_this_frame(self):
        return bool(lib().prosper_host_camera_changed_this_frame(self._h))

    def end_frame(self):
        lib().prosper_host_camera_end_frame(self._h)

    def set_jitter(self, apply_jitter):
        """Camera::setJitter: the TAA jitter of the Halton(2, 3) cycle in the projection from the next update_buffer on."""
        lib().prosper_host_camera_set_jitter(self._h, 1 if apply_jitter else 0)

    @classmethod
    def from_world(cls, world, width, height):
        cam = cls()
        c = world.camera
        cam.set_parameters(c["fov"], c["zN"], c["zF"])
        cam.look_at(c["eye"], c["target"], c["up"])
        cam.update_resolution(width, height)
        return cam


class RtReference:
    """render::RtReference: init / recompileShaders / drawUi / record / releasePreserved."""

    sMaxBounces = S.RT_MAX_BOUNCES

    class Options:
        def __init__(self, depthOfField=False, ibl=False, colorDirty=False, drawType="Default"):
            self.depthOfField = depthOfField
            self.ibl = ibl
            self.colorDirty = colorDirty
            self.drawType = drawType

    def __init__(self):
        self._h = None
        self._ctx = None
        self._world = None

    def init(self, device=0, flags=0):
        h = C.c_void_p()
        rc = lib().prosper_host_rt_reference_create(device, flags, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = Context(_borrowed=lib().prosper_host_rt_reference_context(h))

    def close(self):
        if self._h:
            lib().prosper_host_rt_reference_destroy(self._h)
            self._h = None
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def context(self):
        return self._ctx

    def set_world(self, world):
        """World::buildAccelerationStructures for this pass's GPU (App.cpp:573-578)."""
        view = world.view()
        rc = lib().prosper_host_rt_reference_set_scene(self._h, C.byref(view))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._world = world

    def recompile_shaders(self):
        lib().prosper_host_rt_reference_recompile_shaders(self._h)

    def draw_ui(self, accumulate=True, clampIndirect=True, rouletteStartBounce=3, maxBounces=S.RT_MAX_BOUNCES):
        lib().prosper_host_rt_reference_draw_ui(self._h, int(accumulate), int(clampIndirect), rouletteStartBounce,
                                                maxBounces)

    def record(self, camera, width, height, options=None, frame_count=1, tile=None, render_flags=0, stream=None):
        """Camera::updateBuffer + RtReference::record; returns the ReferencePC that was pushed."""
        options = options or RtReference.Options()
        o = RecordOptions(int(options.depthOfField), int(options.ibl), int(options.colorDirty),
                          S.DrawType[options.drawType] if isinstance(options.drawType, str) else int(options.drawType))
        pc = S.ReferencePC()
        rc = lib().prosper_host_rt_reference_record(
            self._h, camera._h, width, height, C.byref(o), frame_count, C.byref(tile) if tile is not None else None,
            render_flags, C.c_void_p(stream), C.byref(pc))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return pc

    def release_preserved(self):
        lib().prosper_host_rt_reference_release_preserved(self._h)


class RtDirectIllumination:
    """render::rtdi::RtDirectIllumination (csrc/host/rt_direct_illumination.hpp) on a Context the scene was uploaded
    to: drawUi's "Spatial reuse" toggle, record over a G-buffer (initial reservoirs, spatial reuse, trace)."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_rt_direct_illumination_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    @property
    def context(self):
        return self._ctx

    def draw_ui(self, spatial_reuse=True):
        lib().prosper_host_rt_direct_illumination_draw_ui(self._h, int(spatial_reuse))

    def recompile_shaders(self):
        lib().prosper_host_rt_direct_illumination_recompile_shaders(self._h)

    def release_preserved(self):
        lib().prosper_host_rt_direct_illumination_release_preserved(self._h)

    def record(self, camera, albedo_roughness, normal_metallic, depth, reset_accumulation=False, draw_type="Default",
               next_frame=0, stream=None):
        """Camera::updateBuffer + RtDirectIllumination::record over host G-buffer arrays ([h, w, 4], [h, w, 4],
        [h, w] float32); returns the TracePC that was pushed."""
        inp, keep, w, h = Context._restir_host_inputs(albedo_roughness, normal_metallic, depth)
        pc = S.RestirTracePC()
        rc = lib().prosper_host_rt_direct_illumination_record(
            self._h, camera._h, w, h, C.byref(inp), int(reset_accumulation),
            S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type), next_frame, C.c_void_p(stream),
            C.byref(pc))
        del keep
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._ctx._restir_extent = (w, h)
        return pc

    def record_device(self, camera, gbuffer, width, height, reset_accumulation=False, draw_type="Default",
                      next_frame=0, stream=None):
        """Same over a device G-buffer (S.RestirInputs with onDevice = 1, e.g. GBufferTracer.record's)."""
        pc = S.RestirTracePC()
        rc = lib().prosper_host_rt_direct_illumination_record(
            self._h, camera._h, width, height, C.byref(gbuffer), int(reset_accumulation),
            S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type), next_frame, C.c_void_p(stream),
            C.byref(pc))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._ctx._restir_extent = (width, height)
        return pc

    def close(self):
        if self._h:
            lib().prosper_host_rt_direct_illumination_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def renderer_lod_bias(apply_taa):
    """Renderer::lodBias() (Renderer.cpp:709-715): -1 while TAA is applied, otherwise 0."""
    return float(lib().prosper_host_renderer_lod_bias(int(bool(apply_taa))))


class GBufferTracer:
    """render::GBufferTracer (csrc/host/gbuffer_tracer.hpp) on a Context the scene was uploaded to: record traces the
    G-buffer into the context's buffers and returns them as device inputs (S.RestirInputs, onDevice = 1)."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_gbuffer_tracer_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def set_opaque_only(self, opaque_only):
        """GBufferTracer::setOpaqueOnly: later records leave BLEND surfaces to ForwardRenderer.record_transparent."""
        rc = lib().prosper_host_gbuffer_tracer_set_opaque_only(self._h, int(opaque_only))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def set_texture_lod(self, enabled, lod_bias=0.0):
        """GBufferTracer::setTextureLod / setLodBias: later records sample materials through the mip chains (a
        CREATE_TEXTURE_MIPS context) with `lod_bias` - renderer_lod_bias(taa) is what prosper passes."""
        rc = lib().prosper_host_gbuffer_tracer_set_texture_lod(self._h, int(bool(enabled)), lod_bias)
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def record(self, camera, width, height, draw_type="Default", frame_index=0, jitter=True, stream=None, opaque_only=None):
        if opaque_only is not None:
            self.set_opaque_only(opaque_only)
        out = S.RestirInputs()
        rc = lib().prosper_host_gbuffer_tracer_record(
            self._h, camera._h, width, height, S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type),
            frame_index, int(jitter), C.c_void_p(stream), C.byref(out))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return out

    def record_velocity(self, camera, width, height, draw_type="Default", frame_index=0, transforms=None, stream=None,
                        opaque_only=None):
        """GBufferTracer::recordVelocity: the G-buffer through the camera's (jittered) pixel centres and the velocity
        image; (S.RestirInputs, velocity device pointer).  `transforms`: this frame's ctypes array of
        S.ModelInstanceTransforms (world.freeze()["transforms"]); the pass keeps it as the next call's previous frame."""
        if opaque_only is not None:
            self.set_opaque_only(opaque_only)
        out, velocity = S.RestirInputs(), C.c_void_p()
        rc = lib().prosper_host_gbuffer_tracer_record_velocity(
            self._h, camera._h, width, height, S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type),
            frame_index, None if transforms is None else C.cast(transforms, C.c_void_p), 0 if transforms is None else len(transforms),
            C.c_void_p(stream), C.byref(out), C.byref(velocity))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return out, velocity.value

    def close(self):
        if self._h:
            lib().prosper_host_gbuffer_tracer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LightClustering:
    """render::LightClustering (csrc/host/light_clustering.hpp) on a Context the scene was uploaded to: record clusters
    the lights for the camera into the context's buffers (Context.read_light_clusters reads them)."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_light_clustering_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def record(self, camera, width, height, stream=None):
        rc = lib().prosper_host_light_clustering_record(self._h, camera._h, width, height, C.c_void_p(stream))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def close(self):
        if self._h:
            lib().prosper_host_light_clustering_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeferredShading:
    """render::DeferredShading (csrc/host/deferred_shading.hpp) on a Context the scene was uploaded to: record clusters
    the lights and shades the G-buffer into the context's HDR image (Context.read_hdr); returns the DeferredShadingPC."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_deferred_shading_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def record(self, camera, albedo_roughness, normal_metallic, depth, apply_ibl=False, draw_type="Default",
               stream=None):
        """Over host G-buffer arrays ([h, w, 4], [h, w, 4], [h, w] float32)."""
        ar = np.ascontiguousarray(albedo_roughness, np.float32)
        nm = np.ascontiguousarray(normal_metallic, np.float32)
        dp = np.ascontiguousarray(depth, np.float32)
        h, w = dp.shape
        inp = S.RestirInputs(ar.ctypes.data, nm.ctypes.data, dp.ctypes.data, None, 0, 0)
        return self.record_device(camera, inp, w, h, apply_ibl, draw_type, stream)

    def record_device(self, camera, gbuffer, width, height, apply_ibl=False, draw_type="Default", stream=None):
        """Over a G-buffer given as S.RestirInputs (e.g. GBufferTracer.record's)."""
        pc = S.DeferredShadingPC()
        rc = lib().prosper_host_deferred_shading_record(
            self._h, camera._h, width, height, C.byref(gbuffer), int(apply_ibl),
            S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type), C.c_void_p(stream), C.byref(pc))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return pc

    def close(self):
        if self._h:
            lib().prosper_host_deferred_shading_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HierarchicalDepthDownsampler:
    """render::HierarchicalDepthDownsampler (csrc/host/hierarchical_depth_downsampler.hpp) on a Context: record makes the
    depth pyramid (Context.hiz_downsample) in the slot `next_frame` & 1 picks and returns its levels' device pointers."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_hiz_downsampler_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def record(self, width, height, next_frame=0, depth=None, depth_ptr=None, stream=None):
        """`depth`: a host array [h, w]; `depth_ptr`: a device pointer; neither: the last traced G-buffer's depth."""
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        count, mips = C.c_uint32(), (C.c_void_p * 12)()
        rc = lib().prosper_host_hiz_downsampler_record(
            self._h, C.c_void_p(depth_ptr if dp is None else dp.ctypes.data), 1 if dp is None else 0, width, height,
            next_frame, C.byref(count), mips, C.c_void_p(stream))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return [mips[l] for l in range(count.value)]

    def close(self):
        if self._h:
            lib().prosper_host_hiz_downsampler_destroy(self._h)
            self._h = None


class GBufferRenderer:
    """render::GBufferRenderer (csrc/host/gbuffer_renderer.hpp) on a Context the scene was uploaded to: record is
    prosper_pt_raster_gbuffer into the context's own targets and returns S.GBufferRendererOutput (device pointers);
    read_draw_stats is render::DrawStats; release_preserved forgets the kept pyramid and transforms."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_gbuffer_renderer_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def record(self, camera, width, height, draw_type="Default", transforms=None, stream=None):
        """`camera`: a Camera; `transforms`: this frame's ctypes array of S.ModelInstanceTransforms, kept as the next
        record's previous frame"""
        out = S.GBufferRendererOutput()
        rc = lib().prosper_host_gbuffer_renderer_record(
            self._h, camera._h, width, height, S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type),
            None if transforms is None else C.cast(transforms, C.c_void_p), 0 if transforms is None else len(transforms),
            C.c_void_p(stream), C.byref(out))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return out

    def read_draw_stats(self, wait=True):
        """(S.DrawStats, landed)"""
        out = S.DrawStats()
        rc = lib().prosper_host_gbuffer_renderer_read_draw_stats(self._h, C.byref(out), 1 if wait else 0)
        if rc not in (0, S.NOT_READY):
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return out, rc == 0

    def release_preserved(self):
        lib().prosper_host_gbuffer_renderer_release_preserved(self._h)

    def close(self):
        if self._h:
            lib().prosper_host_gbuffer_renderer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeshletCuller:
    """render::MeshletCuller (csrc/host/meshlet_culler.hpp) on a Context the scene was uploaded to: record_first_phase /
    record_second_phase return S.MeshletCullerOutput (device pointers of the lists and argument triples);
    read_draw_stats is render::DrawStats."""

    MODE_OPAQUE, MODE_TRANSPARENT = 0, 1

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_meshlet_culler_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def record_first_phase(self, camera, width, height, mode=0, hierarchical_depth=None, stream=None):
        """`camera`: a Camera; `hierarchical_depth`: a pyramid slot (0 or 1) or None"""
        out = S.MeshletCullerOutput()
        slot = S.NO_HIZ if hierarchical_depth is None else hierarchical_depth
        rc = lib().prosper_host_meshlet_culler_record_first_phase(self._h, mode, camera._h, width, height, slot, C.byref(out),
                                                                   C.c_void_p(stream))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return out

    def record_second_phase(self, camera, width, height, hierarchical_depth, stream=None):
        out = S.MeshletCullerOutput()
        rc = lib().prosper_host_meshlet_culler_record_second_phase(self._h, camera._h, width, height, hierarchical_depth,
                                                                    C.byref(out), C.c_void_p(stream))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return out

    def read_draw_stats(self, wait=True):
        """(S.DrawStats, landed): with wait=False the totals come at once, the two device counts once `landed`"""
        out = S.DrawStats()
        rc = lib().prosper_host_meshlet_culler_read_draw_stats(self._h, C.byref(out), 1 if wait else 0)
        if rc not in (0, S.NOT_READY):
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return out, rc == 0

    def close(self):
        if self._h:
            lib().prosper_host_meshlet_culler_destroy(self._h)
            self._h = None


class SkyboxRenderer:
    """render::SkyboxRenderer (csrc/host/skybox_renderer.hpp) on a Context the scene was uploaded to: record fills the sky
    into the context's HDR image wherever the depth is the far plane's (Context.skybox_fill)."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_skybox_renderer_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def record(self, camera, width, height, depth=None, depth_ptr=None, stream=None):
        """`depth`: a host array [h, w]; `depth_ptr`: a device pointer; neither: the last traced G-buffer's depth."""
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        rc = lib().prosper_host_skybox_renderer_record(
            self._h, camera._h, width, height, C.c_void_p(depth_ptr if dp is None else dp.ctypes.data),
            1 if dp is None else 0, C.c_void_p(stream))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def close(self):
        if self._h:
            lib().prosper_host_skybox_renderer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ForwardRenderer:
    """render::ForwardRenderer (csrc/host/forward_renderer.hpp) on a Context the scene was uploaded to: record_opaque is
    prosper_pt_raster_forward into the context's HDR image, depth and velocity and returns S.ForwardRendererOutput (device
    pointers); release_preserved forgets the kept pyramid and transforms; record_transparent blends the BLEND layers over
    the context's HDR image (Context.forward_transparent) and returns the S.ForwardPC it pushed."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_forward_renderer_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def set_texture_lod(self, enabled, lod_bias=0.0):
        """ForwardRenderer::setTextureLod / setLodBias: later records sample the layers' materials through the mip chains."""
        rc = lib().prosper_host_forward_renderer_set_texture_lod(self._h, int(bool(enabled)), lod_bias)
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def record_opaque(self, camera, width, height, apply_ibl=False, draw_type="Default", transforms=None, stream=None):
        """`camera`: a Camera; `transforms`: this frame's ctypes array of S.ModelInstanceTransforms, kept as the next
        record's previous frame"""
        out = S.ForwardRendererOutput()
        rc = lib().prosper_host_forward_renderer_record_opaque(
            self._h, camera._h, width, height, int(apply_ibl), S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type),
            None if transforms is None else C.cast(transforms, C.c_void_p), 0 if transforms is None else len(transforms),
            C.c_void_p(stream), C.byref(out))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._ctx._forward_extent = (width, height)
        return out

    def release_preserved(self):
        lib().prosper_host_forward_renderer_release_preserved(self._h)

    def record_transparent(self, camera, width, height, depth=None, depth_ptr=None, ray_flags=0, frame_index=0,
                           apply_ibl=False, draw_type="Default", stream=None):
        """`depth`: a host array [h, w]; `depth_ptr`: a device pointer; neither: the last traced G-buffer's depth.
        `ray_flags`: 0, S.TRANSPARENT_JITTER (with `frame_index`) or S.TRANSPARENT_CAMERA_JITTER."""
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        pc = S.ForwardPC()
        rc = lib().prosper_host_forward_renderer_record_transparent(
            self._h, camera._h, width, height, C.c_void_p(depth_ptr if dp is None else dp.ctypes.data),
            1 if dp is None else 0, ray_flags, frame_index, int(apply_ibl),
            S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type), C.c_void_p(stream), C.byref(pc))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return pc

    def record_transparent_raster(self, camera, width, height, depth=None, depth_ptr=None, apply_ibl=False, draw_type="Default",
                                  stream=None):
        """ForwardRenderer::recordTransparentRaster: the raster frame's transparents (Context.raster_forward_transparent) -
        the TRANSPARENT draw list culled once, listed per pixel and resolved over the context's HDR image.  `depth`,
        `depth_ptr`: as record_transparent (neither: the context's last depth, a forward frame's included)."""
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        pc = S.ForwardPC()
        rc = lib().prosper_host_forward_renderer_record_transparent_raster(
            self._h, camera._h, width, height, C.c_void_p(depth_ptr if dp is None else dp.ctypes.data), 1 if dp is None else 0,
            int(apply_ibl), S.DrawType[draw_type] if isinstance(draw_type, str) else int(draw_type), C.c_void_p(stream), C.byref(pc))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._ctx._raster_transparent_extent = (width, height)
        return pc

    def close(self):
        if self._h:
            lib().prosper_host_forward_renderer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Particles:
    """render::particles::Particles (csrc/host/particles.hpp) on a Context: record runs decay, init while a reset is
    pending, simulate and render over the context's HDR image and the depth; returns (S.ParticlesPC pushed, init recorded)."""

    def __init__(self, ctx, source_draw_instance=0, max_particle_count=0):
        h = C.c_void_p()
        rc = lib().prosper_host_particles_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx
        lib().prosper_host_particles_set_source(h, source_draw_instance)
        lib().prosper_host_particles_set_max_particle_count(h, max_particle_count)
        ctx._particles_max = max_particle_count

    def record(self, camera, width, height, delta_time_s, depth_ptr=None, stream=None):
        """`depth_ptr`: a device pointer the pass reads and writes; None: the last traced G-buffer's depth."""
        pc = S.ParticlesPC()
        recorded = C.c_uint32()
        rc = lib().prosper_host_particles_record(self._h, camera._h, width, height, C.c_void_p(depth_ptr), delta_time_s,
                                                 C.c_void_p(stream), C.byref(pc), C.byref(recorded))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return pc, bool(recorded.value)

    def close(self):
        if self._h:
            lib().prosper_host_particles_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostDebugLines:
    """scene::DebugLines (csrc/host/debug_renderer.hpp): the C++ line list, for DebugRenderer.record."""

    def __init__(self):
        h = C.c_void_p()
        rc = lib().prosper_host_debug_lines_create(C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, "prosper_host_debug_lines_create failed")
        self._h = h

    @property
    def count(self):
        return lib().prosper_host_debug_lines_count(self._h)

    def reset(self):
        lib().prosper_host_debug_lines_reset(self._h)

    def add_line(self, p0, p1, color):
        v = np.concatenate([np.asarray(a, np.float32).reshape(3) for a in (p0, p1, color)])
        rc = lib().prosper_host_debug_lines_add_line(self._h, v.ctypes.data, v[3:].ctypes.data, v[6:].ctypes.data)
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def close(self):
        if self._h:
            lib().prosper_host_debug_lines_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DebugRenderer:
    """render::DebugRenderer (csrc/host/debug_renderer.hpp) on a Context: record draws a HostDebugLines list, depth-tested,
    in place over the context's HDR image and the last traced G-buffer's depth."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_debug_renderer_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def record(self, camera, lines, width, height, stream=None):
        rc = lib().prosper_host_debug_renderer_record(self._h, camera._h, lines._h, width, height, C.c_void_p(stream))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def close(self):
        if self._h:
            lib().prosper_host_debug_renderer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DepthOfField:
    """render::dof::DepthOfField (csrc/host/depth_of_field.hpp) on a Context: record computes the push constants from the
    camera's aperture, focus distance and focal length and runs the seven passes into the context's HDR image
    (Context.read_hdr); returns the S.DofPC it pushed."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_depth_of_field_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def record(self, camera, width, height, illumination=None, depth=None, stream=None):
        """Over host arrays ([h, w, 4], [h, w] float32); None: the HDR image in place / the last traced G-buffer's depth."""
        il = None if illumination is None else np.ascontiguousarray(illumination, np.float32)
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        host = il is not None or dp is not None
        inp = S.DofInputs(None if il is None else il.ctypes.data, None if dp is None else dp.ctypes.data, 0 if host else 1, 0)
        return self.record_inputs(camera, width, height, inp, stream)

    def record_inputs(self, camera, width, height, inputs, stream=None):
        """Over S.DofInputs (device pointers with onDevice = 1)."""
        pc = S.DofPC()
        rc = lib().prosper_host_depth_of_field_record(self._h, camera._h, width, height, C.byref(inputs),
                                                      C.c_void_p(stream), C.byref(pc))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return pc

    def close(self):
        if self._h:
            lib().prosper_host_depth_of_field_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bloom:
    """render::bloom::Bloom (csrc/host/bloom.hpp) on a Context, with prosper's defaults: draw_ui sets the threshold, the
    blend factors, the sampling and the resolution scale; record runs the passes of the technique (S.BLOOM_MULTI_RESOLUTION_BLUR,
    the default, or S.BLOOM_FFT) into the context's HDR image (Context.read_hdr) and returns the S.BloomPC, or with the
    FFT technique the S.BloomFftPC, it pushed."""

    def __init__(self, ctx, technique=S.BLOOM_MULTI_RESOLUTION_BLUR):
        h = C.c_void_p()
        rc = lib().prosper_host_bloom_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx
        self._technique = technique
        self.set_technique(technique)

    def set_technique(self, technique, regenerate_kernel=False):
        """render::bloom::Technique and GenerateKernel's "Re-generate kernel" checkbox"""
        self._technique = technique
        lib().prosper_host_bloom_set_technique(self._h, technique, 1 if regenerate_kernel else 0)

    def release_preserved(self):
        """drops the kernel's DFT the context keeps"""
        lib().prosper_host_bloom_release_preserved(self._h)

    def draw_ui(self, threshold=1.0, blend_factors=(0.9, 0.04, 0.04), biquadratic=True, resolution_scale=S.BLOOM_HALF):
        lib().prosper_host_bloom_draw_ui(self._h, threshold, blend_factors[0], blend_factors[1], blend_factors[2],
                                         1 if biquadratic else 0, resolution_scale)

    def record(self, width, height, illumination=None, illumination_ptr=None, stream=None):
        """`illumination`: a host array [h, w, 4]; `illumination_ptr`: a device pointer; neither: the HDR image in place."""
        il = None if illumination is None else np.ascontiguousarray(illumination, np.float32)
        pc = S.BloomPC()
        rc = lib().prosper_host_bloom_record(self._h, width, height, C.c_void_p(illumination_ptr if il is None else il.ctypes.data),
                                             1 if il is None else 0, C.c_void_p(stream), C.byref(pc))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        if self._technique == S.BLOOM_FFT:
            pc = S.BloomFftPC()
            lib().prosper_host_bloom_fft_push_constants(self._h, C.byref(pc))
        return pc

    def close(self):
        if self._h:
            lib().prosper_host_bloom_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TemporalAntiAliasing:
    """render::TemporalAntiAliasing (csrc/host/temporal_anti_aliasing.hpp) on a Context, with prosper's defaults: draw_ui
    sets the four settings; record resolves into the context's HDR image (Context.read_hdr) and the preserved history
    and returns the S.TaaPC it pushed; release_preserved drops the history."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_taa_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def draw_ui(self, catmull_rom=True, color_clipping=S.TAA_CLIPPING_VARIANCE, velocity_sampling=S.TAA_VELOCITY_CLOSEST,
                luminance_weighting=True):
        lib().prosper_host_taa_draw_ui(self._h, 1 if catmull_rom else 0, color_clipping, velocity_sampling,
                                       1 if luminance_weighting else 0)

    def record(self, width, height, velocity=None, depth=None, illumination=None, velocity_ptr=None, depth_ptr=None,
               illumination_ptr=None, stream=None):
        """Host arrays (`velocity` [h, w, 2], `depth` [h, w], `illumination` [h, w, 4]) or device pointers (`_ptr`), not
        both; no illumination: the HDR image in place; no depth: the last traced G-buffer's."""
        host = velocity is not None or depth is not None or illumination is not None
        assert not (host and (velocity_ptr or depth_ptr or illumination_ptr)), "host and device inputs cannot be mixed"
        arrays = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (illumination, velocity, depth)]
        if host:
            inp = S.TaaInputs(*[None if a is None else a.ctypes.data for a in arrays], 0)
        else:
            inp = S.TaaInputs(illumination_ptr, velocity_ptr, depth_ptr, 1)
        pc = S.TaaPC()
        rc = lib().prosper_host_taa_record(self._h, width, height, C.byref(inp), C.c_void_p(stream), C.byref(pc))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return pc

    def release_preserved(self):
        lib().prosper_host_taa_release_preserved(self._h)

    def close(self):
        if self._h:
            lib().prosper_host_taa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ImageBasedLighting:
    """render::ImageBasedLighting (csrc/host/image_based_lighting.hpp) on a Context the scene was uploaded to:
    record_generation makes the irradiance and radiance cubes and the BRDF LUT that DeferredShading reads with
    apply_ibl=True; is_generated is False again after a scene upload."""

    def __init__(self, ctx):
        h = C.c_void_p()
        rc = lib().prosper_host_image_based_lighting_create(ctx._h, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = ctx

    def is_generated(self):
        rc = lib().prosper_host_image_based_lighting_is_generated(self._h)
        if rc < 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return rc == 1

    def record_generation(self, stream=None):
        rc = lib().prosper_host_image_based_lighting_record_generation(self._h, C.c_void_p(stream))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def close(self):
        if self._h:
            lib().prosper_host_image_based_lighting_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TiledRtReference:
    """render::TiledRtReference (csrc/host/tiled_rt_reference.hpp): one rank of a multi-GPU job.  record() renders the
    rank's stripes and enqueues the RCCL gather + de-interleave to the root; read_gathered() there returns the image."""

    @staticmethod
    def create_comm_id():
        return Context.comm_unique_id()

    def __init__(self, device, rank, ranks, comm_id=None, root=0, flags=0):
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(comm_id) if comm_id is not None else bytes(128))
        rc = lib().prosper_host_tiled_rt_reference_create(device, rank, ranks, buf, root, flags, C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h
        self._ctx = Context(_borrowed=lib().prosper_host_tiled_rt_reference_context(h))
        self.rank, self.ranks, self.root = rank, ranks, root
        self._world = None

    @property
    def context(self):
        return self._ctx

    def set_world(self, world):
        view = world.view()
        rc = lib().prosper_host_tiled_rt_reference_set_scene(self._h, C.byref(view))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._world = world

    def record(self, camera, width, height, options=None, frame_count=1, render_flags=0, stream=None):
        """-> device pointer of the gathered image on the root (None elsewhere)."""
        options = options or RtReference.Options()
        o = RecordOptions(int(options.depthOfField), int(options.ibl), int(options.colorDirty),
                          S.DrawType[options.drawType] if isinstance(options.drawType, str) else int(options.drawType))
        out = C.POINTER(C.c_float)()
        rc = lib().prosper_host_tiled_rt_reference_record(
            self._h, camera._h, width, height, C.byref(o), frame_count, render_flags, C.c_void_p(stream), C.byref(out))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        return C.cast(out, C.c_void_p).value

    def wait_for_gather(self, stream=None):
        rc = lib().prosper_host_tiled_rt_reference_wait_for_gather(self._h, C.c_void_p(stream))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def close(self):
        if self._h:
            lib().prosper_host_tiled_rt_reference_destroy(self._h)
            self._h = None
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ToneMap:
    """Handle on the C++ render::ToneMap (csrc/host/tone_map.hpp; reference src/render/ToneMap.hpp)."""

    def __init__(self, ctx, lut_path=None, lut_texels=None):
        h = C.c_void_p()
        if lut_path is not None:
            rc = lib().prosper_host_tone_map_create(ctx._h, os.fsencode(lut_path), C.byref(h))
        else:
            lut = np.ascontiguousarray(lut_texels, dtype=np.uint32)
            rc = lib().prosper_host_tone_map_create_from_texels(ctx._h, lut.ctypes.data, lut.shape[0], C.byref(h))
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())
        self._h = h

    def draw_ui(self, exposure, contrast):
        lib().prosper_host_tone_map_draw_ui(self._h, exposure, contrast)

    def record(self, device_ptr, byte_size, stream=None):
        rc = lib().prosper_host_tone_map_record(self._h, C.c_void_p(stream), C.c_void_p(device_ptr), byte_size)
        if rc != 0:
            raise ProsperPtError(rc, lib().prosper_host_last_error().decode())

    def close(self):
        if self._h:
            lib().prosper_host_tone_map_destroy(self._h)
            self._h = None
