"""ctypes binding of libprosper_pt.so (include/prosper_pt/prosper_pt.h, prosper_host.h).

There is no Python or CPU fallback behind these calls: if the HIP library is missing, or no
gfx950 device is visible, they raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import structs as S

_HERE = os.path.dirname(os.path.abspath(__file__))
# PROSPER_PT_LIB (read by this BINDING, i.e. by tests and measurement scripts - the library itself never looks): another
# build of the library, e.g. a tuning variant of scripts/build_variant.sh
LIB_PATH = os.environ.get("PROSPER_PT_LIB") or os.path.join(_HERE, "libprosper_pt.so")


class ProsperPtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("prosper_pt error %d: %s" % (code, message))
        self.code = code


def build(force=False):
    """Compile the HIP library for gfx950 in-tree (prosper_amd/csrc/Makefile)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-s"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


_lib = None


def lib():
    """Loads libprosper_pt.so; raises if it has not been built (never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ProsperPtError(-2, "HIP extension %s is missing: run prosper_amd.capi.build()" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    L.prosper_pt_last_error.restype = C.c_char_p
    L.prosper_pt_abi_version.restype = u32
    L.prosper_pt_has_experiments.restype = u32
    L.prosper_pt_debug_magic_divisor.argtypes = [u32, C.POINTER(u32), C.POINTER(u32)]
    L.prosper_pt_debug_magic_divisor.restype = None
    L.prosper_pt_debug_options_default.argtypes = [C.POINTER(S.DebugOptions)]
    L.prosper_pt_debug_options_default.restype = None
    L.prosper_pt_set_debug_options.argtypes = [vp, C.POINTER(S.DebugOptions)]
    L.prosper_pt_get_debug_options.argtypes = [vp, C.POINTER(S.DebugOptions)]
    L.prosper_pt_create.argtypes = [C.POINTER(S.DeviceDesc), C.POINTER(vp)]
    L.prosper_pt_destroy.argtypes = [vp]
    L.prosper_pt_destroy.restype = None
    L.prosper_pt_upload_scene.argtypes = [vp, C.POINTER(S.SceneView)]
    L.prosper_pt_update_lights.argtypes = [
        vp, C.POINTER(S.DirectionalLightParameters), C.POINTER(S.PointLightsBuffer), C.POINTER(S.SpotLightsBuffer)]
    L.prosper_pt_get_scene_stats.argtypes = [vp, C.POINTER(S.SceneStats)]
    L.prosper_pt_update_textures.argtypes = [vp, vp, u32, u32]
    L.prosper_pt_update_materials.argtypes = [vp, vp, u32, u32]
    L.prosper_pt_texture_mip_level_count.argtypes = [u32, u32]
    L.prosper_pt_texture_mip_level_count.restype = u32
    L.prosper_pt_check_texture_desc.argtypes = [C.POINTER(S.TextureDesc), u32]
    L.prosper_pt_get_texture_mips_info.argtypes = [vp, u32, C.POINTER(S.TextureMipsInfo)]
    L.prosper_pt_read_texture_level.argtypes = [vp, u32, u32, vp, C.c_uint64, vp]
    L.prosper_pt_debug_sample_texture_lod.argtypes = [vp, u32, u32, vp, u32, C.c_float, vp]
    L.prosper_pt_compressed_texture_layout.argtypes = [u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64)]
    L.prosper_pt_compress_texture.argtypes = [vp, C.POINTER(S.TextureDesc), u32, vp, C.c_uint64, vp]
    L.prosper_pt_debug_bc7_encode_blocks.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.prosper_pt_get_compress_texture_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.prosper_pt_prepare_mesh.argtypes = [vp, C.POINTER(S.MeshSource), u32, C.POINTER(S.PreparedMesh), vp]
    L.prosper_pt_read_prepared_mesh.argtypes = [vp, vp, C.c_uint64]
    L.prosper_pt_read_prepared_tangents.argtypes = [vp, vp, C.c_uint64]
    L.prosper_pt_get_prepare_mesh_timing.argtypes = [vp] + [C.POINTER(C.c_float)] * 5
    L.prosper_pt_set_texture_lod.argtypes = [vp, C.c_int, C.c_float]
    L.prosper_pt_set_texture_lod_debug.argtypes = [vp, C.c_int]
    L.prosper_pt_read_texture_lod_derivatives.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_update_meshes.argtypes = [vp, vp, u32]
    L.prosper_pt_finish_mesh_updates.argtypes = [vp]
    L.prosper_pt_update_transforms.argtypes = [vp, vp, u32]
    L.prosper_pt_update_transforms_async.argtypes = [vp, vp, u32, u32, vp]
    L.prosper_pt_set_animations.argtypes = [vp, C.POINTER(S.AnimationDesc)]
    L.prosper_pt_animate.argtypes = [vp, C.c_float, u32, vp]
    L.prosper_pt_get_animation_state.argtypes = [vp, C.POINTER(S.AnimationStateInfo)]
    L.prosper_pt_read_animated_transforms.argtypes = [vp, u32, vp, u32]
    L.prosper_pt_read_lights.argtypes = [
        vp, C.POINTER(S.DirectionalLightParameters), C.POINTER(S.PointLightsBuffer), C.POINTER(S.SpotLightsBuffer)]
    L.prosper_pt_debug_read_animation_nodes.argtypes = [vp, vp, vp, u32]
    L.prosper_pt_rebuild_hierarchy.argtypes = [vp]
    L.prosper_pt_get_hierarchy_state.argtypes = [vp, C.POINTER(S.HierarchyState)]
    L.prosper_pt_debug_read_nodes.argtypes = [vp, vp, C.c_size_t]
    L.prosper_pt_build_hierarchy_gpu.argtypes = [vp]
    L.prosper_pt_set_hierarchy_builder.argtypes = [vp, u32]
    L.prosper_pt_get_hierarchy_build_info.argtypes = [vp, C.POINTER(S.HierarchyBuildInfo)]
    L.prosper_pt_set_gpu_hierarchy_method.argtypes = [vp, u32, u32]
    L.prosper_pt_get_gpu_hierarchy_method_info.argtypes = [vp, C.POINTER(S.GpuHierarchyMethodInfo)]
    L.prosper_pt_set_gpu_hierarchy_sites.argtypes = [vp, u32]
    L.prosper_pt_get_gpu_hierarchy_sites.argtypes = [vp, C.POINTER(u32)]
    L.prosper_pt_debug_read_hierarchy_arrays.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    L.prosper_pt_set_output_buffer.argtypes = [vp, vp, C.c_size_t]
    L.prosper_pt_render.argtypes = [
        vp, C.POINTER(S.ReferencePC), C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.TileDesc), u32, vp]
    L.prosper_pt_render_frames.argtypes = [
        vp, C.POINTER(S.ReferencePC), C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.TileDesc), u32, u32, vp]
    L.prosper_pt_get_local_extent.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.prosper_pt_get_hdr_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.prosper_pt_read_hdr.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_blit_rgba16f.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_restir_di_trace.argtypes = [
        vp, C.POINTER(S.RestirTracePC), C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.RestirInputs), vp]
    L.prosper_pt_restir_di_resample.argtypes = [
        vp, u32, u32, C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.RestirInputs), vp, vp]
    L.prosper_pt_restir_di_record.argtypes = [
        vp, C.POINTER(S.RestirTracePC), u32, C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.RestirInputs), vp]
    L.prosper_pt_get_restir_reservoirs_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.prosper_pt_read_restir_reservoirs.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_trace_gbuffer.argtypes = [
        vp, u32, u32, u32, C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.GBufferTargets), vp]
    L.prosper_pt_get_gbuffer_device_ptrs.argtypes = [vp, C.POINTER(S.RestirInputs), C.POINTER(u32), C.POINTER(u32)]
    L.prosper_pt_trace_gbuffer_velocity.argtypes = [
        vp, u32, u32, u32, C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.VelocityGBufferDesc), vp]
    L.prosper_pt_get_velocity_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    L.prosper_pt_read_velocity.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_read_gbuffer.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.prosper_pt_cluster_lights.argtypes = [vp, C.POINTER(S.CameraUniforms), u32, u32, vp]
    L.prosper_pt_get_light_cluster_dims.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.prosper_pt_read_light_clusters.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.prosper_pt_deferred_shading.argtypes = [
        vp, C.POINTER(S.DeferredShadingPC), u32, u32, C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.RestirInputs), vp]
    L.prosper_pt_forward_transparent.argtypes = [vp, C.POINTER(S.ForwardPC), u32, u32, C.POINTER(S.CameraUniforms), u32, u32, vp, u32, vp]
    L.prosper_pt_get_transparent_info.argtypes = [vp, C.POINTER(S.TransparentInfo)]
    L.prosper_pt_set_transparent_debug_layers.argtypes = [vp, u32]
    L.prosper_pt_read_transparent_layers.argtypes = [vp, vp, vp, C.c_size_t, u32, vp]
    L.prosper_pt_particles.argtypes = [vp, C.POINTER(S.ParticlesPC), u32, C.POINTER(S.CameraUniforms), u32, u32, vp, vp]
    L.prosper_pt_get_particles_info.argtypes = [vp, C.POINTER(S.ParticlesInfo)]
    L.prosper_pt_read_particles.argtypes = [vp, vp, vp, u32, vp]
    L.prosper_pt_set_particles.argtypes = [vp, vp, vp, u32, vp]
    L.prosper_pt_debug_lines.argtypes = [vp, vp, u32, C.POINTER(S.CameraUniforms), u32, u32, vp]
    L.prosper_pt_get_debug_lines_info.argtypes = [vp, C.POINTER(S.DebugLinesInfo)]
    L.prosper_pt_debug_resource_count.argtypes = [vp]
    L.prosper_pt_debug_resource_count.restype = u32
    L.prosper_pt_get_debug_resource.argtypes = [vp, u32, C.POINTER(S.DebugResource)]
    L.prosper_pt_texture_readback.argtypes = [vp, u32, C.c_float, C.c_float, vp]
    L.prosper_pt_try_texture_readback.argtypes = [vp, C.POINTER(C.c_float * 4)]
    L.prosper_pt_texture_debug.argtypes = [vp, u32, C.POINTER(S.TextureDebugPC), u32, vp, vp, C.c_size_t, vp]
    L.prosper_pt_get_texture_debug_peek.argtypes = [vp, C.POINTER(C.c_float * 4)]
    L.prosper_pt_hiz_downsample.argtypes = [vp, u32, vp, u32, u32, u32, vp]
    L.prosper_pt_get_hiz_info.argtypes = [vp, u32, C.POINTER(S.HizInfo)]
    L.prosper_pt_get_hiz_device_ptr.argtypes = [vp, u32, u32, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    L.prosper_pt_hiz_wait.argtypes = [vp, u32, vp]
    L.prosper_pt_cull_meshlets_first_phase.argtypes = [vp, u32, C.POINTER(S.CameraUniforms), u32, vp]
    L.prosper_pt_cull_meshlets_second_phase.argtypes = [vp, C.POINTER(S.CameraUniforms), u32, vp]
    L.prosper_pt_cull_gbuffer.argtypes = [vp, C.POINTER(S.CameraUniforms), vp]
    L.prosper_pt_read_draw_list.argtypes = [vp, u32, C.POINTER(u32), vp, u32, C.POINTER(u32 * 3), vp]
    L.prosper_pt_get_draw_list_device_ptr.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(u32)]
    L.prosper_pt_get_draw_stats.argtypes = [vp, C.POINTER(S.DrawStats), u32]
    L.prosper_pt_get_cull_stage_ms.argtypes = [vp, C.POINTER(C.c_float * 3)]
    L.prosper_pt_raster_meshlets.argtypes = [vp, u32, u32, C.POINTER(S.CameraUniforms), vp]
    L.prosper_pt_raster_visibility.argtypes = [vp, C.POINTER(S.CameraUniforms), vp]
    L.prosper_pt_raster_resolve.argtypes = [vp, u32, C.POINTER(S.CameraUniforms), C.POINTER(S.VelocityGBufferDesc), vp]
    L.prosper_pt_raster_gbuffer.argtypes = [vp, u32, C.POINTER(S.CameraUniforms), C.POINTER(S.VelocityGBufferDesc), vp]
    L.prosper_pt_read_raster_visibility.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.prosper_pt_raster_forward_shade.argtypes = [vp, C.POINTER(S.ForwardPC), C.POINTER(S.CameraUniforms), C.POINTER(S.ForwardOpaqueDesc), vp]
    L.prosper_pt_raster_forward.argtypes = [vp, C.POINTER(S.ForwardPC), C.POINTER(S.CameraUniforms), C.POINTER(S.ForwardOpaqueDesc), vp]
    L.prosper_pt_set_forward_debug_surfaces.argtypes = [vp, C.c_int]
    L.prosper_pt_read_forward_surfaces.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_get_forward_opaque_info.argtypes = [vp, C.POINTER(S.ForwardOpaqueInfo)]
    L.prosper_pt_raster_transparent_draw.argtypes = [vp, u32, C.POINTER(S.ForwardPC), C.POINTER(S.CameraUniforms), vp, u32, vp]
    L.prosper_pt_raster_forward_transparent.argtypes = [vp, C.POINTER(S.ForwardPC), C.POINTER(S.CameraUniforms), vp, u32, vp]
    L.prosper_pt_get_raster_transparent_info.argtypes = [vp, C.POINTER(S.RasterTransparentInfo)]
    L.prosper_pt_read_raster_fragments.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint64), vp]
    L.prosper_pt_set_raster_transparent_debug_layers.argtypes = [vp, u32]
    L.prosper_pt_read_raster_transparent_layers.argtypes = [vp, vp, vp, C.c_size_t, u32, vp]
    L.prosper_pt_get_forward_depth_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    L.prosper_pt_read_forward_depth.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_get_raster_info.argtypes = [vp, C.POINTER(S.RasterInfo)]
    L.prosper_pt_read_instance_scales.argtypes = [vp, vp, u32, vp]
    L.prosper_pt_read_hiz_level.argtypes = [vp, u32, u32, vp, C.c_size_t, vp]
    L.prosper_pt_generate_ibl.argtypes = [vp, vp]
    L.prosper_pt_get_ibl_info.argtypes = [vp, C.POINTER(S.IblInfo)]
    L.prosper_pt_read_ibl.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp]
    L.prosper_pt_skybox_fill.argtypes = [vp, C.POINTER(S.CameraUniforms), u32, u32, vp, u32, vp]
    L.prosper_pt_depth_of_field.argtypes = [
        vp, C.POINTER(S.DofPC), C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.DofInputs), vp]
    L.prosper_pt_dof_sample_offsets.argtypes = [vp]
    L.prosper_pt_dof_sample_offsets.restype = None
    L.prosper_pt_read_dof_stage.argtypes = [vp, u32, u32, vp, C.c_size_t, vp]
    L.prosper_pt_get_dof_info.argtypes = [vp, C.POINTER(S.DofInfo)]
    L.prosper_pt_bloom.argtypes = [vp, C.POINTER(S.BloomPC), u32, u32, vp, u32, vp]
    L.prosper_pt_bloom_streak_weights.argtypes = [u32, vp, vp]
    L.prosper_pt_bloom_streak_weights.restype = None
    L.prosper_pt_read_bloom_stage.argtypes = [vp, u32, u32, vp, C.c_size_t, vp]
    L.prosper_pt_get_bloom_info.argtypes = [vp, C.POINTER(S.BloomInfo)]
    L.prosper_pt_bloom_fft_plan.argtypes = [u32, u32, u32, C.POINTER(S.BloomFftPlan)]
    L.prosper_pt_bloom_fft.argtypes = [vp, C.POINTER(S.BloomFftPC), u32, u32, vp, u32, vp]
    L.prosper_pt_bloom_fft_transform.argtypes = [vp, u32, u32, vp, vp, u32, vp]
    L.prosper_pt_bloom_fft_release_kernel.argtypes = [vp]
    L.prosper_pt_bloom_fft_release_kernel.restype = None
    L.prosper_pt_read_bloom_fft_stage.argtypes = [vp, u32, vp, C.c_size_t, vp]
    L.prosper_pt_get_bloom_fft_info.argtypes = [vp, C.POINTER(S.BloomFftInfo)]
    L.prosper_pt_taa_resolve.argtypes = [vp, C.POINTER(S.TaaPC), u32, u32, C.POINTER(S.TaaInputs), vp]
    L.prosper_pt_taa_release_history.argtypes = [vp]
    L.prosper_pt_taa_release_history.restype = None
    L.prosper_pt_read_taa_history.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_get_taa_info.argtypes = [vp, C.POINTER(S.TaaInfo)]
    L.prosper_pt_taa_jitter.argtypes = [u32, u32, u32, C.POINTER(C.c_float * 2)]
    L.prosper_pt_taa_jitter.restype = None
    L.prosper_pt_denoise_pc_default.argtypes = [C.POINTER(S.DenoisePC)]
    L.prosper_pt_denoise_pc_default.restype = None
    L.prosper_pt_denoise.argtypes = [vp, C.POINTER(S.DenoisePC), C.POINTER(S.CameraUniforms), u32, u32, C.POINTER(S.DenoiseInputs), vp]
    L.prosper_pt_denoise_release_history.argtypes = [vp]
    L.prosper_pt_denoise_release_history.restype = None
    L.prosper_pt_read_denoise_stage.argtypes = [vp, u32, vp, C.c_size_t, vp]
    L.prosper_pt_get_denoise_info.argtypes = [vp, C.POINTER(S.DenoiseInfo)]
    L.prosper_pt_set_tone_map_lut.argtypes = [vp, vp, u32]
    L.prosper_pt_tone_map.argtypes = [vp, C.c_float, C.c_float, vp, vp, C.c_size_t, vp]
    L.prosper_pt_get_counters.argtypes = [vp, C.POINTER(S.Counters), vp]
    L.prosper_pt_reset_counters.argtypes = [vp, vp]
    L.prosper_pt_get_stage_counters.argtypes = [vp, u32, C.POINTER(S.Counters), vp]
    L.prosper_pt_get_last_render_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(u32)]
    L.prosper_pt_get_last_render_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.prosper_pt_kernel_name.argtypes = [u32]
    L.prosper_pt_kernel_name.restype = C.c_char_p
    L.prosper_pt_set_kernel_timing.argtypes = [vp, C.c_int]
    L.prosper_pt_eval_device_fn.argtypes = [vp, u32, vp, u32, vp, u32, u32]
    L.prosper_pt_debug_srgb_monotonicity.argtypes = [vp, u32, u32, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    # multi-GPU: stripes + RCCL gather + de-interleave
    L.prosper_pt_comm_get_unique_id.argtypes = [vp]
    L.prosper_pt_comm_init.argtypes = [vp, vp, u32, u32]
    L.prosper_pt_comm_adopt.argtypes = [vp, vp, u32, u32]
    L.prosper_pt_comm_destroy.argtypes = [vp]
    L.prosper_pt_gather_tiles.argtypes = [vp, u32, vp, C.c_size_t, u32, vp]
    L.prosper_pt_gather_wait.argtypes = [vp, vp]
    L.prosper_pt_comm_query.argtypes = [vp, C.POINTER(S.CommInfo)]
    L.prosper_pt_get_gathered_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    L.prosper_pt_read_gathered.argtypes = [vp, vp, C.c_size_t, vp]
    L.prosper_pt_deinterleave_tiles.argtypes = [vp, vp, u32, u32, u32, u32, vp, C.c_size_t, vp]
    # host layer
    L.prosper_host_last_error.restype = C.c_char_p
    L.prosper_host_camera_create.restype = vp
    L.prosper_host_camera_destroy.argtypes = [vp]
    L.prosper_host_camera_destroy.restype = None
    f3 = C.POINTER(C.c_float)
    L.prosper_host_camera_look_at.argtypes = [vp, f3, f3, f3]
    L.prosper_host_camera_look_at.restype = None
    L.prosper_host_camera_set_parameters.argtypes = [vp] + [C.c_float] * 5
    L.prosper_host_camera_set_parameters.restype = None
    L.prosper_host_camera_update_resolution.argtypes = [vp, u32, u32]
    L.prosper_host_camera_update_resolution.restype = None
    L.prosper_host_camera_update_buffer.argtypes = [vp, C.POINTER(S.CameraUniforms), C.POINTER(C.c_float)]
    L.prosper_host_camera_update_buffer.restype = None
    L.prosper_host_camera_changed_this_frame.argtypes = [vp]
    L.prosper_host_camera_end_frame.argtypes = [vp]
    L.prosper_host_camera_end_frame.restype = None
    L.prosper_host_camera_set_jitter.argtypes = [vp, C.c_int]
    L.prosper_host_camera_set_jitter.restype = None
    L.prosper_host_rt_reference_create.argtypes = [i32, u32, C.POINTER(vp)]
    L.prosper_host_rt_reference_destroy.argtypes = [vp]
    L.prosper_host_rt_reference_destroy.restype = None
    L.prosper_host_rt_reference_context.argtypes = [vp]
    L.prosper_host_rt_reference_context.restype = vp
    L.prosper_host_rt_reference_set_scene.argtypes = [vp, C.POINTER(S.SceneView)]
    L.prosper_host_rt_reference_draw_ui.argtypes = [vp, C.c_int, C.c_int, u32, u32]
    L.prosper_host_rt_reference_draw_ui.restype = None
    L.prosper_host_rt_reference_recompile_shaders.argtypes = [vp]
    L.prosper_host_rt_reference_recompile_shaders.restype = None
    L.prosper_host_rt_reference_release_preserved.argtypes = [vp]
    L.prosper_host_rt_reference_release_preserved.restype = None
    L.prosper_host_rt_reference_record.argtypes = [
        vp, vp, u32, u32, C.POINTER(RecordOptions), u32, C.POINTER(S.TileDesc), u32, vp, C.POINTER(S.ReferencePC)]
    L.prosper_host_rt_direct_illumination_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_rt_direct_illumination_destroy.argtypes = [vp]
    L.prosper_host_rt_direct_illumination_destroy.restype = None
    L.prosper_host_rt_direct_illumination_draw_ui.argtypes = [vp, C.c_int]
    L.prosper_host_rt_direct_illumination_draw_ui.restype = None
    L.prosper_host_rt_direct_illumination_recompile_shaders.argtypes = [vp]
    L.prosper_host_rt_direct_illumination_recompile_shaders.restype = None
    L.prosper_host_rt_direct_illumination_release_preserved.argtypes = [vp]
    L.prosper_host_rt_direct_illumination_release_preserved.restype = None
    L.prosper_host_rt_direct_illumination_record.argtypes = [
        vp, vp, u32, u32, C.POINTER(S.RestirInputs), C.c_int, u32, u32, vp, C.POINTER(S.RestirTracePC)]
    L.prosper_host_gbuffer_tracer_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_gbuffer_tracer_destroy.argtypes = [vp]
    L.prosper_host_gbuffer_tracer_destroy.restype = None
    L.prosper_host_gbuffer_tracer_set_opaque_only.argtypes = [vp, C.c_int]
    L.prosper_host_gbuffer_tracer_set_texture_lod.argtypes = [vp, C.c_int, C.c_float]
    L.prosper_host_renderer_lod_bias.argtypes = [C.c_int]
    L.prosper_host_renderer_lod_bias.restype = C.c_float
    L.prosper_host_gbuffer_tracer_record.argtypes = [vp, vp, u32, u32, u32, u32, C.c_int, vp, C.POINTER(S.RestirInputs)]
    L.prosper_host_gbuffer_tracer_record_velocity.argtypes = [vp, vp, u32, u32, u32, u32, vp, u32, vp, C.POINTER(S.RestirInputs),
                                                              C.POINTER(vp)]
    L.prosper_host_light_clustering_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_light_clustering_destroy.argtypes = [vp]
    L.prosper_host_light_clustering_destroy.restype = None
    L.prosper_host_light_clustering_record.argtypes = [vp, vp, u32, u32, vp]
    L.prosper_host_deferred_shading_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_deferred_shading_destroy.argtypes = [vp]
    L.prosper_host_deferred_shading_destroy.restype = None
    L.prosper_host_deferred_shading_record.argtypes = [
        vp, vp, u32, u32, C.POINTER(S.RestirInputs), C.c_int, u32, vp, C.POINTER(S.DeferredShadingPC)]
    L.prosper_host_image_based_lighting_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_image_based_lighting_destroy.argtypes = [vp]
    L.prosper_host_image_based_lighting_destroy.restype = None
    L.prosper_host_image_based_lighting_is_generated.argtypes = [vp]
    L.prosper_host_image_based_lighting_record_generation.argtypes = [vp, vp]
    L.prosper_host_skybox_renderer_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_skybox_renderer_destroy.argtypes = [vp]
    L.prosper_host_skybox_renderer_destroy.restype = None
    L.prosper_host_skybox_renderer_record.argtypes = [vp, vp, u32, u32, vp, u32, vp]
    L.prosper_pt_raster_release_preserved.argtypes = [vp]
    L.prosper_host_gbuffer_renderer_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_gbuffer_renderer_destroy.argtypes = [vp]
    L.prosper_host_gbuffer_renderer_destroy.restype = None
    L.prosper_host_gbuffer_renderer_record.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp, C.POINTER(S.GBufferRendererOutput)]
    L.prosper_host_gbuffer_renderer_read_draw_stats.argtypes = [vp, C.POINTER(S.DrawStats), u32]
    L.prosper_host_gbuffer_renderer_release_preserved.argtypes = [vp]
    L.prosper_host_meshlet_culler_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_meshlet_culler_destroy.argtypes = [vp]
    L.prosper_host_meshlet_culler_destroy.restype = None
    L.prosper_host_meshlet_culler_record_first_phase.argtypes = [vp, u32, vp, u32, u32, u32, C.POINTER(S.MeshletCullerOutput), vp]
    L.prosper_host_meshlet_culler_record_second_phase.argtypes = [vp, vp, u32, u32, u32, C.POINTER(S.MeshletCullerOutput), vp]
    L.prosper_host_meshlet_culler_read_draw_stats.argtypes = [vp, C.POINTER(S.DrawStats), u32]
    L.prosper_host_hiz_downsampler_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_hiz_downsampler_destroy.argtypes = [vp]
    L.prosper_host_hiz_downsampler_destroy.restype = None
    L.prosper_host_hiz_downsampler_record.argtypes = [vp, vp, u32, u32, u32, u32, C.POINTER(u32), C.POINTER(vp), vp]
    L.prosper_host_forward_renderer_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_forward_renderer_destroy.argtypes = [vp]
    L.prosper_host_forward_renderer_set_texture_lod.argtypes = [vp, C.c_int, C.c_float]
    L.prosper_host_forward_renderer_destroy.restype = None
    L.prosper_host_forward_renderer_record_opaque.argtypes = [vp, vp, u32, u32, C.c_int, u32, vp, u32, vp, C.POINTER(S.ForwardRendererOutput)]
    L.prosper_host_forward_renderer_release_preserved.argtypes = [vp]
    L.prosper_host_forward_renderer_record_transparent_raster.argtypes = [vp, vp, u32, u32, vp, u32, C.c_int, u32, vp, C.POINTER(S.ForwardPC)]
    L.prosper_host_forward_renderer_record_transparent.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, C.c_int, u32, vp,
                                                                   C.POINTER(S.ForwardPC)]
    L.prosper_host_particles_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_particles_destroy.argtypes = [vp]
    L.prosper_host_particles_destroy.restype = None
    L.prosper_host_particles_set_source.argtypes = [vp, u32]
    L.prosper_host_particles_set_source.restype = None
    L.prosper_host_particles_set_max_particle_count.argtypes = [vp, u32]
    L.prosper_host_particles_set_max_particle_count.restype = None
    L.prosper_host_particles_record.argtypes = [vp, vp, u32, u32, vp, C.c_float, vp, C.POINTER(S.ParticlesPC),
                                                C.POINTER(u32)]
    L.prosper_host_debug_lines_create.argtypes = [C.POINTER(vp)]
    L.prosper_host_debug_lines_destroy.argtypes = [vp]
    L.prosper_host_debug_lines_destroy.restype = None
    L.prosper_host_debug_lines_reset.argtypes = [vp]
    L.prosper_host_debug_lines_reset.restype = None
    L.prosper_host_debug_lines_add_line.argtypes = [vp, vp, vp, vp]
    L.prosper_host_debug_lines_count.argtypes = [vp]
    L.prosper_host_debug_lines_count.restype = u32
    L.prosper_host_debug_lines_data.argtypes = [vp]
    L.prosper_host_debug_lines_data.restype = vp
    L.prosper_host_debug_renderer_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_debug_renderer_destroy.argtypes = [vp]
    L.prosper_host_debug_renderer_destroy.restype = None
    L.prosper_host_debug_renderer_record.argtypes = [vp, vp, vp, u32, u32, vp]
    L.prosper_host_texture_readback_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_texture_readback_destroy.argtypes = [vp]
    L.prosper_host_texture_readback_destroy.restype = None
    L.prosper_host_texture_readback_start_frame.argtypes = [vp]
    L.prosper_host_texture_readback_frames_until_ready.argtypes = [vp]
    L.prosper_host_texture_readback_frames_until_ready.restype = i32
    L.prosper_host_texture_readback_record.argtypes = [vp, u32, C.c_float, C.c_float, vp]
    L.prosper_host_texture_readback_readback.argtypes = [vp, C.POINTER(C.c_float * 4), C.POINTER(u32)]
    L.prosper_host_texture_debug_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_texture_debug_destroy.argtypes = [vp]
    L.prosper_host_texture_debug_destroy.restype = None
    L.prosper_host_texture_debug_set_target.argtypes = [vp, C.c_char_p]
    L.prosper_host_texture_debug_set_target.restype = None
    L.prosper_host_texture_debug_texture_selected.argtypes = [vp]
    L.prosper_host_texture_debug_set_settings.argtypes = [vp, C.c_char_p, C.c_float, C.c_float, i32, u32, C.c_int, C.c_int]
    L.prosper_host_texture_debug_set_settings.restype = None
    L.prosper_host_texture_debug_set_zoom.argtypes = [vp, C.c_int]
    L.prosper_host_texture_debug_set_zoom.restype = None
    L.prosper_host_texture_debug_record.argtypes = [vp, u32, u32, vp, vp, vp, C.c_size_t, vp, C.POINTER(S.TextureDebugPC)]
    L.prosper_host_texture_debug_peeked_value.argtypes = [vp, C.POINTER(C.c_float * 4)]
    L.prosper_host_depth_of_field_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_depth_of_field_destroy.argtypes = [vp]
    L.prosper_host_depth_of_field_destroy.restype = None
    L.prosper_host_depth_of_field_record.argtypes = [vp, vp, u32, u32, C.POINTER(S.DofInputs), vp, C.POINTER(S.DofPC)]
    L.prosper_host_bloom_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_bloom_destroy.argtypes = [vp]
    L.prosper_host_bloom_destroy.restype = None
    L.prosper_host_bloom_draw_ui.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float, u32, u32]
    L.prosper_host_bloom_draw_ui.restype = None
    L.prosper_host_bloom_set_technique.argtypes = [vp, u32, u32]
    L.prosper_host_bloom_set_technique.restype = None
    L.prosper_host_bloom_release_preserved.argtypes = [vp]
    L.prosper_host_bloom_release_preserved.restype = None
    L.prosper_host_bloom_fft_push_constants.argtypes = [vp, C.POINTER(S.BloomFftPC)]
    L.prosper_host_bloom_fft_push_constants.restype = None
    L.prosper_host_bloom_record.argtypes = [vp, u32, u32, vp, u32, vp, C.POINTER(S.BloomPC)]
    L.prosper_host_taa_create.argtypes = [vp, C.POINTER(vp)]
    L.prosper_host_taa_destroy.argtypes = [vp]
    L.prosper_host_taa_destroy.restype = None
    L.prosper_host_taa_draw_ui.argtypes = [vp, u32, u32, u32, u32]
    L.prosper_host_taa_draw_ui.restype = None
    L.prosper_host_taa_record.argtypes = [vp, u32, u32, C.POINTER(S.TaaInputs), vp, C.POINTER(S.TaaPC)]
    L.prosper_host_taa_release_preserved.argtypes = [vp]
    L.prosper_host_taa_release_preserved.restype = None
    L.prosper_host_animations_create.argtypes = [vp, C.POINTER(S.AnimationDesc), C.POINTER(vp)]
    L.prosper_host_animations_destroy.argtypes = [vp]
    L.prosper_host_animations_destroy.restype = None
    L.prosper_host_animations_update.argtypes = [vp, C.c_float]
    L.prosper_host_animations_end_time.argtypes = [vp]
    L.prosper_host_animations_end_time.restype = C.c_float
    L.prosper_host_tiled_rt_reference_create.argtypes = [i32, u32, u32, vp, u32, u32, C.POINTER(vp)]
    L.prosper_host_tiled_rt_reference_destroy.argtypes = [vp]
    L.prosper_host_tiled_rt_reference_destroy.restype = None
    L.prosper_host_tiled_rt_reference_context.argtypes = [vp]
    L.prosper_host_tiled_rt_reference_context.restype = vp
    L.prosper_host_tiled_rt_reference_set_scene.argtypes = [vp, C.POINTER(S.SceneView)]
    L.prosper_host_tiled_rt_reference_record.argtypes = [
        vp, vp, u32, u32, C.POINTER(RecordOptions), u32, u32, vp, C.POINTER(C.POINTER(C.c_float))]
    L.prosper_host_tiled_rt_reference_wait_for_gather.argtypes = [vp, vp]
    L.prosper_host_tone_map_create.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.prosper_host_tone_map_create_from_texels.argtypes = [vp, vp, u32, C.POINTER(vp)]
    L.prosper_host_tone_map_destroy.argtypes = [vp]
    L.prosper_host_tone_map_destroy.restype = None
    L.prosper_host_tone_map_draw_ui.argtypes = [vp, C.c_float, C.c_float]
    L.prosper_host_tone_map_draw_ui.restype = None
    L.prosper_host_tone_map_record.argtypes = [vp, vp, vp, C.c_size_t]
    _lib = L
    return L


class RecordOptions(C.Structure):
    """prosper_host_record_options == RtReference::Options (src/render/RtReference.hpp:44-50)"""

    _fields_ = [("depthOfField", C.c_uint32), ("ibl", C.c_uint32), ("colorDirty", C.c_uint32),
                ("drawType", C.c_uint32)]


def compressed_texture_layout(width, height, mips=True):
    """What prosper's compress() decides for an extent -> (PROSPER_PT_FORMAT_*, level count, payload bytes)."""
    fmt, levels, nbytes = C.c_uint32(), C.c_uint32(), C.c_uint64()
    _check(lib().prosper_pt_compressed_texture_layout(width, height, int(bool(mips)), C.byref(fmt), C.byref(levels), C.byref(nbytes)))
    return fmt.value, levels.value, nbytes.value


def _check(rc):
    if rc != 0:
        raise ProsperPtError(rc, lib().prosper_pt_last_error().decode())


def _tile_ref(tile):
    return C.byref(tile) if tile is not None else None


def dof_sample_offsets():
    """prosper_pt_dof_sample_offsets: the octaweb's 121 unit offsets, float32 [121, 2] (needs no GPU)."""
    out = np.empty((S.DOF_TAPS, 2), np.float32)
    lib().prosper_pt_dof_sample_offsets(out.ctypes.data)
    return out


def taa_jitter(jitter_index, width, height):
    """prosper_pt_taa_jitter: Camera::perspective's jitter of sample `jitter_index` of the Halton(2, 3) cycle, float32 [2]"""
    out = (C.c_float * 2)()
    lib().prosper_pt_taa_jitter(jitter_index, width, height, C.byref(out))
    return np.array(out[:], np.float32)


def bloom_streak_weights(half_width):
    """prosper_pt_bloom_streak_weights: (rg, b), float32 [2 * half_width] each, for i = -half_width .. half_width - 1
    (needs no GPU)."""
    rg, b = np.empty(2 * half_width, np.float32), np.empty(2 * half_width, np.float32)
    lib().prosper_pt_bloom_streak_weights(half_width, rg.ctypes.data, b.ctypes.data)
    return rg, b


def bloom_fft_plan(width, height, resolution_scale=0):
    """prosper_pt_bloom_fft_plan: S.BloomFftPlan of an extent (needs no GPU); ProsperPtError on one bloom_fft refuses."""
    plan = S.BloomFftPlan()
    _check(lib().prosper_pt_bloom_fft_plan(width, height, resolution_scale, C.byref(plan)))
    return plan


def magic_divisor(divisor):
    """prosper_pt_debug_magic_divisor: (mul, sh1, sh2) with n // divisor == (t + ((n - t) >> sh1)) >> sh2, t = (mul * n) >> 32,
    for every 32-bit n - the terms the wavefront kernels divide by a launch's tile counts with.  Needs no device."""
    mul, shifts = C.c_uint32(), C.c_uint32()
    lib().prosper_pt_debug_magic_divisor(divisor, C.byref(mul), C.byref(shifts))
    return mul.value, shifts.value & 0xFF, shifts.value >> 8


def has_experiments():
    """prosper_pt_has_experiments: always False (the measured-slower variants were removed from the library); kept for the
    ABI and for tests/conftest.py."""
    return bool(lib().prosper_pt_has_experiments())


# Process-wide debug options of THIS BINDING (tests, sweeps): every Context applies them - on top of the library's defaults
# and under its own set_debug() - before its next upload, update or render.  The library keeps options per context and
# never reads the environment; this dict is what monkeypatch.setenv used to be for the tests.
_debug_defaults = {}
_debug_version = 0


def debug(**options):
    """capi.debug(ldsStackEntries=16) sets, capi.debug(ldsStackEntries=None) clears a process-wide option; capi.debug()
    with no argument clears them all."""
    global _debug_version
    if not options:
        _debug_defaults.clear()
    for k, v in options.items():
        if k not in dict(S.DebugOptions._fields_):
            raise KeyError("unknown debug option %r" % k)
        if v is None:
            _debug_defaults.pop(k, None)
        else:
            _debug_defaults[k] = v
    _debug_version += 1


class Context:
    """One prosper_pt context = one GPU (prosper_pt_create .. prosper_pt_destroy)."""

    def __init__(self, device=0, flags=0, _borrowed=None):
        self._owned = _borrowed is None
        self._own_debug = {}
        self._base_debug = None
        self._debug_seen = -1
        self._world = None
        self._animation_nodes = 0
        self._restir_extent = None
        if _borrowed is not None:
            self._h = C.c_void_p(_borrowed)
            return
        desc = S.DeviceDesc(C.sizeof(S.DeviceDesc), device, flags, 0)
        h = C.c_void_p()
        _check(lib().prosper_pt_create(C.byref(desc), C.byref(h)))
        self._h = h

    def set_debug(self, **options):
        """This context's debug options (prosper_pt_set_debug_options): ctx.set_debug(segments=2560); None clears one,
        no argument clears all.  Applied with the process-wide capi.debug() options before the next call."""
        if not options:
            self._own_debug = {}
        for k, v in options.items():
            if k not in dict(S.DebugOptions._fields_):
                raise KeyError("unknown debug option %r" % k)
            if v is None:
                self._own_debug.pop(k, None)
            else:
                self._own_debug[k] = v
        self._debug_seen = -1
        self._sync_debug()

    def debug_options(self):
        o = S.DebugOptions()
        _check(lib().prosper_pt_get_debug_options(self._h, C.byref(o)))
        return o

    def _sync_debug(self):
        if self._debug_seen == _debug_version:
            return
        if self._base_debug is None:
            # what the context was created with: the library's defaults, or PROSPER_PT_DEBUG_OPTIONS under PROSPER_PT_DEBUG=1
            self._base_debug = self.debug_options()
        o = S.DebugOptions.from_buffer_copy(bytes(self._base_debug))
        for k, v in list(_debug_defaults.items()) + list(self._own_debug.items()):
            setattr(o, k, v)
        _check(lib().prosper_pt_set_debug_options(self._h, C.byref(o)))
        self._debug_seen = _debug_version

    def close(self):
        if getattr(self, "_h", None) and self._owned:
            lib().prosper_pt_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, world):
        self._sync_debug()
        view = world.view()
        _check(lib().prosper_pt_upload_scene(self._h, C.byref(view)))
        self._world = world

    def update_lights(self, world):
        world.freeze()  # "honor scene lighting": a scene with punctual lights and no sun of its own has none (WorldData.cpp:1537-1542)
        _check(lib().prosper_pt_update_lights(self._h, C.byref(world.directional), C.byref(world.point_lights),
                                              C.byref(world.spot_lights)))

    def update_transforms(self, world, stream=None, now=None):
        """New ModelInstanceTransforms of the uploaded scene from `world` (same scene, moved instances).  The table is
        staged and the refit runs at the head of the next render's own chain of launches; with `now` (default: whenever a
        stream is given) it is enqueued on `stream` by this call instead (PROSPER_PT_UPDATE_NOW; stream None / 0 = the
        null stream)."""
        self._sync_debug()
        world._frozen = None
        f = world.freeze()
        t = f["transforms"]
        if now is None:
            now = stream is not None
        _check(lib().prosper_pt_update_transforms_async(self._h, C.cast(t, C.c_void_p), len(world.model_instances),
                                                         S.UPDATE_NOW if now else 0, C.c_void_p(stream)))
        self._world = world

    # ---- keyframe animation (prosper_amd/animation.py makes the tables of a glTF) ----
    def set_animations(self, tables):
        """The node tree and channels of the uploaded scene: an `animation.AnimationTables`."""
        desc = tables.desc()
        _check(lib().prosper_pt_set_animations(self._h, C.byref(desc)))
        self._animation_nodes = len(tables.nodes)

    def animate(self, time_s, stream=None, now=None):
        """World::updateAnimations(timeS) + updateScene: staged; the kernels run ahead of the refit at the head of the next
        render's chain, or on `stream` inside the call with `now` (default: whenever a stream is given)."""
        if now is None:
            now = stream is not None
        _check(lib().prosper_pt_animate(self._h, float(time_s), S.UPDATE_NOW if now else 0, C.c_void_p(stream)))

    def animation_state(self):
        st = S.AnimationStateInfo()
        _check(lib().prosper_pt_get_animation_state(self._h, C.byref(st)))
        return st

    def read_animated_transforms(self, previous=False):
        """The ModelInstanceTransforms table the device holds (or held before the last animated update): a ctypes array
        that prosper_pt_update_transforms / a velocity trace's previousTransforms take as it is."""
        n = len(self._world.model_instances)
        out = (S.ModelInstanceTransforms * max(1, n))()
        _check(lib().prosper_pt_read_animated_transforms(self._h, 1 if previous else 0, C.cast(out, C.c_void_p), n))
        return out

    def read_lights(self):
        """(DirectionalLightParameters, PointLightsBuffer, SpotLightsBuffer) as the device holds them."""
        d, p, s = S.DirectionalLightParameters(), S.PointLightsBuffer(), S.SpotLightsBuffer()
        _check(lib().prosper_pt_read_lights(self._h, C.byref(d), C.byref(p), C.byref(s)))
        return d, p, s

    def read_animation_nodes(self):
        """Test hook: (trs [nodes, 10], world [nodes, 4, 4] with world[n, column, row]) of the last update."""
        n = self._animation_nodes
        trs, world = np.zeros((n, 10), np.float32), np.zeros((n, 4, 4), np.float32)
        _check(lib().prosper_pt_debug_read_animation_nodes(self._h, trs.ctypes.data, world.ctypes.data, n))
        return trs, world

    def update_textures(self, textures, first):
        """Replaces materialTextures[first .. first + len(textures)): numpy [h, w, 4] uint8 arrays, world.Bc7Texture or
        world.TextureChain."""
        from .world import fill_texture_desc
        self._sync_debug()
        descs = (S.TextureDesc * len(textures))()
        keep = [fill_texture_desc(descs[i], t) for i, t in enumerate(textures)]
        _check(lib().prosper_pt_update_textures(self._h, C.cast(descs, C.c_void_p), first, len(textures)))
        del keep

    def texture_mips_info(self, texture):
        """structs.TextureMipsInfo of materialTextures[texture] (a CREATE_TEXTURE_MIPS context)."""
        info = S.TextureMipsInfo()
        _check(lib().prosper_pt_get_texture_mips_info(self._h, texture, C.byref(info)))
        return info

    def read_texture_level(self, texture, level, width, height, stream=None):
        """Level `level` of materialTextures[texture] as the device holds it: uint8 [h, w, 4] of the LEVEL's extent,
        derived from the level-0 extent given."""
        w, h = max(width >> level, 1), max(height >> level, 1)
        out = np.zeros((h, w, 4), np.uint8)
        _check(lib().prosper_pt_read_texture_level(self._h, texture, level, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def compress_texture(self, texture, srgb=False, mips=True, stream=None):
        """prosper's compress() on the GPU: a numpy [h, w, 4] uint8 array (its chain is generated when `mips`; `srgb`:
        in linear light) or a world.TextureChain / list of levels (taken as it is) -> (PROSPER_PT_FORMAT_*, [payload
        bytes of every level]): BC7 blocks when every level divides by 4, otherwise the raw RGBA8 chain."""
        from .world import TextureChain, fill_texture_desc
        if isinstance(texture, (list, tuple)):
            texture = TextureChain(texture)
        desc = S.TextureDesc()
        keep = fill_texture_desc(desc, texture)
        supplied = desc.mipLevelCount if desc.mipLevelCount > 1 else 0
        levels = supplied or (lib().prosper_pt_texture_mip_level_count(desc.width, desc.height) if mips else 1)
        extents = [(max(desc.width >> l, 1), max(desc.height >> l, 1)) for l in range(levels)]
        bc7 = desc.format == S.FORMAT_RGBA8_UNORM and all(w % 4 == 0 and h % 4 == 0 for w, h in extents)
        sizes = [(w // 4) * (h // 4) * 16 if bc7 else w * h * 4 for w, h in extents]
        out = np.zeros(max(sum(sizes), 1), np.uint8)
        flags = (S.COMPRESS_SRGB if srgb else 0) | (S.COMPRESS_GENERATE_MIPS if mips else 0)
        _check(lib().prosper_pt_compress_texture(self._h, C.byref(desc), flags, out.ctypes.data, sum(sizes), C.c_void_p(stream)))
        del keep
        offsets = np.concatenate([[0], np.cumsum(sizes)])
        return (S.FORMAT_BC7_UNORM if bc7 else S.FORMAT_RGBA8_UNORM), [out[offsets[l]:offsets[l + 1]].tobytes() for l in range(levels)]

    def compress_texture_timing(self):
        """(prepare, encode, read back) device milliseconds of the last compress_texture."""
        ms = [C.c_float(), C.c_float(), C.c_float()]
        _check(lib().prosper_pt_get_compress_texture_timing(self._h, *[C.byref(m) for m in ms]))
        return tuple(m.value for m in ms)

    def debug_bc7_encode_blocks(self, texels, mode_mask=0, stream=None):
        """Test hook: the encoder's device function over uint8 [n, 16, 4] loose blocks -> (blocks uint8 [n, 16],
        sse uint32 [n]); mode_mask as bc7.encode_blocks."""
        texels = np.ascontiguousarray(texels, np.uint8).reshape(-1, 16, 4)
        n = texels.shape[0]
        blocks, sse = np.zeros((n, 16), np.uint8), np.zeros(n, np.uint32)
        _check(lib().prosper_pt_debug_bc7_encode_blocks(
            self._h, texels.ctypes.data, n, mode_mask, blocks.ctypes.data, sse.ctypes.data, C.c_void_p(stream)))
        return blocks, sse

    def prepare_mesh(self, positions, indices, normals=None, tangents=None, uvs=None, generate_tangents=True, meshlets=True, stream=None):
        """prosper's loadNextMesh on the GPU: a primitive's accessors -> (header dict, blob words, tangents), what
        mesh_cache.pack_cache(..., with_meshlets=meshlets, ordered=True) gives.  `generate_tangents` acts when `tangents`
        is None and `uvs` is not (tangents.generate_tangents, on the GPU); the third result is then the float32 [n, 4]
        tangents, otherwise None."""
        arrays = {"positions": np.ascontiguousarray(positions, np.float32).reshape(-1, 3), "indices": np.ascontiguousarray(indices, np.uint32).reshape(-1)}
        n = arrays["positions"].shape[0]
        for name, value, width in (("normals", normals, 3), ("tangents", tangents, 4), ("texCoord0s", uvs, 2)):
            if value is not None:
                arrays[name] = np.ascontiguousarray(value, np.float32).reshape(n, width)
        src = S.MeshSource(vertexCount=n, indexCount=arrays["indices"].size)
        for name, a in arrays.items():
            setattr(src, name, a.ctypes.data if a.size else None)
        flags = (S.PREPARE_GENERATE_TANGENTS if generate_tangents else 0) | (S.PREPARE_MESHLETS if meshlets else 0)
        out = S.PreparedMesh()
        _check(lib().prosper_pt_prepare_mesh(self._h, C.byref(src), flags, C.byref(out), C.c_void_p(stream)))
        header = {name: getattr(out, name) for name, _ in S.PreparedMesh._fields_}
        blob = np.zeros(out.blobByteCount // 4, np.uint32)
        _check(lib().prosper_pt_read_prepared_mesh(self._h, blob.ctypes.data, blob.nbytes))
        generated = None
        if generate_tangents and tangents is None and uvs is not None:
            generated = np.zeros((n, 4), np.float32)
            _check(lib().prosper_pt_read_prepared_tangents(self._h, generated.ctypes.data, generated.nbytes))
        return header, blob, generated

    def prepare_mesh_timing(self):
        """(tangents, pack, meshlet partition on the host, bounds, read back) milliseconds of the last prepare_mesh."""
        ms = [C.c_float() for _ in range(5)]
        _check(lib().prosper_pt_get_prepare_mesh_timing(self._h, *[C.byref(m) for m in ms]))
        return tuple(m.value for m in ms)

    def set_texture_lod(self, enabled, lod_bias=0.0):
        """The traced G-buffer samples materials through the mip chains (a CREATE_TEXTURE_MIPS context), with `lod_bias`."""
        _check(lib().prosper_pt_set_texture_lod(self._h, int(bool(enabled)), lod_bias))

    def set_texture_lod_debug(self, enabled):
        _check(lib().prosper_pt_set_texture_lod_debug(self._h, int(bool(enabled))))

    def read_texture_lod_derivatives(self, width, height, stream=None):
        """float32 [h, w, 4] = (du/dx, dv/dx, du/dy, dv/dy) the last traced G-buffer sampled with (zeros on a miss)."""
        out = np.zeros((height, width, 4), np.float32)
        _check(lib().prosper_pt_read_texture_lod_derivatives(self._h, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def debug_sample_texture_lod(self, texture, sampler, records, bias=0.0):
        """sample_texture_lod over float32 [n, 6] records (u, v, du/dx, dv/dx, du/dy, dv/dy) -> float32 [n, 5]
        (R, G, B, A, lambda)."""
        self._sync_debug()
        rec = np.ascontiguousarray(records, np.float32).reshape(-1, 6)
        out = np.zeros((rec.shape[0], 5), np.float32)
        _check(lib().prosper_pt_debug_sample_texture_lod(self._h, texture, sampler, rec.ctypes.data, rec.shape[0], bias, out.ctypes.data))
        return out

    def update_materials(self, materials, first):
        """Replaces MaterialData[first .. first + len(materials)) (structs.MaterialData)."""
        self._sync_debug()
        arr = (S.MaterialData * len(materials))(*materials)
        _check(lib().prosper_pt_update_materials(self._h, C.cast(arr, C.c_void_p), first, len(materials)))

    def update_meshes(self, world, mesh_indices, wait=True):
        """Hands over meshes of `world` (a World that holds them) that the uploaded scene marked as not loaded
        (World.with_meshes_loaded): metadata, MeshInfo and the mesh's bytes of its geometry buffer.  wait: also
        prosper_pt_finish_mesh_updates - the next render shows them (otherwise the first render after the context's worker
        thread has built their geometry does)."""
        self._sync_debug()
        f = world.freeze()
        ups = (S.MeshUpdate * max(1, len(mesh_indices)))()
        for u, i in zip(ups, mesh_indices):
            buffer_index, first_word, words = world.mesh_ranges[i]
            buf = f["geometry_buffers"][buffer_index]
            u.meshIndex = i
            u.metadata = world.metadatas[i]
            u.info = world.mesh_infos[i]
            u.bytes = buf.ctypes.data + 4 * first_word
            u.byteOffset, u.byteCount, u.bufferByteSize = 4 * first_word, 4 * words, buf.nbytes
        _check(lib().prosper_pt_update_meshes(self._h, C.cast(ups, C.c_void_p), len(mesh_indices)))
        if wait:
            self.finish_mesh_updates()

    def finish_mesh_updates(self):
        _check(lib().prosper_pt_finish_mesh_updates(self._h))

    def rebuild_hierarchy(self):
        self._sync_debug()
        _check(lib().prosper_pt_rebuild_hierarchy(self._h))

    def hierarchy_state(self):
        st = S.HierarchyState()
        _check(lib().prosper_pt_get_hierarchy_state(self._h, C.byref(st)))
        return st

    def read_nodes(self):
        """The node array as the device holds it: (nodeCount, 20) uint32 (80-byte nodes)."""
        n = int(self.scene_stats().nodeCount)
        out = np.zeros((n, 20), np.uint32)
        _check(lib().prosper_pt_debug_read_nodes(self._h, out.ctypes.data, out.nbytes))
        return out

    def build_hierarchy_gpu(self):
        """prosper_pt_build_hierarchy_gpu: the whole tree again, made on the device (prosper_amd/lbvh.py states the rule)."""
        self._sync_debug()
        _check(lib().prosper_pt_build_hierarchy_gpu(self._h))

    def set_hierarchy_builder(self, builder):
        """structs.BUILDER_HOST (the default) or BUILDER_GPU: who rebuilds - prosper_pt_rebuild_hierarchy and the drift trigger."""
        _check(lib().prosper_pt_set_hierarchy_builder(self._h, builder))

    def set_gpu_hierarchy_method(self, method, radius=0):
        """structs.GPU_HIERARCHY_LINEAR (the default) or GPU_HIERARCHY_PLOC with a search radius of 1 .. 32 (0: the default):
        how every later GPU build makes its binary tree (prosper_amd/ploc.py states the PLOC rule)."""
        _check(lib().prosper_pt_set_gpu_hierarchy_method(self._h, method, radius))

    def gpu_hierarchy_method_info(self):
        """The selected method and radius, and method, radius and rounds of the build that made the tree in use."""
        info = S.GpuHierarchyMethodInfo()
        _check(lib().prosper_pt_get_gpu_hierarchy_method_info(self._h, C.byref(info)))
        return info

    def set_gpu_hierarchy_sites(self, sites):
        """A mask of structs.GPU_BUILD_SITE_UPLOAD, _MESH_UPDATES and _DRIFT (0, the default: none): the builds besides
        rebuilds that the GPU builder makes - the scene's first tree, the worker thread's generations, the drift re-split."""
        _check(lib().prosper_pt_set_gpu_hierarchy_sites(self._h, sites))

    def gpu_hierarchy_sites(self):
        sites = C.c_uint32(0)
        _check(lib().prosper_pt_get_gpu_hierarchy_sites(self._h, C.byref(sites)))
        return int(sites.value)

    def hierarchy_build_info(self):
        info = S.HierarchyBuildInfo()
        _check(lib().prosper_pt_get_hierarchy_build_info(self._h, C.byref(info)))
        return info

    def read_hierarchy_arrays(self):
        """The flat world triangles, (n, 12) uint32 words, and the leaf-order permutation, (n,) uint32, as the device holds them."""
        n = int(self.scene_stats().triangleCount)
        tris, perm = np.zeros((n, 12), np.uint32), np.zeros(n, np.uint32)
        _check(lib().prosper_pt_debug_read_hierarchy_arrays(self._h, tris.ctypes.data, tris.nbytes, perm.ctypes.data, perm.nbytes))
        return tris, perm

    def scene_stats(self):
        self._sync_debug()
        st = S.SceneStats()
        _check(lib().prosper_pt_get_scene_stats(self._h, C.byref(st)))
        return st

    def set_output_buffer(self, device_ptr, byte_size):
        _check(lib().prosper_pt_set_output_buffer(self._h, C.c_void_p(device_ptr), byte_size))

    def render(self, pc, camera, width, height, tile=None, frames=1, flags=0, stream=None):
        self._sync_debug()
        _check(lib().prosper_pt_render_frames(self._h, C.byref(pc), C.byref(camera), width, height, _tile_ref(tile),
                                              frames, flags, C.c_void_p(stream)))

    def local_extent(self):
        lw, h = C.c_uint32(), C.c_uint32()
        _check(lib().prosper_pt_get_local_extent(self._h, C.byref(lw), C.byref(h)))
        return lw.value, h.value

    def hdr_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().prosper_pt_get_hdr_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def read_hdr(self, stream=None):
        lw, h = self.local_extent()
        out = np.empty((h, lw, 4), np.float32)
        _check(lib().prosper_pt_read_hdr(self._h, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def blit_rgba16f(self, stream=None):
        lw, h = self.local_extent()
        out = np.empty((h, lw, 4), np.float16)
        _check(lib().prosper_pt_blit_rgba16f(self._h, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def restir_di_trace(self, pc, camera, albedo_roughness, normal_metallic, depth, reservoirs, stream=None):
        """ReSTIR-DI trace over host G-buffer arrays ([h, w, 4], [h, w, 4], [h, w], [h, w, 2] float32)."""
        ar = np.ascontiguousarray(albedo_roughness, np.float32)
        nm = np.ascontiguousarray(normal_metallic, np.float32)
        dp = np.ascontiguousarray(depth, np.float32)
        rs = np.ascontiguousarray(reservoirs, np.float32)
        h, w = dp.shape
        assert ar.shape == (h, w, 4) and nm.shape == (h, w, 4) and rs.shape == (h, w, 2)
        inp = S.RestirInputs(ar.ctypes.data, nm.ctypes.data, dp.ctypes.data, rs.ctypes.data, 0, 0)
        _check(lib().prosper_pt_restir_di_trace(self._h, C.byref(pc), C.byref(camera), w, h, C.byref(inp), C.c_void_p(stream)))

    def restir_di_trace_device(self, pc, camera, width, height, ar_ptr, nm_ptr, depth_ptr, res_ptr, stream=None):
        """Same with device-resident inputs (raw device pointers, e.g. torch tensors' data_ptr())."""
        inp = S.RestirInputs(ar_ptr, nm_ptr, depth_ptr, res_ptr, 1, 0)
        _check(lib().prosper_pt_restir_di_trace(self._h, C.byref(pc), C.byref(camera), width, height, C.byref(inp),
                                                C.c_void_p(stream)))

    @staticmethod
    def _restir_host_inputs(albedo_roughness, normal_metallic, depth, reservoirs=None):
        ar = np.ascontiguousarray(albedo_roughness, np.float32)
        nm = np.ascontiguousarray(normal_metallic, np.float32)
        dp = np.ascontiguousarray(depth, np.float32)
        h, w = dp.shape
        assert ar.shape == (h, w, 4) and nm.shape == (h, w, 4)
        rs = None
        if reservoirs is not None:
            rs = np.ascontiguousarray(reservoirs, np.float32)
            assert rs.shape == (h, w, 2)
        inp = S.RestirInputs(ar.ctypes.data, nm.ctypes.data, dp.ctypes.data, None if rs is None else rs.ctypes.data, 0, 0)
        return inp, (ar, nm, dp, rs), w, h

    def restir_di_resample(self, stage, frame_index, camera, albedo_roughness, normal_metallic, depth, reservoirs=None,
                           stream=None):
        """One resampling pass (S.RESTIR_INITIAL / S.RESTIR_SPATIAL) over host G-buffer arrays shaped as for
        restir_di_trace (`reservoirs` [h, w, 2]: the spatial pass's input).  Returns the reservoirs, float32 [h, w, 2]
        (the light index's bits in [..., 0])."""
        inp, keep, w, h = self._restir_host_inputs(albedo_roughness, normal_metallic, depth, reservoirs)
        _check(lib().prosper_pt_restir_di_resample(self._h, stage, frame_index, C.byref(camera), w, h, C.byref(inp), None,
                                                   C.c_void_p(stream)))
        del keep
        self._restir_extent = (w, h)
        return self.read_restir_reservoirs(stream)

    def restir_di_resample_device(self, stage, frame_index, camera, width, height, ar_ptr, nm_ptr, depth_ptr,
                                  res_ptr=None, out_ptr=None, stream=None):
        """Same with device-resident inputs; writes `out_ptr` (device) or, with None, the context's reservoirs."""
        inp = S.RestirInputs(ar_ptr, nm_ptr, depth_ptr, res_ptr, 1, 0)
        _check(lib().prosper_pt_restir_di_resample(self._h, stage, frame_index, C.byref(camera), width, height,
                                                   C.byref(inp), C.c_void_p(out_ptr), C.c_void_p(stream)))
        if out_ptr is None:
            self._restir_extent = (width, height)

    def restir_di_record(self, pc, camera, albedo_roughness, normal_metallic, depth, spatial_reuse=True, stream=None):
        """RtDirectIllumination::record over host G-buffer arrays: initial reservoirs, optional spatial reuse, trace."""
        inp, keep, w, h = self._restir_host_inputs(albedo_roughness, normal_metallic, depth)
        flags = S.RESTIR_SPATIAL_REUSE if spatial_reuse else 0
        _check(lib().prosper_pt_restir_di_record(self._h, C.byref(pc), flags, C.byref(camera), w, h, C.byref(inp),
                                                 C.c_void_p(stream)))
        del keep
        self._restir_extent = (w, h)

    def restir_di_record_device(self, pc, camera, width, height, ar_ptr, nm_ptr, depth_ptr, spatial_reuse=True,
                                stream=None):
        inp = S.RestirInputs(ar_ptr, nm_ptr, depth_ptr, None, 1, 0)
        flags = S.RESTIR_SPATIAL_REUSE if spatial_reuse else 0
        _check(lib().prosper_pt_restir_di_record(self._h, C.byref(pc), flags, C.byref(camera), width, height,
                                                 C.byref(inp), C.c_void_p(stream)))
        self._restir_extent = (width, height)

    def restir_reservoirs_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().prosper_pt_get_restir_reservoirs_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def read_restir_reservoirs(self, stream=None, extent=None):
        """The reservoirs the last record traced with (or the last resample wrote to the context's buffers), float32
        [h, w, 2]; synchronises `stream`.  `extent` (w, h): of a record made through another handle of the context."""
        w, h = extent or self._restir_extent
        out = np.empty((h, w, 2), np.float32)
        _check(lib().prosper_pt_read_restir_reservoirs(self._h, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def trace_gbuffer(self, camera, width, height, draw_type=0, frame_index=0, jitter=True, targets=None, stream=None,
                      opaque_only=False):
        """prosper_pt_trace_gbuffer: the ray-traced G-buffer of the uploaded scene.  With `targets` None it goes to the
        context's own buffers and is read back: returns (albedoRoughness [h, w, 4], normalMetallic [h, w, 4],
        nonLinearDepth [h, w]) float32.  `targets`: three device pointers (ar, nm, depth), written; returns None.
        `opaque_only`: PROSPER_PT_GBUFFER_OPAQUE_ONLY, BLEND surfaces left to forward_transparent."""
        self._sync_debug()
        t = None if targets is None else S.GBufferTargets(*targets)
        flags = (S.GBUFFER_JITTER if jitter else 0) | (S.GBUFFER_OPAQUE_ONLY if opaque_only else 0)
        _check(lib().prosper_pt_trace_gbuffer(self._h, int(draw_type), frame_index, flags, C.byref(camera), width, height,
                                              None if t is None else C.byref(t), C.c_void_p(stream)))
        if targets is not None:
            return None
        return self.read_gbuffer(stream)

    def trace_gbuffer_velocity(self, camera, width, height, draw_type=0, frame_index=0, previous_transforms=None, targets=None,
                               velocity_ptr=None, stream=None, opaque_only=False):
        """prosper_pt_trace_gbuffer_velocity: the traced G-buffer through camera.cameraToClip's (jittered) pixel centres,
        with the velocity target.  `previous_transforms`: a ctypes array of S.ModelInstanceTransforms, one per model
        instance (None: the instances did not move).  `targets` (ar, nm, depth) and `velocity_ptr`: device pointers;
        None: the context's own buffers.  Returns (albedoRoughness, normalMetallic, nonLinearDepth, velocity [h, w, 2])
        read back, each None where the caller gave the buffer."""
        self._sync_debug()
        desc = S.VelocityGBufferDesc()
        if targets is not None:
            desc.targets = S.GBufferTargets(*targets)
        desc.velocity = velocity_ptr
        if previous_transforms is not None:
            desc.previousTransforms = C.cast(previous_transforms, C.c_void_p)
            desc.previousTransformCount = len(previous_transforms)
        flags = S.GBUFFER_OPAQUE_ONLY if opaque_only else 0
        _check(lib().prosper_pt_trace_gbuffer_velocity(self._h, int(draw_type), frame_index, flags, C.byref(camera), width, height,
                                                       C.byref(desc), C.c_void_p(stream)))
        gbuffer = (None, None, None) if targets is not None else self.read_gbuffer(stream)
        return gbuffer + (None if velocity_ptr is not None else self.read_velocity(stream),)

    def velocity_device_ptr(self):
        """The last traced velocity target: (device pointer, width, height)."""
        p, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
        _check(lib().prosper_pt_get_velocity_device_ptr(self._h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def read_velocity(self, stream=None):
        """The last traced velocity target as a host array [h, w, 2] float32; synchronises `stream`."""
        _, w, h = self.velocity_device_ptr()
        out = np.empty((h, w, 2), np.float32)
        _check(lib().prosper_pt_read_velocity(self._h, out.ctypes.data, w * h, C.c_void_p(stream)))
        return out

    def gbuffer_device_ptrs(self):
        """The last traced G-buffer: (S.RestirInputs with onDevice = 1, width, height)."""
        inp, w, h = S.RestirInputs(), C.c_uint32(), C.c_uint32()
        _check(lib().prosper_pt_get_gbuffer_device_ptrs(self._h, C.byref(inp), C.byref(w), C.byref(h)))
        return inp, w.value, h.value

    def read_gbuffer(self, stream=None):
        """The last traced G-buffer as host arrays (ar [h, w, 4], nm [h, w, 4], depth [h, w]); synchronises `stream`."""
        _, w, h = self.gbuffer_device_ptrs()
        ar, nm = np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.float32)
        depth = np.empty((h, w), np.float32)
        _check(lib().prosper_pt_read_gbuffer(self._h, ar.ctypes.data, nm.ctypes.data, depth.ctypes.data, w * h,
                                             C.c_void_p(stream)))
        return ar, nm, depth

    def restir_di_record_traced(self, pc, camera, width, height, spatial_reuse=True, jitter=True, stream=None):
        """RtDirectIllumination::record over the G-buffer it traces first (PROSPER_PT_RESTIR_TRACE_GBUFFER) with
        pc.drawType and pc.frameIndex: from the scene alone to the direct-illumination image."""
        self._sync_debug()
        flags = S.RESTIR_TRACE_GBUFFER | (S.RESTIR_SPATIAL_REUSE if spatial_reuse else 0) | (
            S.RESTIR_JITTER_GBUFFER if jitter else 0)
        _check(lib().prosper_pt_restir_di_record(self._h, C.byref(pc), flags, C.byref(camera), width, height, None,
                                                 C.c_void_p(stream)))
        self._restir_extent = (width, height)

    def cluster_lights(self, camera, width, height, stream=None):
        """LightClustering::record (prosper_pt_cluster_lights) into the context's buffers; read_light_clusters reads them."""
        self._sync_debug()
        _check(lib().prosper_pt_cluster_lights(self._h, C.byref(camera), width, height, C.c_void_p(stream)))

    def light_cluster_dims(self):
        """(x, y, z) of the last clustering."""
        x, y, z = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().prosper_pt_get_light_cluster_dims(self._h, C.byref(x), C.byref(y), C.byref(z)))
        return x.value, y.value, z.value

    def read_light_clusters(self, stream=None):
        """The last clustering: dict with pointers uint32 [z, y, x, 2], indices uint16 [z, y, x, 256], and the counters
        count (entries kept), dropped (entries past the 128 of a type), overflowing (clusters that dropped any)."""
        x, y, z = self.light_cluster_dims()
        n = x * y * z
        ptrs = np.empty((z, y, x, 2), np.uint32)
        idx = np.empty((z, y, x, S.CLUSTER_MAX_POINTS + S.CLUSTER_MAX_SPOTS), np.uint16)
        count, dropped, overflowing = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().prosper_pt_read_light_clusters(self._h, ptrs.ctypes.data, idx.ctypes.data, C.byref(count),
                                                    C.byref(dropped), C.byref(overflowing), n, C.c_void_p(stream)))
        return {"pointers": ptrs, "indices": idx, "count": count.value, "dropped": dropped.value,
                "overflowing": overflowing.value}

    def deferred_shading(self, camera, albedo_roughness, normal_metallic, depth, draw_type=0, ibl=0, stream=None):
        """LightClustering + DeferredShading over host G-buffer arrays ([h, w, 4], [h, w, 4], [h, w] float32) into the
        HDR image (read_hdr)."""
        self._sync_debug()
        inp, keep, w, h = self._restir_host_inputs(albedo_roughness, normal_metallic, depth)
        pc = S.DeferredShadingPC(int(draw_type), ibl)
        _check(lib().prosper_pt_deferred_shading(self._h, C.byref(pc), 0, 0, C.byref(camera), w, h, C.byref(inp),
                                                 C.c_void_p(stream)))
        del keep

    def deferred_shading_device(self, camera, width, height, ar_ptr, nm_ptr, depth_ptr, draw_type=0, stream=None, ibl=0):
        """Same over device G-buffer pointers."""
        self._sync_debug()
        inp = S.RestirInputs(ar_ptr, nm_ptr, depth_ptr, None, 1, 0)
        pc = S.DeferredShadingPC(int(draw_type), int(ibl))
        _check(lib().prosper_pt_deferred_shading(self._h, C.byref(pc), 0, 0, C.byref(camera), width, height,
                                                 C.byref(inp), C.c_void_p(stream)))

    def deferred_shading_traced(self, camera, width, height, draw_type=0, frame_index=0, jitter=False, stream=None,
                                ibl=0):
        """Same over the G-buffer it traces first (PROSPER_PT_DEFERRED_TRACE_GBUFFER): from the scene alone to the image."""
        self._sync_debug()
        flags = S.DEFERRED_TRACE_GBUFFER | (S.DEFERRED_JITTER_GBUFFER if jitter else 0)
        pc = S.DeferredShadingPC(int(draw_type), int(ibl))
        _check(lib().prosper_pt_deferred_shading(self._h, C.byref(pc), flags, frame_index, C.byref(camera), width,
                                                 height, None, C.c_void_p(stream)))

    def forward_transparent(self, camera, width, height, draw_type=0, ibl=0, flags=0, frame_index=0, depth=None,
                            depth_ptr=None, stream=None):
        """ForwardRenderer::recordTransparent (prosper_pt_forward_transparent): the BLEND layers of every pixel, lit over
        the light clusters and blended in place over the HDR image.  `flags`: 0 (pixel centre), S.TRANSPARENT_JITTER or
        S.TRANSPARENT_CAMERA_JITTER - the ray the G-buffer was traced with.  `depth`: a host array [h, w]; `depth_ptr`:
        a device pointer; neither: the last traced G-buffer's depth."""
        self._sync_debug()
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        assert dp is None or dp.shape == (height, width)
        ptr = depth_ptr if dp is None else dp.ctypes.data
        pc = S.ForwardPC(int(draw_type), int(ibl), 0)
        _check(lib().prosper_pt_forward_transparent(self._h, C.byref(pc), flags, frame_index, C.byref(camera), width, height,
                                                    C.c_void_p(ptr), 1 if dp is None else 0, C.c_void_p(stream)))
        self._transparent_extent = (width, height)

    def transparent_info(self):
        """S.TransparentInfo of the last forward_transparent (waits for it)."""
        info = S.TransparentInfo()
        _check(lib().prosper_pt_get_transparent_info(self._h, C.byref(info)))
        return info

    def set_transparent_debug_layers(self, layers_per_pixel):
        """Debug mode of forward_transparent: later calls record each pixel's first `layers_per_pixel` layers (0: off)."""
        _check(lib().prosper_pt_set_transparent_debug_layers(self._h, layers_per_pixel))
        self._transparent_layers = layers_per_pixel

    def read_transparent_layers(self, stream=None):
        """What the last forward_transparent in debug mode recorded: (counts uint32 [h, w], layers [h, w, N] of the
        structured dtype of S.TransparentLayer, front to back; entries past a pixel's count are unspecified)."""
        w, h = self._transparent_extent
        n = self._transparent_layers
        counts = np.empty((h, w), np.uint32)
        layers = np.empty((h, w, n), np.dtype(S.TransparentLayer))
        _check(lib().prosper_pt_read_transparent_layers(self._h, counts.ctypes.data, layers.ctypes.data, w * h, n,
                                                        C.c_void_p(stream)))
        return counts, layers

    # ---- particles (prosper_pt_particles) ----

    def particles(self, pc, stages=S.PARTICLES_ALL, camera=None, width=0, height=0, depth_ptr=None, stream=None):
        """particles::Particles::record (prosper_pt_particles): the stages `stages` names (S.PARTICLES_DECAY | _INIT |
        _SIMULATE | _RENDER) of the push constants `pc` (S.ParticlesPC) over the context's pool and freelist; render
        works in place over the HDR image and the depth.  `depth_ptr`: a device pointer the pass reads AND writes;
        None: the last traced G-buffer's depth.  `camera`, `width`, `height`: read by render only."""
        self._sync_debug()
        cam = None if camera is None else C.byref(camera)
        _check(lib().prosper_pt_particles(self._h, C.byref(pc), stages, cam, width, height, C.c_void_p(depth_ptr),
                                          C.c_void_p(stream)))
        self._particles_max = pc.maxParticleCount

    def particles_info(self):
        """S.ParticlesInfo of the last particles() (waits for it)."""
        info = S.ParticlesInfo()
        _check(lib().prosper_pt_get_particles_info(self._h, C.byref(info)))
        return info

    def read_particles(self, stream=None):
        """The pool as the device holds it: (records [max] of S.PARTICLE_DTYPE, count, indices int32 [max])."""
        asked = getattr(self, "_particles_max", 0)
        n = asked or S.MAX_PARTICLE_COUNT
        records = np.empty(n, S.PARTICLE_DTYPE)
        freelist = np.empty(n + 1, np.int32)
        _check(lib().prosper_pt_read_particles(self._h, records.ctypes.data, freelist.ctypes.data, asked, C.c_void_p(stream)))
        return records, int(freelist[0]), freelist[1:]

    def set_particles(self, records, count, indices, stream=None):
        """prosper_pt_set_particles: a designed pool.  `records` [max] of S.PARTICLE_DTYPE, `count` free slots, `indices`
        int32 [max] (all of them inside the pool; the first `count` are the free ones)."""
        rec = np.ascontiguousarray(records, S.PARTICLE_DTYPE)
        idx = np.ascontiguousarray(indices, np.int32)
        assert rec.ndim == 1 and idx.shape == rec.shape
        freelist = np.concatenate([np.array([count], np.int32), idx])
        _check(lib().prosper_pt_set_particles(self._h, rec.ctypes.data, freelist.ctypes.data, rec.size, C.c_void_p(stream)))
        self._particles_max = rec.size

    # ---- debug lines (prosper_pt_debug_lines) ----

    def debug_lines(self, lines, camera, width, height, stream=None):
        """DebugRenderer::record (prosper_pt_debug_lines): `lines` [n, 9] float32 (p0, p1, colour; a
        debug_geometry.DebugLines' .array()) drawn depth-tested, in place, over the HDR image and the last traced
        G-buffer's depth."""
        self._sync_debug()
        arr = np.ascontiguousarray(lines, np.float32).reshape(-1, 9)
        ptr = C.c_void_p(arr.ctypes.data) if arr.shape[0] else None
        _check(lib().prosper_pt_debug_lines(self._h, ptr, arr.shape[0], C.byref(camera), width, height, C.c_void_p(stream)))

    def debug_lines_info(self):
        """S.DebugLinesInfo of the last debug_lines() (waits for it)."""
        info = S.DebugLinesInfo()
        _check(lib().prosper_pt_get_debug_lines_info(self._h, C.byref(info)))
        return info

    # ---- hierarchical depth (prosper_pt_hiz_downsample) ----

    def hiz_downsample(self, width, height, slot=0, depth=None, depth_ptr=None, stream=None):
        """HierarchicalDepthDownsampler::record (prosper_pt_hiz_downsample): the minimum pyramid of a reverse-Z depth into
        `slot` (0 or 1).  `depth`: a host array [h, w]; `depth_ptr`: a device pointer; neither: the last traced
        G-buffer's depth."""
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        assert dp is None or dp.shape == (height, width)
        ptr = depth_ptr if dp is None else dp.ctypes.data
        _check(lib().prosper_pt_hiz_downsample(self._h, slot, C.c_void_p(ptr), 1 if dp is None else 0, width, height,
                                               C.c_void_p(stream)))

    def hiz_info(self, slot=0):
        """S.HizInfo of `slot` (never waits)."""
        info = S.HizInfo()
        _check(lib().prosper_pt_get_hiz_info(self._h, slot, C.byref(info)))
        return info

    def hiz_device_ptr(self, slot, level):
        """(device pointer, width, height) of one level of the slot's pyramid."""
        ptr, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
        _check(lib().prosper_pt_get_hiz_device_ptr(self._h, slot, level, C.byref(ptr), C.byref(w), C.byref(h)))
        return ptr.value, w.value, h.value

    def hiz_wait(self, slot, stream):
        """prosper_pt_hiz_wait: `stream` waits on the device for the last hiz_downsample into `slot`."""
        _check(lib().prosper_pt_hiz_wait(self._h, slot, C.c_void_p(stream)))

    def read_hiz_level(self, slot, level, stream=None):
        """One level of the slot's pyramid as float32 [h, w] (waits for it)."""
        _, w, h = self.hiz_device_ptr(slot, level)
        out = np.empty((h, w), np.float32)
        _check(lib().prosper_pt_read_hiz_level(self._h, slot, level, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def read_hiz(self, slot=0, stream=None):
        """Every level of the slot's pyramid, finest first."""
        return [self.read_hiz_level(slot, l, stream) for l in range(self.hiz_info(slot).levelCount)]

    # ---- meshlet culling (prosper_pt_cull_meshlets_*) ----

    def cull_first_phase(self, camera, mode=S.CULL_MODE_OPAQUE, hiz_slot=None, stream=None):
        """MeshletCuller::recordFirstPhase: generate the list of `mode`, cull it against `camera` and, with `hiz_slot`
        (0 or 1), against that pyramid."""
        slot = S.NO_HIZ if hiz_slot is None else hiz_slot
        _check(lib().prosper_pt_cull_meshlets_first_phase(self._h, mode, C.byref(camera), slot, C.c_void_p(stream)))

    def cull_second_phase(self, camera, hiz_slot, stream=None):
        """MeshletCuller::recordSecondPhase: the first phase's occluded list against the pyramid of `hiz_slot`."""
        _check(lib().prosper_pt_cull_meshlets_second_phase(self._h, C.byref(camera), hiz_slot, C.c_void_p(stream)))

    def cull_gbuffer(self, camera, stream=None):
        """prosper_pt_cull_gbuffer: first phase against the kept pyramid, the traced depth's pyramid, second phase."""
        _check(lib().prosper_pt_cull_gbuffer(self._h, C.byref(camera), C.c_void_p(stream)))

    def read_draw_list(self, which, stream=None):
        """-> (pairs uint32 [count, 2] of (drawInstanceIndex, meshletIndex), args uint32 [3])"""
        n, args = C.c_uint32(), (C.c_uint32 * 3)()
        _check(lib().prosper_pt_read_draw_list(self._h, which, C.byref(n), None, 0, C.byref(args), C.c_void_p(stream)))
        pairs = np.empty((n.value, 2), np.uint32)
        if n.value:
            _check(lib().prosper_pt_read_draw_list(self._h, which, C.byref(n), pairs.ctypes.data, pairs.shape[0], C.byref(args),
                                                   C.c_void_p(stream)))
        return pairs, np.array(args[:], np.uint32)

    def draw_list_device_ptr(self, which):
        """(list pointer, argument triple pointer or None, capacity in pairs)"""
        lp, ap, cap = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _check(lib().prosper_pt_get_draw_list_device_ptr(self._h, which, C.byref(lp), C.byref(ap), C.byref(cap)))
        return lp.value, ap.value, cap.value

    def draw_stats(self, wait=True):
        """S.DrawStats of the last culling calls; None with wait=False while the counts have not landed."""
        out = S.DrawStats()
        rc = lib().prosper_pt_get_draw_stats(self._h, C.byref(out), 1 if wait else 0)
        if rc == S.NOT_READY:
            return None
        _check(rc)
        return out

    def cull_stage_ms(self):
        """(generator, first-phase culler, second-phase culler) device milliseconds of the last phases (waits for them)."""
        ms = (C.c_float * 3)()
        _check(lib().prosper_pt_get_cull_stage_ms(self._h, C.byref(ms)))
        return tuple(ms)

    # ---- the rasteriser over the draw lists (prosper_pt_raster_*) ----

    def raster_meshlets(self, camera, which=S.DRAW_LIST_GENERATED, clear=True, stream=None):
        """GBufferRenderer::recordDraw: list `which` of the last culling calls into the visibility image; `clear` sets
        every key to 0 first and gives the image camera.resolution."""
        _check(lib().prosper_pt_raster_meshlets(self._h, which, S.RASTER_CLEAR if clear else 0, C.byref(camera), C.c_void_p(stream)))

    def raster_visibility(self, camera, stream=None):
        """prosper_pt_raster_visibility: both culling phases and their draws over the rasteriser's own depth."""
        _check(lib().prosper_pt_raster_visibility(self._h, C.byref(camera), C.c_void_p(stream)))

    def _raster_targets(self, entry, camera, draw_type, previous_transforms, targets, velocity_ptr, stream):
        self._sync_debug()
        desc = S.VelocityGBufferDesc()
        if targets is not None:
            desc.targets = S.GBufferTargets(*targets)
        desc.velocity = velocity_ptr
        if previous_transforms is not None:
            desc.previousTransforms = C.cast(previous_transforms, C.c_void_p)
            desc.previousTransformCount = len(previous_transforms)
        _check(entry(self._h, int(draw_type), C.byref(camera), C.byref(desc), C.c_void_p(stream)))
        gbuffer = (None, None, None) if targets is not None else self.read_gbuffer(stream)
        return gbuffer + (None if velocity_ptr is not None else self.read_velocity(stream),)

    def raster_resolve(self, camera, draw_type=0, previous_transforms=None, targets=None, velocity_ptr=None, stream=None):
        """prosper_pt_raster_resolve: the visibility image into the G-buffer targets; arguments and result as
        trace_gbuffer_velocity's.  With the context's own targets the result is the context's last G-buffer."""
        return self._raster_targets(lib().prosper_pt_raster_resolve, camera, draw_type, previous_transforms, targets, velocity_ptr, stream)

    def raster_gbuffer(self, camera, draw_type=0, previous_transforms=None, targets=None, velocity_ptr=None, stream=None):
        """prosper_pt_raster_gbuffer (GBufferRenderer::record): raster_visibility, then raster_resolve."""
        return self._raster_targets(lib().prosper_pt_raster_gbuffer, camera, draw_type, previous_transforms, targets, velocity_ptr, stream)

    def raster_release_preserved(self):
        """GBufferRenderer::releasePreserved: the next raster_visibility / raster_gbuffer has no previous pyramid."""
        _check(lib().prosper_pt_raster_release_preserved(self._h))

    # ---- the forward opaque pass over the visibility image (prosper_pt_raster_forward*) ----

    def _forward_opaque(self, entry, camera, draw_type, ibl, previous_transforms, depth_ptr, velocity_ptr, stream):
        self._sync_debug()
        pc = S.ForwardPC(int(draw_type), int(ibl), 0)
        desc = S.ForwardOpaqueDesc()
        desc.nonLinearDepth = depth_ptr
        desc.velocity = velocity_ptr
        if previous_transforms is not None:
            desc.previousTransforms = C.cast(previous_transforms, C.c_void_p)
            desc.previousTransformCount = len(previous_transforms)
        _check(entry(self._h, C.byref(pc), C.byref(camera), C.byref(desc), C.c_void_p(stream)))
        self._forward_extent = (int(camera.resolution[0]), int(camera.resolution[1]))

    def raster_forward_shade(self, camera, draw_type=0, ibl=0, previous_transforms=None, depth_ptr=None, velocity_ptr=None, stream=None):
        """prosper_pt_raster_forward_shade: the visibility image as drawn, shaded forward over the light clusters into the
        HDR image (read_hdr), with the depth (read_forward_depth) and the velocity (read_velocity) of the resolve.
        `previous_transforms`: a ctypes array of S.ModelInstanceTransforms, one per model instance; `depth_ptr`,
        `velocity_ptr`: device targets of the caller's (None: context-owned, the context's last depth and velocity)."""
        self._forward_opaque(lib().prosper_pt_raster_forward_shade, camera, draw_type, ibl, previous_transforms, depth_ptr, velocity_ptr, stream)

    def raster_forward(self, camera, draw_type=0, ibl=0, previous_transforms=None, depth_ptr=None, velocity_ptr=None, stream=None):
        """prosper_pt_raster_forward (ForwardRenderer::recordOpaque): raster_visibility, then raster_forward_shade."""
        self._forward_opaque(lib().prosper_pt_raster_forward, camera, draw_type, ibl, previous_transforms, depth_ptr, velocity_ptr, stream)

    def read_forward_depth(self, stream=None):
        """The context-owned depth of the last forward frame as a host array [h, w] float32; synchronises `stream`."""
        _, w, h = self.forward_depth_device_ptr()
        out = np.empty((h, w), np.float32)
        _check(lib().prosper_pt_read_forward_depth(self._h, out.ctypes.data, w * h, C.c_void_p(stream)))
        return out

    def forward_depth_device_ptr(self):
        """The depth of the last forward frame: (device pointer, width, height)."""
        p, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
        _check(lib().prosper_pt_get_forward_depth_device_ptr(self._h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def set_forward_debug_surfaces(self, enabled):
        """Debug mode of the forward opaque pass: later shades also record every pixel's surface."""
        _check(lib().prosper_pt_set_forward_debug_surfaces(self._h, 1 if enabled else 0))

    def read_forward_surfaces(self, stream=None):
        """What the last forward shade in debug mode recorded: [h, w] of the structured dtype of S.TransparentLayer
        (drawInstance 0xFFFFFFFF where nothing is drawn)."""
        w, h = getattr(self, "_forward_extent", (0, 0))  # (before the first shade the library refuses)
        out = np.empty((h, w), np.dtype(S.TransparentLayer))
        _check(lib().prosper_pt_read_forward_surfaces(self._h, out.ctypes.data, w * h, C.c_void_p(stream)))
        return out

    def forward_opaque_info(self):
        """S.ForwardOpaqueInfo of the last forward shade; None while it is still running (never waits)."""
        out = S.ForwardOpaqueInfo()
        rc = lib().prosper_pt_get_forward_opaque_info(self._h, C.byref(out))
        if rc == S.NOT_READY:
            return None
        _check(rc)
        return out

    # ---- the rasterised transparent pass over the draw lists (prosper_pt_raster_*transparent*) ----

    def _raster_transparent(self, entry, head, camera, draw_type, ibl, depth, depth_ptr, stream):
        self._sync_debug()
        w, h = int(camera.resolution[0]), int(camera.resolution[1])
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        assert dp is None or dp.shape == (h, w)
        ptr = depth_ptr if dp is None else dp.ctypes.data
        pc = S.ForwardPC(int(draw_type), int(ibl), 0)
        _check(entry(self._h, *head, C.byref(pc), C.byref(camera), C.c_void_p(ptr), 1 if dp is None else 0, C.c_void_p(stream)))
        self._raster_transparent_extent = (w, h)

    def raster_transparent_draw(self, camera, which=S.DRAW_LIST_FIRST_PHASE, draw_type=0, ibl=0, depth=None, depth_ptr=None, stream=None):
        """prosper_pt_raster_transparent_draw: the per-pixel fragment lists of draw list `which` (count, scan, fill) against
        the depth, resolved front to back in place over the HDR image.  `depth`: a host array [h, w]; `depth_ptr`: a device
        pointer; neither: the context's last depth.  Blocks the host once, for the scan's total."""
        self._raster_transparent(lib().prosper_pt_raster_transparent_draw, (which,), camera, draw_type, ibl, depth, depth_ptr, stream)

    def raster_forward_transparent(self, camera, draw_type=0, ibl=0, depth=None, depth_ptr=None, stream=None):
        """prosper_pt_raster_forward_transparent (ForwardRenderer::recordTransparent): the first phase in TRANSPARENT mode
        without a pyramid, then raster_transparent_draw of its list.  The context's draw lists are then the transparent ones."""
        self._raster_transparent(lib().prosper_pt_raster_forward_transparent, (), camera, draw_type, ibl, depth, depth_ptr, stream)

    def raster_transparent_info(self):
        """S.RasterTransparentInfo of the last rasterised transparent pass; None while its counts have not landed (never waits)."""
        out = S.RasterTransparentInfo()
        rc = lib().prosper_pt_get_raster_transparent_info(self._h, C.byref(out))
        if rc == S.NOT_READY:
            return None
        _check(rc)
        return out

    def read_raster_fragments(self, stream=None):
        """The lists of the last rasterised transparent pass: (counts uint32 [h, w], fragments [total] of the structured dtype
        of S.RasterFragment, pixel after pixel in row-major order, each pixel's run sorted front to back)."""
        w, h = getattr(self, "_raster_transparent_extent", (0, 0))  # (before the first pass the library refuses)
        total = C.c_uint64()
        _check(lib().prosper_pt_read_raster_fragments(self._h, None, 0, None, 0, C.byref(total), C.c_void_p(stream)))
        counts = np.empty((h, w), np.uint32)
        fragments = np.empty(total.value, np.dtype(S.RasterFragment))
        _check(lib().prosper_pt_read_raster_fragments(self._h, counts.ctypes.data, w * h, fragments.ctypes.data, len(fragments),
                                                      C.byref(total), C.c_void_p(stream)))
        return counts, fragments

    def set_raster_transparent_debug_layers(self, layers_per_pixel):
        """Debug mode of the rasterised transparent pass: later calls record each pixel's first `layers_per_pixel` shaded
        layers (0: off)."""
        _check(lib().prosper_pt_set_raster_transparent_debug_layers(self._h, layers_per_pixel))
        self._raster_transparent_layers = layers_per_pixel

    def read_raster_transparent_layers(self, stream=None):
        """What the last rasterised transparent pass in debug mode recorded: (counts uint32 [h, w] of the layers shaded,
        layers [h, w, N] of the structured dtype of S.TransparentLayer, front to back)."""
        w, h = getattr(self, "_raster_transparent_extent", (0, 0))
        n = getattr(self, "_raster_transparent_layers", 0)
        counts = np.empty((h, w), np.uint32)
        layers = np.empty((h, w, n), np.dtype(S.TransparentLayer))
        _check(lib().prosper_pt_read_raster_transparent_layers(self._h, counts.ctypes.data, layers.ctypes.data, w * h, n, C.c_void_p(stream)))
        return counts, layers

    def read_raster_visibility(self, width, height, stream=None):
        """-> (ids uint32 [h, w, 3] of (drawInstanceIndex, meshletIndex, triangle), 0xFFFFFFFF where nothing is drawn;
        depth float32 [h, w]) of the visibility image, whose extent is width x height (waits for it)"""
        ids, depth = np.empty((height, width, 3), np.uint32), np.empty((height, width), np.float32)
        _check(lib().prosper_pt_read_raster_visibility(self._h, ids.ctypes.data, depth.ctypes.data, width * height, C.c_void_p(stream)))
        return ids, depth

    def raster_info(self):
        """S.RasterInfo of the last draws; None while the counts have not landed (never waits)."""
        out = S.RasterInfo()
        rc = lib().prosper_pt_get_raster_info(self._h, C.byref(out))
        if rc == S.NOT_READY:
            return None
        _check(rc)
        return out

    def read_instance_scales(self, count, stream=None):
        """The current scene version's per-model-instance uniform scales, float32 [count] (0: non-uniform)."""
        out = np.empty(count, np.float32)
        _check(lib().prosper_pt_read_instance_scales(self._h, out.ctypes.data, count, C.c_void_p(stream)))
        return out

    # ---- the registry of the context's images and the one-texel readback ----

    def debug_resources(self):
        """The registry: a list of S.DebugResource, index = the resource's number."""
        out = []
        for i in range(lib().prosper_pt_debug_resource_count(self._h)):
            r = S.DebugResource()
            _check(lib().prosper_pt_get_debug_resource(self._h, i, C.byref(r)))
            out.append(r)
        return out

    def debug_resource_index(self, name):
        for i, r in enumerate(self.debug_resources()):
            if r.name.decode() == name:
                return i
        raise KeyError(name)

    def texture_readback(self, resource, px_x, px_y, stream=None):
        """TextureReadback::record (prosper_pt_texture_readback): one nearest clamp-to-edge texel of level 0 of registry
        entry `resource` (index or name) at uv = px / extent, queued; try_texture_readback hands it out."""
        if isinstance(resource, str):
            resource = self.debug_resource_index(resource)
        _check(lib().prosper_pt_texture_readback(self._h, resource, px_x, px_y, C.c_void_p(stream)))

    def try_texture_readback(self):
        """The queued texel as float32 [4], once; None while nothing is queued or it has not finished (never blocks)."""
        out = (C.c_float * 4)()
        rc = lib().prosper_pt_try_texture_readback(self._h, C.byref(out))
        if rc == S.NOT_READY:
            return None
        _check(rc)
        return np.array(out[:], np.float32)

    def texture_debug(self, resource, out_res, value_range=(0.0, 1.0), lod=0, flags=S.TEXTURE_DEBUG_CHANNEL_RGB,
                      cursor_uv=(0.0, 0.0), bilinear=False, device_ptr=None, to_host=True, stream=None):
        """TextureDebug::record (prosper_pt_texture_debug): level `lod` of registry entry `resource` (index or name) viewed
        as out_res = (width, height) RGBA8 -> uint8 [h, w, 4] (None with to_host=False).  `flags`: a channel (0-3, or
        S.TEXTURE_DEBUG_CHANNEL_RGB) | S.TEXTURE_DEBUG_ABS_BEFORE_RANGE | _ZOOM | _MAGNIFIER."""
        if isinstance(resource, str):
            resource = self.debug_resource_index(resource)
        r = S.DebugResource()
        _check(lib().prosper_pt_get_debug_resource(self._h, resource, C.byref(r)))
        w, h = int(out_res[0]), int(out_res[1])
        pc = S.TextureDebugPC((C.c_int32 * 2)(r.width, r.height), (C.c_int32 * 2)(w, h), (C.c_float * 2)(*value_range), lod, flags,
                              (C.c_float * 2)(*cursor_uv))
        out = np.empty((max(h, 0), max(w, 0), 4), np.uint8) if to_host else None
        _check(lib().prosper_pt_texture_debug(self._h, resource, C.byref(pc), 1 if bilinear else 0, C.c_void_p(device_ptr),
                                              out.ctypes.data if to_host else None, max(w, 0) * max(h, 0) * 4, C.c_void_p(stream)))
        return out

    def texture_debug_peek(self):
        """The magnifier's peeked texel of the last texture_debug with S.TEXTURE_DEBUG_MAGNIFIER: float32 [4] (waits)."""
        out = (C.c_float * 4)()
        _check(lib().prosper_pt_get_texture_debug_peek(self._h, C.byref(out)))
        return np.array(out[:], np.float32)

    def generate_ibl(self, stream=None):
        """ImageBasedLighting::recordGeneration (prosper_pt_generate_ibl): the irradiance and radiance cubes and the BRDF
        LUT of the current scene's sky, which deferred shading with ibl=1 reads."""
        self._sync_debug()
        _check(lib().prosper_pt_generate_ibl(self._h, C.c_void_p(stream)))

    def ibl_info(self):
        """S.IblInfo: generated (0/1), the maps' sizes and the last generation's per-pass device times."""
        info = S.IblInfo()
        _check(lib().prosper_pt_get_ibl_info(self._h, C.byref(info)))
        return info

    def read_ibl(self, stream=None):
        """The maps without borders: dict with irradiance float16 [6, 64, 64, 4], radiance a list of float16
        [6, n, n, 4] for n = 512 ... 1, lut uint16 [512, 512, 2] (UNORM scale, bias; row = roughness, column = NoV)."""
        n0, mips = S.IBL_RADIANCE_SIZE, S.IBL_RADIANCE_MIPS
        irr = np.empty((6, S.IBL_IRRADIANCE_SIZE, S.IBL_IRRADIANCE_SIZE, 4), np.float16)
        rad = np.empty(sum(6 * (n0 >> m) ** 2 * 4 for m in range(mips)), np.float16)
        lut = np.empty((S.IBL_LUT_SIZE, S.IBL_LUT_SIZE, 2), np.uint16)
        _check(lib().prosper_pt_read_ibl(self._h, irr.ctypes.data, irr.nbytes, rad.ctypes.data, rad.nbytes,
                                         lut.ctypes.data, lut.nbytes, C.c_void_p(stream)))
        levels, at = [], 0
        for m in range(mips):
            n = n0 >> m
            levels.append(rad[at:at + 6 * n * n * 4].reshape(6, n, n, 4))
            at += 6 * n * n * 4
        return {"irradiance": irr, "radiance": levels, "lut": lut}

    def skybox_fill(self, camera, width, height, depth=None, depth_ptr=None, stream=None):
        """SkyboxRenderer (prosper_pt_skybox_fill): the sky into every HDR texel whose depth is 0.  `depth`: a host array
        [h, w]; `depth_ptr`: a device pointer; neither: the last traced G-buffer's depth."""
        self._sync_debug()
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        assert dp is None or dp.shape == (height, width)
        ptr = depth_ptr if dp is None else dp.ctypes.data
        _check(lib().prosper_pt_skybox_fill(self._h, C.byref(camera), width, height, C.c_void_p(ptr),
                                            1 if dp is None else 0, C.c_void_p(stream)))

    def depth_of_field(self, pc, camera, width, height, illumination=None, depth=None, illumination_ptr=None,
                       depth_ptr=None, stream=None):
        """render::dof::DepthOfField (prosper_pt_depth_of_field) with the push constants `pc` (S.DofPC) into the HDR image.
        `illumination` [h, w, 4] and `depth` [h, w]: host arrays (both or neither); `illumination_ptr`, `depth_ptr`:
        device pointers.  No illumination: the HDR image in place; no depth: the last traced G-buffer's."""
        host = illumination is not None or depth is not None
        assert not (host and (illumination_ptr or depth_ptr)), "host and device inputs cannot be mixed"
        il = None if illumination is None else np.ascontiguousarray(illumination, np.float32)
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        assert il is None or il.shape == (height, width, 4)
        assert dp is None or dp.shape == (height, width)
        if host:
            inp = S.DofInputs(None if il is None else il.ctypes.data, None if dp is None else dp.ctypes.data, 0, 0)
        else:
            inp = S.DofInputs(illumination_ptr, depth_ptr, 1, 0)
        _check(lib().prosper_pt_depth_of_field(self._h, C.byref(pc), C.byref(camera), width, height, C.byref(inp),
                                               C.c_void_p(stream)))

    def dof_info(self):
        """S.DofInfo: the last depth-of-field call's extents, mip count and per-stage device times."""
        info = S.DofInfo()
        _check(lib().prosper_pt_get_dof_info(self._h, C.byref(info)))
        return info

    def read_dof_stage(self, stage, level=0, stream=None):
        """One intermediate of the last depth_of_field as float16: [h, w, 4] for the half-resolution illumination (mip
        `level`), the gathers and the filtered layers, [h, w] for the CoC, [th, tw, 2] (min, max) for the tiles."""
        i = self.dof_info()
        hw, hh = i.halfWidth, i.halfHeight
        if stage == S.DOF_HALF_ILLUMINATION:
            shape = (max(hh >> level, 1), max(hw >> level, 1), 4)
        elif stage == S.DOF_HALF_COC:
            shape = (hh, hw)
        elif stage in (S.DOF_TILE_MIN_MAX, S.DOF_DILATED_TILE_MIN_MAX):
            shape = (i.tileHeight, i.tileWidth, 2)
        else:
            shape = (hh, hw, 4)
        out = np.empty(shape, np.float16)
        _check(lib().prosper_pt_read_dof_stage(self._h, stage, level, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def bloom(self, pc, width, height, illumination=None, illumination_ptr=None, stream=None):
        """render::bloom::Bloom's multi-resolution blur (prosper_pt_bloom) with `pc` (S.BloomPC) into the HDR image.
        `illumination`: a host array [h, w, 4]; `illumination_ptr`: a device pointer; neither: the HDR image in place."""
        assert illumination is None or illumination_ptr is None, "host and device inputs cannot be mixed"
        il = None if illumination is None else np.ascontiguousarray(illumination, np.float32)
        assert il is None or il.shape == (height, width, 4)
        ptr = illumination_ptr if il is None else il.ctypes.data
        _check(lib().prosper_pt_bloom(self._h, C.byref(pc), width, height, C.c_void_p(ptr), 1 if il is None else 0,
                                      C.c_void_p(stream)))

    def bloom_info(self):
        """S.BloomInfo: the last bloom call's extents, first blurred level, streak half-width and per-stage device times."""
        info = S.BloomInfo()
        _check(lib().prosper_pt_get_bloom_info(self._h, C.byref(info)))
        return info

    def read_bloom_stage(self, stage, level, stream=None):
        """Level `level` of one working image of the last bloom (S.BLOOM_HIGHLIGHTS, _HORIZONTAL, _BLURRED) as float16
        [h, w, 4]."""
        i = self.bloom_info()
        out = np.empty((max(i.workingHeight >> level, 1), max(i.workingWidth >> level, 1), 4), np.float16)
        _check(lib().prosper_pt_read_bloom_stage(self._h, stage, level, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def bloom_fft(self, pc, width, height, illumination=None, illumination_ptr=None, stream=None):
        """render::bloom::Bloom's FFT technique (prosper_pt_bloom_fft) with `pc` (S.BloomFftPC) into the HDR image; the
        inputs as `bloom`."""
        assert illumination is None or illumination_ptr is None, "host and device inputs cannot be mixed"
        il = None if illumination is None else np.ascontiguousarray(illumination, np.float32)
        assert il is None or il.shape == (height, width, 4)
        ptr = illumination_ptr if il is None else il.ctypes.data
        _check(lib().prosper_pt_bloom_fft(self._h, C.byref(pc), width, height, C.c_void_p(ptr), 1 if il is None else 0,
                                          C.c_void_p(stream)))

    def bloom_fft_transform(self, image, inverse=False, stream=None):
        """One 2-D transform (prosper_pt_bloom_fft_transform) of a host array [dim, dim, 4] float32, a texel the complex
        numbers r + i g and b + i a: the DFT divided by dim, or the unnormalised inverse."""
        src = np.ascontiguousarray(image, np.float32)
        assert src.ndim == 3 and src.shape[0] == src.shape[1] and src.shape[2] == 4
        out = np.empty_like(src)
        _check(lib().prosper_pt_bloom_fft_transform(self._h, src.shape[0], 1 if inverse else 0, src.ctypes.data, out.ctypes.data, 0,
                                                    C.c_void_p(stream)))
        return out

    def bloom_fft_release_kernel(self):
        lib().prosper_pt_bloom_fft_release_kernel(self._h)

    def bloom_fft_info(self):
        """S.BloomFftInfo: the last FFT bloom's extents, whether the kernel was remade and the per-stage device times."""
        info = S.BloomFftInfo()
        _check(lib().prosper_pt_get_bloom_fft_info(self._h, C.byref(info)))
        return info

    def read_bloom_fft_stage(self, stage, stream=None):
        """One image of the last FFT bloom: S.BLOOM_FFT_HIGHLIGHTS float16 [dim, dim, 4], _KERNEL float32 [kernelDim,
        kernelDim, 4], _KERNEL_DFT and _CONVOLVED float32 [dim, dim, 4]."""
        i = self.bloom_fft_info()
        n = i.kernelDim if stage == S.BLOOM_FFT_KERNEL else i.dim
        out = np.empty((n, n, 4), np.float16 if stage == S.BLOOM_FFT_HIGHLIGHTS else np.float32)
        _check(lib().prosper_pt_read_bloom_fft_stage(self._h, stage, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def taa_resolve(self, pc, width, height, velocity=None, depth=None, illumination=None, velocity_ptr=None,
                    depth_ptr=None, illumination_ptr=None, stream=None):
        """render::TemporalAntiAliasing::record (prosper_pt_taa_resolve) with `pc` (S.TaaPC) into the HDR image and the
        history.  `velocity` [h, w, 2], `depth` [h, w], `illumination` [h, w, 4]: host arrays; the `_ptr` ones: device
        pointers.  No illumination: the HDR image in place; no depth: the last traced G-buffer's (Closest reads it)."""
        host = velocity is not None or depth is not None or illumination is not None
        assert not (host and (velocity_ptr or depth_ptr or illumination_ptr)), "host and device inputs cannot be mixed"
        ve = None if velocity is None else np.ascontiguousarray(velocity, np.float32)
        dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
        il = None if illumination is None else np.ascontiguousarray(illumination, np.float32)
        assert ve is None or ve.shape == (height, width, 2)
        assert dp is None or dp.shape == (height, width)
        assert il is None or il.shape == (height, width, 4)
        if host:
            inp = S.TaaInputs(*[None if a is None else a.ctypes.data for a in (il, ve, dp)], 0)
        else:
            inp = S.TaaInputs(illumination_ptr, velocity_ptr, depth_ptr, 1)
        _check(lib().prosper_pt_taa_resolve(self._h, C.byref(pc), width, height, C.byref(inp), C.c_void_p(stream)))

    def taa_release_history(self):
        """TemporalAntiAliasing::releasePreserved: the next taa_resolve ignores the history."""
        lib().prosper_pt_taa_release_history(self._h)

    def taa_info(self):
        """S.TaaInfo: the last resolve's extent, history flags and the device times of its two kernels."""
        info = S.TaaInfo()
        _check(lib().prosper_pt_get_taa_info(self._h, C.byref(info)))
        return info

    def read_taa_history(self, stream=None):
        """The history the next taa_resolve will read (what the last one wrote) as float16 [h, w, 4]."""
        i = self.taa_info()
        out = np.empty((i.height, i.width, 4), np.float16)
        _check(lib().prosper_pt_read_taa_history(self._h, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def denoise(self, pc, camera, width, height, illumination=None, albedo_roughness=None, normal_metallic=None, depth=None,
                velocity=None, illumination_ptr=None, albedo_roughness_ptr=None, normal_metallic_ptr=None, depth_ptr=None,
                velocity_ptr=None, stream=None):
        """prosper_pt_denoise with `pc` (S.DenoisePC) into the HDR image and the history.  `illumination`,
        `albedo_roughness`, `normal_metallic` [h, w, 4], `depth` [h, w], `velocity` [h, w, 2]: host arrays; the `_ptr`
        ones: device pointers.  No illumination: the HDR image in place; no G-buffer (all three): the last traced one;
        no velocity: the last traced velocity target."""
        arrays = (illumination, albedo_roughness, normal_metallic, depth, velocity)
        pointers = (illumination_ptr, albedo_roughness_ptr, normal_metallic_ptr, depth_ptr, velocity_ptr)
        host = any(a is not None for a in arrays)
        assert not (host and any(pointers)), "host and device inputs cannot be mixed"
        held = [None if a is None else np.ascontiguousarray(a, np.float32) for a in arrays]
        for a, shape in zip(held, ((height, width, 4),) * 3 + ((height, width), (height, width, 2))):
            assert a is None or a.shape == shape
        if host:
            inp = S.DenoiseInputs(*[None if a is None else a.ctypes.data for a in held], 0)
        else:
            inp = S.DenoiseInputs(*pointers, 1)
        _check(lib().prosper_pt_denoise(self._h, C.byref(pc), C.byref(camera), width, height, C.byref(inp), C.c_void_p(stream)))

    def denoise_release_history(self):
        """The next denoise ignores the history."""
        lib().prosper_pt_denoise_release_history(self._h)

    def denoise_info(self):
        """S.DenoiseInfo: the last denoise's extent, history flags, history counts and per-stage device times."""
        info = S.DenoiseInfo()
        _check(lib().prosper_pt_get_denoise_info(self._h, C.byref(info)))
        return info

    def read_denoise_stage(self, stage, stream=None):
        """One image of the last denoise (S.DENOISE_*) as float32 [h, w, 4]; the geometry flag and the history length are
        uint32 bits (prosper_amd.denoise.bits)."""
        i = self.denoise_info()
        out = np.empty((i.height, i.width, 4), np.float32)
        _check(lib().prosper_pt_read_denoise_stage(self._h, stage, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def set_tone_map_lut(self, lut_r9g9b9e5):
        """lut: uint32 [dim, dim, dim] (z, y, x) R9G9B9E5 texels, e.g. from prosper_amd.dds.read_lut."""
        lut = np.ascontiguousarray(lut_r9g9b9e5, dtype=np.uint32)
        assert lut.ndim == 3 and lut.shape[0] == lut.shape[1] == lut.shape[2]
        _check(lib().prosper_pt_set_tone_map_lut(self._h, lut.ctypes.data, lut.shape[0]))

    def tone_map(self, exposure=1.0, contrast=1.0, device_ptr=None, to_host=True, stream=None):
        """tone_map.comp over the current HDR tile -> uint8 [h, localWidth, 4] (or None with to_host=False)."""
        lw, h = self.local_extent()
        out = np.empty((h, lw, 4), np.uint8) if to_host else None
        _check(lib().prosper_pt_tone_map(self._h, exposure, contrast, C.c_void_p(device_ptr),
                                         out.ctypes.data if to_host else None, lw * h * 4, C.c_void_p(stream)))
        return out

    def counters(self, stream=None):
        c = S.Counters()
        _check(lib().prosper_pt_get_counters(self._h, C.byref(c), C.c_void_p(stream)))
        return c

    def stage_counters(self, stage, stream=None):
        c = S.Counters()
        _check(lib().prosper_pt_get_stage_counters(self._h, stage, C.byref(c), C.c_void_p(stream)))
        return c

    def last_render_timing(self):
        """-> (total_ms, {kernel name: (sum_ms, launches)}) of the last render, from hipEvents."""
        total = C.c_float()
        per = (C.c_float * S.MAX_KERNELS)()
        launches = (C.c_uint32 * S.MAX_KERNELS)()
        _check(lib().prosper_pt_get_last_render_timing(self._h, C.byref(total), per, launches))
        names = [lib().prosper_pt_kernel_name(i).decode() for i in range(S.MAX_KERNELS)]
        return total.value, {n: (per[i], launches[i]) for i, n in enumerate(names) if n}

    def reset_counters(self, stream=None):
        _check(lib().prosper_pt_reset_counters(self._h, C.c_void_p(stream)))

    def set_kernel_timing(self, enabled):
        _check(lib().prosper_pt_set_kernel_timing(self._h, 1 if enabled else 0))

    def last_render_ms(self):
        total = C.c_float()
        per = (C.c_float * S.MAX_KERNELS)()
        _check(lib().prosper_pt_get_last_render_ms(self._h, C.byref(total), per))
        names = [lib().prosper_pt_kernel_name(i).decode() for i in range(S.MAX_KERNELS)]
        return total.value, {n: per[i] for i, n in enumerate(names) if n}

    # ---- multi-GPU (include/prosper_pt/prosper_pt.h, "multi-GPU") ----
    @staticmethod
    def comm_unique_id():
        """ncclGetUniqueId: 128 bytes to hand to every rank's comm_init."""
        buf = (C.c_uint8 * 128)()
        _check(lib().prosper_pt_comm_get_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, ranks):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().prosper_pt_comm_init(self._h, buf, rank, ranks))

    def comm_destroy(self):
        _check(lib().prosper_pt_comm_destroy(self._h))

    def gather_tiles(self, root=0, device_ptr=None, byte_size=0, flags=0, stream=None):
        """RCCL gather of the ranks' tiles to `root` + de-interleave there (enqueue only)."""
        _check(lib().prosper_pt_gather_tiles(self._h, root, C.c_void_p(device_ptr), byte_size, flags, C.c_void_p(stream)))

    def gather_wait(self, stream=None):
        _check(lib().prosper_pt_gather_wait(self._h, C.c_void_p(stream)))

    def comm_info(self, stream=None):
        """The communicator's own view (ncclCommCount, rank, device) and the last gather's device time (waits for it)."""
        info = S.CommInfo()
        _check(lib().prosper_pt_comm_query(self._h, C.byref(info)))
        return info

    def read_gathered(self, stream=None):
        """Root only: the gathered [height, width, 4] float32 image (synchronises)."""
        p, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
        _check(lib().prosper_pt_get_gathered_device_ptr(self._h, C.byref(p), C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 4), np.float32)
        _check(lib().prosper_pt_read_gathered(self._h, out.ctypes.data, out.nbytes, C.c_void_p(stream)))
        return out

    def deinterleave_tiles(self, tiles_ptr, ranks, stripe_width, width, height, full_ptr, stream=None):
        """The root's kernel alone, on raw device pointers."""
        _check(lib().prosper_pt_deinterleave_tiles(self._h, C.c_void_p(tiles_ptr), ranks, stripe_width, width, height,
                                                   C.c_void_p(full_ptr), width * height * 16, C.c_void_p(stream)))

    def srgb_monotonicity(self, first_bits, last_bits):
        """(max defect, decreasing adjacent pairs) of the device's sRGBtoLinear over every float in the bit range."""
        defect, decreases = C.c_float(0.0), C.c_uint64(0)
        _check(lib().prosper_pt_debug_srgb_monotonicity(self._h, first_bits, last_bits, C.byref(defect), C.byref(decreases)))
        return float(defect.value), int(decreases.value)

    def eval_device_fn(self, fn, inputs, in_stride, out_stride):
        a = np.ascontiguousarray(inputs, dtype=np.float32).reshape(-1, in_stride)
        out = np.zeros((a.shape[0], out_stride), np.float32)
        _check(lib().prosper_pt_eval_device_fn(self._h, fn, a.ctypes.data, in_stride, out.ctypes.data, out_stride,
                                               a.shape[0]))
        return out
