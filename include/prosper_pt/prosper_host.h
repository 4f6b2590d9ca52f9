/*
 * prosper_pt/prosper_host.h — plain-C handles onto the C++ host layer
 * (prosper_amd/csrc/host/{camera,rt_reference}.hpp) so that non-C++ callers — the Python tests and
 * bench.py — drive the same `scene::Camera` / `render::RtReference` code a C++ application links.
 *
 * Replaces, for a headless caller:
 *   scene::Camera::{lookAt, perspective, updateBuffer}   src/scene/Camera.cpp:105-204,366-395
 *   render::RtReference::{init, drawUi, record, recompileShaders, releasePreserved}
 *                                                        src/render/RtReference.hpp:32-60
 *   World::buildAccelerationStructures                   src/scene/World.cpp:538-575
 */
#ifndef PROSPER_HOST_H
#define PROSPER_HOST_H

#include "prosper_pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct prosper_host_camera prosper_host_camera;
typedef struct prosper_host_rt_reference prosper_host_rt_reference;

/* RtReference::Options (src/render/RtReference.hpp:44-50) */
typedef struct prosper_host_record_options
{
    uint32_t depthOfField;
    uint32_t ibl;
    uint32_t colorDirty;
    uint32_t drawType; /* prosper_DrawType */
} prosper_host_record_options;

const char *prosper_host_last_error(void);

prosper_host_camera *prosper_host_camera_create(void);
void prosper_host_camera_destroy(prosper_host_camera *camera);
void prosper_host_camera_look_at(prosper_host_camera *camera, const float eye[3], const float target[3], const float up[3]);
void prosper_host_camera_set_parameters(
    prosper_host_camera *camera, float fov, float zN, float zF, float apertureDiameter, float focusDistance);
void prosper_host_camera_update_resolution(prosper_host_camera *camera, uint32_t width, uint32_t height);
void prosper_host_camera_update_buffer(prosper_host_camera *camera, prosper_CameraUniforms *out, float *focalLength);
int prosper_host_camera_changed_this_frame(const prosper_host_camera *camera);
void prosper_host_camera_end_frame(prosper_host_camera *camera);
/* Camera::setJitter: from the next update_buffer on the projection carries the TAA jitter of the 8-sample Halton(2, 3)
 * cycle (prosper_pt_taa_jitter of the camera's jitter index, which end_frame advances).  Off by default. */
void prosper_host_camera_set_jitter(prosper_host_camera *camera, int applyJitter);

int prosper_host_rt_reference_create(int32_t deviceOrdinal, uint32_t createFlags, prosper_host_rt_reference **out);
void prosper_host_rt_reference_destroy(prosper_host_rt_reference *pass);
prosper_pt_ctx *prosper_host_rt_reference_context(prosper_host_rt_reference *pass);
/* World::setSceneView + buildAccelerationStructures */
int prosper_host_rt_reference_set_scene(prosper_host_rt_reference *pass, const prosper_pt_scene_view *view);
void prosper_host_rt_reference_draw_ui(
    prosper_host_rt_reference *pass, int accumulate, int clampIndirect, uint32_t rouletteStartBounce,
    uint32_t maxBounces);
void prosper_host_rt_reference_recompile_shaders(prosper_host_rt_reference *pass);
void prosper_host_rt_reference_release_preserved(prosper_host_rt_reference *pass);
/* Camera::updateBuffer + RtReference::record + end of frame; returns the ReferencePC it pushed. */
int prosper_host_rt_reference_record(
    prosper_host_rt_reference *pass, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const prosper_host_record_options *options, uint32_t frameCount, const prosper_pt_tile_desc *tile,
    uint32_t renderFlags, void *stream, prosper_ReferencePC *outPushConstants);

/* render::TiledRtReference (host/tiled_rt_reference.hpp): the pass on one rank of a multi-GPU job - RtReference::record
 * for the rank's interleaved 16-pixel stripes, then the RCCL gather of the ranks' HDR tiles to `root` and the
 * de-interleave kernel there (prosper_pt_gather_tiles).  No counterpart in the reference, which asserts
 * renderArea.offset == 0 (src/render/RtReference.cpp:327).  `commId`: prosper_pt_comm_get_unique_id of one rank.
 * record() returns, on the root, the device pointer of the gathered width*height RGBA32F image; readers enqueue
 * wait_for_gather on their stream first. */
typedef struct prosper_host_tiled_rt_reference prosper_host_tiled_rt_reference;
int prosper_host_tiled_rt_reference_create(
    int32_t deviceOrdinal, uint32_t rank, uint32_t ranks, const uint8_t commId[PROSPER_PT_COMM_ID_BYTES], uint32_t root,
    uint32_t createFlags, prosper_host_tiled_rt_reference **out);
void prosper_host_tiled_rt_reference_destroy(prosper_host_tiled_rt_reference *pass);
prosper_pt_ctx *prosper_host_tiled_rt_reference_context(prosper_host_tiled_rt_reference *pass);
int prosper_host_tiled_rt_reference_set_scene(prosper_host_tiled_rt_reference *pass, const prosper_pt_scene_view *view);
int prosper_host_tiled_rt_reference_record(
    prosper_host_tiled_rt_reference *pass, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const prosper_host_record_options *options, uint32_t frameCount, uint32_t renderFlags, void *stream,
    const float **outIllumination);
int prosper_host_tiled_rt_reference_wait_for_gather(prosper_host_tiled_rt_reference *pass, void *stream);

/* render::ToneMap (host/tone_map.hpp; reference src/render/ToneMap.hpp:16-52): init with the LUT file
 * (res/texture/tony_mc_mapface.dds) or its texels, drawUi's two sliders, record into caller-owned device memory. */
typedef struct prosper_host_tone_map prosper_host_tone_map;
int prosper_host_tone_map_create(prosper_pt_ctx *ctx, const char *lutDdsPath, prosper_host_tone_map **out);
int prosper_host_tone_map_create_from_texels(
    prosper_pt_ctx *ctx, const uint32_t *lutR9G9B9E5, uint32_t dim, prosper_host_tone_map **out);
void prosper_host_tone_map_destroy(prosper_host_tone_map *pass);
void prosper_host_tone_map_draw_ui(prosper_host_tone_map *pass, float exposure, float contrast);
int prosper_host_tone_map_record(prosper_host_tone_map *pass, void *stream, void *deviceRgba8, size_t byteSize);

/* render::rtdi::RtDirectIllumination (host/rt_direct_illumination.hpp; reference
 * src/render/rtdi/RtDirectIllumination.hpp:19-58) on a context the scene was uploaded to (borrowed): drawUi's
 * "Spatial reuse" toggle (default on), record = Camera::updateBuffer + initial reservoirs + optional spatial reuse +
 * trace (prosper_pt_restir_di_record) + end of frame; returns the TracePC it pushed. */
typedef struct prosper_host_rt_direct_illumination prosper_host_rt_direct_illumination;
int prosper_host_rt_direct_illumination_create(prosper_pt_ctx *ctx, prosper_host_rt_direct_illumination **out);
void prosper_host_rt_direct_illumination_destroy(prosper_host_rt_direct_illumination *pass);
void prosper_host_rt_direct_illumination_draw_ui(prosper_host_rt_direct_illumination *pass, int spatialReuse);
void prosper_host_rt_direct_illumination_recompile_shaders(prosper_host_rt_direct_illumination *pass);
void prosper_host_rt_direct_illumination_release_preserved(prosper_host_rt_direct_illumination *pass);
int prosper_host_rt_direct_illumination_record(
    prosper_host_rt_direct_illumination *pass, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const prosper_pt_restir_inputs *gbuffer, int resetAccumulation, uint32_t drawType, uint32_t nextFrame, void *stream,
    prosper_pt_restir_trace_pc *outPushConstants);

/* render::GBufferTracer (host/gbuffer_tracer.hpp): the ray-traced stand-in for GBufferRenderer::record's output on a
 * context the scene was uploaded to (borrowed).  record = Camera::updateBuffer + prosper_pt_trace_gbuffer into the
 * context-owned targets; *outGBuffer receives them as device inputs (onDevice = 1) for
 * prosper_host_rt_direct_illumination_record or the prosper_pt_restir_di_* entries. */
typedef struct prosper_host_gbuffer_tracer prosper_host_gbuffer_tracer;
int prosper_host_gbuffer_tracer_create(prosper_pt_ctx *ctx, prosper_host_gbuffer_tracer **out);
void prosper_host_gbuffer_tracer_destroy(prosper_host_gbuffer_tracer *pass);
/* GBufferTracer::setOpaqueOnly: both records leave BLEND surfaces out (PROSPER_PT_GBUFFER_OPAQUE_ONLY), for
 * prosper_host_forward_renderer_record_transparent to draw.  Off by default. */
int prosper_host_gbuffer_tracer_set_opaque_only(prosper_host_gbuffer_tracer *pass, int opaqueOnly);
/* GBufferTracer::setTextureLod / setLodBias: later records sample material textures through their mip chains
 * (prosper_pt_set_texture_lod) with `lodBias`; prosper_host_renderer_lod_bias is Renderer::lodBias(): -1 while TAA is
 * applied, otherwise 0. */
int prosper_host_gbuffer_tracer_set_texture_lod(prosper_host_gbuffer_tracer *pass, int enabled, float lodBias);
float prosper_host_renderer_lod_bias(int applyTaa);
int prosper_host_gbuffer_tracer_record(
    prosper_host_gbuffer_tracer *pass, prosper_host_camera *camera, uint32_t width, uint32_t height, uint32_t drawType,
    uint32_t frameIndex, int jitter, void *stream, prosper_pt_restir_inputs *outGBuffer);
/* GBufferTracer::recordVelocity = Camera::updateBuffer + prosper_pt_trace_gbuffer_velocity: the G-buffer through the
 * pixel centres of the camera's (jittered) projection and the velocity image (*outVelocity, device, float2).
 * `transforms` (may be NULL; `transformCount` = the scene's model instances): this frame's instance transforms, kept
 * and handed to the next call as the previous frame's; the first call sees unmoved instances. */
int prosper_host_gbuffer_tracer_record_velocity(
    prosper_host_gbuffer_tracer *pass, prosper_host_camera *camera, uint32_t width, uint32_t height, uint32_t drawType,
    uint32_t frameIndex, const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount, void *stream,
    prosper_pt_restir_inputs *outGBuffer, void **outVelocity);

/* render::LightClustering (host/light_clustering.hpp; reference src/render/LightClustering.hpp:22-64) on a context the
 * scene was uploaded to (borrowed): record = Camera::updateBuffer + prosper_pt_cluster_lights into the context-owned
 * buffers (prosper_pt_read_light_clusters). */
typedef struct prosper_host_light_clustering prosper_host_light_clustering;
int prosper_host_light_clustering_create(prosper_pt_ctx *ctx, prosper_host_light_clustering **out);
void prosper_host_light_clustering_destroy(prosper_host_light_clustering *pass);
int prosper_host_light_clustering_record(
    prosper_host_light_clustering *pass, prosper_host_camera *camera, uint32_t width, uint32_t height, void *stream);

/* render::DeferredShading (host/deferred_shading.hpp; reference src/render/DeferredShading.hpp:18-66) on a context the
 * scene was uploaded to (borrowed): record = Camera::updateBuffer + LightClustering::record + DeferredShading::record
 * (prosper_pt_deferred_shading) over `gbuffer` (host or device) into the context's HDR image; returns the
 * DeferredShadingPC it pushed.  applyIbl != 0 adds evalIBL; it is refused with PROSPER_PT_ERR_UNSUPPORTED until
 * ImageBasedLighting::recordGeneration has run for the current scene. */
typedef struct prosper_host_deferred_shading prosper_host_deferred_shading;
int prosper_host_deferred_shading_create(prosper_pt_ctx *ctx, prosper_host_deferred_shading **out);
void prosper_host_deferred_shading_destroy(prosper_host_deferred_shading *pass);
int prosper_host_deferred_shading_record(
    prosper_host_deferred_shading *pass, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const prosper_pt_restir_inputs *gbuffer, int applyIbl, uint32_t drawType, void *stream,
    prosper_pt_deferred_shading_pc *outPushConstants);

/* render::ImageBasedLighting (host/image_based_lighting.hpp; reference src/render/ImageBasedLighting.hpp) on a context
 * the scene was uploaded to (borrowed): record_generation = prosper_pt_generate_ibl; is_generated returns 1 or 0 (or an
 * error code), 0 again after a scene upload. */
typedef struct prosper_host_image_based_lighting prosper_host_image_based_lighting;
int prosper_host_image_based_lighting_create(prosper_pt_ctx *ctx, prosper_host_image_based_lighting **out);
void prosper_host_image_based_lighting_destroy(prosper_host_image_based_lighting *pass);
int prosper_host_image_based_lighting_is_generated(prosper_host_image_based_lighting *pass);
int prosper_host_image_based_lighting_record_generation(prosper_host_image_based_lighting *pass, void *stream);

/* render::SkyboxRenderer (host/skybox_renderer.hpp; reference src/render/SkyboxRenderer.hpp) on a context the scene was
 * uploaded to (borrowed): record = Camera::updateBuffer + prosper_pt_skybox_fill over the context's HDR image.
 * `nonLinearDepth` NULL: the last traced G-buffer's depth. */
typedef struct prosper_host_skybox_renderer prosper_host_skybox_renderer;
int prosper_host_skybox_renderer_create(prosper_pt_ctx *ctx, prosper_host_skybox_renderer **out);
void prosper_host_skybox_renderer_destroy(prosper_host_skybox_renderer *pass);
int prosper_host_skybox_renderer_record(
    prosper_host_skybox_renderer *pass, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const float *nonLinearDepth, uint32_t onDevice, void *stream);

/* render::HierarchicalDepthDownsampler (host/hierarchical_depth_downsampler.hpp; reference
 * src/render/HierarchicalDepthDownsampler.hpp) on a context (borrowed): record = prosper_pt_hiz_downsample into the slot
 * `nextFrame` & 1 picks, as the reference picks one of its two storage sets.  It needs no scene with a caller's depth;
 * `nonLinearDepth` NULL: the last traced G-buffer's depth.  *mipCount and mips[0 .. *mipCount) (room for 12, either may
 * be NULL) receive the levels' device pointers, which stand in for the reference's image handle. */
typedef struct prosper_host_hiz_downsampler prosper_host_hiz_downsampler;
int prosper_host_hiz_downsampler_create(prosper_pt_ctx *ctx, prosper_host_hiz_downsampler **out);
void prosper_host_hiz_downsampler_destroy(prosper_host_hiz_downsampler *pass);
int prosper_host_hiz_downsampler_record(
    prosper_host_hiz_downsampler *pass, const float *nonLinearDepth, uint32_t onDevice, uint32_t width, uint32_t height,
    uint32_t nextFrame, uint32_t *mipCount, const float **mips, void *stream);

/* render::GBufferRenderer (host/gbuffer_renderer.hpp; reference src/render/GBufferRenderer.hpp): record is
 * prosper_pt_raster_gbuffer - both culling phases around the rasteriser's own depth, the draws and the resolve - into the
 * context's own targets, returned as device pointers; `transforms` (optional) are this frame's instance transforms, kept
 * as the next record's previous ones.  release_preserved forgets the kept pyramid and transforms. */
typedef struct prosper_host_gbuffer_renderer prosper_host_gbuffer_renderer;
typedef struct prosper_host_gbuffer_renderer_output
{
    const void *albedoRoughness;
    const void *normalMetalness;
    const void *velocity;
    const float *depth;
} prosper_host_gbuffer_renderer_output;
int prosper_host_gbuffer_renderer_create(prosper_pt_ctx *ctx, prosper_host_gbuffer_renderer **out);
void prosper_host_gbuffer_renderer_destroy(prosper_host_gbuffer_renderer *pass);
int prosper_host_gbuffer_renderer_record(
    prosper_host_gbuffer_renderer *pass, prosper_host_camera *camera, uint32_t width, uint32_t height, uint32_t drawType,
    const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount, void *stream, prosper_host_gbuffer_renderer_output *out);
int prosper_host_gbuffer_renderer_read_draw_stats(prosper_host_gbuffer_renderer *pass, prosper_pt_draw_stats *out, uint32_t wait);
int prosper_host_gbuffer_renderer_release_preserved(prosper_host_gbuffer_renderer *pass);

/* render::MeshletCuller and render::DrawStats (host/meshlet_culler.hpp; reference src/render/MeshletCuller.hpp,
 * DrawStats.hpp) on a context the scene was uploaded to (borrowed): record_first_phase = Camera::updateBuffer +
 * prosper_pt_cull_meshlets_first_phase (mode 0 Opaque, 1 Transparent; `inHierarchicalDepth` a pyramid slot or
 * PROSPER_PT_NO_HIZ), record_second_phase = Camera::updateBuffer + prosper_pt_cull_meshlets_second_phase.  The output's
 * device pointers stand in for the reference's buffer handles (secondPhaseInput NULL: none) and are valid until the next
 * culling call.  read_draw_stats: prosper_pt_get_draw_stats (PROSPER_PT_NOT_READY with `wait` 0 while the device counts
 * have not landed; the totals are there all the same). */
typedef struct prosper_host_meshlet_culler prosper_host_meshlet_culler;
typedef struct prosper_host_meshlet_culler_output
{
    const uint32_t *dataBuffer;       /* uint count; { drawInstanceIndex, meshletIndex }[] */
    const uint32_t *argumentBuffer;   /* groupsX, groupsY, groupsZ */
    const uint32_t *secondPhaseInput; /* first phase with a hierarchical depth only */
    uint32_t capacity;                /* pairs each list has room for */
    uint32_t reserved;
} prosper_host_meshlet_culler_output;
int prosper_host_meshlet_culler_create(prosper_pt_ctx *ctx, prosper_host_meshlet_culler **out);
void prosper_host_meshlet_culler_destroy(prosper_host_meshlet_culler *pass);
int prosper_host_meshlet_culler_record_first_phase(
    prosper_host_meshlet_culler *pass, uint32_t mode, prosper_host_camera *camera, uint32_t width, uint32_t height,
    uint32_t inHierarchicalDepth, prosper_host_meshlet_culler_output *out, void *stream);
int prosper_host_meshlet_culler_record_second_phase(
    prosper_host_meshlet_culler *pass, prosper_host_camera *camera, uint32_t width, uint32_t height,
    uint32_t inHierarchicalDepth, prosper_host_meshlet_culler_output *out, void *stream);
int prosper_host_meshlet_culler_read_draw_stats(prosper_host_meshlet_culler *pass, prosper_pt_draw_stats *out, uint32_t wait);

/* render::ForwardRenderer (host/forward_renderer.hpp; reference src/render/ForwardRenderer.hpp) on a context the scene was
 * uploaded to (borrowed).  record_opaque = Camera::updateBuffer + prosper_pt_raster_forward - both culling phases around
 * the rasteriser's own depth, the draws and the forward shade - into the context's HDR image and its own
 * depth and velocity, returned as device pointers; `transforms` (optional) are this frame's instance transforms, kept as
 * the next record's previous ones.  release_preserved forgets the kept pyramid and transforms.  record_transparent =
 * Camera::updateBuffer + prosper_pt_forward_transparent over the context's HDR image.  `nonLinearDepth` NULL: the last traced G-buffer's depth;
 * `rayFlags`, `frameIndex`: the ray the G-buffer was traced with (0, PROSPER_PT_TRANSPARENT_JITTER or
 * PROSPER_PT_TRANSPARENT_CAMERA_JITTER).  prosper itself draws transparents with ibl = 0.  *outPushConstants (may be
 * NULL) receives the ForwardPC it pushed. */
typedef struct prosper_host_forward_renderer prosper_host_forward_renderer;
int prosper_host_forward_renderer_create(prosper_pt_ctx *ctx, prosper_host_forward_renderer **out);
void prosper_host_forward_renderer_destroy(prosper_host_forward_renderer *pass);
/* ForwardRenderer::setTextureLod / setLodBias: later records of both passes sample every material through the mip chains. */
int prosper_host_forward_renderer_set_texture_lod(prosper_host_forward_renderer *pass, int enabled, float lodBias);
int prosper_host_forward_renderer_record_transparent(
    prosper_host_forward_renderer *pass, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const float *nonLinearDepth, uint32_t onDevice, uint32_t rayFlags, uint32_t frameIndex, int applyIbl, uint32_t drawType,
    void *stream, prosper_pt_forward_pc *outPushConstants);
/* ForwardRenderer::recordTransparentRaster: Camera::updateBuffer + prosper_pt_raster_forward_transparent -
 * the TRANSPARENT list culled once, its per-pixel fragment lists, their resolve over the context's HDR image, against
 * `nonLinearDepth` (NULL: the context's last depth, a forward frame's included).  The raster frame's transparents; the call
 * waits on the host once.  The context's draw lists are the transparent ones afterwards. */
int prosper_host_forward_renderer_record_transparent_raster(
    prosper_host_forward_renderer *pass, prosper_host_camera *camera, uint32_t width, uint32_t height, const float *nonLinearDepth,
    uint32_t onDevice, int applyIbl, uint32_t drawType, void *stream, prosper_pt_forward_pc *outPushConstants);
typedef struct prosper_host_forward_renderer_output
{
    const void *illumination; /* the context's HDR image */
    const void *velocity;
    const float *depth;
} prosper_host_forward_renderer_output;
int prosper_host_forward_renderer_record_opaque(
    prosper_host_forward_renderer *pass, prosper_host_camera *camera, uint32_t width, uint32_t height, int applyIbl, uint32_t drawType,
    const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount, void *stream, prosper_host_forward_renderer_output *out);
int prosper_host_forward_renderer_release_preserved(prosper_host_forward_renderer *pass);

/* render::particles::Particles (host/particles.hpp; reference src/render/particles/Particles.hpp) on a context
 * (borrowed): record = Camera::updateBuffer + prosper_pt_particles with every stage, over the context's HDR image and
 * `nonLinearDepth` (device, or NULL: the last traced G-buffer's).  It keeps m_resetParticles (true at first, cleared only
 * when init was recorded) and the two frame indices; *outPushConstants (may be NULL) receives what it pushed,
 * *outInitRecorded (may be NULL) whether init was recorded.  set_source / set_max_particle_count: the draw instance the
 * emitters come from (default 0) and the pool's size (0: 500 000). */
typedef struct prosper_host_particles prosper_host_particles;
int prosper_host_particles_create(prosper_pt_ctx *ctx, prosper_host_particles **out);
void prosper_host_particles_destroy(prosper_host_particles *pass);
void prosper_host_particles_set_source(prosper_host_particles *pass, uint32_t sourceDrawInstanceIndex);
void prosper_host_particles_set_max_particle_count(prosper_host_particles *pass, uint32_t maxParticleCount);
int prosper_host_particles_record(
    prosper_host_particles *pass, prosper_host_camera *camera, uint32_t width, uint32_t height, float *nonLinearDepth,
    float deltaTimeS, void *stream, prosper_pt_particles_pc *outPushConstants, uint32_t *outInitRecorded);

/* scene::DebugLines and render::DebugRenderer (host/debug_renderer.hpp; reference src/scene/DebugGeometry.hpp,
 * src/render/DebugRenderer.cpp): a host-side list of at most 100 000 lines (reset / add_line; an add to a full list is
 * refused where the reference would write past its buffer), and record = Camera::updateBuffer + prosper_pt_debug_lines
 * over the context's HDR image and the last traced G-buffer's depth. */
typedef struct prosper_host_debug_lines prosper_host_debug_lines;
int prosper_host_debug_lines_create(prosper_host_debug_lines **out);
void prosper_host_debug_lines_destroy(prosper_host_debug_lines *lines);
void prosper_host_debug_lines_reset(prosper_host_debug_lines *lines);
int prosper_host_debug_lines_add_line(prosper_host_debug_lines *lines, const float *p0, const float *p1, const float *color);
uint32_t prosper_host_debug_lines_count(const prosper_host_debug_lines *lines);
const float *prosper_host_debug_lines_data(const prosper_host_debug_lines *lines);
typedef struct prosper_host_debug_renderer prosper_host_debug_renderer;
int prosper_host_debug_renderer_create(prosper_pt_ctx *ctx, prosper_host_debug_renderer **out);
void prosper_host_debug_renderer_destroy(prosper_host_debug_renderer *pass);
int prosper_host_debug_renderer_record(
    prosper_host_debug_renderer *pass, prosper_host_camera *camera, const prosper_host_debug_lines *lines, uint32_t width,
    uint32_t height, void *stream);

/* render::TextureReadback (host/texture_readback.hpp; reference src/render/TextureReadback.cpp) on a context
 * (borrowed): record queues prosper_pt_texture_readback of registry entry `resource` and sets the reference's
 * m_framesUntilReady to MAX_FRAMES_IN_FLIGHT = 2; start_frame counts it down; readback gives nothing (*outReady 0) while
 * it is above 0 or the copy has not finished, then the value once.  Where the reference asserts - a second record while
 * one is unread, readback with none in flight, a frame started at 0 that nobody polled - the call is refused with
 * PROSPER_PT_ERR_INVALID_ARGUMENT and the assertion's text in prosper_host_last_error. */
typedef struct prosper_host_texture_readback prosper_host_texture_readback;
int prosper_host_texture_readback_create(prosper_pt_ctx *ctx, prosper_host_texture_readback **out);
void prosper_host_texture_readback_destroy(prosper_host_texture_readback *pass);
int prosper_host_texture_readback_start_frame(prosper_host_texture_readback *pass);
int prosper_host_texture_readback_record(prosper_host_texture_readback *pass, uint32_t resource, float pxX, float pxY, void *stream);
int prosper_host_texture_readback_readback(prosper_host_texture_readback *pass, float out[4], uint32_t *outReady);
int32_t prosper_host_texture_readback_frames_until_ready(const prosper_host_texture_readback *pass);

/* render::TextureDebug (host/texture_debug.hpp; reference src/render/TextureDebug.cpp) on a context (borrowed): set_target
 * names a registry image ("" or NULL deselects; texture_selected says whether one is named), set_settings keeps the
 * reference's per-name TargetSettings (range, lod, channel 0-3 or 4 = RGB, abs, bilinear sampler), set_zoom its zoom
 * toggle; record = prosper_pt_texture_debug of the selected image into outWidth x outHeight RGBA8, with the magnifier
 * when cursorUv (two floats, may be NULL) is given, the LOD clamped to the image's last level; *outPushConstants (may be
 * NULL) receives what it pushed.  peeked_value: prosper_pt_get_texture_debug_peek. */
typedef struct prosper_host_texture_debug prosper_host_texture_debug;
int prosper_host_texture_debug_create(prosper_pt_ctx *ctx, prosper_host_texture_debug **out);
void prosper_host_texture_debug_destroy(prosper_host_texture_debug *pass);
void prosper_host_texture_debug_set_target(prosper_host_texture_debug *pass, const char *name);
int prosper_host_texture_debug_texture_selected(const prosper_host_texture_debug *pass);
void prosper_host_texture_debug_set_settings(
    prosper_host_texture_debug *pass, const char *name, float rangeLo, float rangeHi, int32_t lod, uint32_t channelType,
    int absBeforeRange, int useBilinearSampler);
void prosper_host_texture_debug_set_zoom(prosper_host_texture_debug *pass, int zoom);
int prosper_host_texture_debug_record(
    prosper_host_texture_debug *pass, uint32_t outWidth, uint32_t outHeight, const float *cursorUv, void *deviceRgba8,
    uint8_t *hostRgba8, size_t byteSize, void *stream, prosper_pt_texture_debug_pc *outPushConstants);
int prosper_host_texture_debug_peeked_value(prosper_host_texture_debug *pass, float out[4]);

/* render::dof::DepthOfField (host/depth_of_field.hpp; reference src/render/dof/DepthOfField.hpp) on a context
 * (borrowed): record = Camera::updateBuffer + prosper_pt_depth_of_field with the push constants computed from the
 * camera's aperture, focus distance and focal length as dof/Setup.cpp and dof/Dilate.cpp compute them; returns them. */
typedef struct prosper_host_depth_of_field prosper_host_depth_of_field;
int prosper_host_depth_of_field_create(prosper_pt_ctx *ctx, prosper_host_depth_of_field **out);
void prosper_host_depth_of_field_destroy(prosper_host_depth_of_field *pass);
int prosper_host_depth_of_field_record(
    prosper_host_depth_of_field *pass, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const prosper_pt_dof_inputs *inputs, void *stream, prosper_pt_dof_pc *outPushConstants);

/* render::bloom::Bloom (host/bloom.hpp; reference src/render/bloom/Bloom.hpp) on a context (borrowed), with prosper's
 * defaults: threshold 1, blend factors .9, .04, .04, biquadratic sampling, half resolution.  draw_ui sets what prosper's
 * drawUi edits (resolutionScale: 0 Half, 1 Quarter); record = prosper_pt_bloom with those settings over `illumination`
 * (RGBA32F; NULL: the context's HDR image in place) and returns the push constants it used.  set_technique picks
 * render::bloom::Technique (0 MultiResolutionBlur, the default; 1 Fft; any other value is ignored with the checkbox) and
 * sets GenerateKernel's "Re-generate kernel";
 * with Fft, record = prosper_pt_bloom_fft with what fft_push_constants returns, and `outPushConstants` still receives
 * the blur's.  A record with the blur drops the kernel's DFT as Bloom.cpp:117 does; release_preserved drops it too. */
typedef struct prosper_host_bloom prosper_host_bloom;
int prosper_host_bloom_create(prosper_pt_ctx *ctx, prosper_host_bloom **out);
void prosper_host_bloom_destroy(prosper_host_bloom *pass);
void prosper_host_bloom_draw_ui(
    prosper_host_bloom *pass, float threshold, float blendFactor0, float blendFactor1, float blendFactor2,
    uint32_t biquadratic, uint32_t resolutionScale);
void prosper_host_bloom_set_technique(prosper_host_bloom *pass, uint32_t technique, uint32_t regenerateKernel);
void prosper_host_bloom_release_preserved(prosper_host_bloom *pass);
void prosper_host_bloom_fft_push_constants(prosper_host_bloom *pass, prosper_pt_bloom_fft_pc *out);
int prosper_host_bloom_record(
    prosper_host_bloom *pass, uint32_t width, uint32_t height, const void *illumination, uint32_t onDevice, void *stream,
    prosper_pt_bloom_pc *outPushConstants);

/* render::TemporalAntiAliasing (host/temporal_anti_aliasing.hpp; reference src/render/TemporalAntiAliasing.hpp) on a
 * context (borrowed), with prosper's defaults: Catmull-Rom, Variance clipping, Closest velocity, luminance weighting.
 * draw_ui sets what prosper's drawUi edits; record = prosper_pt_taa_resolve with those settings over `inputs` and
 * returns the push constants it used; release_preserved = TemporalAntiAliasing::releasePreserved. */
typedef struct prosper_host_taa prosper_host_taa;
int prosper_host_taa_create(prosper_pt_ctx *ctx, prosper_host_taa **out);
void prosper_host_taa_destroy(prosper_host_taa *pass);
void prosper_host_taa_draw_ui(
    prosper_host_taa *pass, uint32_t catmullRom, uint32_t colorClipping, uint32_t velocitySampling, uint32_t luminanceWeighting);
int prosper_host_taa_record(
    prosper_host_taa *pass, uint32_t width, uint32_t height, const prosper_pt_taa_inputs *inputs, void *stream,
    prosper_pt_taa_pc *outPushConstants);
void prosper_host_taa_release_preserved(prosper_host_taa *pass);

/* scene::Animations (host/animations.hpp; reference src/scene/World.hpp updateAnimations / updateScene) on a context
 * (borrowed) whose scene is uploaded: create = prosper_pt_set_animations of `desc` (borrowed for the call); update =
 * World::updateAnimations(timeS), staged for the next render (prosper_pt_animate); end_time = Scene::endTimeS. */
typedef struct prosper_host_animations prosper_host_animations;
int prosper_host_animations_create(prosper_pt_ctx *ctx, const prosper_pt_animation_desc *desc, prosper_host_animations **out);
void prosper_host_animations_destroy(prosper_host_animations *animations);
int prosper_host_animations_update(prosper_host_animations *animations, float timeS);
float prosper_host_animations_end_time(const prosper_host_animations *animations);

#ifdef __cplusplus
}
#endif

#endif /* PROSPER_HOST_H */
