// pt_gbuffer_passes.cpp — C-ABI of the passes over a G-buffer (include/prosper_pt/prosper_pt.h): ReSTIR-DI
// (prosper_pt_restir_di_*), the ray-traced G-buffer (prosper_pt_trace_gbuffer), clustered lighting and deferred shading
// (prosper_pt_cluster_lights, prosper_pt_deferred_shading), the rasteriser's resolve into the same targets
// (prosper_pt_raster_resolve), image-based lighting (prosper_pt_generate_ibl) and the texture LOD switches, with the
// readbacks of what each produced.  The module owns the context's last frame and the lighting inputs, which the other pass
// modules reach through pt_gbuffer_passes.hpp; the forward passes over them are in pt_forward_passes.cpp.
// Kernels: pt_gbuffer_kernels.hip, pt_ibl.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_context.hpp"
#include "pt_gbuffer_kernels.hpp"
#include "pt_gbuffer_passes.hpp"
#include "pt_kernels.hpp"
#include "pt_pass_support.hpp"
#include "pt_raster.hpp"

using namespace ppt;

namespace ppt
{

struct GBufferPassState
{
    DeviceBuffer hostInputs; // device copies of a call's host G-buffer inputs (and reservoirs): 16 + 16 + 8 + 4 bytes per pixel
    DeviceBuffer reservoirs[2]; // ping-pong reservoir buffers of the ReSTIR-DI passes (width*height float2 each)
    const void *lastReservoirs = nullptr; // prosper_pt_get_restir_reservoirs_device_ptr
    size_t lastReservoirBytes = 0;
    DeviceBuffer gbuffer; // context-owned G-buffer targets (prosper_pt_trace_gbuffer): 16 + 16 + 4 bytes per pixel
    DeviceBuffer velocity;           // context-owned velocity target (prosper_pt_trace_gbuffer_velocity): 8 bytes per pixel
    DeviceBuffer previousTransforms; // the device copy of a call's previous instance transforms
    LastFrame last; // what the last G-buffer or forward frame wrote, here or into the caller's targets
    // prosper_pt_set_texture_lod / _debug: the traced G-buffer samples materials through the mip chains
    bool lodEnabled = false, lodDebug = false;
    float lodBias = 0.0f;
    DeviceBuffer lodDerivatives; // debug: float4 per pixel of the last traced G-buffer (last.derivativesWidth)
    DeviceBuffer clusterPointers; // prosper_pt_cluster_lights: uint2 per cluster
    DeviceBuffer clusterIndices;  // kClusterSlot uint16 entries per cluster
    DeviceBuffer clusterDropped;  // entries dropped, per cluster
    size_t clusterCapacity = 0;   // clusters the buffers hold
    uint32_t clusterDims[3] = {}; // of the last clustering
    DeviceBuffer iblIrradiance; // prosper_pt_generate_ibl: kIblIrradianceTexels RGBA16F, bordered cube
    DeviceBuffer iblRadiance;   // kIblRadianceTexels RGBA16F, 10 bordered mips
    DeviceBuffer iblLut;        // kIblLutSize^2 R16G16 UNORM
    StageEvents<3> iblTiming;   // around the three passes of the last generation
    bool iblGenerated = false;    // the maps describe the current scene's sky (cleared by prosper_pt_upload_scene)
    // what the last clustering was made from: the forward passes reuse it for the same camera and lights
    ClusterParams clusterParams = {};
    uint32_t clusterLightUpdates = 0;
    bool clusterValid = false; // (cleared by prosper_pt_upload_scene)
};

void gbuffer_texture_lod(const prosper_pt_ctx *ctx, bool *enabled, float *bias)
{
    *enabled = ctx->gbufferPasses->lodEnabled;
    *bias = ctx->gbufferPasses->lodBias;
}

const GBufferLodParams *gbuffer_lod_params(const prosper_pt_ctx *ctx, GBufferLodParams &storage)
{
    storage = GBufferLodParams{ctx->textureMips, ctx->gbufferPasses->lodBias, nullptr};
    return ctx->gbufferPasses->lodEnabled && ctx->textureMips ? &storage : nullptr;
}

void LastFrame::set_gbuffer(const prosper_pt_gbuffer_targets &t, void *v, uint32_t w, uint32_t h)
{
    targets = t;
    width = w;
    height = h;
    forwardDepthOwned = false;
    if (!v) return;
    velocity = v;
    velocityWidth = w;
    velocityHeight = h;
}

void LastFrame::set_forward(float *depth, bool depthOwned, void *v, uint32_t w, uint32_t h)
{
    prosper_pt_gbuffer_targets t = {};
    t.nonLinearDepth = depth;
    set_gbuffer(t, v, w, h);
    forwardDepthOwned = depthOwned;
    derivativesWidth = derivativesHeight = 0;
}

void LastFrame::forget_if_in(const DeviceBuffer &b)
{
    if (lies_in(b, targets.albedoRoughness) || lies_in(b, targets.normalMetallic) || lies_in(b, targets.nonLinearDepth))
    {
        targets = prosper_pt_gbuffer_targets{};
        width = height = 0;
        forwardDepthOwned = false;
    }
    if (lies_in(b, velocity))
    {
        velocity = nullptr;
        velocityWidth = velocityHeight = 0;
    }
}

int LastFrame::depth(const float **out, uint32_t *w, uint32_t *h) const
{
    if (!targets.nonLinearDepth) return fail(PROSPER_PT_ERR_NO_SCENE, "no G-buffer has been traced yet");
    *out = targets.nonLinearDepth;
    *w = width;
    *h = height;
    return PROSPER_PT_OK;
}

LastFrame &gbuffer_last_frame(prosper_pt_ctx *ctx) { return ctx->gbufferPasses->last; }

int gbuffer_last_depth(prosper_pt_ctx *ctx, const float **depth, uint32_t *width, uint32_t *height)
{
    return ctx->gbufferPasses->last.depth(depth, width, height);
}

// the G-buffer, the velocity, the IBL LUT
static void list_gbuffer_debug_images(const prosper_pt_ctx *ctx, std::vector<DebugImage> &out)
{
    const GBufferPassState &st = *ctx->gbufferPasses;
    const LastFrame &last = st.last;
    // only targets the context owns: a caller's buffers may be gone by the time someone looks.  A forward frame leaves a
    // depth and no attribute targets (prosper_pt_raster_forward)
    const bool g = LastFrame::lies_in(st.gbuffer, last.targets.albedoRoughness) && LastFrame::lies_in(st.gbuffer, last.targets.normalMetallic) &&
                   LastFrame::lies_in(st.gbuffer, last.targets.nonLinearDepth);
    const struct
    {
        const char *name;
        uint32_t format;
        const void *ptr;
        bool valid;
    } targets[3] = {{"albedoRoughness", PROSPER_PT_DEBUG_FORMAT_RGBA32F, last.targets.albedoRoughness, g},
                    {"normalMetalness", PROSPER_PT_DEBUG_FORMAT_RGBA32F, last.targets.normalMetallic, g},
                    {"depth", PROSPER_PT_DEBUG_FORMAT_R32F, last.targets.nonLinearDepth, g || last.forwardDepthOwned}};
    for (const auto &t : targets)
    {
        DebugImage im;
        im.name = t.name;
        im.format = t.format;
        im.valid = t.valid;
        if (t.valid) im.one_level(t.ptr, last.width, last.height);
        out.push_back(im);
    }
    DebugImage v;
    v.name = "velocity";
    v.format = PROSPER_PT_DEBUG_FORMAT_RG32F;
    v.valid = LastFrame::lies_in(st.velocity, last.velocity);
    if (v.valid) v.one_level(last.velocity, last.velocityWidth, last.velocityHeight);
    out.push_back(v);
    DebugImage lut;
    lut.name = "SpecularBrdfLut";
    lut.format = PROSPER_PT_DEBUG_FORMAT_RG16_UNORM;
    lut.valid = st.iblGenerated && st.iblLut.ptr;
    if (lut.valid) lut.one_level(st.iblLut.ptr, kIblLutSize, kIblLutSize);
    out.push_back(lut);
}

// a new scene: the image-based lighting maps describe the old sky
static void forget_ibl_maps(prosper_pt_ctx *ctx)
{
    ctx->gbufferPasses->iblGenerated = false;
    ctx->gbufferPasses->clusterValid = false; // the clustering describes the old scene's lights too
}

extern const PassModule kGBufferPasses = pass_module<GBufferPassState, &prosper_pt_ctx::gbufferPasses>(forget_ibl_maps, list_gbuffer_debug_images);

RestirCamera gbuffer_camera(const prosper_CameraUniforms *camera)
{
    RestirCamera c;
    c.eye[0] = camera->eye.x;
    c.eye[1] = camera->eye.y;
    c.eye[2] = camera->eye.z;
    std::memcpy(c.clipToWorld, &camera->clipToWorld, 64);
    float c2c[16];
    std::memcpy(c2c, &camera->cameraToClip, 64);
    c.cameraToClip22 = c2c[2 * 4 + 2]; // column 2, row 2
    c.cameraToClip32 = c2c[3 * 4 + 2]; // column 3, row 2
    return c;
}

GBufferTraceParams gbuffer_trace_params(
    uint32_t drawType, uint32_t frameIndex, bool jitter, bool opaqueOnly, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height)
{
    GBufferTraceParams g = {};
    set_camera_ray_params(g.r, camera);
    g.r.width = width;
    g.r.height = height;
    g.r.localWidth = width;
    g.r.stripeCount = 1;
    g.r.frameCount = 1;
    // worldToClip = cameraToClip * worldToCamera (column-major), in double, rounded once
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r)
        {
            double v = 0.0;
            for (int k = 0; k < 4; ++k)
                v += (double)(&camera->cameraToClip.col[k].x)[r] * (double)(&camera->worldToCamera.col[c].x)[k];
            g.worldToClip[c * 4 + r] = (float)v;
        }
    g.drawType = drawType;
    g.frameIndex = frameIndex;
    g.jitter = jitter ? 1u : 0u;
    g.opaqueOnly = opaqueOnly ? 1u : 0u;
    return g;
}

void velocity_camera_terms(GBufferVelocityParams &v, const prosper_CameraUniforms *camera)
{
    std::memcpy(v.worldToCamera, &camera->worldToCamera, 64);
    std::memcpy(v.cameraToClip, &camera->cameraToClip, 64);
    std::memcpy(v.previousWorldToCamera, &camera->previousWorldToCamera, 64);
    std::memcpy(v.previousCameraToClip, &camera->previousCameraToClip, 64);
    for (int k = 0; k < 2; ++k)
    {
        v.currentJitter[k] = camera->currentJitter[k];
        v.previousJitter[k] = camera->previousJitter[k];
    }
}

int velocity_owned_target(prosper_pt_ctx *ctx, size_t pixels, hipStream_t s, float2 **out)
{
    GBufferPassState &st = *ctx->gbufferPasses;
    const int rc = st.last.grow(st.velocity, pixels * 8u, s);
    *out = st.velocity.as<float2>();
    return rc;
}

int upload_previous_transforms(
    prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count, hipStream_t s, const prosper_ModelInstanceTransforms **out)
{
    GBufferPassState &st = *ctx->gbufferPasses;
    const size_t bytes = sizeof(prosper_ModelInstanceTransforms) * (size_t)count;
    const int rc = grow_to(st.previousTransforms, bytes, s);
    if (rc != PROSPER_PT_OK) return rc;
    PPT_HIP(hipMemcpyAsync(st.previousTransforms.ptr, transforms, bytes, hipMemcpyHostToDevice, s));
    *out = st.previousTransforms.as<prosper_ModelInstanceTransforms>();
    return PROSPER_PT_OK;
}

} // namespace ppt

namespace
{

// The G-buffer (and, with `withReservoirs`, the reservoirs) on the device: host inputs are copied into hostInputs,
// 16 + 16 + 8 + 4 bytes per pixel.
struct DeviceGBuffer
{
    const void *ar, *nm, *res;
    const float *depth;
};
int device_gbuffer(
    prosper_pt_ctx *ctx, const prosper_pt_restir_inputs *in, size_t pixels, bool withReservoirs, hipStream_t s,
    DeviceGBuffer &out)
{
    out.ar = in->albedoRoughness;
    out.nm = in->normalMetallic;
    out.res = in->reservoirs;
    out.depth = in->nonLinearDepth;
    if (in->onDevice) return PROSPER_PT_OK;
    DeviceBuffer &scratch = ctx->gbufferPasses->hostInputs;
    const size_t need = pixels * 44u + 64u;
    if (scratch.bytes < need)
    {
        const int rc = grow_buffer(scratch, GrowWait::Stream, s, need, need);
        if (rc != PROSPER_PT_OK) return rc;
    }
    uint8_t *base = scratch.as<uint8_t>();
    PPT_HIP(hipMemcpyAsync(base, in->albedoRoughness, pixels * 16u, hipMemcpyHostToDevice, s));
    PPT_HIP(hipMemcpyAsync(base + pixels * 16u, in->normalMetallic, pixels * 16u, hipMemcpyHostToDevice, s));
    if (withReservoirs) PPT_HIP(hipMemcpyAsync(base + pixels * 32u, in->reservoirs, pixels * 8u, hipMemcpyHostToDevice, s));
    PPT_HIP(hipMemcpyAsync(base + pixels * 40u, in->nonLinearDepth, pixels * 4u, hipMemcpyHostToDevice, s));
    out.ar = base;
    out.nm = base + pixels * 16u;
    out.res = base + pixels * 32u;
    out.depth = reinterpret_cast<const float *>(base + pixels * 40u);
    return PROSPER_PT_OK;
}

// The two context-owned reservoir buffers, grown like hostInputs (what still reads them on `s` finishes first).
int restir_reservoir_buffers(prosper_pt_ctx *ctx, size_t pixels, hipStream_t s)
{
    GBufferPassState &st = *ctx->gbufferPasses;
    const size_t need = pixels * 8u;
    if (st.reservoirs[0].bytes >= need && st.reservoirs[1].bytes >= need) return PROSPER_PT_OK;
    st.lastReservoirs = nullptr;
    st.lastReservoirBytes = 0;
    for (DeviceBuffer &r : st.reservoirs)
    {
        const int rc = grow_buffer(r, GrowWait::Stream, s, need, need);
        if (rc != PROSPER_PT_OK) return rc;
    }
    return PROSPER_PT_OK;
}

// The trace pass over device inputs: the HDR image, the traversal stacks, the launch.
int restir_trace(
    prosper_pt_ctx *ctx, const prosper_pt_restir_trace_pc *pc, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, const DeviceGBuffer &in, hipStream_t s)
{
    const int hrc = prepare_hdr(ctx, width, height, nullptr, s);
    if (hrc != PROSPER_PT_OK) return hrc;

    int32_t *ovf = nullptr;
    const int orc = ensure_stack_overflow(ctx, ctx->slots[0], kTraversalStackDepth, restir_grid_blocks(width, height), &ovf);
    if (orc != PROSPER_PT_OK) return orc;
    wait_for_slot(ctx->slots[0], s);
    launch_restir_di_trace(
        ctx->scene, pc->drawType, pc->frameIndex, pc->flags, width, height, gbuffer_camera(camera), in.ar, in.nm, in.depth,
        in.res, ctx->hdr, ovf, s);
    release_slot(ctx->slots[0], s);
    PPT_HIP(hipGetLastError());
    return PROSPER_PT_OK;
}

// The context-owned targets, one allocation of 16 + 16 + 4 bytes per pixel, grown like hostInputs.
int gbuffer_owned_targets(prosper_pt_ctx *ctx, size_t pixels, hipStream_t s, prosper_pt_gbuffer_targets &out)
{
    GBufferPassState &st = *ctx->gbufferPasses;
    const int rc = st.last.grow(st.gbuffer, pixels * 36u + 64u, s);
    if (rc != PROSPER_PT_OK) return rc;
    uint8_t *base = st.gbuffer.as<uint8_t>();
    out.albedoRoughness = base;
    out.normalMetallic = base + pixels * 16u;
    out.nonLinearDepth = reinterpret_cast<float *>(base + pixels * 32u);
    return PROSPER_PT_OK;
}

// The G-buffer pass on `s` after flush_scene_updates: camera terms, the traversal stacks, the launch.  `velocity`: the
// velocity variant, whose matrices and jitters are filled in here from `camera`.
int gbuffer_trace(
    prosper_pt_ctx *ctx, uint32_t drawType, uint32_t frameIndex, bool jitter, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_gbuffer_targets &t, hipStream_t s, GBufferVelocityParams *velocity = nullptr,
    bool opaqueOnly = false, const RasterResolveTables *raster = nullptr)
{
    const GBufferTraceParams g = gbuffer_trace_params(drawType, frameIndex, jitter, opaqueOnly, camera, width, height);

    int32_t *ovf = nullptr;
    const int orc = ensure_stack_overflow(ctx, ctx->slots[0], kTraversalStackDepth, restir_grid_blocks(width, height), &ovf);
    if (orc != PROSPER_PT_OK) return orc;
    wait_for_slot(ctx->slots[0], s);
    GBufferPassState &st = *ctx->gbufferPasses;
    GBufferLodParams lodParams;
    const GBufferLodParams *lod = gbuffer_lod_params(ctx, lodParams);
    st.last.derivativesWidth = st.last.derivativesHeight = 0;
    if (lod && st.lodDebug)
    {
        const int grc = grow_to(st.lodDerivatives, (size_t)width * height * sizeof(float4), s);
        if (grc != PROSPER_PT_OK) return grc;
        lodParams.derivatives = st.lodDerivatives.as<float4>();
        st.last.derivativesWidth = width;
        st.last.derivativesHeight = height;
    }
    if (velocity)
    {
        velocity_camera_terms(*velocity, camera);
        // `raster`: the resolve of the rasteriser's visibility image writes the targets instead of a trace
        if (raster)
            launch_raster_resolve(ctx->scene, g, *raster, *velocity, t.albedoRoughness, t.normalMetallic, t.nonLinearDepth, s, lod);
        else
            launch_gbuffer_trace_velocity(ctx->scene, g, *velocity, t.albedoRoughness, t.normalMetallic, t.nonLinearDepth, ovf, s, lod);
    }
    else
        launch_gbuffer_trace(ctx->scene, g, t.albedoRoughness, t.normalMetallic, t.nonLinearDepth, ovf, s, lod);
    release_slot(ctx->slots[0], s);
    PPT_HIP(hipGetLastError());
    st.last.set_gbuffer(t, velocity ? velocity->velocity : nullptr, width, height);
    return PROSPER_PT_OK;
}

// The G-buffer a record or shading call reads on `s`: traced first into the context-owned targets (`traced`; never the
// hostInputs a host-input call fills), or the caller's, copied to the device when it is on the host.
int call_gbuffer(
    prosper_pt_ctx *ctx, bool traced, uint32_t drawType, uint32_t frameIndex, bool jitter, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_restir_inputs *gbuffer, hipStream_t s, DeviceGBuffer &out)
{
    const size_t pixels = (size_t)width * height;
    if (!traced) return device_gbuffer(ctx, gbuffer, pixels, false, s, out);
    prosper_pt_gbuffer_targets t = {};
    int rc = gbuffer_owned_targets(ctx, pixels, s, t);
    if (rc == PROSPER_PT_OK) rc = gbuffer_trace(ctx, drawType, frameIndex, jitter, camera, width, height, t, s);
    out.ar = t.albedoRoughness;
    out.nm = t.normalMetallic;
    out.depth = t.nonLinearDepth;
    out.res = nullptr;
    return rc;
}

ClusterParams cluster_params(const prosper_CameraUniforms *camera, uint32_t width, uint32_t height)
{
    ClusterParams c;
    std::memcpy(c.worldToCamera, &camera->worldToCamera, 64);
    float c2c[16];
    std::memcpy(c2c, &camera->cameraToClip, 64);
    c.cameraToClip00 = c2c[0];
    c.cameraToClip11 = c2c[1 * 4 + 1];
    c.resolution[0] = (float)camera->resolution[0];
    c.resolution[1] = (float)camera->resolution[1];
    c.near_ = camera->near_;
    c.far_ = camera->far_;
    c.dimX = (width + kClusterDim - 1u) / kClusterDim;
    c.dimY = (height + kClusterDim - 1u) / kClusterDim;
    return c;
}

// The clustering pass on `s` after flush_scene_updates: buffers grown as needed (the index buffer starts as 0xFFFF), the
// launch.  Every cluster writes its pointer and dropped count, so nothing is cleared (LightClustering.cpp's fillBuffer
// of the counter is replaced by summing the pointers' counts in prosper_pt_read_light_clusters).
int cluster_lights(prosper_pt_ctx *ctx, const ClusterParams &c, hipStream_t s)
{
    GBufferPassState &st = *ctx->gbufferPasses;
    const size_t clusters = (size_t)c.dimX * c.dimY * (kClusterZSlices + 1u);
    if (st.clusterCapacity < clusters || !st.clusterPointers.ptr)
    {
        st.clusterCapacity = 0;
        st.clusterDims[0] = st.clusterDims[1] = st.clusterDims[2] = 0;
        int rc = grow_buffer(st.clusterPointers, GrowWait::Stream, s, clusters * 8u, clusters * 8u);
        if (rc == PROSPER_PT_OK)
            rc = grow_buffer(st.clusterIndices, GrowWait::Stream, s, clusters * kClusterSlot * 2u, clusters * kClusterSlot * 2u, 0xFF);
        if (rc == PROSPER_PT_OK) rc = grow_buffer(st.clusterDropped, GrowWait::Stream, s, clusters * 4u, clusters * 4u);
        if (rc != PROSPER_PT_OK) return rc;
        st.clusterCapacity = clusters;
    }
    launch_light_clustering(
        ctx->scene, c, st.clusterPointers.ptr, st.clusterIndices.as<uint16_t>(), st.clusterDropped.as<uint32_t>(), s);
    PPT_HIP(hipGetLastError());
    st.clusterDims[0] = c.dimX;
    st.clusterDims[1] = c.dimY;
    st.clusterDims[2] = kClusterZSlices + 1u;
    st.clusterParams = c;
    st.clusterLightUpdates = ctx->lights ? ctx->lights->updates : 0u;
    st.clusterValid = true;
    return PROSPER_PT_OK;
}

// near_ and far_ feed log(far / near) and pow(far / near, s): both positive and ordered
bool cluster_camera_ok(const prosper_CameraUniforms *camera)
{
    return camera->near_ > 0.0f && camera->far_ > camera->near_ && camera->resolution[0] > 0 && camera->resolution[1] > 0;
}

// The interior texels of `levels` bordered cubes (6 faces of (n + 2)^2 RGBA16F each, n halving per level) to host
void strip_cube_borders(const std::vector<uint16_t> &bordered, uint32_t n, uint32_t levels, uint16_t *out)
{
    size_t src = 0;
    for (uint32_t m = 0; m < levels; ++m, n >>= 1)
    {
        const size_t n2 = n + 2u;
        for (uint32_t face = 0; face < 6u; ++face)
            for (uint32_t j = 0; j < n; ++j)
            {
                std::memcpy(out, &bordered[4u * (src + ((size_t)face * n2 + j + 1u) * n2 + 1u)], (size_t)n * 8u);
                out += 4u * (size_t)n;
            }
        src += 6u * n2 * n2;
    }
}

} // namespace

int ppt::check_lit_pass(const char *what, const prosper_pt_ctx *ctx, uint32_t drawType, uint32_t ibl, const prosper_CameraUniforms *camera)
{
    if (drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    if (ibl > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": ibl is 0 or 1");
    if (ibl == 1u && (!ctx || !ctx->gbufferPasses->iblGenerated))
        return fail(PROSPER_PT_ERR_UNSUPPORTED,
                    std::string(what) + ": ibl = 1 needs ImageBasedLighting's maps and BRDF LUT: call prosper_pt_generate_ibl after the scene upload");
    if (!cluster_camera_ok(camera))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": camera needs 0 < near_ < far_ and a resolution");
    return PROSPER_PT_OK;
}

int ppt::check_velocity_inputs(
    const char *what, prosper_pt_ctx *ctx, const void *velocity, const prosper_ModelInstanceTransforms *previousTransforms, uint32_t previousTransformCount)
{
    if (reinterpret_cast<uintptr_t>(velocity) & 7u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the velocity target must be 8-byte aligned");
    if (!previousTransforms && previousTransformCount != 0u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": previousTransformCount without previousTransforms");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    const int crc = check_scene(ctx, what);
    if (crc != PROSPER_PT_OK) return crc;
    if (previousTransforms && previousTransformCount != ctx->scene.modelInstanceCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": previousTransformCount differs from the scene's modelInstanceCount");
    return PROSPER_PT_OK;
}

int ppt::clustered_lights(
    prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, bool ibl, hipStream_t s, ClusteredLights *out,
    bool *reused)
{
    const GBufferPassState &st = *ctx->gbufferPasses;
    const ClusterParams c = cluster_params(camera, width, height);
    const uint32_t lightUpdates = ctx->lights ? ctx->lights->updates : 0u;
    const bool current = reused && st.clusterValid && std::memcmp(&st.clusterParams, &c, sizeof(c)) == 0 && st.clusterLightUpdates == lightUpdates;
    if (reused) *reused = current;
    if (!current)
        if (const int rc = cluster_lights(ctx, c, s)) return rc;
    *out = ClusteredLights{c, st.clusterPointers.ptr, st.clusterIndices.as<uint16_t>(), nullptr, nullptr, nullptr};
    if (ibl)
    {
        out->irradiance = st.iblIrradiance.as<uint16_t>();
        out->radiance = st.iblRadiance.as<uint16_t>();
        out->lut = st.iblLut.as<uint32_t>();
    }
    return PROSPER_PT_OK;
}

extern "C" {

// ---- ReSTIR-DI (src/render/rtdi/RtDirectIllumination.cpp:70-115) ----

int prosper_pt_restir_di_trace(
    prosper_pt_ctx *ctx, const prosper_pt_restir_trace_pc *pc, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, const prosper_pt_restir_inputs *in, void *stream)
{
    if (!ctx || !pc || !camera || !in || !in->albedoRoughness || !in->normalMetallic || !in->nonLinearDepth || !in->reservoirs)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_trace: null argument");
    const int crc = check_scene(ctx, "prosper_pt_restir_di_trace");
    if (crc != PROSPER_PT_OK) return crc;
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_trace: empty extent");
    if (pc->drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    DeviceGBuffer din;
    rc = device_gbuffer(ctx, in, (size_t)width * height, true, s, din);
    if (rc == PROSPER_PT_OK) rc = restir_trace(ctx, pc, camera, width, height, din, s);
    if (rc != PROSPER_PT_OK) return rc;
    return mark_versions_read(ctx, s);
}

int prosper_pt_restir_di_resample(
    prosper_pt_ctx *ctx, uint32_t stage, uint32_t frameIndex, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, const prosper_pt_restir_inputs *in, void *device_out_reservoirs, void *stream)
{
    if (!ctx || !camera || !in || !in->albedoRoughness || !in->normalMetallic || !in->nonLinearDepth)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_resample: null argument");
    if (stage != PROSPER_PT_RESTIR_INITIAL && stage != PROSPER_PT_RESTIR_SPATIAL)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_resample: unknown stage");
    const bool spatial = stage == PROSPER_PT_RESTIR_SPATIAL;
    if (spatial && !in->reservoirs)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_resample: the spatial pass needs input reservoirs");
    if (device_out_reservoirs && (reinterpret_cast<uintptr_t>(device_out_reservoirs) & 7u))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_resample: output reservoirs must be 8-byte aligned");
    if (spatial && in->onDevice && device_out_reservoirs == in->reservoirs)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_resample: the spatial pass cannot write its input");
    const int crc = check_scene(ctx, "prosper_pt_restir_di_resample");
    if (crc != PROSPER_PT_OK) return crc;
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_resample: empty extent");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t pixels = (size_t)width * height;
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    GBufferPassState &st = *ctx->gbufferPasses;
    void *out = device_out_reservoirs;
    if (!out)
    {
        rc = restir_reservoir_buffers(ctx, pixels, s);
        if (rc != PROSPER_PT_OK) return rc;
        // the spatial pass writes the buffer it does not read
        out = spatial && in->onDevice && in->reservoirs == st.reservoirs[1].ptr ? st.reservoirs[0].ptr
                                                                                : st.reservoirs[spatial ? 1 : 0].ptr;
    }
    DeviceGBuffer din;
    rc = device_gbuffer(ctx, in, pixels, spatial, s, din);
    if (rc != PROSPER_PT_OK) return rc;
    const RestirCamera cam = gbuffer_camera(camera);
    if (spatial)
        launch_restir_di_spatial(ctx->scene, frameIndex, width, height, cam, din.ar, din.nm, din.depth, din.res, out, s);
    else
        launch_restir_di_initial(ctx->scene, frameIndex, width, height, cam, din.ar, din.nm, din.depth, out, s);
    PPT_HIP(hipGetLastError());
    if (!device_out_reservoirs)
    {
        st.lastReservoirs = out;
        st.lastReservoirBytes = pixels * 8u;
    }
    return mark_versions_read(ctx, s);
}

// ---- ray-traced G-buffer (the ReSTIR-DI passes' input; a stand-in for src/render/GBufferRenderer.cpp) ----

int prosper_pt_trace_gbuffer(
    prosper_pt_ctx *ctx, uint32_t drawType, uint32_t frameIndex, uint32_t flags, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_gbuffer_targets *targets, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (flags & ~(uint32_t)(PROSPER_PT_GBUFFER_JITTER | PROSPER_PT_GBUFFER_OPAQUE_ONLY))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_trace_gbuffer: unknown flags");
    if (drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_trace_gbuffer: empty extent");
    if (!ctx || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_trace_gbuffer: null argument");
    if (targets)
    {
        if (!targets->albedoRoughness || !targets->normalMetallic || !targets->nonLinearDepth)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_trace_gbuffer: null target");
        if ((reinterpret_cast<uintptr_t>(targets->albedoRoughness) | reinterpret_cast<uintptr_t>(targets->normalMetallic) |
             reinterpret_cast<uintptr_t>(targets->nonLinearDepth)) & 15u)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_trace_gbuffer: targets must be 16-byte aligned");
    }
    const int crc = check_scene(ctx, "prosper_pt_trace_gbuffer");
    if (crc != PROSPER_PT_OK) return crc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    prosper_pt_gbuffer_targets t = {};
    if (rc == PROSPER_PT_OK)
    {
        if (targets)
            t = *targets;
        else
            rc = gbuffer_owned_targets(ctx, (size_t)width * height, s, t);
    }
    if (rc == PROSPER_PT_OK)
        rc = gbuffer_trace(
            ctx, drawType, frameIndex, (flags & PROSPER_PT_GBUFFER_JITTER) != 0, camera, width, height, t, s, nullptr,
            (flags & PROSPER_PT_GBUFFER_OPAQUE_ONLY) != 0);
    if (rc != PROSPER_PT_OK) return rc;
    return mark_versions_read(ctx, s);
}

// ---- the same with a velocity target (what TemporalAntiAliasing reads) ----

// What the velocity entry, the rasteriser's resolve and prosper_pt_raster_gbuffer refuse of a descriptor, before anything
// is enqueued (and, for the last, before the culling phases replace the lists): one copy for the three
static int check_velocity_desc(
    const char *what, prosper_pt_ctx *ctx, uint32_t drawType, const prosper_CameraUniforms *camera, const prosper_pt_velocity_gbuffer_desc *desc)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    if (!camera || !desc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    const prosper_pt_gbuffer_targets &given = desc->targets;
    const int targetCount = (given.albedoRoughness ? 1 : 0) + (given.normalMetallic ? 1 : 0) + (given.nonLinearDepth ? 1 : 0);
    if (targetCount != 0 && targetCount != 3)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the three targets are given together or not at all");
    if ((reinterpret_cast<uintptr_t>(given.albedoRoughness) | reinterpret_cast<uintptr_t>(given.normalMetallic) |
         reinterpret_cast<uintptr_t>(given.nonLinearDepth)) & 15u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": targets must be 16-byte aligned");
    return check_velocity_inputs(what, ctx, desc->velocity, desc->previousTransforms, desc->previousTransformCount);
}

// The velocity entry, and the rasteriser's resolve (`raster`), which takes the same targets under the same rules
static int velocity_gbuffer(
    const char *what, bool raster, prosper_pt_ctx *ctx, uint32_t drawType, uint32_t frameIndex, uint32_t flags, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_velocity_gbuffer_desc *desc, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (flags & ~(uint32_t)PROSPER_PT_GBUFFER_OPAQUE_ONLY) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown flags");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": empty extent");
    if (const int rc = check_velocity_desc(what, ctx, drawType, camera, desc)) return rc;
    const prosper_pt_gbuffer_targets &given = desc->targets;
    const int targetCount = given.albedoRoughness ? 3 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    const size_t pixels = (size_t)width * height;
    prosper_pt_gbuffer_targets t = given;
    if (targetCount == 0) rc = gbuffer_owned_targets(ctx, pixels, s, t);
    GBufferVelocityParams v = {};
    v.velocity = static_cast<float2 *>(desc->velocity);
    if (rc == PROSPER_PT_OK && !desc->velocity) rc = velocity_owned_target(ctx, pixels, s, &v.velocity);
    if (rc == PROSPER_PT_OK && desc->previousTransforms)
        rc = upload_previous_transforms(ctx, desc->previousTransforms, desc->previousTransformCount, s, &v.previousTransforms);
    RasterResolveTables tables = {};
    if (rc == PROSPER_PT_OK && raster) rc = raster_resolve_tables(ctx, what, width, height, s, &tables);
    if (rc == PROSPER_PT_OK)
        rc = gbuffer_trace(ctx, drawType, frameIndex, false, camera, width, height, t, s, &v, (flags & PROSPER_PT_GBUFFER_OPAQUE_ONLY) != 0,
                           raster ? &tables : nullptr);
    if (rc == PROSPER_PT_OK && raster) rc = raster_resolve_enqueued(ctx, s);
    if (rc != PROSPER_PT_OK) return rc;
    return mark_versions_read(ctx, s);
}

int prosper_pt_trace_gbuffer_velocity(
    prosper_pt_ctx *ctx, uint32_t drawType, uint32_t frameIndex, uint32_t flags, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_velocity_gbuffer_desc *desc, void *stream)
{
    return velocity_gbuffer("prosper_pt_trace_gbuffer_velocity", false, ctx, drawType, frameIndex, flags, camera, width, height, desc, stream);
}

// ---- the rasteriser's resolve (GBufferRenderer::record's attribute outputs) ----

int prosper_pt_raster_resolve(
    prosper_pt_ctx *ctx, uint32_t drawType, const prosper_CameraUniforms *camera, const prosper_pt_velocity_gbuffer_desc *desc, void *stream)
{
    if (!camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_raster_resolve: null argument");
    return velocity_gbuffer("prosper_pt_raster_resolve", true, ctx, drawType, 0u, 0u, camera, camera->resolution[0], camera->resolution[1], desc, stream);
}

int prosper_pt_raster_gbuffer(
    prosper_pt_ctx *ctx, uint32_t drawType, const prosper_CameraUniforms *camera, const prosper_pt_velocity_gbuffer_desc *desc, void *stream)
{
    const char *what = "prosper_pt_raster_gbuffer";
    // what the resolve would refuse of its arguments is refused before the culling phases replace the lists
    if (const int rc = check_velocity_desc(what, ctx, drawType, camera, desc)) return rc;
    const int rc = prosper_pt_raster_visibility(ctx, camera, stream);
    if (rc != PROSPER_PT_OK) return rc;
    return velocity_gbuffer(what, true, ctx, drawType, 0u, 0u, camera, camera->resolution[0], camera->resolution[1], desc, stream);
}

int prosper_pt_get_velocity_device_ptr(prosper_pt_ctx *ctx, void **out, uint32_t *width, uint32_t *height)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_velocity_device_ptr: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.last.velocity) return fail(PROSPER_PT_ERR_NO_SCENE, "no velocity target has been traced yet");
    *out = st.last.velocity;
    if (width) *width = st.last.velocityWidth;
    if (height) *height = st.last.velocityHeight;
    return PROSPER_PT_OK;
}

int prosper_pt_read_velocity(prosper_pt_ctx *ctx, float *host_float2, size_t pixels, void *stream)
{
    if (!ctx || !host_float2) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_velocity: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.last.velocity) return fail(PROSPER_PT_ERR_NO_SCENE, "no velocity target has been traced yet");
    if (pixels != (size_t)st.last.velocityWidth * st.last.velocityHeight)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_velocity: pixel count differs from the velocity target's");
    return read_back(ctx, static_cast<hipStream_t>(stream), {{host_float2, st.last.velocity, pixels * 8u}});
}

int prosper_pt_get_gbuffer_device_ptrs(prosper_pt_ctx *ctx, prosper_pt_restir_inputs *out, uint32_t *width, uint32_t *height)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_gbuffer_device_ptrs: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.last.targets.albedoRoughness) return fail(PROSPER_PT_ERR_NO_SCENE, "no G-buffer has been traced yet");
    *out = prosper_pt_restir_inputs{};
    out->albedoRoughness = st.last.targets.albedoRoughness;
    out->normalMetallic = st.last.targets.normalMetallic;
    out->nonLinearDepth = st.last.targets.nonLinearDepth;
    out->onDevice = 1;
    if (width) *width = st.last.width;
    if (height) *height = st.last.height;
    return PROSPER_PT_OK;
}

int prosper_pt_read_gbuffer(
    prosper_pt_ctx *ctx, float *host_albedo_roughness, float *host_normal_metallic, float *host_depth, size_t pixels,
    void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_gbuffer: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.last.targets.albedoRoughness) return fail(PROSPER_PT_ERR_NO_SCENE, "no G-buffer has been traced yet");
    if (pixels != (size_t)st.last.width * st.last.height)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_gbuffer: pixel count differs from the G-buffer's");
    const prosper_pt_gbuffer_targets &t = st.last.targets;
    return read_back(
        ctx, static_cast<hipStream_t>(stream),
        {{host_albedo_roughness, t.albedoRoughness, pixels * 16u}, {host_normal_metallic, t.normalMetallic, pixels * 16u}, {host_depth, t.nonLinearDepth, pixels * 4u}});
}

int prosper_pt_restir_di_record(
    prosper_pt_ctx *ctx, const prosper_pt_restir_trace_pc *pc, uint32_t recordFlags, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_restir_inputs *gbuffer, void *stream)
{
    if ((recordFlags & PROSPER_PT_RESTIR_JITTER_GBUFFER) && !(recordFlags & PROSPER_PT_RESTIR_TRACE_GBUFFER))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_record: JITTER_GBUFFER without TRACE_GBUFFER");
    const bool traced = (recordFlags & PROSPER_PT_RESTIR_TRACE_GBUFFER) != 0;
    if (!ctx || !pc || !camera ||
        (!traced && (!gbuffer || !gbuffer->albedoRoughness || !gbuffer->normalMetallic || !gbuffer->nonLinearDepth)))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_record: null argument");
    if (recordFlags & ~(uint32_t)(PROSPER_PT_RESTIR_SPATIAL_REUSE | PROSPER_PT_RESTIR_TRACE_GBUFFER | PROSPER_PT_RESTIR_JITTER_GBUFFER))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_record: unknown record flags");
    const int crc = check_scene(ctx, "prosper_pt_restir_di_record");
    if (crc != PROSPER_PT_OK) return crc;
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_restir_di_record: empty extent");
    if (pc->drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t pixels = (size_t)width * height;
    int rc = flush_scene_updates(ctx, s, s);
    if (rc == PROSPER_PT_OK) rc = restir_reservoir_buffers(ctx, pixels, s);
    DeviceGBuffer din;
    if (rc == PROSPER_PT_OK)
        rc = call_gbuffer(
            ctx, traced, pc->drawType, pc->frameIndex, (recordFlags & PROSPER_PT_RESTIR_JITTER_GBUFFER) != 0, camera, width,
            height, gbuffer, s, din);
    if (rc != PROSPER_PT_OK) return rc;
    GBufferPassState &st = *ctx->gbufferPasses;
    const RestirCamera cam = gbuffer_camera(camera);
    // InitialReservoirs, then SpatialReuse when the toggle is on, then Trace (RtDirectIllumination.cpp:80-109)
    launch_restir_di_initial(
        ctx->scene, pc->frameIndex, width, height, cam, din.ar, din.nm, din.depth, st.reservoirs[0].ptr, s);
    din.res = st.reservoirs[0].ptr;
    if (recordFlags & PROSPER_PT_RESTIR_SPATIAL_REUSE)
    {
        launch_restir_di_spatial(
            ctx->scene, pc->frameIndex, width, height, cam, din.ar, din.nm, din.depth, st.reservoirs[0].ptr,
            st.reservoirs[1].ptr, s);
        din.res = st.reservoirs[1].ptr;
    }
    PPT_HIP(hipGetLastError());
    st.lastReservoirs = din.res;
    st.lastReservoirBytes = pixels * 8u;
    rc = restir_trace(ctx, pc, camera, width, height, din, s);
    if (rc != PROSPER_PT_OK) return rc;
    return mark_versions_read(ctx, s);
}

int prosper_pt_get_restir_reservoirs_device_ptr(prosper_pt_ctx *ctx, void **out_ptr, size_t *out_bytes)
{
    if (!ctx || !out_ptr) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_restir_reservoirs_device_ptr: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.lastReservoirs) return fail(PROSPER_PT_ERR_NO_SCENE, "no ReSTIR reservoirs have been produced yet");
    *out_ptr = const_cast<void *>(st.lastReservoirs);
    if (out_bytes) *out_bytes = st.lastReservoirBytes;
    return PROSPER_PT_OK;
}

int prosper_pt_read_restir_reservoirs(prosper_pt_ctx *ctx, float *host_float2, size_t byte_size, void *stream)
{
    if (!ctx || !host_float2) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_restir_reservoirs: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.lastReservoirs) return fail(PROSPER_PT_ERR_NO_SCENE, "no ReSTIR reservoirs have been produced yet");
    if (byte_size != st.lastReservoirBytes)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_restir_reservoirs: size differs from the reservoirs'");
    return read_back(ctx, static_cast<hipStream_t>(stream), {{host_float2, st.lastReservoirs, byte_size}});
}

// ---- clustered lighting and deferred shading (src/render/LightClustering.cpp, src/render/DeferredShading.cpp) ----

int prosper_pt_cluster_lights(
    prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cluster_lights: null argument");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cluster_lights: empty extent");
    if (!cluster_camera_ok(camera))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cluster_lights: camera needs 0 < near_ < far_ and a resolution");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cluster_lights: null argument");
    const int crc = check_scene(ctx, "prosper_pt_cluster_lights");
    if (crc != PROSPER_PT_OK) return crc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    if (rc == PROSPER_PT_OK) rc = cluster_lights(ctx, cluster_params(camera, width, height), s);
    if (rc != PROSPER_PT_OK) return rc;
    return mark_versions_read(ctx, s);
}

int prosper_pt_get_light_cluster_dims(prosper_pt_ctx *ctx, uint32_t *x, uint32_t *y, uint32_t *z)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_light_cluster_dims: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.clusterDims[0]) return fail(PROSPER_PT_ERR_NO_SCENE, "no lights have been clustered yet");
    if (x) *x = st.clusterDims[0];
    if (y) *y = st.clusterDims[1];
    if (z) *z = st.clusterDims[2];
    return PROSPER_PT_OK;
}

int prosper_pt_read_light_clusters(
    prosper_pt_ctx *ctx, uint32_t *host_pointers, uint16_t *host_indices, uint32_t *host_count, uint32_t *host_dropped,
    uint32_t *host_overflowing, size_t clusters, void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_light_clusters: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.clusterDims[0]) return fail(PROSPER_PT_ERR_NO_SCENE, "no lights have been clustered yet");
    if (clusters != (size_t)st.clusterDims[0] * st.clusterDims[1] * st.clusterDims[2])
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_light_clusters: cluster count differs from the last clustering's");
    std::vector<uint32_t> ptrs(clusters * 2u), dropped(clusters);
    const int rc = read_back(
        ctx, static_cast<hipStream_t>(stream),
        {{ptrs.data(), st.clusterPointers.ptr, clusters * 8u}, {dropped.data(), st.clusterDropped.ptr, clusters * 4u}, {host_indices, st.clusterIndices.ptr, clusters * kClusterSlot * 2u}});
    if (rc != PROSPER_PT_OK) return rc;
    if (host_pointers) std::memcpy(host_pointers, ptrs.data(), clusters * 8u);
    uint32_t count = 0, droppedSum = 0, overflowing = 0;
    for (size_t k = 0; k < clusters; ++k)
    {
        count += (ptrs[2 * k + 1] >> 16) + (ptrs[2 * k + 1] & 0xFFFFu);
        droppedSum += dropped[k];
        overflowing += dropped[k] != 0u;
    }
    if (host_count) *host_count = count;
    if (host_dropped) *host_dropped = droppedSum;
    if (host_overflowing) *host_overflowing = overflowing;
    return PROSPER_PT_OK;
}

int prosper_pt_deferred_shading(
    prosper_pt_ctx *ctx, const prosper_pt_deferred_shading_pc *pc, uint32_t flags, uint32_t frameIndex,
    const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, const prosper_pt_restir_inputs *gbuffer,
    void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (flags & ~(uint32_t)(PROSPER_PT_DEFERRED_TRACE_GBUFFER | PROSPER_PT_DEFERRED_JITTER_GBUFFER))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_deferred_shading: unknown flags");
    if ((flags & PROSPER_PT_DEFERRED_JITTER_GBUFFER) && !(flags & PROSPER_PT_DEFERRED_TRACE_GBUFFER))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_deferred_shading: JITTER_GBUFFER without TRACE_GBUFFER");
    const bool traced = (flags & PROSPER_PT_DEFERRED_TRACE_GBUFFER) != 0;
    if (!pc || !camera ||
        (!traced && (!gbuffer || !gbuffer->albedoRoughness || !gbuffer->normalMetallic || !gbuffer->nonLinearDepth)))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_deferred_shading: null argument");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_deferred_shading: empty extent");
    if (const int rc = check_lit_pass("prosper_pt_deferred_shading", ctx, pc->drawType, pc->ibl, camera)) return rc;
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_deferred_shading: null argument");
    const int crc = check_scene(ctx, "prosper_pt_deferred_shading");
    if (crc != PROSPER_PT_OK) return crc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    DeviceGBuffer din = {};
    if (rc == PROSPER_PT_OK)
        rc = call_gbuffer(
            ctx, traced, pc->drawType, frameIndex, (flags & PROSPER_PT_DEFERRED_JITTER_GBUFFER) != 0, camera, width, height,
            gbuffer, s, din);
    ClusteredLights lights = {};
    if (rc == PROSPER_PT_OK) rc = clustered_lights(ctx, camera, width, height, pc->ibl == 1u, s, &lights, nullptr); // (clusters every frame)
    if (rc == PROSPER_PT_OK) rc = prepare_hdr(ctx, width, height, nullptr, s);
    if (rc != PROSPER_PT_OK) return rc;
    launch_deferred_shading(ctx->scene, pc->drawType, width, height, gbuffer_camera(camera), lights, din.ar, din.nm, din.depth, ctx->hdr, s);
    PPT_HIP(hipGetLastError());
    return mark_versions_read(ctx, s);
}

// ---- image-based lighting (src/render/ImageBasedLighting.cpp) ----

int prosper_pt_generate_ibl(prosper_pt_ctx *ctx, void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_generate_ibl: null argument");
    const int crc = check_scene(ctx, "prosper_pt_generate_ibl");
    if (crc != PROSPER_PT_OK) return crc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    GBufferPassState &st = *ctx->gbufferPasses;
    // allocated once: the maps' sizes are fixed
    auto allocate_once = [&](DeviceBuffer &b, size_t bytes) {
        return b.ptr ? PROSPER_PT_OK : grow_buffer(b, GrowWait::None, s, bytes, bytes);
    };
    rc = allocate_once(st.iblIrradiance, kIblIrradianceTexels * 8u);
    if (rc == PROSPER_PT_OK) rc = allocate_once(st.iblRadiance, kIblRadianceTexels * 8u);
    if (rc == PROSPER_PT_OK) rc = allocate_once(st.iblLut, (size_t)kIblLutSize * kIblLutSize * 4u);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.iblTiming.create())) return rc;
    launch_ibl_generation(
        ctx->scene, st.iblIrradiance.as<uint16_t>(), st.iblRadiance.as<uint16_t>(), st.iblLut.as<uint32_t>(), st.iblTiming.events, s);
    PPT_HIP(hipGetLastError());
    st.iblGenerated = true;
    return mark_versions_read(ctx, s);
}

int prosper_pt_get_ibl_info(prosper_pt_ctx *ctx, prosper_pt_ibl_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_ibl_info: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    prosper_pt_ibl_info info = {};
    info.generated = st.iblGenerated ? 1u : 0u;
    info.irradianceSize = kIblIrradianceSize;
    info.radianceSize = kIblRadianceSize;
    info.radianceMips = kIblRadianceMips;
    info.lutSize = kIblLutSize;
    if (st.iblTiming.created())
    {
        PPT_HIP(hipSetDevice(ctx->device));
        if (const int rc = st.iblTiming.elapsed(&info.irradianceMs)) return rc; // (irradianceMs, radianceMs, lutMs)
    }
    *out = info;
    return PROSPER_PT_OK;
}

int prosper_pt_read_ibl(
    prosper_pt_ctx *ctx, uint16_t *irradiance_rgba16f, size_t irradiance_bytes, uint16_t *radiance_rgba16f,
    size_t radiance_bytes, uint16_t *lut_rg16, size_t lut_bytes, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (irradiance_rgba16f && irradiance_bytes != 6u * kIblIrradianceSize * kIblIrradianceSize * 8u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_ibl: irradiance_bytes is not 6 x 64 x 64 RGBA16F");
    size_t radianceTexels = 0;
    for (uint32_t m = 0; m < kIblRadianceMips; ++m) radianceTexels += 6u * (size_t)(kIblRadianceSize >> m) * (kIblRadianceSize >> m);
    if (radiance_rgba16f && radiance_bytes != radianceTexels * 8u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_ibl: radiance_bytes is not the 10 mips of 6 x 512 x 512 RGBA16F");
    if (lut_rg16 && lut_bytes != (size_t)kIblLutSize * kIblLutSize * 4u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_ibl: lut_bytes is not 512 x 512 R16G16");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_ibl: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.iblGenerated) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_ibl: no maps were generated for the current scene (prosper_pt_generate_ibl)");
    // (a map the caller does not want is an empty vector: zero bytes, no copy)
    std::vector<uint16_t> irr(irradiance_rgba16f ? 4u * kIblIrradianceTexels : 0u);
    std::vector<uint16_t> rad(radiance_rgba16f ? 4u * kIblRadianceTexels : 0u);
    const int rc = read_back(
        ctx, static_cast<hipStream_t>(stream),
        {{irr.data(), st.iblIrradiance.ptr, irr.size() * 2u}, {rad.data(), st.iblRadiance.ptr, rad.size() * 2u}, {lut_rg16, st.iblLut.ptr, lut_bytes}});
    if (rc != PROSPER_PT_OK) return rc;
    if (irradiance_rgba16f) strip_cube_borders(irr, kIblIrradianceSize, 1u, irradiance_rgba16f);
    if (radiance_rgba16f) strip_cube_borders(rad, kIblRadianceSize, kIblRadianceMips, radiance_rgba16f);
    return PROSPER_PT_OK;
}

int prosper_pt_set_texture_lod(prosper_pt_ctx *ctx, int enabled, float lodBias)
{
    if (!std::isfinite(lodBias)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_texture_lod: lodBias is not finite");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_texture_lod: null context");
    if (enabled && !(ctx->flags & PROSPER_PT_CREATE_TEXTURE_MIPS))
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_set_texture_lod: the context was created without PROSPER_PT_CREATE_TEXTURE_MIPS");
    ctx->gbufferPasses->lodEnabled = enabled != 0;
    ctx->gbufferPasses->lodBias = lodBias;
    return PROSPER_PT_OK;
}

int prosper_pt_set_texture_lod_debug(prosper_pt_ctx *ctx, int enabled)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_texture_lod_debug: null context");
    ctx->gbufferPasses->lodDebug = enabled != 0;
    return PROSPER_PT_OK;
}

int prosper_pt_read_texture_lod_derivatives(prosper_pt_ctx *ctx, float *out, size_t bytes, void *stream)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_lod_derivatives: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (st.last.derivativesWidth == 0)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_lod_derivatives: the last traced G-buffer wrote no derivatives (prosper_pt_set_texture_lod, prosper_pt_set_texture_lod_debug)");
    if (bytes != (size_t)st.last.derivativesWidth * st.last.derivativesHeight * sizeof(float4))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_lod_derivatives: size mismatch");
    return read_back(ctx, static_cast<hipStream_t>(stream), {{out, st.lodDerivatives.ptr, bytes}});
}

} // extern "C"
