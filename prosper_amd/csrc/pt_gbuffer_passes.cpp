// pt_gbuffer_passes.cpp — C-ABI of the passes over a G-buffer (include/prosper_pt/prosper_pt.h): ReSTIR-DI
// (prosper_pt_restir_di_*), the ray-traced G-buffer (prosper_pt_trace_gbuffer), clustered lighting and deferred shading
// (prosper_pt_cluster_lights, prosper_pt_deferred_shading), image-based lighting (prosper_pt_generate_ibl) and the forward
// passes (prosper_pt_forward_transparent, prosper_pt_raster_forward, prosper_pt_raster_forward_transparent), with the
// readbacks of what each produced.  Kernels: pt_gbuffer_kernels.hip, pt_ibl.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_context.hpp"
#include "pt_gbuffer_kernels.hpp"
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
    prosper_pt_gbuffer_targets gbufferLast = {}; // what the last prosper_pt_trace_gbuffer wrote
    uint32_t gbufferLastWidth = 0, gbufferLastHeight = 0;
    DeviceBuffer velocity;           // context-owned velocity target (prosper_pt_trace_gbuffer_velocity): 8 bytes per pixel
    DeviceBuffer previousTransforms; // the device copy of a call's previous instance transforms
    void *velocityLast = nullptr;    // what the last prosper_pt_trace_gbuffer_velocity wrote
    // prosper_pt_set_texture_lod / _debug: the traced G-buffer samples materials through the mip chains
    bool lodEnabled = false, lodDebug = false;
    float lodBias = 0.0f;
    DeviceBuffer lodDerivatives; // debug: float4 per pixel of the last traced G-buffer
    uint32_t lodDerivativesWidth = 0, lodDerivativesHeight = 0; // 0: the last traced G-buffer wrote none
    uint32_t velocityLastWidth = 0, velocityLastHeight = 0;
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
    // what the last clustering was made from: prosper_pt_forward_transparent reuses it for the same camera and lights
    ClusterParams clusterParams = {};
    uint32_t clusterLightUpdates = 0;
    bool clusterValid = false; // (cleared by prosper_pt_upload_scene)
    // prosper_pt_forward_transparent
    DeviceBuffer transparentDepth; // device copy of a call's host depth
    DeviceBuffer transparentStats; // four uint32: covered pixels, deepest pixel, total layers (64 bits)
    DeviceBuffer transparentLayers; // debug mode: width*height counts, then width*height*N layer records
    StageEvents<1> transparentTiming;
    uint32_t transparentDebugLayers = 0; // prosper_pt_set_transparent_debug_layers
    bool transparentRan = false, transparentReclustered = false;
    size_t transparentLayerPixels = 0; // of the last call in debug mode (0: it did not run in debug mode)
    uint32_t transparentLayerCount = 0;
    // prosper_pt_raster_forward / _shade
    DeviceBuffer forwardDepth;    // context-owned depth target: 4 bytes per pixel
    DeviceBuffer forwardCount;    // kForwardCountSlots counters a cache line apart: the covered pixels of the last call
    DeviceBuffer forwardSurfaces; // debug mode: one prosper_pt_transparent_layer per pixel
    Pinned<uint32_t> forwardCountHost;
    StageEvents<2> forwardTiming; // the clustering | the shade kernel
    Fence forwardDone;            // behind the last call's copy of the count
    bool forwardDebugSurfaces = false; // prosper_pt_set_forward_debug_surfaces
    bool forwardRan = false, forwardReclustered = false;
    size_t forwardSurfacePixels = 0; // of the last call in debug mode (0: it did not run in debug mode)
    // prosper_pt_raster_transparent_draw / prosper_pt_raster_forward_transparent
    DeviceBuffer rasterTransparentDepth;  // device copy of a call's host depth
    DeviceBuffer rasterTransparentStats;  // kForwardCountSlots sets a cache line apart: pixels with a list, layers shaded, longest list
    DeviceBuffer rasterTransparentLayers; // debug mode: width*height counts, then width*height*N layer records
    Pinned<uint32_t> rasterTransparentStatsHost;
    StageEvents<4> rasterTransparentTiming; // count | scan | fill | resolve (its clustering included)
    Fence rasterTransparentDone;            // behind the last call's copy of the stats
    uint32_t rasterTransparentDebugLayers = 0; // prosper_pt_set_raster_transparent_debug_layers
    uint32_t rasterTransparentFragments = 0;
    bool rasterTransparentRan = false, rasterTransparentReclustered = false;
    size_t rasterTransparentLayerPixels = 0; // of the last call in debug mode (0: it did not run in debug mode)
    uint32_t rasterTransparentLayerCount = 0;
};

void gbuffer_texture_lod(const prosper_pt_ctx *ctx, bool *enabled, float *bias)
{
    *enabled = ctx->gbufferPasses->lodEnabled;
    *bias = ctx->gbufferPasses->lodBias;
}

int gbuffer_last_depth(prosper_pt_ctx *ctx, const float **depth, uint32_t *width, uint32_t *height)
{
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.gbufferLast.nonLinearDepth) return fail(PROSPER_PT_ERR_NO_SCENE, "no G-buffer has been traced yet");
    *depth = st.gbufferLast.nonLinearDepth;
    *width = st.gbufferLastWidth;
    *height = st.gbufferLastHeight;
    return PROSPER_PT_OK;
}

bool create_gbuffer_passes(prosper_pt_ctx *ctx)
{
    ctx->gbufferPasses = new (std::nothrow) GBufferPassState();
    return ctx->gbufferPasses != nullptr;
}

void destroy_gbuffer_passes(prosper_pt_ctx *ctx)
{
    delete ctx->gbufferPasses;
    ctx->gbufferPasses = nullptr;
}

void list_gbuffer_debug_images(const prosper_pt_ctx *ctx, std::vector<DebugImage> &out)
{
    const GBufferPassState &st = *ctx->gbufferPasses;
    // only targets the context owns: a caller's buffers may be gone by the time someone looks
    const auto owned = [](const DeviceBuffer &b, const void *p) {
        return p && b.ptr && (const uint8_t *)p >= b.as<uint8_t>() && (const uint8_t *)p < b.as<uint8_t>() + b.bytes;
    };
    const bool g = owned(st.gbuffer, st.gbufferLast.albedoRoughness) && owned(st.gbuffer, st.gbufferLast.normalMetallic) &&
                   owned(st.gbuffer, st.gbufferLast.nonLinearDepth);
    // a forward frame leaves a depth and no attribute targets (prosper_pt_raster_forward)
    const bool forwardDepth = !st.gbufferLast.albedoRoughness && owned(st.forwardDepth, st.gbufferLast.nonLinearDepth);
    const struct
    {
        const char *name;
        uint32_t format;
        const void *ptr;
        bool valid;
    } targets[3] = {{"albedoRoughness", PROSPER_PT_DEBUG_FORMAT_RGBA32F, st.gbufferLast.albedoRoughness, g},
                    {"normalMetalness", PROSPER_PT_DEBUG_FORMAT_RGBA32F, st.gbufferLast.normalMetallic, g},
                    {"depth", PROSPER_PT_DEBUG_FORMAT_R32F, st.gbufferLast.nonLinearDepth, g || forwardDepth}};
    for (const auto &t : targets)
    {
        DebugImage im;
        im.name = t.name;
        im.format = t.format;
        im.valid = t.valid;
        if (t.valid) im.one_level(t.ptr, st.gbufferLastWidth, st.gbufferLastHeight);
        out.push_back(im);
    }
    DebugImage v;
    v.name = "velocity";
    v.format = PROSPER_PT_DEBUG_FORMAT_RG32F;
    v.valid = owned(st.velocity, st.velocityLast);
    if (v.valid) v.one_level(st.velocityLast, st.velocityLastWidth, st.velocityLastHeight);
    out.push_back(v);
    DebugImage lut;
    lut.name = "SpecularBrdfLut";
    lut.format = PROSPER_PT_DEBUG_FORMAT_RG16_UNORM;
    lut.valid = st.iblGenerated && st.iblLut.ptr;
    if (lut.valid) lut.one_level(st.iblLut.ptr, kIblLutSize, kIblLutSize);
    out.push_back(lut);
}

void forget_ibl_maps(prosper_pt_ctx *ctx)
{
    ctx->gbufferPasses->iblGenerated = false;
    ctx->gbufferPasses->clusterValid = false; // the clustering describes the old scene's lights too
}

} // namespace ppt

namespace
{

// The camera terms a pass needs to rebuild a G-buffer texel's surface (RestirCamera)
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
    const size_t need = pixels * 36u + 64u;
    if (st.gbuffer.bytes < need || !st.gbuffer.ptr)
    {
        if (st.gbufferLast.albedoRoughness == st.gbuffer.ptr)
        {
            st.gbufferLast = prosper_pt_gbuffer_targets{};
            st.gbufferLastWidth = st.gbufferLastHeight = 0;
        }
        const int rc = grow_buffer(st.gbuffer, GrowWait::Stream, s, need, need);
        if (rc != PROSPER_PT_OK) return rc;
    }
    uint8_t *base = st.gbuffer.as<uint8_t>();
    out.albedoRoughness = base;
    out.normalMetallic = base + pixels * 16u;
    out.nonLinearDepth = reinterpret_cast<float *>(base + pixels * 32u);
    return PROSPER_PT_OK;
}

// The camera ray, the depth's worldToClip and the switches of a G-buffer trace (the transparent pass follows the same ray)
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

// the matrices and jitters a velocity target is computed from
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

// the context-owned velocity target, 8 bytes per pixel, grown like hostInputs
int velocity_owned_target(prosper_pt_ctx *ctx, size_t pixels, hipStream_t s, float2 **out)
{
    GBufferPassState &st = *ctx->gbufferPasses;
    if (st.velocity.bytes < pixels * 8u && st.velocityLast == st.velocity.ptr)
    {
        st.velocityLast = nullptr;
        st.velocityLastWidth = st.velocityLastHeight = 0;
    }
    const int rc = grow_to(st.velocity, pixels * 8u, s);
    *out = st.velocity.as<float2>();
    return rc;
}

// the device copy of a call's previous instance transforms, enqueued on `s`
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
    GBufferPassState &lst = *ctx->gbufferPasses;
    GBufferLodParams lodParams{ctx->textureMips, lst.lodBias, nullptr};
    const GBufferLodParams *lod = lst.lodEnabled && ctx->textureMips ? &lodParams : nullptr;
    lst.lodDerivativesWidth = lst.lodDerivativesHeight = 0;
    if (lod && lst.lodDebug)
    {
        const int grc = grow_to(lst.lodDerivatives, (size_t)width * height * sizeof(float4), s);
        if (grc != PROSPER_PT_OK) return grc;
        lodParams.derivatives = lst.lodDerivatives.as<float4>();
        lst.lodDerivativesWidth = width;
        lst.lodDerivativesHeight = height;
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
    GBufferPassState &st = *ctx->gbufferPasses;
    st.gbufferLast = t;
    st.gbufferLastWidth = width;
    st.gbufferLastHeight = height;
    if (velocity)
    {
        st.velocityLast = velocity->velocity;
        st.velocityLastWidth = width;
        st.velocityLastHeight = height;
    }
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

// The forward passes' clustering: the lists of the last clustering serve when they were made from the same camera terms,
// extent and lights (*reused); otherwise the lights are clustered on `s`
int cluster_lights_unless_current(prosper_pt_ctx *ctx, const ClusterParams &c, hipStream_t s, bool *reused)
{
    const GBufferPassState &st = *ctx->gbufferPasses;
    const uint32_t lightUpdates = ctx->lights ? ctx->lights->updates : 0u;
    *reused = st.clusterValid && std::memcmp(&st.clusterParams, &c, sizeof(c)) == 0 && st.clusterLightUpdates == lightUpdates;
    return *reused ? PROSPER_PT_OK : cluster_lights(ctx, c, s);
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
    if (reinterpret_cast<uintptr_t>(desc->velocity) & 7u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the velocity target must be 8-byte aligned");
    if (!desc->previousTransforms && desc->previousTransformCount != 0u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": previousTransformCount without previousTransforms");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    const int crc = check_scene(ctx, what);
    if (crc != PROSPER_PT_OK) return crc;
    if (desc->previousTransforms && desc->previousTransformCount != ctx->scene.modelInstanceCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": previousTransformCount differs from the scene's modelInstanceCount");
    return PROSPER_PT_OK;
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

// ---- forward opaque pass (src/render/ForwardRenderer.cpp recordOpaque) ----

constexpr size_t kForwardCountBytes = (size_t)kForwardCountSlots * kForwardCountStride * sizeof(uint32_t);

// What both forward entries refuse of their arguments, before anything is enqueued (and, for prosper_pt_raster_forward,
// before the culling phases replace the lists)
static int check_forward_opaque(
    const char *what, prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const prosper_pt_forward_opaque_desc *desc)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!pc || !camera || !desc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (pc->drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    if (pc->ibl > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": ibl is 0 or 1");
    if (pc->ibl == 1u && (!ctx || !ctx->gbufferPasses->iblGenerated))
        return fail(PROSPER_PT_ERR_UNSUPPORTED,
                    std::string(what) + ": ibl = 1 needs ImageBasedLighting's maps and BRDF LUT: call prosper_pt_generate_ibl after the scene upload");
    if (!cluster_camera_ok(camera))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": camera needs 0 < near_ < far_ and a resolution");
    if (reinterpret_cast<uintptr_t>(desc->nonLinearDepth) & 3u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the depth target must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(desc->velocity) & 7u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the velocity target must be 8-byte aligned");
    if (!desc->previousTransforms && desc->previousTransformCount != 0u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": previousTransformCount without previousTransforms");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    const int crc = check_scene(ctx, what);
    if (crc != PROSPER_PT_OK) return crc;
    if (desc->previousTransforms && desc->previousTransformCount != ctx->scene.modelInstanceCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": previousTransformCount differs from the scene's modelInstanceCount");
    return PROSPER_PT_OK;
}

// The shade over the visibility image as it stands: what the resolve refuses is refused before the HDR image, the depth or
// the velocity are touched; then the targets, the clustering (unless the last one serves) and the kernel, all on `s`.
static int forward_shade(
    const char *what, prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const prosper_pt_forward_opaque_desc *desc,
    void *stream)
{
    if (const int rc = check_forward_opaque(what, ctx, pc, camera, desc)) return rc;
    const uint32_t width = camera->resolution[0], height = camera->resolution[1];
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    RasterResolveTables tables = {};
    if ((rc = raster_resolve_tables(ctx, what, width, height, s, &tables)) != PROSPER_PT_OK) return rc;
    GBufferPassState &st = *ctx->gbufferPasses;
    const size_t pixels = (size_t)width * height;
    float *depth = desc->nonLinearDepth;
    if (!depth)
    {
        if (st.forwardDepth.bytes < pixels * 4u && st.gbufferLast.nonLinearDepth == st.forwardDepth.ptr)
        {
            st.gbufferLast = prosper_pt_gbuffer_targets{};
            st.gbufferLastWidth = st.gbufferLastHeight = 0;
        }
        if ((rc = grow_to(st.forwardDepth, pixels * 4u, s)) != PROSPER_PT_OK) return rc;
        depth = st.forwardDepth.as<float>();
    }
    GBufferVelocityParams v = {};
    v.velocity = static_cast<float2 *>(desc->velocity);
    if (!desc->velocity && (rc = velocity_owned_target(ctx, pixels, s, &v.velocity)) != PROSPER_PT_OK) return rc;
    if (desc->previousTransforms &&
        (rc = upload_previous_transforms(ctx, desc->previousTransforms, desc->previousTransformCount, s, &v.previousTransforms)) != PROSPER_PT_OK)
        return rc;
    velocity_camera_terms(v, camera);
    if ((rc = prepare_hdr(ctx, width, height, nullptr, s)) != PROSPER_PT_OK) return rc;
    if ((rc = grow_to(st.forwardCount, kForwardCountBytes, s)) != PROSPER_PT_OK) return rc;
    if (!st.forwardCountHost.ptr && (rc = st.forwardCountHost.allocate(kForwardCountBytes)) != PROSPER_PT_OK) return rc;
    const bool debug = st.forwardDebugSurfaces;
    if (debug && (rc = grow_to(st.forwardSurfaces, pixels * sizeof(prosper_pt_transparent_layer), s)) != PROSPER_PT_OK) return rc;
    if ((rc = st.forwardTiming.create()) != PROSPER_PT_OK) return rc;
    st.forwardRan = false;
    st.forwardSurfacePixels = 0;

    PPT_HIP(hipEventRecord(st.forwardTiming.events[0], s));
    const ClusterParams c = cluster_params(camera, width, height);
    bool reuse = false;
    if ((rc = cluster_lights_unless_current(ctx, c, s, &reuse)) != PROSPER_PT_OK) return rc;
    PPT_HIP(hipMemsetAsync(st.forwardCount.ptr, 0, kForwardCountBytes, s));
    PPT_HIP(hipEventRecord(st.forwardTiming.events[1], s));

    // previousTransformValid is not read: desc->previousTransforms decides
    const GBufferTraceParams g = gbuffer_trace_params(pc->drawType, 0u, false, false, camera, width, height);
    const GBufferLodParams lodParams{ctx->textureMips, st.lodBias, nullptr};
    const bool ibl = pc->ibl == 1u;
    launch_forward_opaque(
        ctx->scene, g, tables, v, c, st.clusterPointers.ptr, st.clusterIndices.as<uint16_t>(), ibl ? st.iblIrradiance.as<uint16_t>() : nullptr,
        ibl ? st.iblRadiance.as<uint16_t>() : nullptr, ibl ? st.iblLut.as<uint32_t>() : nullptr, ctx->hdr, depth, st.forwardCount.as<uint32_t>(),
        debug ? st.forwardSurfaces.as<prosper_pt_transparent_layer>() : nullptr, s, st.lodEnabled && ctx->textureMips ? &lodParams : nullptr);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(st.forwardTiming.events[2], s));
    PPT_HIP(hipMemcpyAsync(st.forwardCountHost.ptr, st.forwardCount.ptr, kForwardCountBytes, hipMemcpyDeviceToHost, s));
    if ((rc = st.forwardDone.record(s)) != PROSPER_PT_OK) return rc;
    if ((rc = raster_resolve_enqueued(ctx, s)) != PROSPER_PT_OK) return rc;
    st.forwardRan = true;
    st.forwardReclustered = !reuse;
    st.forwardSurfacePixels = debug ? pixels : 0u;
    // a forward frame has a depth and a velocity, and no attribute targets
    st.gbufferLast = prosper_pt_gbuffer_targets{};
    st.gbufferLast.nonLinearDepth = depth;
    st.gbufferLastWidth = width;
    st.gbufferLastHeight = height;
    st.lodDerivativesWidth = st.lodDerivativesHeight = 0;
    st.velocityLast = v.velocity;
    st.velocityLastWidth = width;
    st.velocityLastHeight = height;
    return mark_versions_read(ctx, s);
}

int prosper_pt_raster_forward_shade(
    prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const prosper_pt_forward_opaque_desc *desc, void *stream)
{
    return forward_shade("prosper_pt_raster_forward_shade", ctx, pc, camera, desc, stream);
}

int prosper_pt_raster_forward(
    prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const prosper_pt_forward_opaque_desc *desc, void *stream)
{
    const char *what = "prosper_pt_raster_forward";
    // what the shade would refuse of its arguments is refused before the culling phases replace the lists
    if (const int rc = check_forward_opaque(what, ctx, pc, camera, desc)) return rc;
    const int rc = prosper_pt_raster_visibility(ctx, camera, stream);
    if (rc != PROSPER_PT_OK) return rc;
    return forward_shade(what, ctx, pc, camera, desc, stream);
}

// ---- rasterised transparent pass (ForwardRenderer::recordTransparent over the draw lists) ----

// What both entries refuse, before anything is enqueued (and, for prosper_pt_raster_forward_transparent, before the culling
// phase replaces the lists): the draw's refusals, prosper_pt_forward_transparent's for pc, ibl, the camera and the depth
// argument, and an HDR image or a depth of another extent than camera->resolution.  *depth: the device depth to test
// against, nullptr where a host depth has to be copied first.
static int check_raster_transparent(
    const char *what, prosper_pt_ctx *ctx, uint32_t which, bool listNeeded, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera,
    const float *nonLinearDepth, uint32_t onDevice, const float **depth)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (which != PROSPER_PT_DRAW_LIST_GENERATED && which != PROSPER_PT_DRAW_LIST_FIRST_PHASE && which != PROSPER_PT_DRAW_LIST_SECOND_PHASE)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the list is GENERATED, FIRST_PHASE or SECOND_PHASE");
    if (!pc || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (pc->drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    if (pc->ibl > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": ibl is 0 or 1");
    if (pc->ibl == 1u && (!ctx || !ctx->gbufferPasses->iblGenerated))
        return fail(PROSPER_PT_ERR_UNSUPPORTED,
                    std::string(what) + ": ibl = 1 needs ImageBasedLighting's maps and BRDF LUT: call prosper_pt_generate_ibl after the scene upload");
    if (!cluster_camera_ok(camera))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": camera needs 0 < near_ < far_ and a resolution");
    if (reinterpret_cast<uintptr_t>(nonLinearDepth) & 3u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the depth must be 4-byte aligned");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (const int rc = raster_layers_check(ctx, what, which, listNeeded, camera)) return rc;
    const uint32_t width = camera->resolution[0], height = camera->resolution[1];
    if (!hdr_has_extent(ctx, width, height))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the HDR image's extent is not camera->resolution");
    *depth = onDevice ? nonLinearDepth : nullptr;
    if (!nonLinearDepth)
    {
        uint32_t w = 0, h = 0;
        if (const int rc = gbuffer_last_depth(ctx, depth, &w, &h)) return rc;
        if (w != width || h != height)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the context's last depth has another extent than camera->resolution");
    }
    return PROSPER_PT_OK;
}

static int raster_transparent(
    const char *what, prosper_pt_ctx *ctx, uint32_t which, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera,
    const float *nonLinearDepth, uint32_t onDevice, void *stream)
{
    const float *depth = nullptr;
    if (const int rc = check_raster_transparent(what, ctx, which, true, pc, camera, nonLinearDepth, onDevice, &depth)) return rc;
    const uint32_t width = camera->resolution[0], height = camera->resolution[1];
    const size_t pixels = (size_t)width * height;
    GBufferPassState &st = *ctx->gbufferPasses;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PPT_HIP(hipSetDevice(ctx->device));
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.rasterTransparentDone.wait(s)) != PROSPER_PT_OK) return rc; // (a call on another stream may still copy the stats)
    if (!depth)
    {
        if ((rc = grow_to(st.rasterTransparentDepth, pixels * 4u, s)) != PROSPER_PT_OK) return rc;
        PPT_HIP(hipMemcpyAsync(st.rasterTransparentDepth.ptr, nonLinearDepth, pixels * 4u, hipMemcpyHostToDevice, s));
        depth = st.rasterTransparentDepth.as<float>();
    }
    if ((rc = grow_to(st.rasterTransparentStats, kForwardCountBytes, s)) != PROSPER_PT_OK) return rc;
    if (!st.rasterTransparentStatsHost.ptr && (rc = st.rasterTransparentStatsHost.allocate(kForwardCountBytes)) != PROSPER_PT_OK) return rc;
    const uint32_t debugLayers = st.rasterTransparentDebugLayers;
    if (debugLayers &&
        (rc = grow_to(st.rasterTransparentLayers, pixels * (4u + (size_t)debugLayers * sizeof(prosper_pt_transparent_layer)), s)) != PROSPER_PT_OK)
        return rc;
    if ((rc = st.rasterTransparentTiming.create()) != PROSPER_PT_OK) return rc;
    st.rasterTransparentRan = false;
    st.rasterTransparentLayerPixels = 0;

    RasterLayerLists lists = {};
    RasterResolveTables tables = {};
    if ((rc = raster_layers_build(ctx, what, which, camera, depth, s, st.rasterTransparentTiming.events, &lists, &tables)) != PROSPER_PT_OK) return rc;
    bool reuse = true;
    PPT_HIP(hipMemsetAsync(st.rasterTransparentStats.ptr, 0, kForwardCountBytes, s));
    uint32_t *counts = debugLayers ? st.rasterTransparentLayers.as<uint32_t>() : nullptr;
    if (lists.total != 0u)
    {
        const ClusterParams c = cluster_params(camera, width, height);
        if ((rc = cluster_lights_unless_current(ctx, c, s, &reuse)) != PROSPER_PT_OK) return rc;
        GBufferVelocityParams v = {};
        velocity_camera_terms(v, camera);
        const GBufferTraceParams g = gbuffer_trace_params(pc->drawType, 0u, false, false, camera, width, height);
        const GBufferLodParams lodParams{ctx->textureMips, st.lodBias, nullptr};
        const bool ibl = pc->ibl == 1u;
        launch_raster_transparent(
            ctx->scene, g, tables, lists, v, c, st.clusterPointers.ptr, st.clusterIndices.as<uint16_t>(), ibl ? st.iblIrradiance.as<uint16_t>() : nullptr,
            ibl ? st.iblRadiance.as<uint16_t>() : nullptr, ibl ? st.iblLut.as<uint32_t>() : nullptr, ctx->hdr, st.rasterTransparentStats.as<uint32_t>(),
            debugLayers, counts, debugLayers ? reinterpret_cast<prosper_pt_transparent_layer *>(counts + pixels) : nullptr, s,
            st.lodEnabled && ctx->textureMips ? &lodParams : nullptr);
        PPT_HIP(hipGetLastError());
    }
    else if (debugLayers)
        PPT_HIP(hipMemsetAsync(counts, 0, pixels * 4u, s)); // (no list anywhere: every pixel has 0 layers)
    PPT_HIP(hipEventRecord(st.rasterTransparentTiming.events[4], s));
    PPT_HIP(hipMemcpyAsync(st.rasterTransparentStatsHost.ptr, st.rasterTransparentStats.ptr, kForwardCountBytes, hipMemcpyDeviceToHost, s));
    if ((rc = st.rasterTransparentDone.record(s)) != PROSPER_PT_OK) return rc;
    if ((rc = raster_resolve_enqueued(ctx, s)) != PROSPER_PT_OK) return rc;
    st.rasterTransparentRan = true;
    st.rasterTransparentReclustered = !reuse;
    st.rasterTransparentFragments = lists.total;
    st.rasterTransparentLayerPixels = debugLayers ? pixels : 0u;
    st.rasterTransparentLayerCount = debugLayers;
    return mark_versions_read(ctx, s);
}

int prosper_pt_raster_transparent_draw(
    prosper_pt_ctx *ctx, uint32_t which, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const float *nonLinearDepth,
    uint32_t onDevice, void *stream)
{
    return raster_transparent("prosper_pt_raster_transparent_draw", ctx, which, pc, camera, nonLinearDepth, onDevice, stream);
}

int prosper_pt_raster_forward_transparent(
    prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const float *nonLinearDepth, uint32_t onDevice,
    void *stream)
{
    const char *what = "prosper_pt_raster_forward_transparent";
    // what the draw would refuse of its arguments is refused before the culling phase replaces the lists
    const float *depth = nullptr;
    if (const int rc = check_raster_transparent(what, ctx, PROSPER_PT_DRAW_LIST_FIRST_PHASE, false, pc, camera, nonLinearDepth, onDevice, &depth)) return rc;
    // ForwardRenderer.cpp:222-260: the TRANSPARENT list culled once, without a pyramid and without a second phase
    const int rc = prosper_pt_cull_meshlets_first_phase(ctx, PROSPER_PT_CULL_MODE_TRANSPARENT, camera, PROSPER_PT_NO_HIZ, stream);
    if (rc != PROSPER_PT_OK) return rc;
    return raster_transparent(what, ctx, PROSPER_PT_DRAW_LIST_FIRST_PHASE, pc, camera, nonLinearDepth, onDevice, stream);
}

int prosper_pt_get_raster_transparent_info(prosper_pt_ctx *ctx, prosper_pt_raster_transparent_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_raster_transparent_info: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.rasterTransparentRan) return fail(PROSPER_PT_ERR_NO_SCENE, "the rasterised transparent pass has not run yet");
    PPT_HIP(hipSetDevice(ctx->device));
    prosper_pt_raster_transparent_info info = {};
    info.fragments = st.rasterTransparentFragments; // (the host read it between scan and fill)
    info.reclustered = st.rasterTransparentReclustered ? 1u : 0u;
    *out = info;
    if (!st.rasterTransparentDone.passed()) return PROSPER_PT_NOT_READY;
    for (uint32_t k = 0; k < kForwardCountSlots; ++k)
    {
        const uint32_t *slot = st.rasterTransparentStatsHost.ptr + k * kForwardCountStride;
        info.coveredPixels += slot[0];
        info.shadedLayers += slot[1];
        info.maxLayers = slot[2] > info.maxLayers ? slot[2] : info.maxLayers;
    }
    float ms[4] = {};
    if (const int rc = st.rasterTransparentTiming.elapsed(ms)) return rc; // (behind the fence that has passed: no wait)
    info.countMs = ms[0];
    info.scanMs = ms[1];
    info.fillMs = ms[2];
    info.resolveMs = ms[3];
    *out = info;
    return PROSPER_PT_OK;
}

int prosper_pt_set_raster_transparent_debug_layers(prosper_pt_ctx *ctx, uint32_t layersPerPixel)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_raster_transparent_debug_layers: null argument");
    if (layersPerPixel > 128u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_raster_transparent_debug_layers: at most 128 layers per pixel");
    ctx->gbufferPasses->rasterTransparentDebugLayers = layersPerPixel;
    return PROSPER_PT_OK;
}

int prosper_pt_read_raster_transparent_layers(
    prosper_pt_ctx *ctx, uint32_t *host_counts, prosper_pt_transparent_layer *host_layers, size_t pixels, uint32_t layersPerPixel, void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_raster_transparent_layers: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.rasterTransparentRan || !st.rasterTransparentLayerPixels)
        return fail(PROSPER_PT_ERR_NO_SCENE, "the last rasterised transparent pass did not run in debug mode (prosper_pt_set_raster_transparent_debug_layers)");
    if (pixels != st.rasterTransparentLayerPixels || layersPerPixel != st.rasterTransparentLayerCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_raster_transparent_layers: pixels or layersPerPixel differ from the call's");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = st.rasterTransparentDone.wait(s)) return rc;
    const uint32_t *counts = st.rasterTransparentLayers.as<uint32_t>();
    if (host_counts) PPT_HIP(hipMemcpyAsync(host_counts, counts, pixels * 4u, hipMemcpyDeviceToHost, s));
    if (host_layers)
        PPT_HIP(hipMemcpyAsync(host_layers, counts + pixels, pixels * layersPerPixel * sizeof(prosper_pt_transparent_layer), hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

int prosper_pt_set_forward_debug_surfaces(prosper_pt_ctx *ctx, int enabled)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_forward_debug_surfaces: null argument");
    ctx->gbufferPasses->forwardDebugSurfaces = enabled != 0;
    return PROSPER_PT_OK;
}

int prosper_pt_read_forward_surfaces(prosper_pt_ctx *ctx, prosper_pt_transparent_layer *out, size_t pixels, void *stream)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_forward_surfaces: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.forwardRan || !st.forwardSurfacePixels)
        return fail(PROSPER_PT_ERR_NO_SCENE, "the last forward opaque pass did not run in debug mode (prosper_pt_set_forward_debug_surfaces)");
    if (pixels != st.forwardSurfacePixels)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_forward_surfaces: pixel count differs from the call's");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = st.forwardDone.wait(s)) return rc;
    PPT_HIP(hipMemcpyAsync(out, st.forwardSurfaces.ptr, pixels * sizeof(prosper_pt_transparent_layer), hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

int prosper_pt_get_forward_opaque_info(prosper_pt_ctx *ctx, prosper_pt_forward_opaque_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_forward_opaque_info: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.forwardRan) return fail(PROSPER_PT_ERR_NO_SCENE, "the forward opaque pass has not run yet");
    PPT_HIP(hipSetDevice(ctx->device));
    prosper_pt_forward_opaque_info info = {};
    info.reclustered = st.forwardReclustered ? 1u : 0u;
    *out = info;
    if (!st.forwardDone.passed()) return PROSPER_PT_NOT_READY;
    float ms[2] = {};
    if (const int rc = st.forwardTiming.elapsed(ms)) return rc; // (behind the fence that has passed: no wait)
    for (uint32_t k = 0; k < kForwardCountSlots; ++k) info.shadedPixels += st.forwardCountHost.ptr[k * kForwardCountStride];
    info.ms = ms[0] + ms[1];
    info.shadeMs = ms[1];
    *out = info;
    return PROSPER_PT_OK;
}

int prosper_pt_get_forward_depth_device_ptr(prosper_pt_ctx *ctx, float **out, uint32_t *width, uint32_t *height)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_forward_depth_device_ptr: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.forwardRan || st.gbufferLast.albedoRoughness || !st.gbufferLast.nonLinearDepth)
        return fail(PROSPER_PT_ERR_NO_SCENE, "the context's last depth is not a forward frame's");
    *out = st.gbufferLast.nonLinearDepth;
    if (width) *width = st.gbufferLastWidth;
    if (height) *height = st.gbufferLastHeight;
    return PROSPER_PT_OK;
}

int prosper_pt_read_forward_depth(prosper_pt_ctx *ctx, float *host_depth, size_t pixels, void *stream)
{
    if (!ctx || !host_depth) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_forward_depth: null argument");
    float *depth = nullptr;
    uint32_t w = 0, h = 0;
    if (const int rc = prosper_pt_get_forward_depth_device_ptr(ctx, &depth, &w, &h)) return rc;
    if (pixels != (size_t)w * h) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_forward_depth: pixel count differs from the depth's");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = ctx->gbufferPasses->forwardDone.wait(s)) return rc;
    PPT_HIP(hipMemcpyAsync(host_depth, depth, pixels * 4u, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

int prosper_pt_get_velocity_device_ptr(prosper_pt_ctx *ctx, void **out, uint32_t *width, uint32_t *height)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_velocity_device_ptr: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.velocityLast) return fail(PROSPER_PT_ERR_NO_SCENE, "no velocity target has been traced yet");
    *out = st.velocityLast;
    if (width) *width = st.velocityLastWidth;
    if (height) *height = st.velocityLastHeight;
    return PROSPER_PT_OK;
}

int prosper_pt_read_velocity(prosper_pt_ctx *ctx, float *host_float2, size_t pixels, void *stream)
{
    if (!ctx || !host_float2) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_velocity: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.velocityLast) return fail(PROSPER_PT_ERR_NO_SCENE, "no velocity target has been traced yet");
    if (pixels != (size_t)st.velocityLastWidth * st.velocityLastHeight)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_velocity: pixel count differs from the velocity target's");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PPT_HIP(hipMemcpyAsync(host_float2, st.velocityLast, pixels * 8u, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

int prosper_pt_get_gbuffer_device_ptrs(prosper_pt_ctx *ctx, prosper_pt_restir_inputs *out, uint32_t *width, uint32_t *height)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_gbuffer_device_ptrs: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.gbufferLast.albedoRoughness) return fail(PROSPER_PT_ERR_NO_SCENE, "no G-buffer has been traced yet");
    *out = prosper_pt_restir_inputs{};
    out->albedoRoughness = st.gbufferLast.albedoRoughness;
    out->normalMetallic = st.gbufferLast.normalMetallic;
    out->nonLinearDepth = st.gbufferLast.nonLinearDepth;
    out->onDevice = 1;
    if (width) *width = st.gbufferLastWidth;
    if (height) *height = st.gbufferLastHeight;
    return PROSPER_PT_OK;
}

int prosper_pt_read_gbuffer(
    prosper_pt_ctx *ctx, float *host_albedo_roughness, float *host_normal_metallic, float *host_depth, size_t pixels,
    void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_gbuffer: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.gbufferLast.albedoRoughness) return fail(PROSPER_PT_ERR_NO_SCENE, "no G-buffer has been traced yet");
    if (pixels != (size_t)st.gbufferLastWidth * st.gbufferLastHeight)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_gbuffer: pixel count differs from the G-buffer's");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const prosper_pt_gbuffer_targets &t = st.gbufferLast;
    if (host_albedo_roughness)
        PPT_HIP(hipMemcpyAsync(host_albedo_roughness, t.albedoRoughness, pixels * 16u, hipMemcpyDeviceToHost, s));
    if (host_normal_metallic)
        PPT_HIP(hipMemcpyAsync(host_normal_metallic, t.normalMetallic, pixels * 16u, hipMemcpyDeviceToHost, s));
    if (host_depth) PPT_HIP(hipMemcpyAsync(host_depth, t.nonLinearDepth, pixels * 4u, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
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
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PPT_HIP(hipMemcpyAsync(host_float2, st.lastReservoirs, byte_size, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
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
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<uint32_t> ptrs(clusters * 2u), dropped(clusters);
    PPT_HIP(hipMemcpyAsync(ptrs.data(), st.clusterPointers.ptr, clusters * 8u, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipMemcpyAsync(dropped.data(), st.clusterDropped.ptr, clusters * 4u, hipMemcpyDeviceToHost, s));
    if (host_indices)
        PPT_HIP(hipMemcpyAsync(host_indices, st.clusterIndices.ptr, clusters * kClusterSlot * 2u, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
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
    if (pc->drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    if (pc->ibl > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_deferred_shading: ibl is 0 or 1");
    if (pc->ibl == 1u && (!ctx || !ctx->gbufferPasses->iblGenerated))
        return fail(PROSPER_PT_ERR_UNSUPPORTED,
                    "prosper_pt_deferred_shading: ibl = 1 needs ImageBasedLighting's maps and BRDF LUT: call prosper_pt_generate_ibl after the scene upload");
    if (!cluster_camera_ok(camera))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_deferred_shading: camera needs 0 < near_ < far_ and a resolution");
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
    const ClusterParams c = cluster_params(camera, width, height);
    if (rc == PROSPER_PT_OK) rc = cluster_lights(ctx, c, s);
    if (rc == PROSPER_PT_OK) rc = prepare_hdr(ctx, width, height, nullptr, s);
    if (rc != PROSPER_PT_OK) return rc;
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (pc->ibl == 1u)
        launch_deferred_shading_ibl(
            ctx->scene, pc->drawType, width, height, gbuffer_camera(camera), c, din.ar, din.nm, din.depth,
            st.clusterPointers.ptr, st.clusterIndices.as<uint16_t>(), st.iblIrradiance.as<uint16_t>(),
            st.iblRadiance.as<uint16_t>(), st.iblLut.as<uint32_t>(), ctx->hdr, s);
    else
        launch_deferred_shading(
            ctx->scene, pc->drawType, width, height, gbuffer_camera(camera), c, din.ar, din.nm, din.depth,
            st.clusterPointers.ptr, st.clusterIndices.as<uint16_t>(), ctx->hdr, s);
    PPT_HIP(hipGetLastError());
    return mark_versions_read(ctx, s);
}

// ---- forward transparent pass (src/render/ForwardRenderer.cpp recordTransparent) ----

int prosper_pt_forward_transparent(
    prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, uint32_t flags, uint32_t frameIndex,
    const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, const float *nonLinearDepth, uint32_t onDevice,
    void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    const char *what = "prosper_pt_forward_transparent";
    if (flags & ~(uint32_t)(PROSPER_PT_TRANSPARENT_JITTER | PROSPER_PT_TRANSPARENT_CAMERA_JITTER))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown flags");
    if ((flags & PROSPER_PT_TRANSPARENT_JITTER) && (flags & PROSPER_PT_TRANSPARENT_CAMERA_JITTER))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": JITTER and CAMERA_JITTER exclude each other");
    if (!pc || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": empty extent");
    if (pc->drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    if (pc->ibl > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": ibl is 0 or 1");
    if (pc->ibl == 1u && (!ctx || !ctx->gbufferPasses->iblGenerated))
        return fail(PROSPER_PT_ERR_UNSUPPORTED,
                    std::string(what) + ": ibl = 1 needs ImageBasedLighting's maps and BRDF LUT: call prosper_pt_generate_ibl after the scene upload");
    if (!cluster_camera_ok(camera))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": camera needs 0 < near_ < far_ and a resolution");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    const int crc = check_scene(ctx, what);
    if (crc != PROSPER_PT_OK) return crc;
    if (!hdr_has_extent(ctx, width, height))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the HDR image has another extent");
    GBufferPassState &st = *ctx->gbufferPasses;
    const size_t pixels = (size_t)width * height;
    const float *depth = nonLinearDepth;
    if (!depth)
    {
        if (!st.gbufferLast.nonLinearDepth) return fail(PROSPER_PT_ERR_NO_SCENE, "no G-buffer has been traced yet");
        if (st.gbufferLastWidth != width || st.gbufferLastHeight != height)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the last traced G-buffer has another extent");
        depth = st.gbufferLast.nonLinearDepth;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    if (nonLinearDepth && !onDevice)
    {
        rc = grow_to(st.transparentDepth, pixels * 4u, s);
        if (rc != PROSPER_PT_OK) return rc;
        PPT_HIP(hipMemcpyAsync(st.transparentDepth.ptr, nonLinearDepth, pixels * 4u, hipMemcpyHostToDevice, s));
        depth = st.transparentDepth.as<float>();
    }
    rc = grow_to(st.transparentStats, 16u, s);
    const uint32_t debugLayers = st.transparentDebugLayers;
    if (rc == PROSPER_PT_OK && debugLayers) rc = grow_to(st.transparentLayers, pixels * (4u + (size_t)debugLayers * sizeof(prosper_pt_transparent_layer)), s);
    if (rc == PROSPER_PT_OK) rc = st.transparentTiming.create();
    if (rc != PROSPER_PT_OK) return rc;
    st.transparentRan = false;
    st.transparentLayerPixels = 0;
    PPT_HIP(hipEventRecord(st.transparentTiming.events[0], s));

    const ClusterParams c = cluster_params(camera, width, height);
    bool reuse = false;
    rc = cluster_lights_unless_current(ctx, c, s, &reuse);
    if (rc != PROSPER_PT_OK) return rc;

    TransparentParams p = {};
    p.g = gbuffer_trace_params(pc->drawType, frameIndex, (flags & PROSPER_PT_TRANSPARENT_JITTER) != 0, false, camera, width, height);
    std::memcpy(p.worldToCamera, &camera->worldToCamera, 64);
    const RestirCamera rc2 = gbuffer_camera(camera);
    p.cameraToClip22 = rc2.cameraToClip22;
    p.cameraToClip32 = rc2.cameraToClip32;
    p.cameraJitter = (flags & PROSPER_PT_TRANSPARENT_CAMERA_JITTER) ? 1u : 0u;
    p.currentJitter[0] = camera->currentJitter[0];
    p.currentJitter[1] = camera->currentJitter[1];
    p.near_ = c.near_;
    p.far_ = c.far_;
    p.clustersX = c.dimX;
    p.clustersY = c.dimY;
    p.debugLayers = debugLayers;

    int32_t *ovf = nullptr;
    rc = ensure_stack_overflow(ctx, ctx->slots[0], kTraversalStackDepth, restir_grid_blocks(width, height), &ovf);
    if (rc != PROSPER_PT_OK) return rc;
    PPT_HIP(hipMemsetAsync(st.transparentStats.ptr, 0, 16u, s));
    wait_for_slot(ctx->slots[0], s);
    const bool ibl = pc->ibl == 1u;
    uint32_t *counts = debugLayers ? st.transparentLayers.as<uint32_t>() : nullptr;
    const GBufferLodParams lodParams{ctx->textureMips, st.lodBias, nullptr};
    launch_forward_transparent(
        ctx->scene, p, depth, st.clusterPointers.ptr, st.clusterIndices.as<uint16_t>(), ibl ? st.iblIrradiance.as<uint16_t>() : nullptr,
        ibl ? st.iblRadiance.as<uint16_t>() : nullptr, ibl ? st.iblLut.as<uint32_t>() : nullptr, ctx->hdr, ovf,
        st.transparentStats.as<uint32_t>(), counts,
        debugLayers ? reinterpret_cast<prosper_pt_transparent_layer *>(counts + pixels) : nullptr, s,
        st.lodEnabled && ctx->textureMips ? &lodParams : nullptr);
    release_slot(ctx->slots[0], s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(st.transparentTiming.events[1], s));
    st.transparentRan = true;
    st.transparentReclustered = !reuse;
    st.transparentLayerPixels = debugLayers ? pixels : 0u;
    st.transparentLayerCount = debugLayers;
    return mark_versions_read(ctx, s);
}

int prosper_pt_get_transparent_info(prosper_pt_ctx *ctx, prosper_pt_transparent_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_transparent_info: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.transparentRan) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_forward_transparent has not run yet");
    PPT_HIP(hipSetDevice(ctx->device));
    prosper_pt_transparent_info info = {};
    if (const int rc = st.transparentTiming.elapsed(&info.ms)) return rc; // (waits for the call's last kernel)
    uint32_t stats[4] = {};
    PPT_HIP(hipMemcpy(stats, st.transparentStats.ptr, 16u, hipMemcpyDeviceToHost));
    info.coveredPixels = stats[0];
    info.maxLayers = stats[1];
    info.totalLayers = ((uint64_t)stats[3] << 32) | stats[2];
    info.reclustered = st.transparentReclustered ? 1u : 0u;
    *out = info;
    return PROSPER_PT_OK;
}

int prosper_pt_set_transparent_debug_layers(prosper_pt_ctx *ctx, uint32_t layersPerPixel)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_transparent_debug_layers: null argument");
    if (layersPerPixel > 64u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_transparent_debug_layers: at most 64 layers per pixel");
    ctx->gbufferPasses->transparentDebugLayers = layersPerPixel;
    return PROSPER_PT_OK;
}

int prosper_pt_read_transparent_layers(
    prosper_pt_ctx *ctx, uint32_t *host_counts, prosper_pt_transparent_layer *host_layers, size_t pixels,
    uint32_t layersPerPixel, void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_transparent_layers: null argument");
    const GBufferPassState &st = *ctx->gbufferPasses;
    if (!st.transparentRan || !st.transparentLayerPixels)
        return fail(PROSPER_PT_ERR_NO_SCENE, "the last prosper_pt_forward_transparent did not run in debug mode (prosper_pt_set_transparent_debug_layers)");
    if (pixels != st.transparentLayerPixels || layersPerPixel != st.transparentLayerCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_transparent_layers: pixels or layersPerPixel differ from the call's");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t *counts = st.transparentLayers.as<uint32_t>();
    if (host_counts) PPT_HIP(hipMemcpyAsync(host_counts, counts, pixels * 4u, hipMemcpyDeviceToHost, s));
    if (host_layers)
        PPT_HIP(hipMemcpyAsync(host_layers, counts + pixels, pixels * layersPerPixel * sizeof(prosper_pt_transparent_layer), hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
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
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<uint16_t> irr(irradiance_rgba16f ? 4u * kIblIrradianceTexels : 0u);
    std::vector<uint16_t> rad(radiance_rgba16f ? 4u * kIblRadianceTexels : 0u);
    if (irradiance_rgba16f) PPT_HIP(hipMemcpyAsync(irr.data(), st.iblIrradiance.ptr, irr.size() * 2u, hipMemcpyDeviceToHost, s));
    if (radiance_rgba16f) PPT_HIP(hipMemcpyAsync(rad.data(), st.iblRadiance.ptr, rad.size() * 2u, hipMemcpyDeviceToHost, s));
    if (lut_rg16) PPT_HIP(hipMemcpyAsync(lut_rg16, st.iblLut.ptr, lut_bytes, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
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
    if (st.lodDerivativesWidth == 0)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_lod_derivatives: the last traced G-buffer wrote no derivatives (prosper_pt_set_texture_lod, prosper_pt_set_texture_lod_debug)");
    if (bytes != (size_t)st.lodDerivativesWidth * st.lodDerivativesHeight * sizeof(float4))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_lod_derivatives: size mismatch");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PPT_HIP(hipMemcpyAsync(out, st.lodDerivatives.ptr, bytes, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

} // extern "C"
