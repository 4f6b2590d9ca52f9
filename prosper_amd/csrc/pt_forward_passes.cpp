// pt_forward_passes.cpp — C-ABI of ForwardRenderer's passes (include/prosper_pt/prosper_pt.h): the traced transparent pass
// (prosper_pt_forward_transparent), the forward opaque pass over the visibility image
// (prosper_pt_raster_forward, _shade; f19) and the rasterised transparent pass over the draw lists
// (prosper_pt_raster_transparent_draw, prosper_pt_raster_forward_transparent; f20), with the readbacks of what each produced.
// The last frame, the lighting inputs and the pieces of a G-buffer trace are the G-buffer module's (pt_gbuffer_passes.hpp).
// Kernels: pt_gbuffer_kernels.hip; the draw lists and the visibility image: pt_raster_passes.cpp.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#include "pt_context.hpp"
#include "pt_gbuffer_kernels.hpp"
#include "pt_gbuffer_passes.hpp"
#include "pt_kernels.hpp"
#include "pt_pass_support.hpp"
#include "pt_raster.hpp"

using namespace ppt;

namespace ppt
{

#pragma GCC visibility push(hidden) // (not part of the library's exports)

// The debug layers of a transparent pass: a count per pixel, then the first `layersPerPixel` layer records of each pixel.
struct LayerStore
{
    DeviceBuffer buffer;
    uint32_t requested = 0;      // layers per pixel of the calls to come (the pass's setter)
    size_t pixels = 0;           // of the call in hand or the last one (0: not in debug mode)
    uint32_t layersPerPixel = 0; // of the same call
    bool filled = false;         // the last call succeeded and left layers

    int request(const char *what, uint32_t layers, uint32_t most)
    {
        if (layers > most)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": at most " + std::to_string(most) + " layers per pixel");
        requested = layers;
        return PROSPER_PT_OK;
    }
    // a call over `callPixels` pixels begins: what the last one left is void until the pass calls written()
    int prepare(size_t callPixels, hipStream_t s)
    {
        filled = false;
        pixels = 0;
        layersPerPixel = requested;
        if (!requested) return PROSPER_PT_OK;
        if (const int rc = grow_to(buffer, callPixels * (4u + (size_t)requested * sizeof(prosper_pt_transparent_layer)), s)) return rc;
        pixels = callPixels;
        return PROSPER_PT_OK;
    }
    // what the launch writes: both nullptr outside debug mode
    uint32_t *counts() const { return pixels ? buffer.as<uint32_t>() : nullptr; }
    prosper_pt_transparent_layer *layers() const { return pixels ? reinterpret_cast<prosper_pt_transparent_layer *>(counts() + pixels) : nullptr; }
    void written() { filled = pixels != 0; }
    // `notDebug`: the refusal when the last call left no layers; `done`: what the copies wait for on `s`, if anything
    int read(
        const prosper_pt_ctx *ctx, const char *what, const char *notDebug, const Fence *done, uint32_t *host_counts,
        prosper_pt_transparent_layer *host_layers, size_t readPixels, uint32_t readLayers, hipStream_t s) const
    {
        if (!filled) return fail(PROSPER_PT_ERR_NO_SCENE, notDebug);
        if (readPixels != pixels || readLayers != layersPerPixel)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": pixels or layersPerPixel differ from the call's");
        return read_back(
            ctx, s, {{host_counts, counts(), pixels * 4u}, {host_layers, layers(), pixels * layersPerPixel * sizeof(prosper_pt_transparent_layer)}},
            done);
    }
};

// The statistics a pass's waves add up in kForwardCountSlots sets of device words a cache line apart (a single address
// serialises the waves: DESIGN.md f19), and their pinned copy, which is read once `done` has passed: no call blocks.
constexpr size_t kSlotStatsBytes = (size_t)kForwardCountSlots * kForwardCountStride * sizeof(uint32_t);
struct SlotStats
{
    DeviceBuffer slots;
    Pinned<uint32_t> host;
    Fence done; // behind the last call's copy
    // `s` waits for the last call, which may have run on another stream: its copy into the pinned words, and with it its
    // kernels and whatever else of the pass's buffers they read.  A pass calls this before it touches any of them.
    int prepare(hipStream_t s)
    {
        if (const int rc = grow_to(slots, kSlotStatsBytes, s)) return rc;
        if (!host.ptr)
            if (const int rc = host.allocate(kSlotStatsBytes)) return rc;
        return done.wait(s);
    }
    int zero(hipStream_t s) const
    {
        PPT_HIP(hipMemsetAsync(slots.ptr, 0, kSlotStatsBytes, s));
        return PROSPER_PT_OK;
    }
    int copy_back(hipStream_t s)
    {
        PPT_HIP(hipMemcpyAsync(host.ptr, slots.ptr, kSlotStatsBytes, hipMemcpyDeviceToHost, s));
        return done.record(s);
    }
    bool passed() const { return done.passed(); }
    const uint32_t *slot(uint32_t k) const { return host.ptr + k * kForwardCountStride; }
};

struct ForwardPassState
{
    struct Traced // prosper_pt_forward_transparent
    {
        DeviceBuffer depth; // device copy of a call's host depth
        DeviceBuffer stats; // four uint32: covered pixels, deepest pixel, total layers (64 bits)
        LayerStore layers;  // prosper_pt_set_transparent_debug_layers
        StageEvents<1> timing;
        bool ran = false, reclustered = false;
    } traced;
    struct Opaque // prosper_pt_raster_forward / _shade
    {
        DeviceBuffer depth;    // context-owned depth target: 4 bytes per pixel
        DeviceBuffer surfaces; // debug mode: one prosper_pt_transparent_layer per pixel
        SlotStats count;       // the covered pixels of the last call
        StageEvents<2> timing; // the clustering | the shade kernel
        bool debugSurfaces = false; // prosper_pt_set_forward_debug_surfaces
        bool ran = false, reclustered = false;
        size_t surfacePixels = 0; // of the last call in debug mode (0: it did not run in debug mode)
    } opaque;
    struct Raster // prosper_pt_raster_transparent_draw / prosper_pt_raster_forward_transparent
    {
        DeviceBuffer depth;    // device copy of a call's host depth
        SlotStats stats;       // per set: pixels with a list, layers shaded, longest list
        LayerStore layers;     // prosper_pt_set_raster_transparent_debug_layers
        StageEvents<4> timing; // count | scan | fill | resolve (its clustering included)
        uint32_t fragments = 0;
        bool ran = false, reclustered = false;
    } raster;
};

extern const PassModule kForwardPasses = pass_module<ForwardPassState, &prosper_pt_ctx::forwardPasses>();

#pragma GCC visibility pop

} // namespace ppt

extern "C" {

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
    if (const int rc = check_lit_pass(what, ctx, pc->drawType, pc->ibl, camera)) return rc;
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    const int crc = check_scene(ctx, what);
    if (crc != PROSPER_PT_OK) return crc;
    if (!hdr_has_extent(ctx, width, height))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the HDR image has another extent");
    ForwardPassState::Traced &st = ctx->forwardPasses->traced;
    const size_t pixels = (size_t)width * height;
    const float *depth = nullptr;
    if (const int rc = resolve_depth(ctx, what, nonLinearDepth, onDevice != 0u, width, height, &depth)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    st.ran = false;
    rc = stage_depth(st.depth, 0, nonLinearDepth, pixels, s, &depth);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.stats, 16u, s);
    if (rc == PROSPER_PT_OK) rc = st.layers.prepare(pixels, s);
    if (rc == PROSPER_PT_OK) rc = st.timing.create();
    if (rc != PROSPER_PT_OK) return rc;
    PPT_HIP(hipEventRecord(st.timing.events[0], s));

    ClusteredLights lights = {};
    bool reuse = false;
    if ((rc = clustered_lights(ctx, camera, width, height, pc->ibl == 1u, s, &lights, &reuse)) != PROSPER_PT_OK) return rc;

    TransparentParams p = {};
    p.g = gbuffer_trace_params(pc->drawType, frameIndex, (flags & PROSPER_PT_TRANSPARENT_JITTER) != 0, false, camera, width, height);
    std::memcpy(p.worldToCamera, &camera->worldToCamera, 64);
    const RestirCamera rc2 = gbuffer_camera(camera);
    p.cameraToClip22 = rc2.cameraToClip22;
    p.cameraToClip32 = rc2.cameraToClip32;
    p.cameraJitter = (flags & PROSPER_PT_TRANSPARENT_CAMERA_JITTER) ? 1u : 0u;
    p.currentJitter[0] = camera->currentJitter[0];
    p.currentJitter[1] = camera->currentJitter[1];
    p.near_ = lights.params.near_;
    p.far_ = lights.params.far_;
    p.clustersX = lights.params.dimX;
    p.clustersY = lights.params.dimY;
    p.debugLayers = st.layers.layersPerPixel;

    int32_t *ovf = nullptr;
    rc = ensure_stack_overflow(ctx, ctx->slots[0], kTraversalStackDepth, restir_grid_blocks(width, height), &ovf);
    if (rc != PROSPER_PT_OK) return rc;
    PPT_HIP(hipMemsetAsync(st.stats.ptr, 0, 16u, s));
    wait_for_slot(ctx->slots[0], s);
    GBufferLodParams lodParams;
    launch_forward_transparent(
        ctx->scene, p, depth, lights, ctx->hdr, ovf, st.stats.as<uint32_t>(), st.layers.counts(), st.layers.layers(), s,
        gbuffer_lod_params(ctx, lodParams));
    release_slot(ctx->slots[0], s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(st.timing.events[1], s));
    st.ran = true;
    st.reclustered = !reuse;
    st.layers.written();
    return mark_versions_read(ctx, s);
}

int prosper_pt_get_transparent_info(prosper_pt_ctx *ctx, prosper_pt_transparent_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_transparent_info: null argument");
    const ForwardPassState::Traced &st = ctx->forwardPasses->traced;
    if (!st.ran) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_forward_transparent has not run yet");
    PPT_HIP(hipSetDevice(ctx->device));
    prosper_pt_transparent_info info = {};
    if (const int rc = st.timing.elapsed(&info.ms)) return rc; // (waits for the call's last kernel)
    uint32_t stats[4] = {};
    PPT_HIP(hipMemcpy(stats, st.stats.ptr, 16u, hipMemcpyDeviceToHost));
    info.coveredPixels = stats[0];
    info.maxLayers = stats[1];
    info.totalLayers = ((uint64_t)stats[3] << 32) | stats[2];
    info.reclustered = st.reclustered ? 1u : 0u;
    *out = info;
    return PROSPER_PT_OK;
}

int prosper_pt_set_transparent_debug_layers(prosper_pt_ctx *ctx, uint32_t layersPerPixel)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_transparent_debug_layers: null argument");
    return ctx->forwardPasses->traced.layers.request("prosper_pt_set_transparent_debug_layers", layersPerPixel, 64u);
}

int prosper_pt_read_transparent_layers(
    prosper_pt_ctx *ctx, uint32_t *host_counts, prosper_pt_transparent_layer *host_layers, size_t pixels,
    uint32_t layersPerPixel, void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_transparent_layers: null argument");
    return ctx->forwardPasses->traced.layers.read(
        ctx, "prosper_pt_read_transparent_layers",
        "the last prosper_pt_forward_transparent did not run in debug mode (prosper_pt_set_transparent_debug_layers)", nullptr, host_counts,
        host_layers, pixels, layersPerPixel, static_cast<hipStream_t>(stream));
}

// ---- forward opaque pass (src/render/ForwardRenderer.cpp recordOpaque) ----

// What both forward entries refuse of their arguments, before anything is enqueued (and, for prosper_pt_raster_forward,
// before the culling phases replace the lists)
static int check_forward_opaque(
    const char *what, prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const prosper_pt_forward_opaque_desc *desc)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!pc || !camera || !desc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (const int rc = check_lit_pass(what, ctx, pc->drawType, pc->ibl, camera)) return rc;
    if (reinterpret_cast<uintptr_t>(desc->nonLinearDepth) & 3u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the depth target must be 4-byte aligned");
    return check_velocity_inputs(what, ctx, desc->velocity, desc->previousTransforms, desc->previousTransformCount);
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
    ForwardPassState::Opaque &st = ctx->forwardPasses->opaque;
    if ((rc = st.count.prepare(s)) != PROSPER_PT_OK) return rc;
    const size_t pixels = (size_t)width * height;
    float *depth = desc->nonLinearDepth;
    if (!depth)
    {
        if ((rc = gbuffer_last_frame(ctx).grow(st.depth, pixels * 4u, s)) != PROSPER_PT_OK) return rc;
        depth = st.depth.as<float>();
    }
    GBufferVelocityParams v = {};
    v.velocity = static_cast<float2 *>(desc->velocity);
    if (!desc->velocity && (rc = velocity_owned_target(ctx, pixels, s, &v.velocity)) != PROSPER_PT_OK) return rc;
    if (desc->previousTransforms &&
        (rc = upload_previous_transforms(ctx, desc->previousTransforms, desc->previousTransformCount, s, &v.previousTransforms)) != PROSPER_PT_OK)
        return rc;
    velocity_camera_terms(v, camera);
    if ((rc = prepare_hdr(ctx, width, height, nullptr, s)) != PROSPER_PT_OK) return rc;
    const bool debug = st.debugSurfaces;
    if (debug && (rc = grow_to(st.surfaces, pixels * sizeof(prosper_pt_transparent_layer), s)) != PROSPER_PT_OK) return rc;
    if ((rc = st.timing.create()) != PROSPER_PT_OK) return rc;
    st.ran = false;
    st.surfacePixels = 0;

    PPT_HIP(hipEventRecord(st.timing.events[0], s));
    ClusteredLights lights = {};
    bool reuse = false;
    if ((rc = clustered_lights(ctx, camera, width, height, pc->ibl == 1u, s, &lights, &reuse)) != PROSPER_PT_OK) return rc;
    if ((rc = st.count.zero(s)) != PROSPER_PT_OK) return rc;
    PPT_HIP(hipEventRecord(st.timing.events[1], s));

    // previousTransformValid is not read: desc->previousTransforms decides
    const GBufferTraceParams g = gbuffer_trace_params(pc->drawType, 0u, false, false, camera, width, height);
    GBufferLodParams lodParams;
    launch_forward_opaque(
        ctx->scene, g, tables, v, lights, ctx->hdr, depth, st.count.slots.as<uint32_t>(),
        debug ? st.surfaces.as<prosper_pt_transparent_layer>() : nullptr, s, gbuffer_lod_params(ctx, lodParams));
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(st.timing.events[2], s));
    if ((rc = st.count.copy_back(s)) != PROSPER_PT_OK) return rc;
    if ((rc = raster_resolve_enqueued(ctx, s)) != PROSPER_PT_OK) return rc;
    st.ran = true;
    st.reclustered = !reuse;
    st.surfacePixels = debug ? pixels : 0u;
    gbuffer_last_frame(ctx).set_forward(depth, LastFrame::lies_in(st.depth, depth), v.velocity, width, height);
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

int prosper_pt_set_forward_debug_surfaces(prosper_pt_ctx *ctx, int enabled)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_forward_debug_surfaces: null argument");
    ctx->forwardPasses->opaque.debugSurfaces = enabled != 0;
    return PROSPER_PT_OK;
}

int prosper_pt_read_forward_surfaces(prosper_pt_ctx *ctx, prosper_pt_transparent_layer *out, size_t pixels, void *stream)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_forward_surfaces: null argument");
    const ForwardPassState::Opaque &st = ctx->forwardPasses->opaque;
    if (!st.ran || !st.surfacePixels)
        return fail(PROSPER_PT_ERR_NO_SCENE, "the last forward opaque pass did not run in debug mode (prosper_pt_set_forward_debug_surfaces)");
    if (pixels != st.surfacePixels)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_forward_surfaces: pixel count differs from the call's");
    return read_back(
        ctx, static_cast<hipStream_t>(stream), {{out, st.surfaces.ptr, pixels * sizeof(prosper_pt_transparent_layer)}}, &st.count.done);
}

int prosper_pt_get_forward_opaque_info(prosper_pt_ctx *ctx, prosper_pt_forward_opaque_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_forward_opaque_info: null argument");
    const ForwardPassState::Opaque &st = ctx->forwardPasses->opaque;
    if (!st.ran) return fail(PROSPER_PT_ERR_NO_SCENE, "the forward opaque pass has not run yet");
    PPT_HIP(hipSetDevice(ctx->device));
    prosper_pt_forward_opaque_info info = {};
    info.reclustered = st.reclustered ? 1u : 0u;
    *out = info;
    if (!st.count.passed()) return PROSPER_PT_NOT_READY;
    float ms[2] = {};
    if (const int rc = st.timing.elapsed(ms)) return rc; // (behind the fence that has passed: no wait)
    for (uint32_t k = 0; k < kForwardCountSlots; ++k) info.shadedPixels += st.count.slot(k)[0];
    info.ms = ms[0] + ms[1];
    info.shadeMs = ms[1];
    *out = info;
    return PROSPER_PT_OK;
}

int prosper_pt_get_forward_depth_device_ptr(prosper_pt_ctx *ctx, float **out, uint32_t *width, uint32_t *height)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_forward_depth_device_ptr: null argument");
    const LastFrame &last = gbuffer_last_frame(ctx);
    if (!ctx->forwardPasses->opaque.ran || last.targets.albedoRoughness || !last.targets.nonLinearDepth)
        return fail(PROSPER_PT_ERR_NO_SCENE, "the context's last depth is not a forward frame's");
    *out = last.targets.nonLinearDepth;
    if (width) *width = last.width;
    if (height) *height = last.height;
    return PROSPER_PT_OK;
}

int prosper_pt_read_forward_depth(prosper_pt_ctx *ctx, float *host_depth, size_t pixels, void *stream)
{
    if (!ctx || !host_depth) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_forward_depth: null argument");
    float *depth = nullptr;
    uint32_t w = 0, h = 0;
    if (const int rc = prosper_pt_get_forward_depth_device_ptr(ctx, &depth, &w, &h)) return rc;
    if (pixels != (size_t)w * h) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_forward_depth: pixel count differs from the depth's");
    return read_back(ctx, static_cast<hipStream_t>(stream), {{host_depth, depth, pixels * 4u}}, &ctx->forwardPasses->opaque.count.done);
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
    if (const int rc = check_lit_pass(what, ctx, pc->drawType, pc->ibl, camera)) return rc;
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
    ForwardPassState::Raster &st = ctx->forwardPasses->raster;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PPT_HIP(hipSetDevice(ctx->device));
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    st.ran = false;
    rc = st.stats.prepare(s); // (first: the last call's resolve may still read the depth copy on another stream)
    if (rc == PROSPER_PT_OK) rc = stage_depth(st.depth, 0, nonLinearDepth, pixels, s, &depth);
    if (rc == PROSPER_PT_OK) rc = st.layers.prepare(pixels, s);
    if (rc == PROSPER_PT_OK) rc = st.timing.create();
    if (rc != PROSPER_PT_OK) return rc;

    RasterLayerLists lists = {};
    RasterResolveTables tables = {};
    if ((rc = raster_layers_build(ctx, what, which, camera, depth, s, st.timing.events, &lists, &tables)) != PROSPER_PT_OK) return rc;
    bool reuse = true;
    if ((rc = st.stats.zero(s)) != PROSPER_PT_OK) return rc;
    if (lists.total != 0u)
    {
        ClusteredLights lights = {};
        if ((rc = clustered_lights(ctx, camera, width, height, pc->ibl == 1u, s, &lights, &reuse)) != PROSPER_PT_OK) return rc;
        GBufferVelocityParams v = {};
        velocity_camera_terms(v, camera);
        const GBufferTraceParams g = gbuffer_trace_params(pc->drawType, 0u, false, false, camera, width, height);
        GBufferLodParams lodParams;
        launch_raster_transparent(
            ctx->scene, g, tables, lists, v, lights, ctx->hdr, st.stats.slots.as<uint32_t>(), st.layers.layersPerPixel, st.layers.counts(),
            st.layers.layers(), s, gbuffer_lod_params(ctx, lodParams));
        PPT_HIP(hipGetLastError());
    }
    else if (st.layers.pixels)
        PPT_HIP(hipMemsetAsync(st.layers.counts(), 0, pixels * 4u, s)); // (no list anywhere: every pixel has 0 layers)
    PPT_HIP(hipEventRecord(st.timing.events[4], s));
    if ((rc = st.stats.copy_back(s)) != PROSPER_PT_OK) return rc;
    if ((rc = raster_resolve_enqueued(ctx, s)) != PROSPER_PT_OK) return rc;
    st.ran = true;
    st.reclustered = !reuse;
    st.fragments = lists.total;
    st.layers.written();
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
    const ForwardPassState::Raster &st = ctx->forwardPasses->raster;
    if (!st.ran) return fail(PROSPER_PT_ERR_NO_SCENE, "the rasterised transparent pass has not run yet");
    PPT_HIP(hipSetDevice(ctx->device));
    prosper_pt_raster_transparent_info info = {};
    info.fragments = st.fragments; // (the host read it between scan and fill)
    info.reclustered = st.reclustered ? 1u : 0u;
    *out = info;
    if (!st.stats.passed()) return PROSPER_PT_NOT_READY;
    for (uint32_t k = 0; k < kForwardCountSlots; ++k)
    {
        const uint32_t *slot = st.stats.slot(k);
        info.coveredPixels += slot[0];
        info.shadedLayers += slot[1];
        info.maxLayers = slot[2] > info.maxLayers ? slot[2] : info.maxLayers;
    }
    float ms[4] = {};
    if (const int rc = st.timing.elapsed(ms)) return rc; // (behind the fence that has passed: no wait)
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
    return ctx->forwardPasses->raster.layers.request("prosper_pt_set_raster_transparent_debug_layers", layersPerPixel, 128u);
}

int prosper_pt_read_raster_transparent_layers(
    prosper_pt_ctx *ctx, uint32_t *host_counts, prosper_pt_transparent_layer *host_layers, size_t pixels, uint32_t layersPerPixel, void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_raster_transparent_layers: null argument");
    const ForwardPassState::Raster &st = ctx->forwardPasses->raster;
    return st.layers.read(
        ctx, "prosper_pt_read_raster_transparent_layers",
        "the last rasterised transparent pass did not run in debug mode (prosper_pt_set_raster_transparent_debug_layers)", &st.stats.done,
        host_counts, host_layers, pixels, layersPerPixel, static_cast<hipStream_t>(stream));
}

} // extern "C"
