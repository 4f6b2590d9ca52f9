// pt_debug_passes.cpp — C-ABI of prosper's inspection passes (include/prosper_pt/prosper_pt.h): prosper_pt_debug_lines
// over the context's HDR image and the last traced G-buffer's depth, the registry of the context's 2-D images (every pass
// module lists its own: PassModule::list_debug_images), the one-texel readback and the texture viewer over an entry.  Kernels:
// pt_debug_view.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "pt_context.hpp"
#include "pt_debug_view.hpp"
#include "pt_gbuffer_passes.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

struct DebugPassState
{
    DeviceBuffer lines, keys, stats;
    Pinned<float> staging; // a host caller's lines on their way to `lines`
    Fence staged;          // behind the copy out of `staging`
    Fence done;            // behind the last call's kernels: a call on another stream waits for it before it touches a buffer
    size_t keyPixels = 0;  // the keys are zero for this many pixels
    bool valid = false;    // a call has run
    uint32_t lineCount = 0; // ... with this many lines (0: it launched nothing)
    StageEvents<1> timing;
    // prosper_pt_texture_readback: the texel on the device, its pinned copy, and the fence behind that copy
    DeviceBuffer readbackTexel;
    Pinned<float> readbackHost;
    Fence readbackDone;
    bool readbackQueued = false; // recorded and not handed out yet
    // prosper_pt_texture_debug: the RGBA8 image when the caller only wants a host copy, the magnifier's peek on the device,
    // its pinned copy and the fence behind that copy
    DeviceBuffer viewerScratch, peekTexel;
    Pinned<float> peekHost;
    Fence peekDone;
    bool peekRecorded = false;
};

extern const PassModule kDebugPasses = pass_module<DebugPassState, &prosper_pt_ctx::debugPasses>();

} // namespace ppt

namespace
{

// The registry: the illumination, then every module's images in the modules' order (kPassModules), each in its fixed order
std::vector<DebugImage> debug_images(const prosper_pt_ctx *ctx)
{
    std::vector<DebugImage> images;
    DebugImage hdr;
    hdr.name = "illumination";
    hdr.format = PROSPER_PT_DEBUG_FORMAT_RGBA32F;
    hdr.valid = ctx->hdr && ctx->localWidth != 0u && ctx->height != 0u;
    if (hdr.valid) hdr.one_level(ctx->hdr, ctx->localWidth, ctx->height);
    images.push_back(hdr);
    for (const PassModule *m : kPassModules)
        if (m->list_debug_images) m->list_debug_images(ctx, images);
    DebugImage tone; // the last tone-mapped image, kept only when the caller asked for a host copy alone
    tone.name = "toneMapped";
    tone.format = PROSPER_PT_DEBUG_FORMAT_RGBA8_UNORM;
    tone.valid = ctx->toneScratch.ptr && ctx->toneKeptWidth != 0u && ctx->toneKeptHeight != 0u;
    if (tone.valid) tone.one_level(ctx->toneScratch.ptr, ctx->toneKeptWidth, ctx->toneKeptHeight);
    images.push_back(tone);
    return images;
}

} // namespace

extern "C" {

uint32_t prosper_pt_debug_resource_count(prosper_pt_ctx *ctx) { return ctx ? (uint32_t)debug_images(ctx).size() : 0u; }

int prosper_pt_get_debug_resource(prosper_pt_ctx *ctx, uint32_t index, prosper_pt_debug_resource *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_debug_resource: null argument");
    const std::vector<DebugImage> images = debug_images(ctx);
    if (index >= images.size()) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_debug_resource: no such resource");
    const DebugImage &im = images[index];
    prosper_pt_debug_resource r = {};
    std::strncpy(r.name, im.name, sizeof(r.name) - 1u);
    r.format = im.format;
    r.valid = im.valid ? 1u : 0u;
    if (im.valid) r.width = im.width, r.height = im.height, r.levelCount = im.levelCount;
    *out = r;
    return PROSPER_PT_OK;
}

int prosper_pt_texture_readback(prosper_pt_ctx *ctx, uint32_t resource, float pxX, float pxY, void *stream)
{
    if (!std::isfinite(pxX) || !std::isfinite(pxY))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_readback: non-finite pixel coordinates");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_readback: null argument");
    const std::vector<DebugImage> images = debug_images(ctx);
    if (resource >= images.size()) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_readback: no such resource");
    const DebugImage &im = images[resource];
    if (!im.valid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_texture_readback: the resource is not valid (its pass has not run)");
    DebugPassState &st = *ctx->debugPasses;
    if (st.readbackQueued)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_readback: a readback is queued and unread");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = grow_to(st.readbackTexel, sizeof(float4), s);
    if (rc != PROSPER_PT_OK) return rc;
    if (!st.readbackHost.ptr)
        if ((rc = st.readbackHost.allocate(sizeof(float4)))) return rc;
    TextureReadbackParams p = {};
    p.image = im.level[0];
    p.format = im.format;
    p.width = im.width;
    p.height = im.height;
    p.pxX = pxX;
    p.pxY = pxY;
    p.out = st.readbackTexel.as<float4>();
    launch_texture_readback(p, s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipMemcpyAsync(st.readbackHost.ptr, st.readbackTexel.ptr, sizeof(float4), hipMemcpyDeviceToHost, s));
    if ((rc = st.readbackDone.record(s)) != PROSPER_PT_OK) return rc;
    st.readbackQueued = true;
    return PROSPER_PT_OK;
}

int prosper_pt_try_texture_readback(prosper_pt_ctx *ctx, float out[4])
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_try_texture_readback: null argument");
    DebugPassState &st = *ctx->debugPasses;
    if (st.readbackQueued) PPT_HIP(hipSetDevice(ctx->device));
    if (!st.readbackQueued || !st.readbackDone.passed()) return PROSPER_PT_NOT_READY;
    std::memcpy(out, st.readbackHost.ptr, sizeof(float4));
    st.readbackQueued = false;
    return PROSPER_PT_OK;
}

int prosper_pt_texture_debug(
    prosper_pt_ctx *ctx, uint32_t resource, const prosper_pt_texture_debug_pc *pc, uint32_t useBilinearSampler,
    void *device_rgba8, uint8_t *host_rgba8, size_t byte_size, void *stream)
{
    // the arguments are checked before the context, so that every refusal that can happens without a GPU
    if (!pc || (!device_rgba8 && !host_rgba8)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: null argument");
    if (useBilinearSampler > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: useBilinearSampler is 0 or 1");
    if (pc->flags >> 6) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: unknown flag bits");
    if (pc->outRes[0] <= 0 || pc->outRes[1] <= 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: empty outRes");
    if (pc->outRes[0] > (int32_t)kMaxExtent || pc->outRes[1] > (int32_t)kMaxExtent)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: an outRes above 32768 is not supported");
    const size_t bytes = (size_t)pc->outRes[0] * (size_t)pc->outRes[1] * 4u;
    if (byte_size < bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: destination too small");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: null argument");
    const std::vector<DebugImage> images = debug_images(ctx);
    if (resource >= images.size()) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: no such resource");
    const DebugImage &im = images[resource];
    if (!im.valid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_texture_debug: the resource is not valid (its pass has not run)");
    if (pc->inRes[0] != (int32_t)im.width || pc->inRes[1] != (int32_t)im.height)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: inRes differs from the resource's extent");
    if (pc->lod >= im.levelCount) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_texture_debug: lod beyond the resource's last level");
    DebugPassState &st = *ctx->debugPasses;
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = PROSPER_PT_OK;
    void *out = device_rgba8;
    if (!out)
    {
        if ((rc = grow_to(st.viewerScratch, bytes, s)) != PROSPER_PT_OK) return rc;
        out = st.viewerScratch.ptr;
    }
    if ((rc = grow_to(st.peekTexel, sizeof(float4), s)) != PROSPER_PT_OK) return rc;
    const bool magnifier = (pc->flags & PROSPER_PT_TEXTURE_DEBUG_MAGNIFIER) != 0u;
    if (magnifier)
    {
        if (!st.peekHost.ptr)
            if ((rc = st.peekHost.allocate(sizeof(float4)))) return rc;
        // the previous peek's copy may still be on its way on another stream
        if ((rc = st.peekDone.wait(s)) != PROSPER_PT_OK) return rc;
    }
    TextureDebugParams p = {};
    p.image = im.level[pc->lod];
    p.format = im.format;
    p.levelW = im.levelW[pc->lod];
    p.levelH = im.levelH[pc->lod];
    p.pc = *pc;
    p.bilinear = useBilinearSampler;
    p.out = static_cast<uint32_t *>(out);
    p.peek = st.peekTexel.as<float4>();
    launch_texture_debug(p, s);
    PPT_HIP(hipGetLastError());
    if (magnifier)
    {
        PPT_HIP(hipMemcpyAsync(st.peekHost.ptr, st.peekTexel.ptr, sizeof(float4), hipMemcpyDeviceToHost, s));
        if ((rc = st.peekDone.record(s)) != PROSPER_PT_OK) return rc;
        st.peekRecorded = true;
    }
    if (host_rgba8)
    {
        PPT_HIP(hipMemcpyAsync(host_rgba8, out, bytes, hipMemcpyDeviceToHost, s));
        PPT_HIP(hipStreamSynchronize(s));
    }
    return PROSPER_PT_OK;
}

int prosper_pt_get_texture_debug_peek(prosper_pt_ctx *ctx, float out[4])
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_texture_debug_peek: null argument");
    const DebugPassState &st = *ctx->debugPasses;
    if (!st.peekRecorded) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_get_texture_debug_peek: no call with the magnifier flag has run yet");
    PPT_HIP(hipSetDevice(ctx->device));
    if (const int rc = st.peekDone.host_wait()) return rc;
    std::memcpy(out, st.peekHost.ptr, sizeof(float4));
    return PROSPER_PT_OK;
}

int prosper_pt_debug_lines(
    prosper_pt_ctx *ctx, const float *lines, uint32_t count, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (count > kMaxDebugLines) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_lines: more than 100 000 lines");
    if (count != 0u && !lines) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_lines: null argument");
    if (!camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_lines: null argument");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_lines: empty extent");
    if (width > kMaxExtent || height > kMaxExtent)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_lines: an extent above 32768 is not supported");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_lines: null argument");
    const float *lastDepth = nullptr;
    uint32_t gw = 0, gh = 0;
    int rc = gbuffer_last_depth(ctx, &lastDepth, &gw, &gh);
    if (rc != PROSPER_PT_OK) return rc;
    if (gw != width || gh != height)
        return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_debug_lines: the last traced G-buffer has another extent");
    if (!hdr_has_extent(ctx, width, height))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_lines: the HDR image has another extent");
    DebugPassState &st = *ctx->debugPasses;
    st.valid = false;
    if (count == 0u)
    {
        st.lineCount = 0;
        st.valid = true;
        return PROSPER_PT_OK;
    }
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lineBytes = (size_t)count * kDebugLineFloats * sizeof(float);
    // the previous call may have run on another stream: `s` takes up behind its kernels, so that a grow (which waits for
    // `s` before it frees) and this call's copies never touch a buffer that call still uses
    if ((rc = st.done.wait(s)) != PROSPER_PT_OK) return rc;
    if ((rc = grow_to(st.lines, lineBytes, s)) != PROSPER_PT_OK) return rc;
    if ((rc = grow_to(st.stats, sizeof(DebugLineStats), s)) != PROSPER_PT_OK) return rc;
    const size_t pixels = (size_t)width * height;
    if (st.keyPixels < pixels || !st.keys.ptr)
    {
        st.keyPixels = 0;
        rc = grow_buffer(st.keys, GrowWait::Stream, s, pixels * 8u, pixels * 8u, 0);
        if (rc != PROSPER_PT_OK) return rc;
        st.keyPixels = pixels;
    }
    if ((rc = st.timing.create())) return rc;
    if (is_device_pointer(lines))
        PPT_HIP(hipMemcpyAsync(st.lines.ptr, lines, lineBytes, hipMemcpyDeviceToDevice, s));
    else
    {
        // through pinned staging: the caller's array may go once this returns, and the copy stays asynchronous
        if (!st.staging.ptr)
            if ((rc = st.staging.allocate((size_t)kMaxDebugLines * kDebugLineFloats * sizeof(float)))) return rc;
        if ((rc = st.staged.host_wait())) return rc;
        std::memcpy(st.staging.ptr, lines, lineBytes);
        PPT_HIP(hipMemcpyAsync(st.lines.ptr, st.staging.ptr, lineBytes, hipMemcpyHostToDevice, s));
        if ((rc = st.staged.record(s))) return rc;
    }
    PPT_HIP(hipMemsetAsync(st.stats.ptr, 0, sizeof(DebugLineStats), s));

    DebugLinesParams p = {};
    std::memcpy(p.worldToCamera, &camera->worldToCamera, sizeof(p.worldToCamera));
    std::memcpy(p.cameraToClip, &camera->cameraToClip, sizeof(p.cameraToClip));
    p.lines = st.lines.as<float>();
    p.count = count;
    p.width = width;
    p.height = height;
    p.hdr = ctx->hdr;
    p.nonLinearDepth = const_cast<float *>(lastDepth);
    p.keys = st.keys.as<unsigned long long>();
    p.stats = st.stats.as<DebugLineStats>();
    PPT_HIP(hipEventRecord(st.timing.events[0], s));
    launch_debug_lines(p, s);
    PPT_HIP(hipEventRecord(st.timing.events[1], s));
    PPT_HIP(hipGetLastError());
    if ((rc = st.done.record(s)) != PROSPER_PT_OK) return rc;
    st.lineCount = count;
    st.valid = true;
    return PROSPER_PT_OK;
}

int prosper_pt_get_debug_lines_info(prosper_pt_ctx *ctx, prosper_pt_debug_lines_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_debug_lines_info: null argument");
    const DebugPassState &st = *ctx->debugPasses;
    prosper_pt_debug_lines_info info = {};
    if (st.valid)
    {
        info.valid = 1u;
        info.lineCount = st.lineCount;
        if (st.lineCount != 0u)
        {
            PPT_HIP(hipSetDevice(ctx->device));
            if (const int rc = st.timing.elapsed(&info.ms)) return rc;
            DebugLineStats stats = {};
            PPT_HIP(hipMemcpy(&stats, st.stats.ptr, sizeof(stats), hipMemcpyDeviceToHost));
            info.fragmentsWritten = stats.fragmentsWritten;
            info.linesClippedAway = stats.linesClippedAway;
        }
    }
    *out = info;
    return PROSPER_PT_OK;
}

} // extern "C"
