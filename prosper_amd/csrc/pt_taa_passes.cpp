// pt_taa_passes.cpp — C-ABI of the temporal anti-aliasing resolve (include/prosper_pt/prosper_pt.h):
// prosper_pt_taa_resolve over the context's HDR image, its history and what reads them back.  Kernels: pt_taa.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include "pt_context.hpp"
#include "pt_pass_support.hpp"
#include "pt_taa.hpp"

using namespace ppt;

namespace ppt
{

struct TaaPassState
{
    DeviceBuffer hostInputs; // device copies of a call's host inputs: 16 + 8 + 4 bytes per pixel
    DeviceBuffer history[2]; // RGBA16F; history[newest] is what the next call reads
    uint32_t newest = 0;
    bool historyValid = false;
    uint32_t width = 0, height = 0; // of the last call
    bool ignoredHistory = false;    // ... and whether it ran IGNORE_HISTORY
    bool valid = false;
    StageEvents<kTaaStages> timing;
};

static void list_taa_debug_images(const prosper_pt_ctx *ctx, std::vector<DebugImage> &out)
{
    const TaaPassState &st = *ctx->taaPasses;
    DebugImage im;
    im.name = "previousResolvedIllumination";
    im.format = PROSPER_PT_DEBUG_FORMAT_RGBA16F;
    im.valid = st.historyValid && st.history[st.newest].ptr;
    if (im.valid) im.one_level(st.history[st.newest].ptr, st.width, st.height);
    out.push_back(im);
}

void forget_taa_history(prosper_pt_ctx *ctx)
{
    ctx->taaPasses->historyValid = false;
}

extern const PassModule kTaaPasses = pass_module<TaaPassState, &prosper_pt_ctx::taaPasses>(forget_taa_history, list_taa_debug_images);

} // namespace ppt

extern "C" {

void prosper_pt_taa_jitter(uint32_t jitterIndex, uint32_t width, uint32_t height, float out[2])
{
    if (!out) return;
    const float *h = kTaaHalton23[jitterIndex % 8u];
    out[0] = (h[0] * 2.f - 1.f) / (float)width;
    out[1] = (h[1] * 2.f - 1.f) / (float)height;
}

int prosper_pt_taa_resolve(
    prosper_pt_ctx *ctx, const prosper_pt_taa_pc *pc, uint32_t width, uint32_t height, const prosper_pt_taa_inputs *inputs,
    void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!pc || !inputs) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: null argument");
    if (pc->catmullRom > 1u || pc->luminanceWeighting > 1u || pc->resetHistory > 1u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: catmullRom, luminanceWeighting and resetHistory are 0 or 1");
    if (pc->colorClipping > PROSPER_PT_TAA_CLIPPING_VARIANCE)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: unknown color clipping type");
    if (pc->velocitySampling > PROSPER_PT_TAA_VELOCITY_CLOSEST)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: unknown velocity sampling type");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: empty extent");
    if (width > kMaxExtent || height > kMaxExtent)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: an extent above 32768 is not supported");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: null argument");
    const bool onDevice = inputs->onDevice != 0u;
    // (an explicit illumination that is the HDR image itself behaves as in place)
    const bool inPlace = inputs->illumination == nullptr || (onDevice && ctx->hdr && inputs->illumination == ctx->hdr);
    if (const int rc = check_in_place_hdr(ctx, "prosper_pt_taa_resolve", inPlace, width, height)) return rc;
    const bool closest = pc->velocitySampling == PROSPER_PT_TAA_VELOCITY_CLOSEST;
    TaaBuffers b = {};
    if (!inputs->velocity)
    {
        void *traced = nullptr;
        uint32_t vw = 0, vh = 0;
        const int rc = prosper_pt_get_velocity_device_ptr(ctx, &traced, &vw, &vh);
        if (rc != PROSPER_PT_OK) return rc;
        if (vw != width || vh != height)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: the last traced velocity target has another extent");
        b.velocity = static_cast<const float2 *>(traced);
    }
    if (closest)
        if (const int rc = resolve_depth(ctx, "prosper_pt_taa_resolve", inputs->nonLinearDepth, onDevice, width, height, &b.nonLinearDepth)) return rc;
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    TaaPassState &st = *ctx->taaPasses;
    const size_t pixels = (size_t)width * height;

    // TemporalAntiAliasing.cpp:199-220: no previous resolve, or one of another extent
    const bool ignore = pc->resetHistory != 0u || !st.historyValid || st.width != width || st.height != height;
    st.valid = false;
    st.historyValid = false;
    int rc = PROSPER_PT_OK;
    if (!onDevice) rc = grow_to(st.hostInputs, pixels * 28u, s);
    for (uint32_t k = 0; k < 2u; ++k)
        if (rc == PROSPER_PT_OK) rc = grow_to(st.history[k], pixels * 8u, s);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.timing.create())) return rc;

    if (inputs->velocity) b.velocity = static_cast<const float2 *>(inputs->velocity);
    if (!onDevice && inputs->velocity)
    {
        uint8_t *staged = st.hostInputs.as<uint8_t>() + pixels * 16u;
        PPT_HIP(hipMemcpyAsync(staged, inputs->velocity, pixels * 8u, hipMemcpyHostToDevice, s));
        b.velocity = reinterpret_cast<const float2 *>(staged);
    }
    if (closest && (rc = stage_depth(st.hostInputs, pixels * 24u, inputs->nonLinearDepth, pixels, s, &b.nonLinearDepth)) != PROSPER_PT_OK) return rc;
    rc = resolve_illumination(ctx, inputs->illumination, inPlace, onDevice, st.hostInputs, width, height, s, &b.illumination);
    if (rc != PROSPER_PT_OK) return rc;
    b.hdr = ctx->hdr;
    const uint32_t oldest = st.newest ^ 1u;
    b.history = st.history[st.newest].as<uint2>();
    b.resolved = st.history[oldest].as<uint2>();
    const uint32_t index =
        taa_specialization_index(ignore ? 1u : 0u, pc->catmullRom, pc->colorClipping, pc->velocitySampling, pc->luminanceWeighting);
    if (!launch_taa_resolve(index, width, height, b, st.timing.events, s))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_taa_resolve: no such specialisation");
    PPT_HIP(hipGetLastError());
    st.newest = oldest;
    st.width = width;
    st.height = height;
    st.ignoredHistory = ignore;
    st.historyValid = true;
    st.valid = true;
    return PROSPER_PT_OK;
}

void prosper_pt_taa_release_history(prosper_pt_ctx *ctx)
{
    if (ctx) forget_taa_history(ctx);
}

int prosper_pt_read_taa_history(prosper_pt_ctx *ctx, uint16_t *rgba16f, size_t bytes, void *stream)
{
    if (!ctx || !rgba16f) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_taa_history: null argument");
    const TaaPassState &st = *ctx->taaPasses;
    if (!st.historyValid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_taa_history: there is no history");
    if (bytes != (size_t)st.width * st.height * 8u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_taa_history: bytes differ from the history's");
    return read_back(ctx, static_cast<hipStream_t>(stream), {{rgba16f, st.history[st.newest].ptr, bytes}});
}

int prosper_pt_get_taa_info(prosper_pt_ctx *ctx, prosper_pt_taa_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_taa_info: null argument");
    const TaaPassState &st = *ctx->taaPasses;
    prosper_pt_taa_info info = {};
    info.historyValid = st.historyValid ? 1u : 0u;
    if (st.valid)
    {
        info.valid = 1u;
        info.width = st.width;
        info.height = st.height;
        info.ignoredHistory = st.ignoredHistory ? 1u : 0u;
        PPT_HIP(hipSetDevice(ctx->device));
        if (const int rc = st.timing.elapsed(&info.resolveMs)) return rc;
    }
    *out = info;
    return PROSPER_PT_OK;
}

} // extern "C"
