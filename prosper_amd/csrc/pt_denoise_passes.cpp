// pt_denoise_passes.cpp — C-ABI of the spatiotemporal denoiser (include/prosper_pt/prosper_pt.h):
// prosper_pt_denoise over the context's HDR image, its history and what reads them back.  Kernels: pt_denoise.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cmath>

#include "pt_context.hpp"
#include "pt_denoise.hpp"
#include "pt_gbuffer_passes.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

struct DenoisePassState
{
    // device copies of a call's host inputs, per pixel: illumination 16, albedo 16, normal 16, velocity 8, depth 4 bytes
    DeviceBuffer hostInputs;
    // colour, moments, guideA, guideB (DenoiseHistory), 16 bytes per pixel each; history[newest] is what the next call reads
    DeviceBuffer history[2][4];
    DeviceBuffer temporal, pingPong[2];
    DeviceBuffer counts; // two uint32
    uint32_t newest = 0;
    bool historyValid = false;
    DenoiseParams last = {}; // of the last call
    bool valid = false;
    StageEvents<kDenoiseStages> timing;
};

static void forget_denoise_history(prosper_pt_ctx *ctx)
{
    ctx->denoisePasses->historyValid = false;
}

// (no debug images: the registry's name list is fixed; prosper_pt_read_denoise_stage reads the pass's images)
extern const PassModule kDenoisePasses = pass_module<DenoisePassState, &prosper_pt_ctx::denoisePasses>(forget_denoise_history);

static DenoiseHistory history_of(DeviceBuffer (&set)[4])
{
    return DenoiseHistory{set[0].as<float4>(), set[1].as<float4>(), set[2].as<float4>(), set[3].as<float4>()};
}

static bool misaligned(const void *p, uintptr_t to)
{
    return (reinterpret_cast<uintptr_t>(p) & (to - 1u)) != 0u;
}

} // namespace ppt

extern "C" {

void prosper_pt_denoise_pc_default(prosper_pt_denoise_pc *out)
{
    if (!out) return;
    prosper_pt_denoise_pc pc = {};
    pc.iterations = 5u;
    pc.demodulate = 1u;
    pc.maxHistoryLength = 32u;
    pc.feedbackIteration = 1u;
    pc.normalPowerLog2 = 7u;
    pc.resetHistory = 0u;
    pc.minAlpha = 0.05f;
    pc.depthTolerance = 0.1f;
    pc.normalThreshold = 0.9f;
    pc.sigmaDepth = 1.0f;
    pc.sigmaLuminance = 4.0f;
    *out = pc;
}

int prosper_pt_denoise(
    prosper_pt_ctx *ctx, const prosper_pt_denoise_pc *pc, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height,
    const prosper_pt_denoise_inputs *inputs, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!pc || !camera || !inputs) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: null argument");
    if (pc->iterations > kDenoiseMaxIterations) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: iterations is 0 .. 5");
    if (pc->demodulate > 1u || pc->resetHistory > 1u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: demodulate and resetHistory are 0 or 1");
    if (pc->maxHistoryLength < 1u || pc->maxHistoryLength > 255u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: maxHistoryLength is 1 .. 255");
    if (pc->normalPowerLog2 > 8u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: normalPowerLog2 is 0 .. 8");
    for (const float f : {pc->minAlpha, pc->depthTolerance, pc->normalThreshold, pc->sigmaDepth, pc->sigmaLuminance})
    {
        if (!std::isfinite(f)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: non-finite push constant");
        if (!(f > 0.0f)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: the float push constants must be positive");
    }
    if (pc->minAlpha > 1.0f) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: minAlpha is above 1");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: empty extent");
    if (width > kMaxExtent || height > kMaxExtent)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: an extent above 32768 is not supported");
    const uint32_t given = (inputs->albedoRoughness ? 1u : 0u) + (inputs->normalMetallic ? 1u : 0u) + (inputs->nonLinearDepth ? 1u : 0u);
    if (given != 0u && given != 3u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: albedoRoughness, normalMetallic and nonLinearDepth are given together or not at all");
    const bool onDevice = inputs->onDevice != 0u;
    if (onDevice)
    {
        if (misaligned(inputs->illumination, 16u) || misaligned(inputs->albedoRoughness, 16u) || misaligned(inputs->normalMetallic, 16u))
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: illumination, albedoRoughness and normalMetallic must be 16-byte aligned");
        if (misaligned(inputs->velocity, 8u)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: the velocity target must be 8-byte aligned");
        if (misaligned(inputs->nonLinearDepth, 4u)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: the depth must be 4-byte aligned");
    }
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: null argument");
    // (an explicit illumination that is the HDR image itself behaves as in place)
    const bool inPlace = inputs->illumination == nullptr || (onDevice && ctx->hdr && inputs->illumination == ctx->hdr);
    if (const int rc = check_in_place_hdr(ctx, "prosper_pt_denoise", inPlace, width, height)) return rc;
    DenoiseBuffers b = {};
    if (!inputs->velocity)
    {
        void *traced = nullptr;
        uint32_t vw = 0, vh = 0;
        const int rc = prosper_pt_get_velocity_device_ptr(ctx, &traced, &vw, &vh);
        if (rc != PROSPER_PT_OK) return rc;
        if (vw != width || vh != height)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_denoise: the last traced velocity target has another extent");
        b.velocity = static_cast<const float2 *>(traced);
    }
    if (const int rc = resolve_depth(ctx, "prosper_pt_denoise", inputs->nonLinearDepth, onDevice, width, height, &b.nonLinearDepth)) return rc;
    if (given == 0u)
    {
        // (resolve_depth has matched the extent)
        const LastFrame &lastFrame = gbuffer_last_frame(ctx);
        if (!lastFrame.targets.albedoRoughness || !lastFrame.targets.normalMetallic)
            return fail(PROSPER_PT_ERR_NO_SCENE, "no G-buffer has been traced yet");
        b.albedoRoughness = static_cast<const float4 *>(lastFrame.targets.albedoRoughness);
        b.normalMetallic = static_cast<const float4 *>(lastFrame.targets.normalMetallic);
    }
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DenoisePassState &st = *ctx->denoisePasses;
    const size_t pixels = (size_t)width * height;

    const bool ignore = pc->resetHistory != 0u || !st.historyValid || st.last.width != width || st.last.height != height;
    st.valid = false;
    st.historyValid = false;
    int rc = PROSPER_PT_OK;
    if (!onDevice && (inputs->illumination || inputs->velocity || given)) rc = grow_to(st.hostInputs, pixels * 60u, s);
    for (auto &set : st.history)
        for (DeviceBuffer &image : set)
            if (rc == PROSPER_PT_OK) rc = grow_to(image, pixels * 16u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.temporal, pixels * 16u, s);
    for (DeviceBuffer &image : st.pingPong)
        if (rc == PROSPER_PT_OK) rc = grow_to(image, pixels * 16u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.counts, 2u * sizeof(uint32_t), s);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.timing.create())) return rc;

    uint8_t *staged = st.hostInputs.as<uint8_t>();
    if (given)
    {
        b.albedoRoughness = static_cast<const float4 *>(inputs->albedoRoughness);
        b.normalMetallic = static_cast<const float4 *>(inputs->normalMetallic);
        if (!onDevice)
        {
            PPT_HIP(hipMemcpyAsync(staged + pixels * 16u, inputs->albedoRoughness, pixels * 16u, hipMemcpyHostToDevice, s));
            PPT_HIP(hipMemcpyAsync(staged + pixels * 32u, inputs->normalMetallic, pixels * 16u, hipMemcpyHostToDevice, s));
            b.albedoRoughness = reinterpret_cast<const float4 *>(staged + pixels * 16u);
            b.normalMetallic = reinterpret_cast<const float4 *>(staged + pixels * 32u);
        }
    }
    if (inputs->velocity)
    {
        b.velocity = static_cast<const float2 *>(inputs->velocity);
        if (!onDevice)
        {
            PPT_HIP(hipMemcpyAsync(staged + pixels * 48u, inputs->velocity, pixels * 8u, hipMemcpyHostToDevice, s));
            b.velocity = reinterpret_cast<const float2 *>(staged + pixels * 48u);
        }
    }
    if ((rc = stage_depth(st.hostInputs, pixels * 56u, inputs->nonLinearDepth, pixels, s, &b.nonLinearDepth)) != PROSPER_PT_OK) return rc;
    rc = resolve_illumination(ctx, inputs->illumination, inPlace, onDevice, st.hostInputs, width, height, s, &b.illumination);
    if (rc != PROSPER_PT_OK) return rc;
    b.hdr = ctx->hdr;
    const uint32_t oldest = st.newest ^ 1u;
    b.previous = history_of(st.history[st.newest]);
    b.next = history_of(st.history[oldest]);
    b.temporal = st.temporal.as<float4>();
    b.pingPong[0] = st.pingPong[0].as<float4>();
    b.pingPong[1] = st.pingPong[1].as<float4>();
    b.counts = st.counts.as<uint32_t>();

    DenoiseParams p = {};
    p.width = width;
    p.height = height;
    p.iterations = pc->iterations;
    p.demodulate = pc->demodulate;
    p.maxHistoryLength = pc->maxHistoryLength;
    p.feedbackIteration = pc->feedbackIteration;
    p.normalPowerLog2 = pc->normalPowerLog2;
    p.ignoreHistory = ignore ? 1u : 0u;
    p.minAlpha = pc->minAlpha;
    p.depthTolerance = pc->depthTolerance;
    p.normalThreshold = pc->normalThreshold;
    p.sigmaDepth = pc->sigmaDepth;
    p.sigmaLuminance = pc->sigmaLuminance;
    p.cameraToClip22 = camera->cameraToClip.col[2].z;
    p.cameraToClip32 = camera->cameraToClip.col[3].z;
    launch_denoise(p, b, st.timing.events, s);
    PPT_HIP(hipGetLastError());
    st.newest = oldest;
    st.last = p;
    st.historyValid = true;
    st.valid = true;
    return PROSPER_PT_OK;
}

void prosper_pt_denoise_release_history(prosper_pt_ctx *ctx)
{
    if (ctx) forget_denoise_history(ctx);
}

int prosper_pt_read_denoise_stage(prosper_pt_ctx *ctx, uint32_t stage, void *host, size_t bytes, void *stream)
{
    if (stage >= PROSPER_PT_DENOISE_STAGE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_denoise_stage: unknown stage");
    if (!ctx || !host) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_denoise_stage: null argument");
    DenoisePassState &st = *ctx->denoisePasses;
    if (!st.valid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_denoise_stage: no denoise has run yet");
    const DenoiseParams &p = st.last;
    if (bytes != (size_t)p.width * p.height * 16u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_denoise_stage: bytes differ from the stage's");
    const void *src = nullptr;
    if (stage >= PROSPER_PT_DENOISE_ATROUS_0 && stage < PROSPER_PT_DENOISE_ATROUS_0 + kDenoiseMaxIterations)
    {
        const uint32_t pass = stage - PROSPER_PT_DENOISE_ATROUS_0;
        if (pass >= p.iterations) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_denoise_stage: that a-trous pass did not run");
        if (pass + 2u < p.iterations)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_denoise_stage: a later a-trous pass has overwritten that image");
        src = st.pingPong[pass & 1u].ptr;
    }
    else if (stage == PROSPER_PT_DENOISE_TEMPORAL)
        src = st.temporal.ptr;
    else
    {
        // the images the next call reads
        if (!st.historyValid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_denoise_stage: there is no history");
        DeviceBuffer(&set)[4] = st.history[st.newest];
        src = stage == PROSPER_PT_DENOISE_HISTORY_COLOUR ? set[0].ptr
              : stage == PROSPER_PT_DENOISE_MOMENTS      ? set[1].ptr
              : stage == PROSPER_PT_DENOISE_GUIDE_A      ? set[2].ptr
                                                         : set[3].ptr;
    }
    return read_back(ctx, static_cast<hipStream_t>(stream), {{host, src, bytes}});
}

int prosper_pt_get_denoise_info(prosper_pt_ctx *ctx, prosper_pt_denoise_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_denoise_info: null argument");
    const DenoisePassState &st = *ctx->denoisePasses;
    prosper_pt_denoise_info info = {};
    info.historyValid = st.historyValid ? 1u : 0u;
    if (st.valid)
    {
        info.valid = 1u;
        info.width = st.last.width;
        info.height = st.last.height;
        info.ignoredHistory = st.last.ignoreHistory;
        info.iterations = st.last.iterations;
        PPT_HIP(hipSetDevice(ctx->device));
        float ms[kDenoiseStages];
        if (const int rc = st.timing.elapsed(ms)) return rc;
        info.temporalMs = ms[0];
        info.varianceMs = ms[1];
        for (uint32_t k = 0; k < kDenoiseMaxIterations; ++k) info.atrousMs[k] = ms[2u + k];
        info.finishMs = ms[2u + kDenoiseMaxIterations];
        PPT_HIP(hipEventElapsedTime(&info.totalMs, st.timing.events[0], st.timing.events[kDenoiseStages]));
        // (the kernels are done: elapsed() has waited for the last event)
        uint32_t counts[2] = {};
        PPT_HIP(hipMemcpy(counts, st.counts.ptr, sizeof(counts), hipMemcpyDeviceToHost));
        info.historyPixels = counts[0];
        info.noHistoryPixels = counts[1];
    }
    *out = info;
    return PROSPER_PT_OK;
}

} // extern "C"
