// pt_bloom_passes.cpp — C-ABI of bloom (include/prosper_pt/prosper_pt.h): prosper_pt_bloom over the context's HDR image,
// with the readbacks of what it produced.  Kernels: pt_bloom.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "pt_bloom.hpp"
#include "pt_context.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

struct BloomPassState
{
    DeviceBuffer hostInput;                       // the device copy of a call's host illumination
    DeviceBuffer highlights, horizontal, blurred; // four levels each, RGBA16F
    DeviceBuffer streakWeights;                   // bloom_streak_weights of weightsHalfWidth
    uint32_t weightsHalfWidth = 0;
    BloomParams last = {}; // of the last prosper_pt_bloom
    bool valid = false;
    StageEvents<kBloomStages> timing;
};

bool create_bloom_passes(prosper_pt_ctx *ctx)
{
    ctx->bloomPasses = new (std::nothrow) BloomPassState();
    return ctx->bloomPasses != nullptr;
}

void destroy_bloom_passes(prosper_pt_ctx *ctx)
{
    delete ctx->bloomPasses;
    ctx->bloomPasses = nullptr;
}

} // namespace ppt

namespace
{

constexpr uint32_t kMaxExtent = 32768; // compose forms (2 coord + 1) * levelSize + extent in 32 bits

bool finite_non_negative(float v) { return std::isfinite(v) && v >= 0.0f; }

// The weights of a streak of `halfWidth` on the device; remade only when the half-width changes.
int ensure_streak_weights(BloomPassState &st, uint32_t halfWidth, hipStream_t s)
{
    if (st.streakWeights.ptr && st.weightsHalfWidth == halfWidth) return PROSPER_PT_OK;
    std::vector<float> w(4u * (size_t)halfWidth);
    bloom_streak_weights(halfWidth, w.data(), w.data() + 2u * (size_t)halfWidth);
    const size_t bytes = w.size() * sizeof(float);
    const int rc = grow_to(st.streakWeights, bytes, s);
    if (rc != PROSPER_PT_OK) return rc;
    // the kernels of an earlier call on `s` may still read the old table, and `w` is gone when this returns
    PPT_HIP(hipStreamSynchronize(s));
    PPT_HIP(hipMemcpyAsync(st.streakWeights.ptr, w.data(), bytes, hipMemcpyHostToDevice, s));
    PPT_HIP(hipStreamSynchronize(s));
    st.weightsHalfWidth = halfWidth;
    return PROSPER_PT_OK;
}

// the level of a stage's image a read may ask for
bool stage_has_level(const BloomParams &p, uint32_t stage, uint32_t level)
{
    if (stage == PROSPER_PT_BLOOM_HIGHLIGHTS) return level < kBloomLevels;
    return level >= p.firstLevel && level < p.firstLevel + kBloomBlurLevels;
}

} // namespace

extern "C" {

void prosper_pt_bloom_streak_weights(uint32_t halfWidth, float *rg, float *b)
{
    if (rg && b) bloom_streak_weights(halfWidth, rg, b);
}

int prosper_pt_bloom(
    prosper_pt_ctx *ctx, const prosper_pt_bloom_pc *pc, uint32_t width, uint32_t height, const void *illumination, uint32_t onDevice,
    void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!pc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: null argument");
    if (!std::isfinite(pc->threshold) || !std::isfinite(pc->blendFactors[0]) || !std::isfinite(pc->blendFactors[1]) ||
        !std::isfinite(pc->blendFactors[2]))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: non-finite push constant");
    if (!finite_non_negative(pc->threshold) || !finite_non_negative(pc->blendFactors[0]) || !finite_non_negative(pc->blendFactors[1]) ||
        !finite_non_negative(pc->blendFactors[2]))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: negative threshold or blend factor");
    if (pc->resolutionScale > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: unknown resolution scale");
    if (pc->biquadratic > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: biquadratic is 0 or 1");
    if (pc->reserved[0] != 0u || pc->reserved[1] != 0u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: reserved words must be 0");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: empty extent");
    if (width > kMaxExtent || height > kMaxExtent)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: an extent above 32768 is not supported");
    BloomParams p = {};
    const size_t texels = bloom_set_extents(p, width, height, pc->resolutionScale);
    const uint32_t last = p.firstLevel + kBloomBlurLevels - 1u;
    if ((width / p.scale) >> last == 0u || (height / p.scale) >> last == 0u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: the extent leaves a blurred level empty");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: null argument");
    const bool inPlace = illumination == nullptr;
    if (inPlace && !hdr_has_extent(ctx, width, height))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom: the HDR image has another extent");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    BloomPassState &st = *ctx->bloomPasses;
    const size_t pixels = (size_t)width * height;
    p.threshold = pc->threshold;
    for (uint32_t k = 0; k < 3u; ++k) p.blendFactors[k] = pc->blendFactors[k];
    p.biquadratic = pc->biquadratic;

    st.valid = false;
    int rc = PROSPER_PT_OK;
    if (!inPlace && !onDevice) rc = grow_to(st.hostInput, pixels * 16u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.highlights, texels * 8u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.horizontal, texels * 8u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.blurred, texels * 8u, s);
    if (rc == PROSPER_PT_OK) rc = ensure_streak_weights(st, p.streakHalfWidth, s);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.timing.create())) return rc;

    BloomBuffers b = {};
    if (!inPlace)
    {
        b.illumination = static_cast<const float4 *>(illumination);
        if (!onDevice)
        {
            PPT_HIP(hipMemcpyAsync(st.hostInput.ptr, illumination, pixels * 16u, hipMemcpyHostToDevice, s));
            b.illumination = st.hostInput.as<float4>();
        }
        // (an explicit illumination that is the HDR image itself behaves as in place)
        rc = prepare_hdr(ctx, width, height, nullptr, s);
        if (rc != PROSPER_PT_OK) return rc;
    }
    else
        b.illumination = ctx->hdr;
    b.out = ctx->hdr;
    b.highlights = st.highlights.as<uint2>();
    b.horizontal = st.horizontal.as<uint2>();
    b.blurred = st.blurred.as<uint2>();
    b.streakWeights = st.streakWeights.as<float>();
    launch_bloom(p, b, st.timing.events, s);
    PPT_HIP(hipGetLastError());
    st.last = p;
    st.valid = true;
    return PROSPER_PT_OK;
}

int prosper_pt_read_bloom_stage(prosper_pt_ctx *ctx, uint32_t stage, uint32_t level, void *host, size_t byte_size, void *stream)
{
    if (stage >= PROSPER_PT_BLOOM_STAGE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_bloom_stage: unknown stage");
    if (!ctx || !host) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_bloom_stage: null argument");
    const BloomPassState &st = *ctx->bloomPasses;
    if (!st.valid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_bloom_stage: no bloom has run yet");
    const BloomParams &p = st.last;
    if (!stage_has_level(p, stage, level))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_bloom_stage: the stage did not write that level");
    const DeviceBuffer &image = stage == PROSPER_PT_BLOOM_HIGHLIGHTS ? st.highlights : (stage == PROSPER_PT_BLOOM_HORIZONTAL ? st.horizontal : st.blurred);
    const size_t bytes = (size_t)p.levelW[level] * p.levelH[level] * 8u;
    if (byte_size != bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_bloom_stage: byte_size differs from the level's");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PPT_HIP(hipMemcpyAsync(host, image.as<uint8_t>() + (size_t)p.levelOffset[level] * 8u, bytes, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

int prosper_pt_get_bloom_info(prosper_pt_ctx *ctx, prosper_pt_bloom_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_bloom_info: null argument");
    const BloomPassState &st = *ctx->bloomPasses;
    prosper_pt_bloom_info info = {};
    if (st.valid)
    {
        const BloomParams &p = st.last;
        info.valid = 1u;
        info.width = p.width;
        info.height = p.height;
        info.workingWidth = p.levelW[0];
        info.workingHeight = p.levelH[0];
        info.firstLevel = p.firstLevel;
        info.streakHalfWidth = p.streakHalfWidth;
        PPT_HIP(hipSetDevice(ctx->device));
        if (const int rc = st.timing.elapsed(&info.separateMs)) return rc;
    }
    *out = info;
    return PROSPER_PT_OK;
}

} // extern "C"
