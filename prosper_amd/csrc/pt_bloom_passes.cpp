// pt_bloom_passes.cpp — C-ABI of bloom (include/prosper_pt/prosper_pt.h): prosper_pt_bloom and prosper_pt_bloom_fft over
// the context's HDR image, with the readbacks of what they produced.  Kernels: pt_bloom.hip, pt_bloom_fft.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "pt_bloom.hpp"
#include "pt_bloom_fft.hpp"
#include "pt_context.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

// The FFT technique.  It shares no image with the blur but the device copy of a host illumination.
struct BloomFftState
{
    DeviceBuffer highlights;            // dim x dim RGBA16F
    DeviceBuffer kernelImage;           // keptKernelDim x keptKernelDim RGBA32F, centred
    DeviceBuffer kernelDft;             // keptDim x keptDim RGBA32F
    DeviceBuffer convolved;             // dim x dim RGBA32F: the highlights' DFT, the product, its inverse
    DeviceBuffer transformWork;         // of prosper_pt_bloom_fft_transform with host images
    DeviceBuffer twiddles[5];           // e^{-2 pi i k / dim} of dim = 256 << n, made at first use
    uint32_t keptKernelDim = 0, keptDim = 0; // what kernelDft was made for; 0: there is none
    uint32_t width = 0, height = 0;     // of the last prosper_pt_bloom_fft
    BloomFftPlan last = {};
    bool remade = false, valid = false;
    StageEvents<kBloomFftStages> timing;
};

struct BloomPassState
{
    DeviceBuffer hostInput;                       // the device copy of a call's host illumination
    DeviceBuffer highlights, horizontal, blurred; // four levels each, RGBA16F
    DeviceBuffer streakWeights;                   // bloom_streak_weights of weightsHalfWidth
    uint32_t weightsHalfWidth = 0;
    BloomParams last = {}; // of the last prosper_pt_bloom
    bool valid = false;
    StageEvents<kBloomStages> timing;
    BloomFftState fft;
};

static void list_bloom_debug_images(const prosper_pt_ctx *ctx, std::vector<DebugImage> &out)
{
    const BloomPassState &st = *ctx->bloomPasses;
    const BloomParams &p = st.last;
    // the multi-resolution blur: the highlights hold levels 0-3; the two blur images only levels firstLevel .. + 2,
    // which the registry numbers from 0
    const struct
    {
        const char *name;
        const DeviceBuffer *buffer;
        bool blur;
    } images[3] = {{"BloomWorkingImage", &st.highlights, false}, {"BloomBlurPong", &st.horizontal, true}, {"BloomBlurred", &st.blurred, true}};
    for (const auto &i : images)
    {
        DebugImage im;
        im.name = i.name;
        im.format = PROSPER_PT_DEBUG_FORMAT_RGBA16F;
        im.valid = st.valid && i.buffer->ptr;
        if (im.valid)
        {
            const uint32_t first = i.blur ? p.firstLevel : 0u;
            im.levelCount = i.blur ? kBloomBlurLevels : kBloomLevels;
            for (uint32_t l = 0; l < im.levelCount; ++l)
            {
                im.level[l] = i.buffer->as<uint8_t>() + (size_t)p.levelOffset[first + l] * 8u;
                im.levelW[l] = p.levelW[first + l];
                im.levelH[l] = p.levelH[first + l];
            }
            im.width = im.levelW[0], im.height = im.levelH[0];
        }
        out.push_back(im);
    }
    // the FFT technique
    const BloomFftState &f = st.fft;
    const struct
    {
        const char *name;
        uint32_t format;
        const DeviceBuffer *buffer;
        uint32_t dim;
    } fft[4] = {{"BloomFftHighlights", PROSPER_PT_DEBUG_FORMAT_RGBA16F, &f.highlights, f.last.dim},
                {"BloomKernelImageCentered", PROSPER_PT_DEBUG_FORMAT_RGBA32F, &f.kernelImage, f.last.kernelDim},
                {"BloomKernelDft", PROSPER_PT_DEBUG_FORMAT_RGBA32F, &f.kernelDft, f.last.dim},
                {"BloomFftConvolved", PROSPER_PT_DEBUG_FORMAT_RGBA32F, &f.convolved, f.last.dim}};
    for (const auto &i : fft)
    {
        DebugImage im;
        im.name = i.name;
        im.format = i.format;
        im.valid = f.valid && i.buffer->ptr && i.dim != 0u;
        if (im.valid) im.one_level(i.buffer->ptr, i.dim, i.dim);
        out.push_back(im);
    }
}

extern const PassModule kBloomPasses = pass_module<BloomPassState, &prosper_pt_ctx::bloomPasses>(nullptr, list_bloom_debug_images);

} // namespace ppt

namespace
{

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

// the twiddle table of `dim` on the device
int ensure_twiddles(BloomFftState &st, uint32_t dim, hipStream_t s, const float2 **out)
{
    uint32_t n = 0;
    while ((kBloomFftMinDim << n) < dim) ++n;
    DeviceBuffer &table = st.twiddles[n];
    if (!table.ptr)
    {
        std::vector<float> w(2u * (size_t)dim);
        bloom_fft_twiddles(dim, w.data());
        const size_t bytes = w.size() * sizeof(float);
        const int rc = grow_buffer(table, GrowWait::None, nullptr, bytes, bytes);
        if (rc != PROSPER_PT_OK) return rc;
        // `w` is gone when this returns; a table that was not filled must not be found by the next call
        hipError_t e = hipMemcpyAsync(table.ptr, w.data(), bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess)
        {
            (void)hipFree(table.ptr);
            table.ptr = nullptr;
            table.bytes = 0;
            PPT_HIP(e);
        }
    }
    *out = table.as<float2>();
    return PROSPER_PT_OK;
}

// what prosper_pt_bloom_fft refuses of its push constants and extent, before it looks at the context
int check_bloom_fft_arguments(const prosper_pt_bloom_fft_pc *pc, uint32_t width, uint32_t height, BloomFftPlan &plan)
{
    if (!pc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: null argument");
    if (!std::isfinite(pc->threshold)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: non-finite threshold");
    if (pc->threshold < 0.0f) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: negative threshold");
    if (pc->resolutionScale > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: unknown resolution scale");
    if (pc->biquadratic > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: biquadratic is 0 or 1");
    if (pc->regenerateKernel > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: regenerateKernel is 0 or 1");
    for (uint32_t r : pc->reserved)
        if (r != 0u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: reserved words must be 0");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: empty extent");
    if (width > 2u * kBloomFftMaxDim || height > 2u * kBloomFftMaxDim)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: an extent above 8192 is not supported");
    if (!bloom_fft_plan(width, height, pc->resolutionScale, plan))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: the extent leaves the working image empty");
    return PROSPER_PT_OK;
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
    if (const int rc = check_in_place_hdr(ctx, "prosper_pt_bloom", inPlace, width, height)) return rc;
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    BloomPassState &st = *ctx->bloomPasses;
    p.threshold = pc->threshold;
    for (uint32_t k = 0; k < 3u; ++k) p.blendFactors[k] = pc->blendFactors[k];
    p.biquadratic = pc->biquadratic;

    st.valid = false;
    int rc = grow_to(st.highlights, texels * 8u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.horizontal, texels * 8u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.blurred, texels * 8u, s);
    if (rc == PROSPER_PT_OK) rc = ensure_streak_weights(st, p.streakHalfWidth, s);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.timing.create())) return rc;

    BloomBuffers b = {};
    // (an explicit illumination that is the HDR image itself behaves as in place)
    rc = resolve_illumination(ctx, illumination, inPlace, onDevice != 0u, st.hostInput, width, height, s, &b.illumination);
    if (rc != PROSPER_PT_OK) return rc;
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
    return read_back(ctx, static_cast<hipStream_t>(stream), {{host, image.as<uint8_t>() + (size_t)p.levelOffset[level] * 8u, bytes}});
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

int prosper_pt_bloom_fft_plan(uint32_t width, uint32_t height, uint32_t resolutionScale, struct prosper_pt_bloom_fft_plan *out)
{
    BloomFftPlan plan = {};
    if (!out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft_plan: null argument");
    if (!bloom_fft_plan(width, height, resolutionScale, plan))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft_plan: an extent or a scale prosper_pt_bloom_fft refuses");
    out->dim = plan.dim;
    out->kernelDim = plan.kernelDim;
    out->convolutionScale = plan.convolutionScale;
    return PROSPER_PT_OK;
}

int prosper_pt_bloom_fft(
    prosper_pt_ctx *ctx, const prosper_pt_bloom_fft_pc *pc, uint32_t width, uint32_t height, const void *illumination, uint32_t onDevice,
    void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    BloomFftPlan plan = {};
    if (const int rc = check_bloom_fft_arguments(pc, width, height, plan)) return rc;
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft: null argument");
    const bool inPlace = illumination == nullptr;
    if (const int rc = check_in_place_hdr(ctx, "prosper_pt_bloom_fft", inPlace, width, height)) return rc;
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    BloomFftState &st = ctx->bloomPasses->fft;
    const size_t texels = (size_t)plan.dim * plan.dim;
    const bool remake = pc->regenerateKernel != 0u || st.keptKernelDim != plan.kernelDim || st.keptDim != plan.dim;

    st.valid = false;
    const float2 *twiddles = nullptr;
    int rc = grow_to(st.highlights, texels * 8u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.convolved, texels * 16u, s);
    if (rc == PROSPER_PT_OK && remake)
    {
        st.keptKernelDim = st.keptDim = 0u;
        rc = grow_to(st.kernelImage, (size_t)plan.kernelDim * plan.kernelDim * 16u, s);
        if (rc == PROSPER_PT_OK) rc = grow_to(st.kernelDft, texels * 16u, s);
    }
    if (rc == PROSPER_PT_OK) rc = ensure_twiddles(st, plan.dim, s, &twiddles);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.timing.create())) return rc;

    const float4 *input = nullptr;
    // (an explicit illumination that is the HDR image itself behaves as in place)
    rc = resolve_illumination(ctx, illumination, inPlace, onDevice != 0u, ctx->bloomPasses->hostInput, width, height, s, &input);
    if (rc != PROSPER_PT_OK) return rc;
    hipEvent_t *events = st.timing.events;
    uint32_t e = 0;
    auto mark = [&]() { (void)hipEventRecord(events[e++], s); };
    float4 *kernelDft = st.kernelDft.as<float4>(), *convolved = st.convolved.as<float4>();
    mark();
    launch_bloom_fft_separate(width, height, plan.scale, pc->threshold, plan.dim, input, st.highlights.as<uint2>(), s);
    mark();
    if (remake) launch_bloom_fft_generate_kernel(plan.kernelDim, st.kernelImage.as<float4>(), s);
    mark();
    if (remake) launch_bloom_fft_prepare_kernel(plan.kernelDim, plan.dim, st.kernelImage.as<float4>(), kernelDft, s);
    mark();
    if (remake)
    {
        launch_bloom_fft_rows(plan.dim, false, kernelDft, false, kernelDft, twiddles, s);
        launch_bloom_fft_columns(plan.dim, false, kernelDft, kernelDft, twiddles, s);
    }
    mark();
    launch_bloom_fft_rows(plan.dim, false, st.highlights.ptr, true, convolved, twiddles, s);
    mark();
    launch_bloom_fft_middle(plan.dim, convolved, kernelDft, twiddles, plan.convolutionScale, s);
    mark();
    launch_bloom_fft_rows(plan.dim, true, convolved, false, convolved, twiddles, s);
    mark();
    launch_bloom_fft_compose(width, height, plan.scale, plan.dim, pc->biquadratic, input, convolved, ctx->hdr, s);
    mark();
    PPT_HIP(hipGetLastError());
    st.keptKernelDim = plan.kernelDim;
    st.keptDim = plan.dim;
    st.width = width;
    st.height = height;
    st.last = plan;
    st.remade = remake;
    st.valid = true;
    return PROSPER_PT_OK;
}

int prosper_pt_bloom_fft_transform(
    prosper_pt_ctx *ctx, uint32_t dim, uint32_t inverse, const void *in, void *out, uint32_t onDevice, void *stream)
{
    if (!bloom_fft_is_dim(dim))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft_transform: dim is a power of two in [256, 4096]");
    if (inverse > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft_transform: inverse is 0 or 1");
    if (!ctx || !in || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_bloom_fft_transform: null argument");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    BloomFftState &st = ctx->bloomPasses->fft;
    const size_t bytes = (size_t)dim * dim * 16u;
    const float2 *twiddles = nullptr;
    int rc = ensure_twiddles(st, dim, s, &twiddles);
    if (rc == PROSPER_PT_OK && !onDevice) rc = grow_to(st.transformWork, bytes, s);
    if (rc != PROSPER_PT_OK) return rc;
    const void *source = in;
    float4 *target = static_cast<float4 *>(out);
    if (!onDevice)
    {
        PPT_HIP(hipMemcpyAsync(st.transformWork.ptr, in, bytes, hipMemcpyHostToDevice, s));
        source = st.transformWork.ptr;
        target = st.transformWork.as<float4>();
    }
    launch_bloom_fft_rows(dim, inverse != 0u, source, false, target, twiddles, s);
    launch_bloom_fft_columns(dim, inverse != 0u, target, target, twiddles, s);
    PPT_HIP(hipGetLastError());
    if (!onDevice)
    {
        PPT_HIP(hipMemcpyAsync(out, target, bytes, hipMemcpyDeviceToHost, s));
        PPT_HIP(hipStreamSynchronize(s));
    }
    return PROSPER_PT_OK;
}

void prosper_pt_bloom_fft_release_kernel(prosper_pt_ctx *ctx)
{
    if (ctx) ctx->bloomPasses->fft.keptKernelDim = ctx->bloomPasses->fft.keptDim = 0u;
}

int prosper_pt_read_bloom_fft_stage(prosper_pt_ctx *ctx, uint32_t stage, void *host, size_t byte_size, void *stream)
{
    if (stage >= PROSPER_PT_BLOOM_FFT_STAGE_COUNT)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_bloom_fft_stage: unknown stage");
    if (!ctx || !host) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_bloom_fft_stage: null argument");
    const BloomFftState &st = ctx->bloomPasses->fft;
    if (!st.valid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_bloom_fft_stage: no bloom_fft has run yet");
    const size_t texels = (size_t)st.last.dim * st.last.dim, kernelTexels = (size_t)st.last.kernelDim * st.last.kernelDim;
    const DeviceBuffer *image = &st.highlights;
    size_t bytes = texels * 8u;
    if (stage == PROSPER_PT_BLOOM_FFT_KERNEL) image = &st.kernelImage, bytes = kernelTexels * 16u;
    if (stage == PROSPER_PT_BLOOM_FFT_KERNEL_DFT) image = &st.kernelDft, bytes = texels * 16u;
    if (stage == PROSPER_PT_BLOOM_FFT_CONVOLVED) image = &st.convolved, bytes = texels * 16u;
    if (byte_size != bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_bloom_fft_stage: byte_size differs from the image's");
    return read_back(ctx, static_cast<hipStream_t>(stream), {{host, image->ptr, bytes}});
}

int prosper_pt_get_bloom_fft_info(prosper_pt_ctx *ctx, prosper_pt_bloom_fft_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_bloom_fft_info: null argument");
    const BloomFftState &st = ctx->bloomPasses->fft;
    prosper_pt_bloom_fft_info info = {};
    if (st.valid)
    {
        info.valid = 1u;
        info.width = st.width;
        info.height = st.height;
        info.dim = st.last.dim;
        info.kernelDim = st.last.kernelDim;
        info.kernelRemade = st.remade ? 1u : 0u;
        info.convolutionScale = st.last.convolutionScale;
        info.fused = 0x70u; // the forward columns, the convolution and the inverse columns are one launch
        PPT_HIP(hipSetDevice(ctx->device));
        if (const int rc = st.timing.elapsed(&info.separateMs)) return rc;
        if (!st.remade) info.generateMs = info.prepareMs = info.kernelFftMs = 0.0f;
    }
    *out = info;
    return PROSPER_PT_OK;
}

} // extern "C"
