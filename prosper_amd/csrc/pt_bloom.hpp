// pt_bloom.hpp — host-callable launcher of the gfx950 kernels of bloom's multi-resolution blur (pt_bloom.hip;
// src/render/bloom/{Separate,Reduce,Blur,Compose}.cpp, res/shader/bloom/*).  C entry points:
// pt_bloom_passes.cpp.
//
// The input is the RGBA32F HDR image of this library; prosper's illumination is RGBA16F.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace ppt
{

constexpr uint32_t kBloomLevels = 4;     // of every working image: separate writes level 0, reduce levels 1-3
constexpr uint32_t kBloomBlurLevels = 3; // firstLevel ... firstLevel + 2 are blurred
constexpr uint32_t kBloomStages = 9;     // separate, reduce, three horizontal blurs, three vertical blurs, compose

// Extents and push constants of one bloom call.  Level l of a working image is levelW[l] x levelH[l] RGBA16F texels,
// levelOffset[l] texels into its buffer.
struct BloomParams
{
    uint32_t width, height;   // full resolution
    uint32_t scale;           // 2 (Half) or 4 (Quarter)
    uint32_t firstLevel;      // 0 (Half) or 1 (Quarter)
    uint32_t streakHalfWidth; // levelW[1] / 2
    uint32_t biquadratic;
    float threshold;
    float blendFactors[3];
    uint32_t levelW[kBloomLevels], levelH[kBloomLevels], levelOffset[kBloomLevels];
};
// scale, firstLevel, streakHalfWidth and the levels from width, height and the resolution scale (0 Half, 1 Quarter);
// returns the texels of one working image
size_t bloom_set_extents(BloomParams &p, uint32_t width, uint32_t height, uint32_t resolutionScale);

struct BloomBuffers
{
    const float4 *illumination; // width * height RGBA32F (may be `out`: compose reads only the texel it writes)
    uint2 *highlights;          // separate and reduce write it
    uint2 *horizontal;          // the horizontal blur's output
    uint2 *blurred;             // the vertical blur's output
    const float *streakWeights; // 2 * streakHalfWidth red / green weights, then as many blue ones, on the device
    float4 *out;                // width * height RGBA32F
};

// The streak's weights w(i), i = -halfWidth .. halfWidth - 1 (blur.comp:56-66), made in double precision from the
// integer i and rounded once to float32: rg[k] the red and green weight, b[k] the blue one of i = k - halfWidth
void bloom_streak_weights(uint32_t halfWidth, float *rg, float *b);
// The four passes on `stream`.  `events` (optional, kBloomStages + 1): recorded before each stage and after the last.
void launch_bloom(const BloomParams &p, const BloomBuffers &b, hipEvent_t *events, hipStream_t stream);

// The two passes the FFT technique (pt_bloom_fft.hpp) shares with the blur.  Separate over dim x dim RGBA16F: a texel
// whose lookups fall outside the illumination reads the border and stores (0, 0, 0, 0), the transform's zero padding.
void launch_bloom_fft_separate(
    uint32_t width, uint32_t height, uint32_t scale, float threshold, uint32_t dim, const float4 *illumination, uint2 *highlights,
    hipStream_t stream);
// compose.comp with MULTI_RESOLUTION = false: out = (illumination.rgb + the lookup of the convolved dim x dim RGBA32F
// image, 1).  `illumination` may be `out`.
void launch_bloom_fft_compose(
    uint32_t width, uint32_t height, uint32_t scale, uint32_t dim, uint32_t biquadratic, const float4 *illumination,
    const float4 *convolved, float4 *out, hipStream_t stream);

} // namespace ppt
