// pt_denoise.hpp — host-callable launcher of the gfx950 kernels of the spatiotemporal denoiser (pt_denoise.hip; DESIGN.md
// f28; the rule: prosper_amd/denoise.py).  Their C entry points: pt_denoise_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ppt
{

constexpr uint32_t kDenoiseMaxIterations = 5;
constexpr uint32_t kDenoiseStages = 3u + kDenoiseMaxIterations; // temporal, variance, the a-trous passes, finish

struct DenoiseParams
{
    uint32_t width, height;
    uint32_t iterations, demodulate, maxHistoryLength, feedbackIteration, normalPowerLog2;
    uint32_t ignoreHistory;
    float minAlpha, depthTolerance, normalThreshold, sigmaDepth, sigmaLuminance;
    float cameraToClip22, cameraToClip32; // linearize_depth
};

// The images a frame hands to the next one.  Everything is float32; nothing is stored narrower.
struct DenoiseHistory
{
    float4 *colour;  // rgb + variance of the fed-back image
    float4 *moments; // m1, m2, the history length's bits, 0
    float4 *guideA;  // view depth z, dz/dx, dz/dy, the geometry flag's bits
    float4 *guideB;  // the decoded normal, 0
};

struct DenoiseBuffers
{
    const float4 *illumination;    // width * height RGBA32F (may be `hdr`)
    const float4 *albedoRoughness; // the G-buffer
    const float4 *normalMetallic;
    const float *nonLinearDepth;
    const float2 *velocity;
    DenoiseHistory previous; // read (not with ignoreHistory)
    DenoiseHistory next;     // written
    float4 *temporal;        // rgb + variance after the temporal stage and the variance estimate
    float4 *pingPong[2];     // a-trous pass i writes pingPong[i & 1]
    uint32_t *counts;        // [2]: geometry pixels with / without a usable history (zeroed by the launcher)
    float4 *hdr;             // the result
};

// One denoise on `stream`: the temporal stage, the variance estimate, p.iterations a-trous passes and the store to `hdr`
// (part of the last a-trous pass; a kernel of its own with no pass).  `events` (optional, kDenoiseStages + 1): recorded
// before each stage and after the last; a pass that does not run takes no time.
void launch_denoise(const DenoiseParams &p, const DenoiseBuffers &b, hipEvent_t *events, hipStream_t stream);

} // namespace ppt
