// pt_taa.hpp — host-callable launchers of the gfx950 kernels of the temporal anti-aliasing resolve (pt_taa.hip;
// src/render/TemporalAntiAliasing.cpp, res/shader/taa_resolve.comp).  Their C entry points:
// pt_taa_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ppt
{

constexpr uint32_t kTaaStages = 2; // resolve, expand

// TemporalAntiAliasing.cpp:50-65: the index of a pipeline among the specialisations of taa_resolve.comp
constexpr uint32_t taa_specialization_index(
    uint32_t ignoreHistory, uint32_t catmullRom, uint32_t colorClipping, uint32_t velocitySampling, uint32_t luminanceWeighting)
{
    return ignoreHistory | (catmullRom << 1) | (colorClipping << 2) | (velocitySampling << 4) | (luminanceWeighting << 6);
}
constexpr uint32_t kTaaSpecializations = 1u << 7;

struct TaaBuffers
{
    const float4 *illumination;  // width * height RGBA32F
    const float2 *velocity;      // width * height (unused by an IGNORE_HISTORY variant)
    const float *nonLinearDepth; // width * height (read by VelocitySampling_Closest alone)
    const uint2 *history;        // width * height RGBA16F: the previous resolve's output (unused by IGNORE_HISTORY)
    uint2 *resolved;             // width * height RGBA16F: the image the next call reads
    float4 *hdr;                 // the float32 expansion of `resolved`
};

// One resolve on `stream`: the variant `specializationIndex` of the resolve kernel, `resolved` from the four inputs.
// With an illumination that is not `hdr` the resolve kernel writes `hdr` as well; with illumination == hdr a second
// kernel expands `resolved` into it (the 3 x 3 neighbourhood reaches texels other blocks write).  `events` (optional,
// kTaaStages + 1): recorded before each stage and after the last.  False: no such variant.
bool launch_taa_resolve(
    uint32_t specializationIndex, uint32_t width, uint32_t height, const TaaBuffers &b, hipEvent_t *events, hipStream_t stream);

// The 8-sample Halton(2, 3) cycle of Camera.cpp:71-80 as float32 pairs
extern const float kTaaHalton23[8][2];

} // namespace ppt
