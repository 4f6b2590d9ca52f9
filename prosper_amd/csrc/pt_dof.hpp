// pt_dof.hpp — host-callable launchers of the gfx950 kernels of the skybox fill and of depth of field (pt_dof.hip;
// src/render/SkyboxRenderer.cpp, src/render/dof/*).  Their C entry points: pt_dof_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_scene.hpp"

namespace ppt
{

constexpr uint32_t kDofMaxLevels = 32;  // 32 - clz(max(hw, hh)) never exceeds it
constexpr uint32_t kDofTaps = 121;      // six octaweb rings: 1 + 8 + 16 + 24 + 32 + 40
constexpr uint32_t kDofStages = 9;      // setup, reduce, flatten, dilate, gather fg, gather bg, filter fg, filter bg, combine

// Extents and push constants of one depth-of-field call.  Level l of the half-resolution illumination is
// max(hw >> l, 1) x max(hh >> l, 1) RGBA16F texels, levelOffset[l] texels into its buffer.
struct DofParams
{
    uint32_t width, height; // full resolution
    uint32_t hw, hh;        // ceil(width / 2), ceil(height / 2)
    uint32_t tw, th;        // ceil(hw / 8), ceil(hh / 8)
    uint32_t levels;        // 32 - clz(max(hw, hh))
    float focusDistance, maxBackgroundCoC, maxCoC;
    int32_t gatherRadius;
    float cameraToClip22, cameraToClip32; // linearizeDepth (scene/camera.glsl:11-22)
    uint32_t levelOffset[kDofMaxLevels];
};
// hw, hh, tw, th, levels and levelOffset from width and height; returns the texels of the whole mip chain
size_t dof_set_extents(DofParams &p, uint32_t width, uint32_t height);

struct DofBuffers
{
    const float4 *illumination; // width * height RGBA32F (may be `out`: combine reads only the texel it writes)
    const float *nonLinearDepth; // width * height
    uint2 *halfIllumination;    // the mip chain, RGBA16F
    uint16_t *halfCoC;          // hw * hh R16F
    uint32_t *tileMinMax;       // tw * th RG16F (min | max << 16)
    uint32_t *dilatedMinMax;    // tw * th RG16F
    uint2 *gather[2];           // hw * hh RGBA16F: foreground, background
    uint2 *filtered[2];         // hw * hh RGBA16F
    const float *sampleOffsets; // 2 * kDofTaps floats (dof_sample_offsets), on the device
    float4 *out;                // width * height RGBA32F
};

// The 121 unit offsets (cos phi, sin phi) of the octaweb, ring by ring, as float32 of double-precision cos / sin
void dof_sample_offsets(float out[2 * kDofTaps]);
// The seven passes on `stream`.  `events` (optional, kDofStages + 1): recorded before each stage and after the last.
void launch_depth_of_field(const DofParams &p, const DofBuffers &b, hipEvent_t *events, hipStream_t stream);
// SkyboxRenderer: (sample_skybox(primary ray of the pixel centre), 1) into every texel of `hdr` whose depth is 0.  `r`
// carries the camera terms of pinhole_camera_ray and the extent, as launch_gbuffer_trace's.
void launch_skybox_fill(const DeviceScene &s, const RenderParams &r, const float *nonLinearDepth, float4 *hdr, hipStream_t stream);

} // namespace ppt
