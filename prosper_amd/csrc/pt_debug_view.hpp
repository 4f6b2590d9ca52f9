// pt_debug_view.hpp — host-callable launchers of the gfx950 kernels of prosper's inspection passes (pt_debug_view.hip;
// src/render/DebugRenderer.cpp, res/shader/debug_lines.vert).  Their C entry points: pt_debug_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/prosper_pt/prosper_pt.h"

namespace ppt
{

constexpr uint32_t kDebugLineFloats = 9;        // DebugGeometry.hpp sLineBytes: p0, p1, colour
constexpr uint32_t kMaxDebugLines = 100000;     // DebugGeometry.hpp sMaxLineCount
constexpr uint32_t kDebugLinesPerBlock = 4;     // one wave per line, 256 lanes per block

// What a call counts on the device (zeroed at its start, read by prosper_pt_get_debug_lines_info)
struct DebugLineStats
{
    uint32_t fragmentsWritten; // pixels the resolve wrote
    uint32_t linesClippedAway; // lines with a non-finite endpoint or an empty clip interval
    uint32_t reserved[2];
};

struct DebugLinesParams
{
    float worldToCamera[16], cameraToClip[16]; // column-major, as prosper_CameraUniforms holds them
    const float *lines;                        // [count * 9], device
    uint32_t count;
    uint32_t width, height;
    float4 *hdr;
    float *nonLinearDepth;
    unsigned long long *keys; // [width * height], zero between calls
    DebugLineStats *stats;
};

// texture_readback.comp: one nearest clamp-to-edge sample of level 0 of a registry image
struct TextureReadbackParams
{
    const void *image;
    uint32_t format; // PROSPER_PT_DEBUG_FORMAT_*
    uint32_t width, height;
    float pxX, pxY;
    float4 *out; // device
};
void launch_texture_readback(const TextureReadbackParams &p, hipStream_t stream);

// texture_debug.comp over one level of a registry image: one lane per output texel
struct TextureDebugParams
{
    const void *image;       // the level PC.lod
    uint32_t format;         // PROSPER_PT_DEBUG_FORMAT_*
    uint32_t levelW, levelH; // its extent: the shader's inRes()
    prosper_pt_texture_debug_pc pc;
    uint32_t bilinear;
    uint32_t *out; // outRes.x * outRes.y RGBA8, device
    float4 *peek;  // device; written by the lane of output texel (0, 0) when the magnifier flag is set
};
void launch_texture_debug(const TextureDebugParams &p, hipStream_t stream);

// rasterise (one wave per line, an atomic maximum per fragment that passes the depth test), then resolve
void launch_debug_lines(const DebugLinesParams &p, hipStream_t stream);

} // namespace ppt
