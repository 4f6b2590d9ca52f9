// pt_texture_mips.hpp — host-callable launchers of the kernels in pt_texture_mips.hip (private to the library).
#pragma once

#include <hip/hip_runtime.h>

#include "pt_scene.hpp"

namespace ppt
{

// One level of a chain from its parent, both in the DeviceTexture tiling (the child's padding is not written: the caller
// zeroes the allocation).  `srgb`: RGB averaged in linear light.
void launch_generate_mip(
    const void *parent, uint32_t parentW, uint32_t parentH, void *child, uint32_t childW, uint32_t childH, bool srgb, hipStream_t stream);
// a tiled level -> width x height row-major RGBA8 texels (device memory)
void launch_untile_level(const void *tiled, uint32_t width, uint32_t height, void *linear, hipStream_t stream);
// sample_texture_lod over n records of (u, v, du/dx, dv/dx, du/dy, dv/dy) -> (RGBA, lambda)
void launch_sample_texture_lod(
    const DeviceScene &s, const DeviceTextureMips *mips, uint32_t texture, uint32_t sampler, const float *in6, uint32_t n, float bias,
    float *out5, hipStream_t stream);

} // namespace ppt
