// pt_bc7_encode.hpp — host-callable launchers of the kernels in pt_bc7_encode.hip (private to the library).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ppt
{

// modeMask of the encoder: bits 4, 5 and 6 enable that BC7 mode; 0 enables all three
constexpr uint32_t kBc7EncodeModes = (1u << 4) | (1u << 5) | (1u << 6);

// One level in the DeviceTexture tiling (width and height multiples of 4) -> its (width / 4) * (height / 4) BC7 blocks,
// row-major, 16 bytes each.
void launch_bc7_encode_level(const void *tiled, uint32_t width, uint32_t height, uint32_t modeMask, void *blocks, hipStream_t stream);
// n loose blocks of 16 row-major RGBA8 texels -> n BC7 blocks (4 words each) and their squared errors
void launch_bc7_encode_blocks(const uint32_t *texels, uint32_t n, uint32_t modeMask, uint32_t *blocks, uint32_t *sse, hipStream_t stream);

} // namespace ppt
