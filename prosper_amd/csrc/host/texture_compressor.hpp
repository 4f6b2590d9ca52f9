// host/texture_compressor.hpp — scene::TextureCompressor of the headless host layer.
//
// Same role as compress() in prosper's Texture.cpp (reference: src/scene/Texture.cpp:213-296): RGBA8 pixels and
// Texture2DOptions in, the levels of the cache file out - BC7 when every level of the chain divides by 4, otherwise the
// raw RGBA8 chain - laid out like utils::Dds (levels back to back, levelByteOffsets).  Below it sit
// prosper_pt_compressed_texture_layout and prosper_pt_compress_texture: mip generation and the BC7 encoder run on the GPU
// (DESIGN.md f21).  Writing the DDS and its tag stays with the caller, as in the reference.
#pragma once

#include <cstdint>
#include <vector>

#include "../../../include/prosper_pt/prosper_pt.h"

namespace scene
{

enum class TextureColorSpace : uint8_t
{
    sRgb,
    Linear,
};

struct Texture2DOptions
{
    bool generateMipMaps{false};
    TextureColorSpace colorSpace{TextureColorSpace::sRgb};
};

// what utils::Dds holds of a compressed texture
struct CompressedTexture
{
    uint32_t width{0};
    uint32_t height{0};
    uint32_t format{PROSPER_PT_FORMAT_RGBA8_UNORM}; // PROSPER_PT_FORMAT_*
    uint32_t mipLevelCount{0};
    std::vector<uint8_t> data;
    std::vector<uint32_t> levelByteOffsets;
};

class TextureCompressor
{
  public:
    TextureCompressor() noexcept = default;
    TextureCompressor(const TextureCompressor &) = delete;
    TextureCompressor &operator=(const TextureCompressor &) = delete;

    // `ctx` is the context whose staging the compression uses (borrowed; it outlives the compressor).
    void init(prosper_pt_ctx *ctx);

    // `pixels`: width * height RGBA8 texels, row-major.  Throws std::runtime_error when the library refuses.
    CompressedTexture compress(const uint8_t *pixels, uint32_t width, uint32_t height, const Texture2DOptions &options, void *stream = nullptr);

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
};

} // namespace scene
