// host/texture_compressor.cpp — see texture_compressor.hpp.
#include "texture_compressor.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "host_common.hpp"

namespace scene
{

void TextureCompressor::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

CompressedTexture TextureCompressor::compress(
    const uint8_t *pixels, uint32_t width, uint32_t height, const Texture2DOptions &options, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    CompressedTexture out;
    out.width = width;
    out.height = height;
    uint64_t bytes = 0;
    if (prosper_pt_compressed_texture_layout(width, height, options.generateMipMaps ? 1u : 0u, &out.format, &out.mipLevelCount, &bytes) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("TextureCompressor::compress: ") + prosper_pt_last_error());
    // Dds.cpp:100-135: levels back to back, BC7 in whole 16-byte blocks
    uint32_t offset = 0;
    for (uint32_t i = 0; i < out.mipLevelCount; ++i)
    {
        const uint32_t w = std::max(width >> i, 1u), h = std::max(height >> i, 1u);
        out.levelByteOffsets.push_back(offset);
        offset += out.format == PROSPER_PT_FORMAT_BC7_UNORM ? (w / 4u) * (h / 4u) * 16u : w * h * 4u;
    }
    PROSPER_ASSERT(offset == bytes);
    out.data.resize((size_t)bytes);
    prosper_pt_texture_desc src = {};
    src.texels = pixels;
    src.width = width;
    src.height = height;
    src.format = PROSPER_PT_FORMAT_RGBA8_UNORM;
    const uint32_t flags = (options.generateMipMaps ? (uint32_t)PROSPER_PT_COMPRESS_GENERATE_MIPS : 0u) |
                           (options.colorSpace == TextureColorSpace::sRgb ? (uint32_t)PROSPER_PT_COMPRESS_SRGB : 0u);
    if (prosper_pt_compress_texture(m_ctx, &src, flags, out.data.data(), bytes, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("TextureCompressor::compress: ") + prosper_pt_last_error());
    return out;
}

} // namespace scene
