// tests/texture_compressor_main.cpp — a C++ consumer of scene::TextureCompressor (csrc/host/texture_compressor.cpp), linked
// against the library like prosper would be:
//   texture_compressor_main <in.rgba> <width> <height> <mips 0|1> <srgb 0|1> <out.bin>
// compresses the raw RGBA8 file and writes format, level count and every level's byte offset as uint32, then the payload.
// A refusal of the library (an empty extent) must arrive as std::runtime_error.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "../prosper_amd/csrc/host/texture_compressor.hpp"

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    const uint32_t width = (uint32_t)std::atoi(argv[2]), height = (uint32_t)std::atoi(argv[3]);
    std::vector<uint8_t> pixels((size_t)width * height * 4u);
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in || std::fread(pixels.data(), 1, pixels.size(), in) != pixels.size()) return 3;
    std::fclose(in);

    prosper_pt_device_desc desc = {};
    desc.struct_size = sizeof(desc);
    prosper_pt_ctx *ctx = nullptr;
    if (prosper_pt_create(&desc, &ctx) != PROSPER_PT_OK)
    {
        std::fprintf(stderr, "%s\n", prosper_pt_last_error());
        return 4;
    }
    int rc = 0;
    try
    {
        scene::TextureCompressor compressor;
        compressor.init(ctx);
        scene::Texture2DOptions options;
        options.generateMipMaps = std::atoi(argv[4]) != 0;
        options.colorSpace = std::atoi(argv[5]) != 0 ? scene::TextureColorSpace::sRgb : scene::TextureColorSpace::Linear;
        const scene::CompressedTexture tex = compressor.compress(pixels.data(), width, height, options);
        bool refused = false;
        try
        {
            (void)compressor.compress(pixels.data(), 0, height, options);
        }
        catch (const std::runtime_error &)
        {
            refused = true;
        }
        if (!refused) throw std::logic_error("an empty extent was not refused");
        std::FILE *out = std::fopen(argv[6], "wb");
        if (!out) throw std::runtime_error("cannot write the output file");
        const uint32_t head[2] = {tex.format, tex.mipLevelCount};
        std::fwrite(head, sizeof(uint32_t), 2, out);
        std::fwrite(tex.levelByteOffsets.data(), sizeof(uint32_t), tex.levelByteOffsets.size(), out);
        std::fwrite(tex.data.data(), 1, tex.data.size(), out);
        std::fclose(out);
    }
    catch (const std::exception &e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    prosper_pt_destroy(ctx);
    return rc;
}
