// tests/mesh_preparer_main.cpp — a C++ consumer of scene::MeshPreparer (csrc/host/mesh_preparer.cpp), linked against the
// library like prosper would be:
//   mesh_preparer_main <in.bin> <out.bin>
// in:  u32 vertexCount, indexCount, hasNormals, hasTangents, hasUvs, meshlets; then positions (3 floats per vertex),
//      normals (3), tangents (4), uvs (2) - those that are there - and the indices (u32)
// out: the 13 header fields (u32), u32 count of tangent floats, the blob, the tangents
// A refusal of the library (zero vertices) must arrive as std::runtime_error.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../prosper_amd/csrc/host/mesh_preparer.hpp"

namespace
{

template <class T> std::vector<T> read_array(std::FILE *in, size_t count)
{
    std::vector<T> out(count);
    if (count && std::fread(out.data(), sizeof(T), count, in) != count) throw std::runtime_error("the input file is short");
    return out;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 3;
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
        const std::vector<uint32_t> head = read_array<uint32_t>(in, 6);
        const size_t n = head[0];
        const std::vector<float> positions = read_array<float>(in, 3 * n), normals = read_array<float>(in, head[2] ? 3 * n : 0);
        const std::vector<float> tangents = read_array<float>(in, head[3] ? 4 * n : 0), uvs = read_array<float>(in, head[4] ? 2 * n : 0);
        const std::vector<uint32_t> indices = read_array<uint32_t>(in, head[1]);
        std::fclose(in);
        prosper_pt_mesh_source source = {};
        source.positions = positions.data();
        source.normals = head[2] ? normals.data() : nullptr;
        source.tangents = head[3] ? tangents.data() : nullptr;
        source.texCoord0s = head[4] ? uvs.data() : nullptr;
        source.indices = indices.data();
        source.vertexCount = head[0];
        source.indexCount = head[1];

        scene::MeshPreparer preparer;
        preparer.init(ctx);
        scene::MeshPrepareOptions options;
        options.generateMeshlets = head[5] != 0;
        const prosper_pt_prepared_mesh header = preparer.prepare(source, options);
        const std::vector<uint32_t> blob = preparer.blob();
        const std::vector<float> generated = preparer.tangents();
        bool refused = false;
        try
        {
            prosper_pt_mesh_source empty = source;
            empty.vertexCount = 0;
            empty.indexCount = 0;
            (void)preparer.prepare(empty, options);
        }
        catch (const std::runtime_error &)
        {
            refused = true;
        }
        if (!refused) throw std::logic_error("zero vertices were not refused");
        // (the refused call left the last result readable)
        if (preparer.blob() != blob) throw std::logic_error("the blob changed behind a refused call");
        std::FILE *out = std::fopen(argv[2], "wb");
        if (!out) throw std::runtime_error("cannot write the output file");
        const uint32_t count = (uint32_t)generated.size();
        std::fwrite(&header, sizeof(uint32_t), 13, out);
        std::fwrite(&count, sizeof(uint32_t), 1, out);
        std::fwrite(blob.data(), sizeof(uint32_t), blob.size(), out);
        std::fwrite(generated.data(), sizeof(float), generated.size(), out);
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
