// tests/meshlet_build_main.cpp — the host partition (prosper_amd/csrc/meshlet_build.cpp) as a stand-alone program, for
// test_meshlet_build_host.py to build with sanitizers and compare with prosper_amd/meshlets.py.
//   meshlet_build_main <in> <out>
// in:  u32 vertexCount, u32 triangleCount, then 3 * triangleCount u32 indices
// out: u32 meshletCount, u32 vertexEntries, u32 triangleBytes, then the three arrays back to back
#include <cstdio>
#include <vector>

#include "meshlet_build.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[2];
    if (std::fread(head, 4, 2, in) != 2) return 4;
    std::vector<uint32_t> indices((size_t)head[1] * 3u);
    if (!indices.empty() && std::fread(indices.data(), 4, indices.size(), in) != indices.size()) return 4;
    std::fclose(in);
    for (uint32_t v : indices)
        if (v >= head[0]) return 5;
    const ppt::MeshletPartition part = ppt::build_meshlet_partition(indices.data(), indices.size(), head[0]);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 6;
    const uint32_t counts[3] = {part.count(), (uint32_t)part.vertices.size(), (uint32_t)part.triangles.size()};
    bool ok = std::fwrite(counts, 4, 3, out) == 3;
    ok = ok && std::fwrite(part.meshlets.data(), 4, part.meshlets.size(), out) == part.meshlets.size();
    ok = ok && std::fwrite(part.vertices.data(), 4, part.vertices.size(), out) == part.vertices.size();
    ok = ok && std::fwrite(part.triangles.data(), 1, part.triangles.size(), out) == part.triangles.size();
    ok = std::fclose(out) == 0 && ok;
    std::printf("%u meshlets\n", counts[0]);
    return ok ? 0 : 7;
}
