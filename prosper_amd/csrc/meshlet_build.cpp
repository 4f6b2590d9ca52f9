// meshlet_build.cpp — see meshlet_build.hpp.
#include "meshlet_build.hpp"

namespace ppt
{

MeshletPartition build_meshlet_partition(const uint32_t *indices, uint64_t indexCount, uint32_t vertexCount)
{
    MeshletPartition out;
    // where a vertex sits in the open meshlet: owner[v] == the open meshlet's ordinal + 1 means slot[v] is valid
    std::vector<uint32_t> owner(vertexCount, 0u);
    std::vector<uint8_t> slot(vertexCount, 0u);
    uint32_t open = 1, localCount = 0, triCount = 0, triOffset = 0;

    const auto close = [&]() {
        if (triCount)
        {
            out.meshlets.push_back((uint32_t)out.vertices.size() - localCount);
            out.meshlets.push_back(triOffset);
            out.meshlets.push_back(localCount);
            out.meshlets.push_back(triCount);
            triOffset = (triOffset + 3u * triCount + 3u) & ~3u; // meshoptimizer keeps every meshlet's triangles 4-byte aligned
            out.triangles.resize(triOffset, 0u);
        }
        ++open;
        localCount = 0;
        triCount = 0;
    };

    for (uint64_t i = 0; i + 2 < indexCount; i += 3)
    {
        const uint32_t tri[3] = {indices[i], indices[i + 1], indices[i + 2]};
        uint32_t fresh = 0;
        for (int k = 0; k < 3; ++k)
        {
            bool seen = owner[tri[k]] == open;
            for (int j = 0; j < k; ++j) seen = seen || tri[j] == tri[k];
            fresh += seen ? 0u : 1u;
        }
        if (localCount + fresh > kMeshletMaxVertices || triCount + 1u > kMeshletMaxTriangles) close();
        for (int k = 0; k < 3; ++k)
        {
            const uint32_t v = tri[k];
            if (owner[v] != open)
            {
                owner[v] = open;
                slot[v] = (uint8_t)localCount++;
                out.vertices.push_back(v);
            }
            out.triangles.push_back(slot[v]);
        }
        ++triCount;
    }
    close();
    if (!out.meshlets.empty())
    {
        // generateMeshlets: aligned_offset(last.triangle_offset + last.triangle_count, 4) * 3 bytes
        const size_t n = out.meshlets.size();
        const size_t size = (((size_t)out.meshlets[n - 3] + out.meshlets[n - 1] + 3u) & ~(size_t)3u) * 3u;
        if (size > out.triangles.size()) out.triangles.resize(size, 0u);
    }
    return out;
}

} // namespace ppt
