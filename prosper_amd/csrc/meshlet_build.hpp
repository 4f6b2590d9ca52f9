// meshlet_build.hpp — the meshlet partition of a mesh on the host: the greedy scan of
// prosper_amd/meshlets.py build_meshlets, byte for byte, in prosper's layout (generateMeshlets,
// src/scene/DeferredLoadingContext.cpp:378-440).  Sequential by nature and integer only; plain C++, no HIP.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ppt
{

constexpr uint32_t kMeshletMaxVertices = 64;   // sMaxMsVertices
constexpr uint32_t kMeshletMaxTriangles = 124; // sMaxMsTriangles

struct MeshletPartition
{
    std::vector<uint32_t> meshlets;  // 4 per meshlet: vertexOffset, triangleOffset (bytes), vertexCount, triangleCount
    std::vector<uint32_t> vertices;  // meshletVertices: indices into the mesh's vertices
    std::vector<uint8_t> triangles;  // meshletTriangles: u8 triplets; every meshlet starts on a 4-byte boundary, and
                                     // the array is padded as generateMeshlets pads it (a multiple of 4 bytes)
    uint32_t count() const { return (uint32_t)(meshlets.size() / 4u); }
};

// A triangle goes into the current meshlet unless it would take it past either limit.  `indices`: indexCount (a multiple
// of 3) values below vertexCount - the caller has checked both.
MeshletPartition build_meshlet_partition(const uint32_t *indices, uint64_t indexCount, uint32_t vertexCount);

} // namespace ppt
