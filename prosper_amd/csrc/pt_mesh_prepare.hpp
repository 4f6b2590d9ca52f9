// pt_mesh_prepare.hpp — host-callable launchers of the kernels in pt_mesh_prepare.hip (private to the library): what
// prosper's loadNextMesh does to a primitive between the glTF accessors and its cache file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ppt
{

// where prosper_pt_prepare_mesh's tangents come from
enum class PrepareTangents : uint32_t
{
    None,
    Supplied,
    Generated,
};

// The source streams on the device and where the packed ones go in the blob (offsets in u32 words, as the cache header
// counts them; a stream without a source is not written).
struct PackMeshArgs
{
    const float *positions; // 3 per vertex
    const float *normals;   // 3 per vertex, or nullptr
    const float *tangents;  // 4 per vertex (PrepareTangents::Supplied), or nullptr
    const float *uvs;       // 2 per vertex, or nullptr
    const long long *sums;  // 6 per vertex (PrepareTangents::Generated): the fixed-point sdir and tdir sums
    float *tangentsOut;     // 4 per vertex (PrepareTangents::Generated): the float32 tangents for the read-back
    uint32_t *blob;
    uint32_t vertexCount;
    uint32_t positionsOffset, normalsOffset, tangentsOffset, texCoord0sOffset;
    PrepareTangents mode;
};

// The meshlet sections of the blob (units as in the cache header: words, words, u16 or u32 entries, bytes)
struct MeshletBoundsArgs
{
    uint32_t *blob;
    uint32_t meshletCount;
    uint32_t positionsOffset, meshletsOffset, meshletBoundsOffset, meshletVerticesOffset, meshletTrianglesByteOffset;
    uint32_t usesShortIndices;
};

// Every corner's weighted unit sdir and tdir, in 2^-32 fixed point, added to its vertex's six sums (zeroed by the
// caller): prosper_amd/tangents.py corner_contributions + vertex_sums.  A lane per triangle; 64-bit integer atomics, so
// the sums do not depend on the order of arrival.
void launch_tangent_sums(const float *positions, const float *uvs, const uint32_t *indices, uint32_t triangleCount, long long *sums, hipStream_t stream);
// tangents.py finish + world.pack_mesh_data: a lane per vertex
void launch_pack_mesh(const PackMeshArgs &args, hipStream_t stream);
// meshlets.py meshlet_bounds(ordered=True) over the positions as the blob holds them: a wave per meshlet
void launch_meshlet_bounds(const MeshletBoundsArgs &args, hipStream_t stream);

} // namespace ppt
