// pt_mesh_passes.cpp — prosper_pt_prepare_mesh and its read-backs: a glTF primitive's accessors ->
// the blob of its `.prosper_mesh` cache file, as loadNextMesh makes it (src/scene/DeferredLoadingContext.cpp:
// generateTangents, generateMeshlets, packMeshData, writeCache).  The layout is mesh_cache.py pack_cache's; the vertex
// streams and the meshlet bounds are written by the kernels of pt_mesh_prepare.hip, the indices and the partition
// (meshlet_build.cpp) by the host.
#include <chrono>
#include <cstring>

#include "meshlet_build.hpp"
#include "pt_context.hpp"
#include "pt_mesh_prepare.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

// prosper_pt_prepare_mesh: on the device the source streams as the caller holds them, the six fixed-point tangent sums of
// every vertex, the float32 tangents and the blob; on the host the sections the partition fills, and what the last call
// left for the read-backs
struct MeshPreparePassState
{
    DeviceBuffer source, sums, tangents, blob;
    StageEvents<4> events; // around the last call's stages: tangents, pack, bounds, read back
    std::vector<uint32_t> image, hostBlob;
    std::vector<float> hostTangents;
    float meshletHostMs = 0.0f;
    bool prepared = false, tangentsValid = false, timed = false;
};

extern const PassModule kMeshPreparePasses = pass_module<MeshPreparePassState, &prosper_pt_ctx::meshPreparePasses>();

} // namespace ppt

namespace
{

constexpr uint32_t kAbsent = 0xFFFFFFFFu;

// 16 bits per index when the vertices allow it, padded to a whole word
uint64_t index_words(uint64_t count, bool isShort) { return isShort ? (count + 1u) / 2u : count; }
void write_indices(uint32_t *words, const uint32_t *indices, uint64_t count, bool isShort)
{
    if (!isShort)
    {
        if (count) std::memcpy(words, indices, count * 4u);
        return;
    }
    uint16_t *out = reinterpret_cast<uint16_t *>(words);
    for (uint64_t i = 0; i < count; ++i) out[i] = (uint16_t)indices[i];
    if (count % 2u) out[count] = 0u;
}

} // namespace

extern "C"
{

int prosper_pt_prepare_mesh(
    prosper_pt_ctx *ctx, const prosper_pt_mesh_source *src, uint32_t flags, prosper_pt_prepared_mesh *out, void *stream)
{
    if (!ctx || !src || !out || !src->positions || (src->indexCount && !src->indices))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_prepare_mesh: null argument");
    if (flags & ~(uint32_t)(PROSPER_PT_PREPARE_GENERATE_TANGENTS | PROSPER_PT_PREPARE_MESHLETS))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_prepare_mesh: unknown flags");
    const uint32_t n = src->vertexCount, indexCount = src->indexCount;
    if (n == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_prepare_mesh: zero vertices");
    if (indexCount % 3u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_prepare_mesh: indexCount " + std::to_string(indexCount) + " is not a multiple of 3");
    for (uint32_t i = 0; i < indexCount; ++i)
        if (src->indices[i] >= n)
            return fail(
                PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_prepare_mesh: index " + std::to_string(i) + " is " + std::to_string(src->indices[i]) +
                                                     ", at or past the " + std::to_string(n) + " vertices");
    // prosper's condition (DeferredLoadingContext.cpp:843-848)
    const bool generate = (flags & PROSPER_PT_PREPARE_GENERATE_TANGENTS) && !src->tangents && src->texCoord0s;
    if (generate && !src->normals)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_prepare_mesh: generating tangents needs normals");
    const PrepareTangents mode = src->tangents ? PrepareTangents::Supplied : (generate ? PrepareTangents::Generated : PrepareTangents::None);
    const bool withMeshlets = (flags & PROSPER_PT_PREPARE_MESHLETS) && indexCount;

    // the partition, on the host's clock
    MeshletPartition part;
    float hostMs = 0.0f;
    if (withMeshlets)
    {
        const auto t0 = std::chrono::steady_clock::now();
        part = build_meshlet_partition(src->indices, indexCount, n);
        hostMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    // the layout: pack_cache's
    const bool isShort = n <= 0xFFFFu;
    prosper_pt_prepared_mesh h = {};
    h.indexCount = indexCount;
    h.vertexCount = n;
    h.meshletCount = part.count();
    h.usesShortIndices = isShort ? 1u : 0u;
    uint64_t words = index_words(indexCount, isShort);
    const uint64_t indexWords = words;
    h.positionsOffset = (uint32_t)words;
    words += 2ull * n;
    h.normalsOffset = src->normals ? (uint32_t)words : kAbsent;
    words += src->normals ? n : 0u;
    h.tangentsOffset = mode != PrepareTangents::None ? (uint32_t)words : kAbsent;
    words += mode != PrepareTangents::None ? n : 0u;
    h.texCoord0sOffset = src->texCoord0s ? (uint32_t)words : kAbsent;
    words += src->texCoord0s ? n : 0u;
    // (empty meshlet sections: every offset points at the end of the vertex data, like computeOffset does)
    const uint64_t unit = isShort ? 2u : 1u;
    const uint64_t meshletWords = words;
    uint64_t verticesOffset = words * unit, trianglesByteOffset = words * 4u;
    h.meshletsOffset = h.meshletBoundsOffset = (uint32_t)words;
    if (h.meshletCount)
    {
        words += 4ull * h.meshletCount;
        h.meshletBoundsOffset = (uint32_t)words;
        words += 5ull * h.meshletCount;
        verticesOffset = words * unit;
        words += index_words(part.vertices.size(), isShort);
        trianglesByteOffset = words * 4u;
        words += part.triangles.size() / 4u;
    }
    if (words * 4u >= (1ull << 32)) return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_prepare_mesh: the blob exceeds 4 GiB");
    h.meshletVerticesOffset = (uint32_t)verticesOffset;
    h.meshletTrianglesByteOffset = (uint32_t)trianglesByteOffset;
    h.blobByteCount = (uint32_t)(words * 4u);

    // the source's streams behind one another in one staging buffer
    const size_t positionsAt = 0, normalsAt = positionsAt + 12ull * n, tangentsAt = normalsAt + (src->normals ? 12ull * n : 0u);
    const size_t uvsAt = tangentsAt + (src->tangents ? 16ull * n : 0u), indicesAt = uvsAt + (src->texCoord0s ? 8ull * n : 0u);
    const size_t sourceBytes = indicesAt + (generate ? 4ull * indexCount : 0u);

    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    MeshPreparePassState &st = *ctx->meshPreparePasses;
    int rc;
    if ((rc = grow_to(st.source, sourceBytes, s))) return rc;
    if ((rc = grow_to(st.blob, (size_t)words * 4u, s))) return rc;
    if (generate)
    {
        if ((rc = grow_to(st.sums, 48ull * n, s))) return rc;
        if ((rc = grow_to(st.tangents, 16ull * n, s))) return rc;
    }
    if ((rc = st.events.create())) return rc;

    // what the host writes of the blob: the indices in front, the partition behind the vertex streams (the bounds' words
    // are the kernel's)
    std::vector<uint32_t> &image = st.image;
    image.assign((size_t)(indexWords + (words - meshletWords)), 0u);
    write_indices(image.data(), src->indices, indexCount, isShort);
    uint32_t *tail = image.data() + indexWords;
    if (h.meshletCount)
    {
        std::memcpy(tail, part.meshlets.data(), part.meshlets.size() * 4u);
        write_indices(tail + 9ull * h.meshletCount, part.vertices.data(), part.vertices.size(), isShort);
        std::memcpy(tail + (trianglesByteOffset / 4u - meshletWords), part.triangles.data(), part.triangles.size());
    }

    st.prepared = false;
    st.timed = false;
    if (generate) st.tangentsValid = false;
    st.hostBlob.resize((size_t)words);
    if (generate) st.hostTangents.resize(4ull * n);
    uint8_t *dSource = st.source.as<uint8_t>();
    uint32_t *dBlob = st.blob.as<uint32_t>();
    const auto enqueue = [&]() -> hipError_t {
        hipError_t e;
        if ((e = hipEventRecord(st.events.events[0], s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(dSource + positionsAt, src->positions, 12ull * n, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
        if (src->normals && (e = hipMemcpyAsync(dSource + normalsAt, src->normals, 12ull * n, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
        if (src->tangents && (e = hipMemcpyAsync(dSource + tangentsAt, src->tangents, 16ull * n, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
        if (src->texCoord0s && (e = hipMemcpyAsync(dSource + uvsAt, src->texCoord0s, 8ull * n, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
        if (generate)
        {
            if (indexCount && (e = hipMemcpyAsync(dSource + indicesAt, src->indices, 4ull * indexCount, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(st.sums.ptr, 0, 48ull * n, s)) != hipSuccess) return e;
            launch_tangent_sums(
                reinterpret_cast<const float *>(dSource + positionsAt), reinterpret_cast<const float *>(dSource + uvsAt),
                reinterpret_cast<const uint32_t *>(dSource + indicesAt), indexCount / 3u, st.sums.as<long long>(), s);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        if ((e = hipEventRecord(st.events.events[1], s)) != hipSuccess) return e;
        PackMeshArgs pack = {};
        pack.positions = reinterpret_cast<const float *>(dSource + positionsAt);
        pack.normals = src->normals ? reinterpret_cast<const float *>(dSource + normalsAt) : nullptr;
        pack.tangents = src->tangents ? reinterpret_cast<const float *>(dSource + tangentsAt) : nullptr;
        pack.uvs = src->texCoord0s ? reinterpret_cast<const float *>(dSource + uvsAt) : nullptr;
        pack.sums = generate ? st.sums.as<long long>() : nullptr;
        pack.tangentsOut = generate ? st.tangents.as<float>() : nullptr;
        pack.blob = dBlob;
        pack.vertexCount = n;
        pack.positionsOffset = h.positionsOffset;
        pack.normalsOffset = h.normalsOffset;
        pack.tangentsOffset = h.tangentsOffset;
        pack.texCoord0sOffset = h.texCoord0sOffset;
        pack.mode = mode;
        launch_pack_mesh(pack, s);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(st.events.events[2], s)) != hipSuccess) return e;
        if (indexWords && (e = hipMemcpyAsync(dBlob, image.data(), indexWords * 4u, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
        if (h.meshletCount)
        {
            if ((e = hipMemcpyAsync(dBlob + meshletWords, tail, (words - meshletWords) * 4u, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
            MeshletBoundsArgs bounds = {};
            bounds.blob = dBlob;
            bounds.meshletCount = h.meshletCount;
            bounds.positionsOffset = h.positionsOffset;
            bounds.meshletsOffset = h.meshletsOffset;
            bounds.meshletBoundsOffset = h.meshletBoundsOffset;
            bounds.meshletVerticesOffset = h.meshletVerticesOffset;
            bounds.meshletTrianglesByteOffset = h.meshletTrianglesByteOffset;
            bounds.usesShortIndices = h.usesShortIndices;
            launch_meshlet_bounds(bounds, s);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        if ((e = hipEventRecord(st.events.events[3], s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(st.hostBlob.data(), dBlob, (size_t)words * 4u, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if (generate && (e = hipMemcpyAsync(st.hostTangents.data(), st.tangents.ptr, 16ull * n, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        return hipEventRecord(st.events.events[4], s);
    };
    // (whatever was enqueued is waited for, also after a failure: `src` is borrowed for the call only)
    const hipError_t e = enqueue();
    const hipError_t f = hipStreamSynchronize(s);
    PPT_HIP(e);
    PPT_HIP(f);
    st.prepared = true;
    st.timed = true;
    if (generate) st.tangentsValid = true;
    st.meshletHostMs = hostMs;
    *out = h;
    return PROSPER_PT_OK;
}

int prosper_pt_read_prepared_mesh(prosper_pt_ctx *ctx, void *dst, uint64_t bytes)
{
    if (!ctx || !dst) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_prepared_mesh: null argument");
    const MeshPreparePassState &st = *ctx->meshPreparePasses;
    if (!st.prepared) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_prepared_mesh: no prosper_pt_prepare_mesh has completed");
    const uint64_t have = (uint64_t)st.hostBlob.size() * 4u;
    if (bytes != have) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_prepared_mesh: the blob holds " + std::to_string(have) + " bytes");
    std::memcpy(dst, st.hostBlob.data(), (size_t)have);
    return PROSPER_PT_OK;
}

int prosper_pt_read_prepared_tangents(prosper_pt_ctx *ctx, float *dst, uint64_t bytes)
{
    if (!ctx || !dst) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_prepared_tangents: null argument");
    const MeshPreparePassState &st = *ctx->meshPreparePasses;
    if (!st.tangentsValid)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_prepared_tangents: no prosper_pt_prepare_mesh has generated tangents");
    const uint64_t have = (uint64_t)st.hostTangents.size() * 4u;
    if (bytes != have) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_prepared_tangents: the tangents hold " + std::to_string(have) + " bytes");
    std::memcpy(dst, st.hostTangents.data(), (size_t)have);
    return PROSPER_PT_OK;
}

int prosper_pt_get_prepare_mesh_timing(
    prosper_pt_ctx *ctx, float *tangentsMs, float *packMs, float *meshletHostMs, float *boundsMs, float *readbackMs)
{
    if (!ctx || !tangentsMs || !packMs || !meshletHostMs || !boundsMs || !readbackMs)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_prepare_mesh_timing: null argument");
    const MeshPreparePassState &st = *ctx->meshPreparePasses;
    if (!st.timed) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_prepare_mesh_timing: no prosper_pt_prepare_mesh has completed");
    PPT_HIP(hipSetDevice(ctx->device));
    float ms[4];
    const int rc = st.events.elapsed(ms);
    if (rc != PROSPER_PT_OK) return rc;
    *tangentsMs = ms[0];
    *packMs = ms[1];
    *meshletHostMs = st.meshletHostMs;
    *boundsMs = ms[2];
    *readbackMs = ms[3];
    return PROSPER_PT_OK;
}

} // extern "C"
