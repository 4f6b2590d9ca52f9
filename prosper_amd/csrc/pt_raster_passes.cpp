// pt_raster_passes.cpp — C-ABI of the compute rasteriser over the meshlet draw lists (include/prosper_pt/prosper_pt.h;
// DESIGN.md f18): GBufferRenderer::recordDraw into the context's visibility image, the two-phase sequence of
// GBufferRenderer::record over the rasteriser's OWN depth, the tables of the resolve (its entry points live with the
// traced G-buffer's in pt_gbuffer_passes.cpp), the per-pixel fragment lists of the rasterised transparent pass (DESIGN.md
// f20; its entry points live beside the forward opaque pass's), and the read-backs.  Kernels: pt_raster.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_context.hpp"
#include "pt_culling_state.hpp"
#include "pt_gbuffer_passes.hpp"
#include "pt_pass_support.hpp"
#include "pt_raster.hpp"

using namespace ppt;

namespace ppt
{

struct RasterPassState
{
    DeviceBuffer keys;     // the visibility image: one 64-bit key per pixel
    DeviceBuffer depth;    // its depth as floats, what the pyramid between the phases is made from
    DeviceBuffer queue;    // the large pass's records
    DeviceBuffer counters; // two RasterCounters: the draw that cleared, the draw on top of it
    DeviceBuffer guards, meshletBase;
    DeviceBuffer meshMeshletBase, meshletTriStart, triMap; // the resolve's meshlet-triangle -> geometry-triangle map
    std::vector<uint32_t> hostMeshMeshletBase, hostMeshletTriStart, hostTriMap;
    // the map of one mesh, kept across geometry generations: a mesh that streams in later leaves the others' as they are
    // (within a scene a mesh's bytes are identified by its metadata and info: meshes arrive once)
    struct MeshMap
    {
        prosper_GeometryMetadata md = {};
        prosper_pt_mesh_info info = {};
        bool valid = false;
        std::vector<uint32_t> counts; // triangles per meshlet
        std::vector<uint32_t> map;    // geometry triangle per meshlet triangle, meshlet after meshlet
    };
    std::vector<MeshMap> meshMaps;
    Pinned<uint8_t> tablesStaging; // what the copies into the two read: never rewritten before they have drained
    Fence tablesCopied;
    std::vector<RasterMeshGuard> hostGuards;
    std::vector<uint32_t> hostBase; // [drawInstanceCount + 1]
    // the tables above were made for this geometry generation
    const void *tablesGeometry = nullptr;
    uint32_t tablesInstalls = 0, tablesUpdates = 0;
    bool tablesValid = false, tablesDirty = true;
    bool anyMeshlets = false, anyMask = false;
    uint32_t width = 0, height = 0;
    bool imageValid = false;
    bool drawn[2] = {};
    Pinned<RasterCounters> countersHost; // both
    Fence countersDone;
    StageEvents<2> timing[2]; // the meshlet kernel | the large pass
    Fence done;               // behind the last call's kernels
    // the rasterised transparent pass's per-pixel lists: grow-only
    DeviceBuffer layerCounts;    // three words per pixel: the count, the scan's offset, the fill pass's cursor
    DeviceBuffer layerBlockSums; // the scan's block sums, then the total
    DeviceBuffer layerFragments; // the keys, list after list
    Pinned<uint32_t> layerTotalHost;
    Fence layerTotalCopied;
    uint32_t layerWidth = 0, layerHeight = 0, layerTotal = 0;
    bool layersValid = false;
};

// a new scene: the visibility image and the ordinal tables describe the old one
static void forget_raster(prosper_pt_ctx *ctx)
{
    if (!ctx->rasterPasses) return;
    RasterPassState &rs = *ctx->rasterPasses;
    rs.tablesValid = false;
    rs.meshMaps.clear(); // (a new scene's buffers are other buffers)
    rs.imageValid = false;
    rs.drawn[0] = rs.drawn[1] = false;
    rs.layersValid = false;
}

extern const PassModule kRasterPasses = pass_module<RasterPassState, &prosper_pt_ctx::rasterPasses>(forget_raster);

} // namespace ppt

namespace
{

constexpr uint32_t kMaxSide = 16384; // the guard band stays above 1

// The meshlet-triangle -> geometry-triangle table of every loaded mesh (evaluate_surface reads the shade record of a
// GEOMETRY triangle).  Per mesh, and only for the meshes whose metadata or info changed since their map was made (a new
// scene: all of them; a mesh that streamed in: that one): its geometry buffer is read back - the host keeps no mirror -,
// every meshlet's sections are checked against the mesh, and a meshlet triangle's three global vertex indices are looked
// up, rotation-invariant, among the index buffer's triangles; duplicates take the lowest match, no match is
// PROSPER_PT_ERR_SCENE.  The device is synchronised once, and only when some mesh has to be read.
int build_mesh_map(
    const char *what, size_t i, const prosper_GeometryMetadata &md, const prosper_pt_mesh_info &info, const std::vector<uint32_t> &words,
    RasterPassState::MeshMap &out)
{
    struct Key
    {
        uint32_t a, b, c, g;
        bool operator<(const Key &o) const { return a != o.a ? a < o.a : b != o.b ? b < o.b : c != o.c ? c < o.c : g < o.g; }
    };
    const auto canonical = [](uint32_t a, uint32_t b, uint32_t c, uint32_t g) {
        // the rotation that starts at the smallest index: the winding is kept
        if (b < a && b <= c) return Key{b, c, a, g};
        if (c < a && c < b) return Key{c, a, b, g};
        return Key{a, b, c, g};
    };
    const std::string mesh = std::string(what) + ": mesh " + std::to_string(i);
    const uint64_t wordCount = words.size();
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words.data());
    const uint16_t *halves = reinterpret_cast<const uint16_t *>(words.data());
    const bool shortIndices = md.usesShortIndices == 1u;
    const uint64_t indexUnits = shortIndices ? wordCount * 2u : wordCount;
    if ((uint64_t)md.indicesOffset + info.indexCount > indexUnits) return fail(PROSPER_PT_ERR_SCENE, mesh + ": indices leave its geometry buffer");
    if ((uint64_t)md.meshletsOffset + 4ull * info.meshletCount > wordCount) return fail(PROSPER_PT_ERR_SCENE, mesh + ": meshlets leave its geometry buffer");
    std::vector<Key> keys;
    keys.reserve(info.indexCount / 3u);
    for (uint32_t g = 0; g < info.indexCount / 3u; ++g)
    {
        uint32_t v[3];
        for (uint32_t k = 0; k < 3u; ++k)
            v[k] = shortIndices ? halves[md.indicesOffset + 3u * g + k] : words[md.indicesOffset + 3u * g + k];
        keys.push_back(canonical(v[0], v[1], v[2], g));
    }
    std::sort(keys.begin(), keys.end());
    out.counts.clear();
    out.map.clear();
    for (uint32_t ml = 0; ml < info.meshletCount; ++ml)
    {
        const uint32_t *h = words.data() + md.meshletsOffset + 4u * ml;
        const uint32_t vo = h[0], to = h[1], vc = std::min(h[2], kRasterMaxVertices), tc = std::min(h[3], kRasterMaxTriangles);
        const std::string where = mesh + " meshlet " + std::to_string(ml);
        if ((uint64_t)md.meshletVerticesOffset + vo + vc > indexUnits) return fail(PROSPER_PT_ERR_SCENE, where + ": meshletVertices leave its geometry buffer");
        if ((uint64_t)md.meshletTrianglesByteOffset + to + 3ull * tc > wordCount * 4u)
            return fail(PROSPER_PT_ERR_SCENE, where + ": meshletTriangles leave its geometry buffer");
        for (uint32_t t = 0; t < tc; ++t)
        {
            uint32_t v[3];
            for (uint32_t k = 0; k < 3u; ++k)
            {
                const uint32_t local = bytes[(size_t)md.meshletTrianglesByteOffset + to + 3u * t + k];
                if (local >= vc) return fail(PROSPER_PT_ERR_SCENE, where + ": a triangle names a vertex past the meshlet's");
                const size_t at = (size_t)md.meshletVerticesOffset + vo + local;
                v[k] = shortIndices ? halves[at] : words[at];
            }
            const Key want = canonical(v[0], v[1], v[2], 0u);
            const auto it = std::lower_bound(keys.begin(), keys.end(), want);
            if (it == keys.end() || it->a != want.a || it->b != want.b || it->c != want.c)
                return fail(PROSPER_PT_ERR_SCENE, where + ": triangle " + std::to_string(t) + " is not a triangle of the mesh's index buffer");
            out.map.push_back(it->g);
        }
        out.counts.push_back(tc);
    }
    out.md = md;
    out.info = info;
    out.valid = true;
    return PROSPER_PT_OK;
}

int make_triangle_map(
    prosper_pt_ctx *ctx, const char *what, std::vector<uint32_t> &meshBase, std::vector<uint32_t> &triStart, std::vector<uint32_t> &triMap)
{
    RasterPassState &rs = *ctx->rasterPasses;
    const GeometryState *gs = ctx->geometry;
    rs.meshMaps.resize(gs->infos.size());
    std::vector<std::vector<uint32_t>> buffers(gs->buffers.size());
    bool synchronised = false;
    for (size_t i = 0; i < gs->infos.size(); ++i)
    {
        RasterPassState::MeshMap &mm = rs.meshMaps[i];
        const prosper_pt_mesh_info &info = gs->infos[i];
        if (i >= gs->metadatas.size() || info.meshletCount == 0u)
        {
            mm.valid = false;
            continue;
        }
        const prosper_GeometryMetadata &md = gs->metadatas[i];
        if (mm.valid && std::memcmp(&mm.md, &md, sizeof md) == 0 && std::memcmp(&mm.info, &info, sizeof info) == 0) continue;
        mm.valid = false;
        if (md.bufferIndex >= gs->buffers.size() || md.bufferIndex >= gs->bufferBytes.size() || !gs->buffers[md.bufferIndex])
            return fail(PROSPER_PT_ERR_SCENE, std::string(what) + ": mesh " + std::to_string(i) + " has meshlets and no geometry buffer");
        std::vector<uint32_t> &words = buffers[md.bufferIndex];
        const uint64_t wordCount = gs->bufferBytes[md.bufferIndex] / 4u;
        if (words.empty() && wordCount)
        {
            PPT_HIP(hipSetDevice(ctx->device));
            if (!synchronised) PPT_HIP(hipDeviceSynchronize()); // (whatever still writes the buffers has finished)
            synchronised = true;
            words.resize((size_t)wordCount);
            PPT_HIP(hipMemcpy(words.data(), gs->buffers[md.bufferIndex], (size_t)wordCount * 4u, hipMemcpyDeviceToHost));
        }
        if (const int rc = build_mesh_map(what, i, md, info, words, mm)) return rc;
    }
    meshBase.assign(gs->infos.size() + 1u, 0u);
    triStart.assign(1u, 0u);
    triMap.clear();
    for (size_t i = 0; i < gs->infos.size(); ++i)
    {
        meshBase[i] = (uint32_t)(triStart.size() - 1u);
        const RasterPassState::MeshMap &mm = rs.meshMaps[i];
        if (!mm.valid) continue;
        triMap.insert(triMap.end(), mm.map.begin(), mm.map.end());
        uint32_t at = triStart.back();
        for (const uint32_t c : mm.counts) triStart.push_back(at += c);
    }
    meshBase[gs->infos.size()] = (uint32_t)(triStart.size() - 1u);
    if (triMap.empty()) triMap.push_back(0u);
    return PROSPER_PT_OK;
}

// The per-mesh guards and the per-draw-instance ordinal bases, once per geometry generation
int make_tables(prosper_pt_ctx *ctx, const char *what)
{
    RasterPassState &rs = *ctx->rasterPasses;
    const GeometryState *gs = ctx->geometry;
    if (rs.tablesValid && rs.tablesGeometry == gs && rs.tablesInstalls == gs->installs && rs.tablesUpdates == gs->meshUpdates)
        return PROSPER_PT_OK;
    const std::vector<prosper_MaterialData> &materials = ctx->materialState->materials;
    std::vector<RasterMeshGuard> guards(gs->infos.size() ? gs->infos.size() : 1u, RasterMeshGuard{});
    for (size_t i = 0; i < gs->infos.size() && i < gs->metadatas.size(); ++i)
    {
        const prosper_GeometryMetadata &md = gs->metadatas[i];
        if (gs->infos[i].meshletCount == 0u || md.bufferIndex >= gs->bufferBytes.size()) continue;
        const uint64_t words = gs->bufferBytes[md.bufferIndex] / 4u;
        guards[i].meshletCount = gs->infos[i].meshletCount;
        guards[i].vertexCount = gs->infos[i].vertexCount;
        guards[i].bufferWords = words > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)words;
    }
    // the ordinal of a draw instance's first meshlet: the prefix sum of the meshlet counts of the instances before it
    std::vector<uint32_t> base(gs->drawInstances.size() + 1u, 0u);
    uint64_t sum = 0;
    bool anyMask = false;
    for (size_t d = 0; d < gs->drawInstances.size(); ++d)
    {
        base[d] = (uint32_t)sum;
        const prosper_DrawInstance &di = gs->drawInstances[d];
        // every instance the generator can emit entries for takes its range, whatever its material: ordinals never collide
        // (a mesh with meshlets has indices - the culling calls check it -, so these are recordGenerateList's instances)
        if (di.meshIndex >= gs->infos.size()) continue;
        const prosper_pt_mesh_info &info = gs->infos[di.meshIndex];
        sum += info.meshletCount;
        if (sum >= kRasterMaxOrdinals)
            return fail(PROSPER_PT_ERR_SCENE, std::string(what) + ": the scene has 2^25 meshlets or more");
        anyMask = anyMask || (info.meshletCount != 0u && di.materialIndex < materials.size() &&
                              materials[di.materialIndex].alphaMode == PROSPER_ALPHA_MODE_MASK);
    }
    base[gs->drawInstances.size()] = (uint32_t)sum;
    std::vector<uint32_t> meshBase, triStart, triMap;
    if (const int rc = make_triangle_map(ctx, what, meshBase, triStart, triMap)) return rc;
    rs.hostMeshMeshletBase.swap(meshBase);
    rs.hostMeshletTriStart.swap(triStart);
    rs.hostTriMap.swap(triMap);
    rs.hostGuards.swap(guards);
    rs.hostBase.swap(base);
    rs.anyMeshlets = sum != 0;
    rs.anyMask = anyMask;
    rs.tablesGeometry = gs;
    rs.tablesInstalls = gs->installs;
    rs.tablesUpdates = gs->meshUpdates;
    rs.tablesValid = true;
    rs.tablesDirty = true;
    return PROSPER_PT_OK;
}

// everything a draw refuses, before anything is enqueued
int check_draw(prosper_pt_ctx *ctx, const char *what, uint32_t which, bool clear, const prosper_CameraUniforms *camera)
{
    int rc = check_scene(ctx, what);
    if (rc != PROSPER_PT_OK) return rc;
    if (!ctx->accel || !ctx->geometry || !ctx->materialState) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": no scene");
    if ((rc = make_tables(ctx, what)) != PROSPER_PT_OK) return rc;
    RasterPassState &rs = *ctx->rasterPasses;
    if (!rs.anyMeshlets) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": the scene has no meshlets");
    if (!ctx->cullingPasses->listValid[which])
        return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": the last culling calls did not produce this list");
    const uint32_t w = camera->resolution[0], h = camera->resolution[1];
    if (w == 0u || h == 0u || w > kMaxSide || h > kMaxSide)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": camera->resolution is empty or a side is above 16384");
    if (!clear && (!rs.imageValid || rs.width != w || rs.height != h))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": a draw without PROSPER_PT_RASTER_CLEAR needs a visibility image of camera->resolution");
    return PROSPER_PT_OK;
}

// What a raster pass over list `which` reads, on `s` behind the calls that still use the lists: the queue grown for the list,
// the tables of this geometry generation on the device, and the kernels' parameters but for the keys and the counters.
// The queue's count is NOT cleared here.
int prepare_raster_params(prosper_pt_ctx *ctx, uint32_t which, const prosper_CameraUniforms *camera, hipStream_t s, RasterParams *out)
{
    RasterPassState &rs = *ctx->rasterPasses;
    CullingPassState &st = *ctx->cullingPasses;
    int rc = PROSPER_PT_OK;
    const uint32_t w = camera->resolution[0], h = camera->resolution[1];
    // the queue holds every triangle of the list at most: 124 per entry, and no more than the meshes' index buffers hold
    const uint64_t triangleBound = std::min<uint64_t>((uint64_t)st.upperBound * kRasterMaxTriangles, st.totals.totalTriangleCount);
    const uint32_t queueCapacity = (uint32_t)std::max<uint64_t>(triangleBound, 1u);
    if ((rc = grow_to(rs.queue, 8u + 8u * (size_t)queueCapacity, s)) != PROSPER_PT_OK) return rc;
    const size_t guardBytes = rs.hostGuards.size() * sizeof(RasterMeshGuard), baseBytes = rs.hostBase.size() * sizeof(uint32_t);
    if (rs.guards.bytes < guardBytes || !rs.guards.ptr || rs.meshletBase.bytes < baseBytes || !rs.meshletBase.ptr) rs.tablesDirty = true;
    if ((rc = grow_to(rs.guards, guardBytes, s)) != PROSPER_PT_OK) return rc;
    if ((rc = grow_to(rs.meshletBase, baseBytes, s)) != PROSPER_PT_OK) return rc;
    if (rs.tablesDirty)
    {
        // through pinned memory of the state's own: the vectors may be remade (a new geometry generation) while a copy waits
        if ((rc = rs.tablesCopied.host_wait()) != PROSPER_PT_OK) return rc;
        if (rs.tablesStaging.bytes < guardBytes + baseBytes || !rs.tablesStaging.ptr)
            if ((rc = rs.tablesStaging.allocate(guardBytes + baseBytes)) != PROSPER_PT_OK) return rc;
        std::memcpy(rs.tablesStaging.ptr, rs.hostGuards.data(), guardBytes);
        std::memcpy(rs.tablesStaging.ptr + guardBytes, rs.hostBase.data(), baseBytes);
        PPT_HIP(hipMemcpyAsync(rs.guards.ptr, rs.tablesStaging.ptr, guardBytes, hipMemcpyHostToDevice, s));
        PPT_HIP(hipMemcpyAsync(rs.meshletBase.ptr, rs.tablesStaging.ptr + guardBytes, baseBytes, hipMemcpyHostToDevice, s));
        if ((rc = rs.tablesCopied.record(s)) != PROSPER_PT_OK) return rc;
        // the resolve's map (read from the vectors: copied synchronously here, once per geometry generation)
        if ((rc = grow_to(rs.meshMeshletBase, rs.hostMeshMeshletBase.size() * 4u, s)) != PROSPER_PT_OK) return rc;
        if ((rc = grow_to(rs.meshletTriStart, rs.hostMeshletTriStart.size() * 4u, s)) != PROSPER_PT_OK) return rc;
        if ((rc = grow_to(rs.triMap, rs.hostTriMap.size() * 4u, s)) != PROSPER_PT_OK) return rc;
        PPT_HIP(hipStreamSynchronize(s));
        PPT_HIP(hipMemcpy(rs.meshMeshletBase.ptr, rs.hostMeshMeshletBase.data(), rs.hostMeshMeshletBase.size() * 4u, hipMemcpyHostToDevice));
        PPT_HIP(hipMemcpy(rs.meshletTriStart.ptr, rs.hostMeshletTriStart.data(), rs.hostMeshletTriStart.size() * 4u, hipMemcpyHostToDevice));
        PPT_HIP(hipMemcpy(rs.triMap.ptr, rs.hostTriMap.data(), rs.hostTriMap.size() * 4u, hipMemcpyHostToDevice));
        rs.tablesDirty = false;
    }
    RasterParams p = {};
    p.geometryBuffers = ctx->scene.geometryBuffers;
    p.metadatas = ctx->scene.geometryMetadatas;
    p.drawInstances = ctx->scene.drawInstances;
    p.transforms = ctx->scene.modelInstanceTransforms;
    p.guards = rs.guards.as<RasterMeshGuard>();
    p.meshletBase = rs.meshletBase.as<uint32_t>();
    p.drawInstanceCount = std::min<uint32_t>(ctx->scene.drawInstanceCount, (uint32_t)(rs.hostBase.size() - 1u));
    p.meshCount = (uint32_t)std::min(ctx->geometry->infos.size(), rs.hostGuards.size());
    p.modelInstanceCount = ctx->scene.modelInstanceCount;
    p.list = st.lists[which].as<uint32_t>();
    p.capacity = st.capacity;
    p.queue = rs.queue.as<uint32_t>();
    p.queueCapacity = queueCapacity;
    // the MASK discard reads what the resolve's surface code reads: the scene, the pixel ray's camera terms, the LOD state
    // (from the materials as they are NOW: prosper_pt_update_materials may have made one MASK since the tables were made)
    p.anyMask = 0u;
    {
        const GeometryState *gs = ctx->geometry;
        const std::vector<prosper_MaterialData> &materials = ctx->materialState->materials;
        for (const prosper_DrawInstance &di : gs->drawInstances)
            if (di.meshIndex < gs->infos.size() && gs->infos[di.meshIndex].meshletCount != 0u && di.materialIndex < materials.size() &&
                materials[di.materialIndex].alphaMode == PROSPER_ALPHA_MODE_MASK)
            {
                p.anyMask = 1u;
                break;
            }
    }
    p.scene = ctx->scene;
    set_camera_ray_params(p.ray, camera);
    p.ray.width = w;
    p.ray.height = h;
    p.ray.localWidth = w;
    p.ray.stripeCount = 1;
    p.ray.frameCount = 1;
    p.currentJitter[0] = camera->currentJitter[0];
    p.currentJitter[1] = camera->currentJitter[1];
    bool lodEnabled = false;
    gbuffer_texture_lod(ctx, &lodEnabled, &p.lodBias);
    p.mips = ctx->textureMips;
    p.lod = lodEnabled && ctx->textureMips ? 1u : 0u;
    p.meshMeshletBase = rs.meshMeshletBase.as<uint32_t>();
    p.meshletTriStart = rs.meshletTriStart.as<uint32_t>();
    p.triMap = rs.triMap.as<uint32_t>();
    std::memcpy(p.view.worldToCamera, &camera->worldToCamera, 64);
    std::memcpy(p.view.cameraToClip, &camera->cameraToClip, 64);
    p.view.width = w;
    p.view.height = h;
    p.view.guardBand = raster_guard_band(w, h);

    *out = p;
    return PROSPER_PT_OK;
}

int draw(prosper_pt_ctx *ctx, const char *what, uint32_t which, bool clear, const prosper_CameraUniforms *camera, hipStream_t s)
{
    int rc = check_draw(ctx, what, which, clear, camera);
    if (rc != PROSPER_PT_OK) return rc;
    RasterPassState &rs = *ctx->rasterPasses;
    CullingPassState &st = *ctx->cullingPasses;
    PPT_HIP(hipSetDevice(ctx->device));
    if ((rc = flush_scene_updates(ctx, s, s)) != PROSPER_PT_OK) return rc;
    // calls on other streams may still use the lists or the image: `s` takes up behind them before anything grows
    if ((rc = st.done.wait(s)) != PROSPER_PT_OK) return rc;
    if ((rc = rs.done.wait(s)) != PROSPER_PT_OK) return rc;
    const uint32_t w = camera->resolution[0], h = camera->resolution[1];
    const size_t pixels = (size_t)w * h;
    const uint32_t slot = clear ? 0u : 1u;
    if (clear)
    {
        rs.imageValid = false;
        rs.drawn[0] = rs.drawn[1] = false;
        if ((rc = grow_to(rs.keys, pixels * 8u, s)) != PROSPER_PT_OK) return rc;
        if ((rc = grow_to(rs.depth, pixels * 4u, s)) != PROSPER_PT_OK) return rc;
    }
    else
        rs.drawn[1] = false;
    if ((rc = grow_to(rs.counters, 2u * sizeof(RasterCounters), s)) != PROSPER_PT_OK) return rc;
    RasterParams p = {};
    if ((rc = prepare_raster_params(ctx, which, camera, s, &p)) != PROSPER_PT_OK) return rc;
    p.keys = rs.keys.as<unsigned long long>();
    p.counters = rs.counters.as<RasterCounters>() + slot;
    if (!rs.countersHost.ptr)
    {
        if ((rc = rs.countersHost.allocate(2u * sizeof(RasterCounters))) != PROSPER_PT_OK) return rc;
        std::memset(rs.countersHost.ptr, 0, 2u * sizeof(RasterCounters));
    }
    if ((rc = rs.timing[slot].create()) != PROSPER_PT_OK) return rc;

    if (clear) PPT_HIP(hipMemsetAsync(rs.keys.ptr, 0, pixels * 8u, s));
    PPT_HIP(hipMemsetAsync(rs.queue.ptr, 0, 8u, s));
    PPT_HIP(hipMemsetAsync(rs.counters.as<RasterCounters>() + slot, 0, sizeof(RasterCounters), s));

    PPT_HIP(hipEventRecord(rs.timing[slot].events[0], s));
    launch_raster_meshlets(p, s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(rs.timing[slot].events[1], s));
    launch_raster_large(p, s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(rs.timing[slot].events[2], s));
    PPT_HIP(hipMemcpyAsync(rs.countersHost.ptr + slot, p.counters, sizeof(RasterCounters), hipMemcpyDeviceToHost, s));
    if ((rc = rs.countersDone.record(s)) != PROSPER_PT_OK) return rc;
    if ((rc = rs.done.record(s)) != PROSPER_PT_OK) return rc;
    if ((rc = st.done.record(s)) != PROSPER_PT_OK) return rc; // (the next culling call clears the list this draw reads)
    rs.width = w;
    rs.height = h;
    rs.imageValid = true;
    rs.drawn[slot] = true;
    return mark_versions_read(ctx, s);
}

// the image's depth as floats, then its pyramid into `slot`
int depth_pyramid(prosper_pt_ctx *ctx, uint32_t slot, hipStream_t s)
{
    RasterPassState &rs = *ctx->rasterPasses;
    launch_raster_depth(rs.keys.as<unsigned long long>(), rs.depth.as<float>(), rs.width, rs.height, s);
    PPT_HIP(hipGetLastError());
    return prosper_pt_hiz_downsample(ctx, slot, rs.depth.as<float>(), 1u, rs.width, rs.height, s);
}

} // namespace

namespace ppt
{

int raster_resolve_tables(prosper_pt_ctx *ctx, const char *what, uint32_t width, uint32_t height, hipStream_t s, RasterResolveTables *out)
{
    RasterPassState &rs = *ctx->rasterPasses;
    if (!rs.imageValid || !rs.tablesValid || rs.tablesDirty)
        return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": nothing has been drawn on this scene");
    if (rs.width != width || rs.height != height)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": camera->resolution differs from the visibility image's extent");
    const GeometryState *gs = ctx->geometry;
    if (rs.tablesGeometry != gs || !gs || rs.tablesInstalls != gs->installs || rs.tablesUpdates != gs->meshUpdates)
        return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": the scene's geometry changed since the image was drawn: nothing has been drawn on this geometry");
    if (const int rc = rs.done.wait(s)) return rc;
    out->keys = rs.keys.as<unsigned long long>();
    out->meshletBase = rs.meshletBase.as<uint32_t>();
    out->drawInstanceCount = std::min<uint32_t>(ctx->scene.drawInstanceCount, (uint32_t)(rs.hostBase.size() - 1u));
    out->meshMeshletBase = rs.meshMeshletBase.as<uint32_t>();
    out->meshCount = (uint32_t)(rs.hostMeshMeshletBase.size() - 1u);
    out->meshletTriStart = rs.meshletTriStart.as<uint32_t>();
    out->triMap = rs.triMap.as<uint32_t>();
    return PROSPER_PT_OK;
}

int raster_resolve_enqueued(prosper_pt_ctx *ctx, hipStream_t s) { return ctx->rasterPasses->done.record(s); }

int raster_layers_check(prosper_pt_ctx *ctx, const char *what, uint32_t which, bool listNeeded, const prosper_CameraUniforms *camera)
{
    if (which != PROSPER_PT_DRAW_LIST_GENERATED && which != PROSPER_PT_DRAW_LIST_FIRST_PHASE && which != PROSPER_PT_DRAW_LIST_SECOND_PHASE)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the list is GENERATED, FIRST_PHASE or SECOND_PHASE");
    if (!ctx || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (listNeeded) return check_draw(ctx, what, which, true, camera);
    // check_draw but for the list, which the culling call ahead produces
    int rc = check_scene(ctx, what);
    if (rc != PROSPER_PT_OK) return rc;
    if (!ctx->accel || !ctx->geometry || !ctx->materialState) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": no scene");
    if ((rc = make_tables(ctx, what)) != PROSPER_PT_OK) return rc;
    if (!ctx->rasterPasses->anyMeshlets) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": the scene has no meshlets");
    const uint32_t w = camera->resolution[0], h = camera->resolution[1];
    if (w == 0u || h == 0u || w > kMaxSide || h > kMaxSide)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": camera->resolution is empty or a side is above 16384");
    return PROSPER_PT_OK;
}

int raster_layers_build(
    prosper_pt_ctx *ctx, const char *what, uint32_t which, const prosper_CameraUniforms *camera, const float *depth, hipStream_t s,
    hipEvent_t *events, RasterLayerLists *lists, RasterResolveTables *tables)
{
    int rc = raster_layers_check(ctx, what, which, true, camera);
    if (rc != PROSPER_PT_OK) return rc;
    RasterPassState &rs = *ctx->rasterPasses;
    CullingPassState &st = *ctx->cullingPasses;
    PPT_HIP(hipSetDevice(ctx->device));
    // calls on other streams may still use the lists, the queue or the fragment lists: `s` takes up behind them
    if ((rc = st.done.wait(s)) != PROSPER_PT_OK) return rc;
    if ((rc = rs.done.wait(s)) != PROSPER_PT_OK) return rc;
    const uint32_t w = camera->resolution[0], h = camera->resolution[1];
    const size_t pixels = (size_t)w * h;
    const uint32_t blocks = raster_scan_blocks(pixels);
    rs.layersValid = false;
    if ((rc = grow_to(rs.layerCounts, pixels * 12u, s)) != PROSPER_PT_OK) return rc;
    if ((rc = grow_to(rs.layerBlockSums, ((size_t)blocks + 1u) * 4u, s)) != PROSPER_PT_OK) return rc;
    if (!rs.layerTotalHost.ptr && (rc = rs.layerTotalHost.allocate(sizeof(uint32_t))) != PROSPER_PT_OK) return rc;
    RasterParams p = {};
    if ((rc = prepare_raster_params(ctx, which, camera, s, &p)) != PROSPER_PT_OK) return rc;
    RasterLayerTargets t = {};
    t.depth = depth;
    t.counts = rs.layerCounts.as<uint32_t>();
    uint32_t *offsets = t.counts + pixels;
    t.offsets = offsets;
    t.cursor = t.counts + 2u * pixels;
    uint32_t *total = rs.layerBlockSums.as<uint32_t>() + blocks;

    // counts and cursors (the offsets between them are all written by the scan)
    PPT_HIP(hipMemsetAsync(t.counts, 0, pixels * 4u, s));
    PPT_HIP(hipMemsetAsync(t.cursor, 0, pixels * 4u, s));
    PPT_HIP(hipMemsetAsync(rs.queue.ptr, 0, 8u, s));
    PPT_HIP(hipEventRecord(events[0], s));
    launch_raster_layers(p, t, false, s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(events[1], s));
    launch_raster_layer_scan(t.counts, offsets, rs.layerBlockSums.as<uint32_t>(), total, pixels, s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(events[2], s));
    // the one host wait of the pass: the total sizes the fragment buffer
    PPT_HIP(hipMemcpyAsync(rs.layerTotalHost.ptr, total, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = rs.layerTotalCopied.record(s)) != PROSPER_PT_OK) return rc;
    if ((rc = rs.layerTotalCopied.host_wait()) != PROSPER_PT_OK) return rc;
    const uint32_t fragments = *rs.layerTotalHost.ptr;
    if (fragments != 0u)
    {
        if ((rc = grow_to(rs.layerFragments, (size_t)fragments * 8u, s)) != PROSPER_PT_OK) return rc;
        t.fragments = rs.layerFragments.as<unsigned long long>();
        t.capacity = fragments;
        PPT_HIP(hipMemsetAsync(rs.queue.ptr, 0, 8u, s));
        launch_raster_layers(p, t, true, s);
        PPT_HIP(hipGetLastError());
    }
    PPT_HIP(hipEventRecord(events[3], s));
    if ((rc = rs.done.record(s)) != PROSPER_PT_OK) return rc;
    if ((rc = st.done.record(s)) != PROSPER_PT_OK) return rc; // (the next culling call clears the list these passes read)
    rs.layerWidth = w;
    rs.layerHeight = h;
    rs.layerTotal = fragments;
    rs.layersValid = true;
    lists->counts = t.counts;
    lists->offsets = offsets;
    lists->fragments = rs.layerFragments.as<unsigned long long>();
    lists->total = fragments;
    tables->keys = nullptr; // (the lists hold the keys)
    tables->meshletBase = rs.meshletBase.as<uint32_t>();
    tables->drawInstanceCount = std::min<uint32_t>(ctx->scene.drawInstanceCount, (uint32_t)(rs.hostBase.size() - 1u));
    tables->meshMeshletBase = rs.meshMeshletBase.as<uint32_t>();
    tables->meshCount = (uint32_t)(rs.hostMeshMeshletBase.size() - 1u);
    tables->meshletTriStart = rs.meshletTriStart.as<uint32_t>();
    tables->triMap = rs.triMap.as<uint32_t>();
    return PROSPER_PT_OK;
}

} // namespace ppt

extern "C" {

int prosper_pt_raster_meshlets(prosper_pt_ctx *ctx, uint32_t which, uint32_t flags, const prosper_CameraUniforms *camera, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (which != PROSPER_PT_DRAW_LIST_GENERATED && which != PROSPER_PT_DRAW_LIST_FIRST_PHASE && which != PROSPER_PT_DRAW_LIST_SECOND_PHASE)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_raster_meshlets: the list is GENERATED, FIRST_PHASE or SECOND_PHASE");
    if (flags & ~(uint32_t)PROSPER_PT_RASTER_CLEAR) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_raster_meshlets: unknown flags");
    if (!ctx || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_raster_meshlets: null argument");
    return draw(ctx, "prosper_pt_raster_meshlets", which, (flags & PROSPER_PT_RASTER_CLEAR) != 0u, camera, static_cast<hipStream_t>(stream));
}

int prosper_pt_raster_visibility(prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, void *stream)
{
    const char *what = "prosper_pt_raster_visibility";
    if (!ctx || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    const uint32_t w = camera->resolution[0], h = camera->resolution[1];
    if (w <= 1u || h <= 1u || w > 4096u || h > 4096u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the sides of camera->resolution are above 1 and at most 4096 (the pyramid's)");
    CullingPassState &st = *ctx->cullingPasses;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // what the draws would refuse is refused before the first phase replaces the lists
    int rc = check_scene(ctx, what);
    if (rc != PROSPER_PT_OK) return rc;
    if (!ctx->accel || !ctx->geometry || !ctx->materialState) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": no scene");
    if ((rc = make_tables(ctx, what)) != PROSPER_PT_OK) return rc;
    if (!ctx->rasterPasses->anyMeshlets) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": the scene has no meshlets");
    // the pyramid the previous call kept, if it is of this extent
    uint32_t previous = PROSPER_PT_NO_HIZ;
    if (st.keptHiz >= 0 && st.hiz[st.keptHiz].valid && st.hiz[st.keptHiz].sourceWidth == w && st.hiz[st.keptHiz].sourceHeight == h)
        previous = (uint32_t)st.keptHiz;
    // From here on a failure is a runtime error (HIP, memory).  The draw lists and the image are then whatever the steps
    // so far left, as after any failed culling call; the kept pyramid survives: this frame's pyramids go into the OTHER
    // slot, so the previous one is intact and stays the next call's previous.
    const int32_t keptBefore = st.keptHiz;
    const uint32_t current = previous == PROSPER_PT_NO_HIZ ? 0u : 1u - previous;
    rc = prosper_pt_cull_meshlets_first_phase(ctx, PROSPER_PT_CULL_MODE_OPAQUE, camera, previous, stream);
    if (rc == PROSPER_PT_OK) rc = draw(ctx, what, PROSPER_PT_DRAW_LIST_FIRST_PHASE, true, camera, s);
    if (rc == PROSPER_PT_OK && previous != PROSPER_PT_NO_HIZ)
    {
        // what was hidden behind the previous frame's depth is tested against THIS frame's, as far as it is drawn
        rc = depth_pyramid(ctx, current, s);
        if (rc == PROSPER_PT_OK) rc = prosper_pt_cull_meshlets_second_phase(ctx, camera, current, stream);
        if (rc == PROSPER_PT_OK) rc = draw(ctx, what, PROSPER_PT_DRAW_LIST_SECOND_PHASE, false, camera, s);
    }
    if (rc == PROSPER_PT_OK) rc = depth_pyramid(ctx, current, s);
    if (rc == PROSPER_PT_OK) rc = ctx->rasterPasses->done.record(s);
    st.keptHiz = rc == PROSPER_PT_OK ? (int32_t)current : (previous != PROSPER_PT_NO_HIZ ? keptBefore : -1);
    return rc;
}

int prosper_pt_raster_release_preserved(prosper_pt_ctx *ctx)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_raster_release_preserved: null argument");
    ctx->cullingPasses->keptHiz = -1; // the next sequence has no previous pyramid: one phase, everything in the frustum drawn
    return PROSPER_PT_OK;
}

int prosper_pt_read_raster_visibility(prosper_pt_ctx *ctx, uint32_t *ids, float *depth, size_t pixels, void *stream)
{
    if (!ctx || (!ids && !depth)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_raster_visibility: null argument");
    RasterPassState &rs = *ctx->rasterPasses;
    if (!rs.imageValid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_raster_visibility: nothing has been drawn on this scene");
    const size_t need = (size_t)rs.width * rs.height;
    if (pixels < need) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_raster_visibility: destination too small");
    std::vector<unsigned long long> keys(need);
    if (const int rc = read_back(ctx, static_cast<hipStream_t>(stream), {{keys.data(), rs.keys.ptr, need * 8u}}, &rs.done)) return rc;
    const std::vector<uint32_t> &base = rs.hostBase;
    for (size_t i = 0; i < need; ++i)
    {
        const unsigned long long key = keys[i];
        if (depth) std::memcpy(depth + i, reinterpret_cast<const char *>(&key) + 4, 4); // the high word (little endian)
        if (!ids) continue;
        uint32_t *o = ids + 3u * i;
        if (key == 0ull)
        {
            o[0] = o[1] = o[2] = 0xFFFFFFFFu;
            continue;
        }
        const uint32_t low = ~(uint32_t)key, ordinal = low >> 7;
        // the last draw instance whose base is not above the ordinal and that has meshlets
        const size_t d = (size_t)(std::upper_bound(base.begin(), base.end() - 1, ordinal) - base.begin()) - 1u;
        o[0] = (uint32_t)d;
        o[1] = ordinal - base[d];
        o[2] = low & 127u;
    }
    return PROSPER_PT_OK;
}

int prosper_pt_read_raster_fragments(
    prosper_pt_ctx *ctx, uint32_t *counts, size_t pixels, prosper_pt_raster_fragment *fragments, size_t capacity, uint64_t *total, void *stream)
{
    const char *what = "prosper_pt_read_raster_fragments";
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    RasterPassState &rs = *ctx->rasterPasses;
    if (!rs.layersValid) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": the rasterised transparent pass has not run on this scene");
    const size_t need = (size_t)rs.layerWidth * rs.layerHeight;
    if (total) *total = rs.layerTotal;
    if ((counts || fragments) && pixels != need) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": pixel count differs from the pass's");
    if (fragments && capacity < rs.layerTotal) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": room for fewer fragments than the lists hold");
    if (!counts && !fragments) return PROSPER_PT_OK;
    std::vector<uint32_t> hostCounts(need);
    std::vector<unsigned long long> keys(rs.layerTotal);
    const int rc = read_back(
        ctx, static_cast<hipStream_t>(stream),
        {{hostCounts.data(), rs.layerCounts.ptr, need * 4u}, {fragments ? keys.data() : nullptr, rs.layerFragments.ptr, (size_t)rs.layerTotal * 8u}}, &rs.done);
    if (rc != PROSPER_PT_OK) return rc;
    if (counts) std::memcpy(counts, hostCounts.data(), need * 4u);
    if (!fragments) return PROSPER_PT_OK;
    const std::vector<uint32_t> &base = rs.hostBase;
    size_t at = 0;
    for (size_t i = 0; i < need; ++i)
    {
        const size_t n = hostCounts[i];
        if (at + n > keys.size()) return fail(PROSPER_PT_ERR_SCENE, std::string(what) + ": the counts exceed the scan's total");
        std::sort(keys.begin() + at, keys.begin() + at + n, [](unsigned long long a, unsigned long long b) { return a > b; }); // nearest first
        for (size_t k = at; k < at + n; ++k)
        {
            const unsigned long long key = keys[k];
            const uint32_t low = ~(uint32_t)key, ordinal = low >> 7;
            const size_t d = (size_t)(std::upper_bound(base.begin(), base.end() - 1, ordinal) - base.begin()) - 1u;
            prosper_pt_raster_fragment &f = fragments[k];
            f.drawInstance = (uint32_t)d;
            f.meshlet = ordinal - base[d];
            f.triangle = low & 127u;
            std::memcpy(&f.depth, reinterpret_cast<const char *>(&key) + 4, 4); // the high word (little endian)
        }
        at += n;
    }
    return PROSPER_PT_OK;
}

int prosper_pt_get_raster_info(prosper_pt_ctx *ctx, prosper_pt_raster_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_raster_info: null argument");
    RasterPassState &rs = *ctx->rasterPasses;
    if (!rs.imageValid || !rs.drawn[0]) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_get_raster_info: nothing has been drawn on this scene");
    PPT_HIP(hipSetDevice(ctx->device));
    prosper_pt_raster_info info = {};
    info.width = rs.width;
    info.height = rs.height;
    if (!rs.countersDone.passed())
    {
        *out = info; // (the extent is known; the counts stay zero)
        return PROSPER_PT_NOT_READY;
    }
    for (uint32_t k = 0; k < 2u; ++k)
    {
        if (!rs.drawn[k]) continue;
        const RasterCounters &c = rs.countersHost.ptr[k];
        prosper_pt_raster_draw_info &d = info.draw[k];
        d.valid = 1u;
        d.triangles = c.triangles;
        d.culledBackface = c.culledBackface;
        d.culledZeroArea = c.culledZeroArea;
        d.culledOutside = c.culledOutside;
        d.clipped = c.clipped;
        d.queued = c.queued;
        d.fragments = c.fragments;
        d.queueOverflow = c.queueOverflow;
        float ms[2] = {};
        if (const int rc = rs.timing[k].elapsed(ms)) return rc; // (behind the fence that has passed: no wait)
        d.meshletsMs = ms[0];
        d.largeMs = ms[1];
    }
    *out = info;
    return PROSPER_PT_OK;
}

} // extern "C"
