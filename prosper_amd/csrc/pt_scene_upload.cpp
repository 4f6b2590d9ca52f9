// pt_scene_upload.cpp — prosper_pt_upload_scene: the scene and acceleration-structure upload the passes depend on
// (src/scene/World.cpp:468-536,585-802), and what frees a scene again.
#include "pt_scene_updates.hpp"

#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <vector>

#include "pt_animation.hpp"
#include "pt_geometry.hpp"
#include "pt_kernels.hpp"
#include "pt_materials.hpp"
#include "pt_scene.hpp"

namespace ppt
{

void delete_retired_accel(prosper_pt_ctx *ctx)
{
    for (AccelState *old : ctx->retiredAccel) delete old;
    ctx->retiredAccel.clear();
}

void free_scene(prosper_pt_ctx *ctx)
{
    discard_mesh_build(ctx);
    delete_retired_accel(ctx);
    for (auto &a : ctx->sceneAllocations) (void)hipFree(a.ptr);
    ctx->sceneAllocations.clear();
    delete ctx->accel; // its device arrays are in the list above
    ctx->accel = nullptr;
    delete ctx->lights;
    ctx->lights = nullptr;
    delete ctx->materialState;
    ctx->materialState = nullptr;
    delete ctx->geometry;
    ctx->geometry = nullptr;
    ctx->dTransforms = nullptr;
    ctx->sceneBytes = 0;
    ctx->haveScene = false;
    ctx->scene = DeviceScene{};
    ctx->textureMips = nullptr;
}

namespace
{

// Everything the kernels index with is range-checked here, so a malformed view can only fail the
// upload, never fault the GPU.
int validate_scene(const prosper_pt_scene_view *v, bool mips)
{
    if (v->struct_size != sizeof(prosper_pt_scene_view))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "scene view struct_size mismatch");
    if (v->geometryBufferCount && (!v->geometryBuffers || !v->geometryBufferByteSizes))
        return fail(PROSPER_PT_ERR_SCENE, "geometry buffers missing");
    if (v->geometryBufferCount > PROSPER_PT_MAX_GEOMETRY_BUFFERS)
        return fail(PROSPER_PT_ERR_SCENE, "more than PROSPER_PT_MAX_GEOMETRY_BUFFERS geometry buffers");
    if (v->meshCount && (!v->geometryMetadatas || !v->meshInfos)) return fail(PROSPER_PT_ERR_SCENE, "mesh tables missing");
    if (v->drawInstanceCount && !v->drawInstances) return fail(PROSPER_PT_ERR_SCENE, "draw instances missing");
    if (v->modelInstanceCount && !v->modelInstanceTransforms) return fail(PROSPER_PT_ERR_SCENE, "transforms missing");
    if (v->materialCount == 0 || !v->materials) return fail(PROSPER_PT_ERR_SCENE, "materials missing (index 0 is required)");
    if (v->samplerCount == 0 || !v->samplers) return fail(PROSPER_PT_ERR_SCENE, "samplers missing (index 0 is required)");
    if (v->textureCount && !v->textures) return fail(PROSPER_PT_ERR_SCENE, "textures missing");
    if (!v->directionalLight || !v->pointLights || !v->spotLights) return fail(PROSPER_PT_ERR_SCENE, "light buffers missing");
    if (v->pointLights->count > PROSPER_MAX_POINT_LIGHT_COUNT || v->spotLights->count > PROSPER_MAX_SPOT_LIGHT_COUNT)
        return fail(PROSPER_PT_ERR_SCENE, "light count exceeds 1024");
    if (v->skybox.texels && v->skybox.faceSize == 0) return fail(PROSPER_PT_ERR_SCENE, "skybox face size is zero");

    for (uint32_t i = 0; i < v->textureCount; ++i)
    {
        const int rc = validate_texture(v->textures[i], i, mips);
        if (rc != PROSPER_PT_OK) return rc;
    }
    for (uint32_t i = 0; i < v->samplerCount; ++i)
    {
        const prosper_pt_sampler_desc &s = v->samplers[i];
        if (s.magFilter > PROSPER_PT_FILTER_LINEAR || s.wrapS > PROSPER_PT_WRAP_CLAMP_TO_EDGE ||
            s.wrapT > PROSPER_PT_WRAP_CLAMP_TO_EDGE)
            return fail(PROSPER_PT_ERR_SCENE, "sampler " + std::to_string(i) + " is invalid");
    }
    for (uint32_t i = 0; i < v->materialCount; ++i)
    {
        const prosper_MaterialData &m = v->materials[i];
        const uint32_t ts[3] = {m.baseColorTextureSampler, m.metallicRoughnessTextureSampler, m.normalTextureSampler};
        for (uint32_t k = 0; k < 3; ++k)
        {
            const uint32_t tex = ts[k] & 0xFFFFFFu, smp = ts[k] >> 24;
            if (tex > 0 && (tex >= v->textureCount || smp >= v->samplerCount))
                return fail(PROSPER_PT_ERR_SCENE, "material " + std::to_string(i) + " references a missing texture/sampler");
        }
        if (m.alphaMode > PROSPER_ALPHA_MODE_BLEND) return fail(PROSPER_PT_ERR_SCENE, "material alpha mode invalid");
    }
    for (uint32_t i = 0; i < v->meshCount; ++i)
    {
        const prosper_GeometryMetadata &m = v->geometryMetadatas[i];
        const prosper_pt_mesh_info &info = v->meshInfos[i];
        const std::string name = "mesh " + std::to_string(i);
        if (m.bufferIndex == PROSPER_PT_ABSENT) continue; // not loaded yet (prosper_pt_update_meshes): nothing else of it is read
        if (m.bufferIndex >= v->geometryBufferCount) return fail(PROSPER_PT_ERR_SCENE, name + ": bufferIndex out of range");
        if (info.materialIndex >= v->materialCount) return fail(PROSPER_PT_ERR_SCENE, name + ": materialIndex out of range");
        if (info.indexCount % 3 != 0) return fail(PROSPER_PT_ERR_SCENE, name + ": indexCount is not a multiple of 3");
        const uint64_t words = v->geometryBufferByteSizes[m.bufferIndex] / 4;
        if (m.indicesOffset == PROSPER_PT_ABSENT || m.positionsOffset == PROSPER_PT_ABSENT)
            return fail(PROSPER_PT_ERR_SCENE, name + ": indices/positions are required");
        const uint64_t indexEndWords = m.usesShortIndices == 1 ? ((uint64_t)m.indicesOffset + info.indexCount + 1) / 2
                                                               : (uint64_t)m.indicesOffset + info.indexCount;
        if (indexEndWords > words) return fail(PROSPER_PT_ERR_SCENE, name + ": indices run past the geometry buffer");
        if ((uint64_t)m.positionsOffset + 2ull * info.vertexCount > words)
            return fail(PROSPER_PT_ERR_SCENE, name + ": positions run past the geometry buffer");
        const uint32_t attrs[3] = {m.normalsOffset, m.tangentsOffset, m.texCoord0sOffset};
        for (uint32_t k = 0; k < 3; ++k)
            if (attrs[k] != PROSPER_PT_ABSENT && (uint64_t)attrs[k] + info.vertexCount > words)
                return fail(PROSPER_PT_ERR_SCENE, name + ": attribute stream runs past the geometry buffer");
        const void *buffer = v->geometryBuffers[m.bufferIndex];
        for (uint32_t k = 0; k < info.indexCount; ++k)
        {
            const uint32_t idx = m.usesShortIndices == 1 ? (uint32_t) static_cast<const uint16_t *>(buffer)[m.indicesOffset + k]
                                                          : static_cast<const uint32_t *>(buffer)[m.indicesOffset + k];
            if (idx >= info.vertexCount) return fail(PROSPER_PT_ERR_SCENE, name + ": vertex index out of range");
        }
    }
    for (uint32_t i = 0; i < v->drawInstanceCount; ++i)
    {
        const prosper_DrawInstance &d = v->drawInstances[i];
        if (d.meshIndex >= v->meshCount || d.materialIndex >= v->materialCount || d.modelInstanceIndex >= v->modelInstanceCount)
            return fail(PROSPER_PT_ERR_SCENE, "draw instance " + std::to_string(i) + " references a missing mesh/material/transform");
    }
    return PROSPER_PT_OK;
}

double seconds_since(std::chrono::steady_clock::time_point t)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

// ---- the steps of upload_scene, in the order it takes them ----

// bindless geometry buffers + pointer table, with the mirrors a later prosper_pt_update_meshes works from
int upload_geometry_tables(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v)
{
    DeviceScene &s = ctx->scene;
    int rc = PROSPER_PT_OK;
    GeometryState *gs = new (std::nothrow) GeometryState();
    if (!gs) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "out of host memory");
    ctx->geometry = gs;
    gs->metadatas.assign(v->geometryMetadatas, v->geometryMetadatas + v->meshCount);
    gs->infos.assign(v->meshInfos, v->meshInfos + v->meshCount);
    gs->drawInstances.assign(v->drawInstances, v->drawInstances + v->drawInstanceCount);
    std::vector<const void *> bufferPtrs(std::max<size_t>(v->geometryBufferCount, PROSPER_PT_MAX_GEOMETRY_BUFFERS), nullptr);
    void *d = nullptr;
    // (fixed sizes: while a mesh build runs the calling thread and the worker both index these, neither may move them)
    gs->buffers.assign(bufferPtrs.size(), nullptr);
    gs->bufferBytes.assign(bufferPtrs.size(), 0);
    for (uint32_t i = 0; i < v->geometryBufferCount; ++i)
    {
        if ((rc = upload(ctx, v->geometryBuffers[i], (size_t)v->geometryBufferByteSizes[i], &d))) return rc;
        bufferPtrs[i] = d;
        gs->buffers[i] = d;
        gs->bufferBytes[i] = v->geometryBufferByteSizes[i];
    }
    if ((rc = upload(ctx, bufferPtrs.data(), bufferPtrs.size() * sizeof(void *), &d))) return rc;
    gs->dBufferTable = static_cast<const void **>(d);
    s.geometryBuffers = gs->dBufferTable;
    if ((rc = upload(ctx, v->geometryMetadatas, sizeof(prosper_GeometryMetadata) * v->meshCount, &d))) return rc;
    gs->dMetadatas = static_cast<prosper_GeometryMetadata *>(d);
    s.geometryMetadatas = gs->dMetadatas;
    if ((rc = upload(ctx, v->drawInstances, sizeof(prosper_DrawInstance) * v->drawInstanceCount, &d))) return rc;
    s.drawInstances = static_cast<const prosper_DrawInstance *>(d);
    if ((rc = upload(ctx, v->modelInstanceTransforms, sizeof(prosper_ModelInstanceTransforms) * v->modelInstanceCount, &d)))
        return rc;
    s.modelInstanceTransforms = static_cast<const prosper_ModelInstanceTransforms *>(d);
    if ((rc = upload(ctx, v->materials, sizeof(prosper_MaterialData) * v->materialCount, &d))) return rc;
    s.materials = static_cast<const prosper_MaterialData *>(d);
    if ((rc = upload(ctx, v->samplers, sizeof(prosper_pt_sampler_desc) * v->samplerCount, &d))) return rc;
    s.samplers = static_cast<const prosper_pt_sampler_desc *>(d);
    s.drawInstanceCount = v->drawInstanceCount;
    s.modelInstanceCount = v->modelInstanceCount;
    return PROSPER_PT_OK;
}

// The world triangles first: the host-side hierarchy build - the longest step of an upload - runs on the host's threads
// while the calling thread goes on with textures, packs, sky, lights and the alpha tables (begin_geometry); the flatten
// kernel runs again in finish_geometry for the shading and any-hit records (the same world triangles a second time).
// With site UPLOAD of prosper_pt_set_gpu_hierarchy_sites there is no host build: finish_geometry touches the
// triangles once and builds on the device.
int begin_scene_geometry(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v, GeometryTarget &target, GeometryJob &job)
{
    DeviceScene &s = ctx->scene;
    int rc = PROSPER_PT_OK;
    AccelState *acc = new (std::nothrow) AccelState();
    if (!acc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "out of host memory");
    ctx->accel = acc;
    acc->transforms.assign(v->modelInstanceTransforms, v->modelInstanceTransforms + v->modelInstanceCount);
    ctx->dTransforms = const_cast<prosper_ModelInstanceTransforms *>(s.modelInstanceTransforms);
    acc->dTransformsV[0] = ctx->dTransforms;
    if ((rc = enqueue_instance_scales(ctx, acc, 0, ctx->dTransforms, v->modelInstanceCount, nullptr))) return rc;
    PPT_HIP(hipStreamSynchronize(nullptr));
    target = context_target(ctx);
    // (site UPLOAD: the first tree from the GPU builder - begin_geometry then only lays the triangles out, and everything
    //  else happens in finish_geometry, in one pass over the geometry)
    target.gpuTree = (ctx->gpuHierarchySites & PROSPER_PT_GPU_BUILD_SITE_UPLOAD) != 0;
    GeometryLayout layout;
    if ((rc = layout_geometry(*ctx->geometry, v->materials, layout))) return rc;
    return begin_geometry(ctx, target, layout, nullptr, job);
}

// textures: one allocation each (256-B aligned by hipMalloc), re-laid out in 8x4-texel tiles of one cache line each
// (pt_scene.hpp DeviceTexture) by a kernel - until round 4 the host did that a texel at a time, 40 ms for
// S-sponza-class - + descriptor table.  The tables a later prosper_pt_update_textures / _materials changes are mirrored
// in ctx->materialState (pt_materials.cpp).
int upload_textures_and_packs(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v)
{
    DeviceScene &s = ctx->scene;
    int rc = PROSPER_PT_OK;
    void *d = nullptr;
    MaterialState *ms = new (std::nothrow) MaterialState();
    if (!ms) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "out of host memory");
    ctx->materialState = ms;
    ms->materials.assign(v->materials, v->materials + v->materialCount);
    ms->samplers.assign(v->samplers, v->samplers + v->samplerCount);
    std::vector<DeviceTexture> &textures = ms->textures;
    textures.assign(v->textureCount ? v->textureCount : 1, DeviceTexture{nullptr, 0u, 0u, 0u, 0u});
    uint64_t texelBytes = 0;
    // mip chains (PROSPER_PT_CREATE_TEXTURE_MIPS): built right behind each level 0, before a packed material's may be freed
    const bool withMips = (ctx->flags & PROSPER_PT_CREATE_TEXTURE_MIPS) != 0;
    const std::vector<uint8_t> baseColour = base_colour_textures(v->materials, v->materialCount, textures.size());
    if (withMips) ms->mips.assign(textures.size(), DeviceTextureMips{nullptr, 1u, 0u, {}});
    {
        size_t stagingBytes = 0;
        for (uint32_t i = 0; i < v->textureCount; ++i) stagingBytes = std::max(stagingBytes, texture_staging_bytes(v->textures[i], withMips));
        void *staging = nullptr;
        if (stagingBytes) PPT_HIP(hipMalloc(&staging, stagingBytes));
        for (uint32_t i = 0; i < v->textureCount && rc == PROSPER_PT_OK; ++i)
        {
            texelBytes += (uint64_t)v->textures[i].width * v->textures[i].height * 4u;
            // (one staging area, one stream: the copy of texture i + 1 queues behind the kernel that reads texture i)
            rc = create_device_texture(
                ctx, v->textures[i], staging, nullptr, &textures[i], nullptr, withMips ? &ms->mips[i] : nullptr, baseColour[i] != 0);
            if (withMips && rc == PROSPER_PT_OK) ms->mipTexelBytes += mip_texel_bytes(textures[i].width, textures[i].height, ms->mips[i].levelCount);
        }
        const hipError_t e = hipDeviceSynchronize();
        if (staging) (void)hipFree(staging);
        if (rc != PROSPER_PT_OK) return rc;
        PPT_HIP(e);
    }
    ms->texelBytes = texelBytes;
    // beyond the 8 x 4 MB of L2 the texels of a hit come from the Infinity Cache or HBM: overlap their fetches
    // (debug option batchedTextures = 0 / 1 forces either path: same pixels, tested)
    s.batchedTextures = texel_set_is_big(texelBytes) ? 1u : 0u;
    if (ctx->debug.batchedTextures >= 0) s.batchedTextures = ctx->debug.batchedTextures ? 1u : 0u;
    // material texture packs (pt_scene.hpp MaterialPack): base / MR / normal interleaved per texel where a material's
    // three textures share extent and sampler.  Debug option noTexturePacks keeps every material unpacked.
    // Compact packs where the texels outgrow the caches (the threshold of the batched loads above): on a small texture set
    // the bytes are not what the shade kernel waits for, and two kinds of pack in one wave cost a divergent branch
    // (FlightHelmet fixture: +1 % on the step).  Debug option widePacks = 1 / 0 forces the 16-byte / the compact pack.
    std::vector<MaterialPack> &packs = ms->packs;
    packs.assign(v->materialCount, MaterialPack{nullptr, 0u, 0u, 0u, 0u});
    uint32_t packedMaterials = 0;
    bool widePacks = !texel_set_is_big(texelBytes);
    if (ctx->debug.widePacks >= 0) widePacks = ctx->debug.widePacks != 0;
    for (uint32_t i = 0; i < v->materialCount; ++i)
    {
        if ((rc = build_material_pack(ctx, v->materials[i], textures, ctx->debug.noTexturePacks != 0, widePacks, nullptr, &packs[i]))) return rc;
        packedMaterials += packs[i].texels ? 1u : 0u;
    }
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipDeviceSynchronize());
    if ((rc = upload(ctx, packs.data(), packs.size() * sizeof(MaterialPack), &d))) return rc;
    s.materialPacks = static_cast<const MaterialPack *>(d);
    ctx->packedMaterials = packedMaterials;
    ms->packedMaterials = packedMaterials;
    return PROSPER_PT_OK;
}

// A texture that only packed materials use is never sampled by itself again (sample_material takes the pack): its
// own copy goes - half of a packed scene's texel memory.  What keeps a texture: an unpacked material, or the any-hit
// of a MASK / BLEND material, which reads the base colour's alpha out of the texture itself.
void free_pack_only_textures(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v)
{
    std::vector<DeviceTexture> &textures = ctx->materialState->textures;
    const std::vector<MaterialPack> &packs = ctx->materialState->packs;
    std::vector<uint8_t> needed(textures.size(), 0);
    needed[0] = 1;
    for (uint32_t i = 0; i < v->materialCount; ++i)
    {
        const prosper_MaterialData &m = v->materials[i];
        const uint32_t t3[3] = {m.baseColorTextureSampler & 0xFFFFFFu, m.metallicRoughnessTextureSampler & 0xFFFFFFu,
                                m.normalTextureSampler & 0xFFFFFFu};
        if (packs[i].texels == nullptr)
            for (uint32_t t : t3) needed[t] = 1;
        if (m.alphaMode != PROSPER_ALPHA_MODE_OPAQUE) needed[t3[0]] = 1;
    }
    // (a texture no material samples yet stays: it is what a streamed-in material will point at)
    std::vector<uint8_t> sampled(textures.size(), 0);
    for (uint32_t i = 0; i < v->materialCount; ++i)
    {
        const prosper_MaterialData &m = v->materials[i];
        sampled[m.baseColorTextureSampler & 0xFFFFFFu] = sampled[m.metallicRoughnessTextureSampler & 0xFFFFFFu] =
            sampled[m.normalTextureSampler & 0xFFFFFFu] = 1;
    }
    for (uint32_t i = 1; i < v->textureCount; ++i)
        if (!needed[i] && sampled[i] && textures[i].texels)
        {
            device_free(ctx, textures[i].texels);
            textures[i].texels = nullptr;
        }
}

// the descriptor tables of the textures that stayed, and of their mip chains
int upload_texture_tables(prosper_pt_ctx *ctx)
{
    MaterialState *ms = ctx->materialState;
    int rc = PROSPER_PT_OK;
    void *d = nullptr;
    if ((rc = upload(ctx, ms->textures.data(), ms->textures.size() * sizeof(DeviceTexture), &d))) return rc;
    ctx->scene.textures = static_cast<const DeviceTexture *>(d);
    if (ctx->flags & PROSPER_PT_CREATE_TEXTURE_MIPS)
    {
        if ((rc = upload(ctx, ms->mips.data(), ms->mips.size() * sizeof(DeviceTextureMips), &d))) return rc;
        ctx->textureMips = static_cast<const DeviceTextureMips *>(d);
    }
    return PROSPER_PT_OK;
}

// lights: one block (directional, point list, spot list), the first of up to three versions
int upload_lights(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v)
{
    LightState *ls = new (std::nothrow) LightState();
    if (ls) ls->mirror = new (std::nothrow) LightBlock();
    if (!ls || !ls->mirror)
    {
        delete ls;
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "out of host memory");
    }
    ctx->lights = ls;
    ls->mirror->directional = *v->directionalLight;
    ls->mirror->points = *v->pointLights;
    ls->mirror->spots = *v->spotLights;
    void *d = nullptr;
    if (const int rc = upload(ctx, ls->mirror, sizeof(LightBlock), &d)) return rc;
    ls->dBlocks[0] = static_cast<LightBlock *>(d);
    point_scene_at_lights(ctx->scene, ls->dBlocks[0]);
    return PROSPER_PT_OK;
}

int upload_skybox(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v)
{
    DeviceScene &s = ctx->scene;
    s.skybox = nullptr;
    s.skyboxFaceSize = 0;
    if (v->skybox.texels)
    {
        // kept with a one-texel seamless border per face (pt_device.hpp fetch_cube_rgb); the plain copy is only the source
        int rc = PROSPER_PT_OK;
        void *d = nullptr;
        const size_t bytes = 6ull * v->skybox.faceSize * v->skybox.faceSize * 4u * sizeof(uint16_t);
        const size_t n2 = (size_t)v->skybox.faceSize + 2u;
        void *plain = nullptr;
        if ((rc = upload(ctx, v->skybox.texels, bytes, &plain))) return rc;
        if ((rc = device_alloc(ctx, 6ull * n2 * n2 * 4u * sizeof(uint16_t), &d))) return rc;
        launch_border_skybox(static_cast<const uint16_t *>(plain), v->skybox.faceSize, d, nullptr);
        PPT_HIP(hipGetLastError());
        PPT_HIP(hipDeviceSynchronize());
        device_free(ctx, plain);
        s.skybox = static_cast<const uint16_t *>(d);
        s.skyboxFaceSize = v->skybox.faceSize;
    }
    return PROSPER_PT_OK;
}

// What the any-hit shader reads of the materials: one record per material and the materials' alpha bounds (pt_scene.hpp
// AlphaMaterial); the 32-byte records per non-opaque triangle (AlphaTriangle) are finish_geometry's.
int upload_alpha_tables(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v)
{
    MaterialState *ms = ctx->materialState;
    int rc = PROSPER_PT_OK;
    void *d = nullptr;
    std::vector<AlphaMaterial> &alphaMaterials = ms->alphaMaterials;
    alphaMaterials.assign(v->materialCount ? v->materialCount : 1, AlphaMaterial{});
    uint64_t boundBytes = 0;
    for (uint32_t i = 0; i < v->materialCount; ++i)
    {
        uint64_t bytes = 0;
        if ((rc = build_alpha_material(ctx, v->materials[i], ms->textures, ms->samplers, nullptr, &alphaMaterials[i], &bytes))) return rc;
        boundBytes += bytes;
    }
    PPT_HIP(hipGetLastError());
    if ((rc = upload(ctx, alphaMaterials.data(), alphaMaterials.size() * sizeof(AlphaMaterial), &d))) return rc;
    ctx->scene.alphaMaterials = static_cast<const AlphaMaterial *>(d);
    ctx->alphaBoundBytes = boundBytes;
    ms->alphaBoundBytes = boundBytes;
    // layout of the table block of a later version (pt_materials.cpp flush_pending_materials)
    auto align16 = [](size_t n) { return (n + 15u) & ~(size_t)15u; };
    ms->packsOffset = align16(ms->materials.size() * sizeof(prosper_MaterialData));
    ms->alphaOffset = ms->packsOffset + align16(ms->packs.size() * sizeof(MaterialPack));
    ms->texturesOffset = ms->alphaOffset + align16(ms->alphaMaterials.size() * sizeof(AlphaMaterial));
    ms->mipsOffset = ms->texturesOffset + align16(ms->textures.size() * sizeof(DeviceTexture));
    ms->blockBytes = ms->mipsOffset + align16(ms->mips.size() * sizeof(DeviceTextureMips));
    return PROSPER_PT_OK;
}

} // namespace

int upload_scene(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v)
{
    DeviceScene &s = ctx->scene;
    int rc = PROSPER_PT_OK;
    ctx->stats = prosper_pt_scene_stats{};
    const auto tUpload = std::chrono::steady_clock::now();
    if ((rc = upload_geometry_tables(ctx, v))) return rc;
    // ---- acceleration structure (replaces buildNextBlas/buildCurrentTlas, World.cpp:585-802): begun here, finished below,
    //      the host's build running beside everything in between ----
    GeometryJob job;
    GeometryTarget target;
    if ((rc = begin_scene_geometry(ctx, v, target, job))) return rc;

    const auto tTextures = std::chrono::steady_clock::now();
    if ((rc = upload_textures_and_packs(ctx, v))) return rc;
    free_pack_only_textures(ctx, v);
    if ((rc = upload_texture_tables(ctx))) return rc;
    const double textureSeconds = seconds_since(tTextures);

    if ((rc = upload_lights(ctx, v))) return rc;
    s.pointLightCount = v->pointLights->count;
    s.spotLightCount = v->spotLights->count;
    s.materialCount = v->materialCount;
    if ((rc = upload_skybox(ctx, v))) return rc;
    if ((rc = upload_alpha_tables(ctx, v))) return rc;

    if ((rc = finish_geometry(ctx, target, job))) return rc;
    ctx->stats.deviceBytes = ctx->sceneBytes;
    ctx->stats.alphaBoundBytes = ctx->alphaBoundBytes;
    ctx->stats.textureSeconds = textureSeconds;
    ctx->stats.uploadSeconds = seconds_since(tUpload);
    return PROSPER_PT_OK;
}

} // namespace ppt

using namespace ppt;

extern "C" {

int prosper_pt_upload_scene(prosper_pt_ctx *ctx, const prosper_pt_scene_view *scene)
{
    if (!ctx || !scene) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_upload_scene: null argument");
    int rc = validate_scene(scene, (ctx->flags & PROSPER_PT_CREATE_TEXTURE_MIPS) != 0);
    if (rc != PROSPER_PT_OK) return rc;
    for (const PassModule *m : kPassModules)
        if (m->forget_scene) m->forget_scene(ctx);
    PPT_HIP(hipSetDevice(ctx->device));
    discard_mesh_build(ctx); // (a worker may still be launching)
    PPT_HIP(hipDeviceSynchronize());
    forget_animations(ctx); // (its read-back with it: the new scene's mirrors are the new scene's)
    free_scene(ctx);
    rc = upload_scene(ctx, scene);
    if (rc != PROSPER_PT_OK)
    {
        free_scene(ctx);
        return rc;
    }
    ctx->haveScene = true;
    return PROSPER_PT_OK;
}

} // extern "C"
