// pt_materials.cpp — see pt_materials.hpp.  C-ABI: prosper_pt_update_textures, prosper_pt_update_materials
// (include/prosper_pt/prosper_pt.h, "incremental adoption").
//
// prosper streams a scene in: the meshes first, then the images a few per frame, and a material switches from its
// placeholder (the default material with the real alpha mode, WorldData.cpp:817-826) to the real one once its three images
// are there (WorldData.cpp:2208-2239); the whole material buffer of the next frame is rewritten when that happened
// (WorldData.cpp:568-586), descriptors of new images are written as they arrive (:2182-2206).  Nothing of that rebuilds an
// acceleration structure.  Here the same two events cost what they touch: a texture update copies and re-tiles the new
// texels (on a stream of its own, beside the frames in flight), a material update rebuilds that material's texture pack and
// alpha bounds, and the next render switches to a new version of the four small tables at the head of its own chain.
#include "pt_materials.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "pt_bc7_encode.hpp"
#include "pt_kernels.hpp"
#include "pt_pass_support.hpp"
#include "pt_scene_updates.hpp"
#include "pt_texture_mips.hpp"

namespace ppt
{

namespace
{

bool is_bc7(const prosper_pt_texture_desc &t) { return t.format == PROSPER_PT_FORMAT_BC7_UNORM; }

// bytes of level `l` as the caller holds it (src/utils/Dds.cpp:100-135: BC7 in whole 16-byte blocks)
size_t level_source_bytes(const prosper_pt_texture_desc &t, uint32_t l)
{
    const size_t w = std::max(t.width >> l, 1u), h = std::max(t.height >> l, 1u);
    return is_bc7(t) ? (w / 4u) * (h / 4u) * 16u : w * h * 4u;
}

// levels the caller supplies in `texels`
uint32_t supplied_levels(const prosper_pt_texture_desc &t, bool mips) { return mips && t.mipLevelCount > 1u ? t.mipLevelCount : 1u; }

size_t source_bytes(const prosper_pt_texture_desc &t, bool mips)
{
    size_t bytes = 0;
    for (uint32_t l = 0; l < supplied_levels(t, mips); ++l) bytes += level_source_bytes(t, l);
    return bytes;
}

size_t tiled_level_words(uint32_t w, uint32_t h)
{
    return (size_t)((w + kTexTileW - 1u) / kTexTileW) * ((h + kTexTileH - 1u) / kTexTileH) * (kTexTileW * kTexTileH);
}

} // namespace

size_t texture_staging_bytes(const prosper_pt_texture_desc &t, bool mips)
{
    return (source_bytes(t, mips) + 255u) & ~(size_t)255u;
}

int validate_texture(const prosper_pt_texture_desc &t, uint32_t index, bool mips)
{
    if (!t.texels || t.width == 0 || t.height == 0 || t.format > PROSPER_PT_FORMAT_BC7_UNORM)
        return fail(PROSPER_PT_ERR_SCENE, "texture " + std::to_string(index) + " is invalid");
    if (t.format == PROSPER_PT_FORMAT_BC7_UNORM && (t.width % 4u != 0u || t.height % 4u != 0u))
        return fail(PROSPER_PT_ERR_SCENE, "BC7 texture " + std::to_string(index) + " is not a whole number of 4x4 blocks");
    if (!mips) return PROSPER_PT_OK;
    const uint32_t count = mip_level_count(t.width, t.height);
    if (count > kMaxMipLevels)
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "texture " + std::to_string(index) + ": a mip chain of more than 16 levels");
    if (t.mipLevelCount > count)
        return fail(
            PROSPER_PT_ERR_SCENE, "texture " + std::to_string(index) + ": mipLevelCount " + std::to_string(t.mipLevelCount) +
                                      " exceeds the " + std::to_string(count) + " levels of prosper's chain for its extent");
    if (is_bc7(t))
        for (uint32_t l = 1; l < supplied_levels(t, true); ++l)
            if ((std::max(t.width >> l, 1u) % 4u) != 0u || (std::max(t.height >> l, 1u) % 4u) != 0u)
                return fail(
                    PROSPER_PT_ERR_SCENE,
                    "BC7 texture " + std::to_string(index) + ": mip level " + std::to_string(l) + " is not a whole number of 4x4 blocks");
    return PROSPER_PT_OK;
}

uint64_t mip_texel_bytes(uint32_t width, uint32_t height, uint32_t levelCount)
{
    uint64_t bytes = 0;
    for (uint32_t l = 1; l < levelCount; ++l) bytes += (uint64_t)std::max(width >> l, 1u) * std::max(height >> l, 1u) * 4u;
    return bytes;
}

std::vector<uint8_t> base_colour_textures(const prosper_MaterialData *materials, size_t materialCount, size_t textureCount)
{
    std::vector<uint8_t> srgb(textureCount, 0);
    for (size_t i = 0; i < materialCount; ++i)
    {
        const uint32_t t = materials[i].baseColorTextureSampler & 0xFFFFFFu;
        if (t > 0 && t < textureCount) srgb[t] = 1;
    }
    return srgb;
}

namespace
{

// Levels >= 1 of `t`'s chain behind its level 0 `dt` (already enqueued on `stream`, its source levels in `staging`).
int build_texture_mips(
    prosper_pt_ctx *ctx, const prosper_pt_texture_desc &t, const DeviceTexture &dt, const void *staging, hipStream_t stream, bool srgb,
    DeviceTextureMips *out)
{
    DeviceTextureMips m{};
    const uint32_t supplied = supplied_levels(t, true);
    m.levelCount = supplied > 1u ? supplied : mip_level_count(t.width, t.height);
    m.srgb = supplied > 1u ? 0u : (srgb ? 1u : 0u);
    if (m.levelCount == 1u)
    {
        *out = m;
        return PROSPER_PT_OK;
    }
    size_t words = 0;
    for (uint32_t l = 1; l < m.levelCount; ++l)
    {
        m.wordOffset[l] = (uint32_t)words;
        words += tiled_level_words(std::max(t.width >> l, 1u), std::max(t.height >> l, 1u));
    }
    if (words >= (1ull << 32)) return fail(PROSPER_PT_ERR_UNSUPPORTED, "a texture's mip chain exceeds 2^32 texels");
    void *d = nullptr;
    const int rc = device_alloc(ctx, words * 4u, &d);
    if (rc != PROSPER_PT_OK) return rc;
    m.texels = static_cast<const uint8_t *>(d);
    PPT_HIP(hipMemsetAsync(d, 0, words * 4u, stream)); // (tile padding)
    size_t source = level_source_bytes(t, 0);
    for (uint32_t l = 1; l < m.levelCount; ++l)
    {
        const uint32_t w = std::max(t.width >> l, 1u), h = std::max(t.height >> l, 1u);
        uint32_t *level = static_cast<uint32_t *>(d) + m.wordOffset[l];
        if (supplied > 1u)
        {
            const uint8_t *src = static_cast<const uint8_t *>(staging) + source;
            if (is_bc7(t))
                launch_decode_bc7(src, w, h, (w + kTexTileW - 1u) / kTexTileW, level, stream);
            else
                launch_retile_rgba8(src, w, h, (w + kTexTileW - 1u) / kTexTileW, level, stream);
            source += level_source_bytes(t, l);
        }
        else
        {
            const uint32_t pw = std::max(t.width >> (l - 1u), 1u), ph = std::max(t.height >> (l - 1u), 1u);
            const void *parent = l == 1u ? static_cast<const void *>(dt.texels) : static_cast<uint32_t *>(d) + m.wordOffset[l - 1u];
            launch_generate_mip(parent, pw, ph, level, w, h, srgb, stream);
        }
    }
    PPT_HIP(hipGetLastError());
    *out = m;
    return PROSPER_PT_OK;
}

} // namespace

int create_device_texture(
    prosper_pt_ctx *ctx, const prosper_pt_texture_desc &t, void *staging, hipStream_t stream, DeviceTexture *out, void *pinned,
    DeviceTextureMips *mipsOut, bool srgb)
{
    const uint32_t tilesX = (t.width + kTexTileW - 1u) / kTexTileW, tilesY = (t.height + kTexTileH - 1u) / kTexTileH;
    const size_t tiledBytes = (size_t)tilesX * tilesY * (kTexTileW * kTexTileH) * 4u;
    void *d = nullptr;
    const int rc = device_alloc(ctx, tiledBytes, &d);
    if (rc != PROSPER_PT_OK) return rc;
    // the caller's bytes - level 0, and with it the levels it supplies - go up as they are
    const size_t srcBytes = source_bytes(t, mipsOut != nullptr);
    const void *src = t.texels;
    if (pinned)
    {
        std::memcpy(pinned, t.texels, srcBytes);
        src = pinned;
    }
    PPT_HIP(hipMemcpyAsync(staging, src, srcBytes, hipMemcpyHostToDevice, stream));
    if (t.format == PROSPER_PT_FORMAT_BC7_UNORM)
    {
        // a kernel decodes the blocks into the tiles (pt_bc7.hpp)
        PPT_HIP(hipMemsetAsync(d, 0, tiledBytes, stream));
        launch_decode_bc7(staging, t.width, t.height, tilesX, d, stream);
    }
    else
    {
        // 8 x 4-texel tiles of one cache line each (pt_scene.hpp DeviceTexture), laid out by a kernel
        launch_retile_rgba8(staging, t.width, t.height, tilesX, d, stream);
    }
    PPT_HIP(hipGetLastError());
    *out = DeviceTexture{static_cast<const uint8_t *>(d), t.width, t.height, tilesX, 0u};
    if (mipsOut)
    {
        const int mrc = build_texture_mips(ctx, t, *out, staging, stream, srgb, mipsOut);
        if (mrc != PROSPER_PT_OK)
        {
            // the texture failed as a whole: its level 0 does not stay in the scene
            device_free(ctx, d);
            *out = DeviceTexture{nullptr, 0u, 0u, 0u, 0u};
        }
        return mrc;
    }
    return PROSPER_PT_OK;
}

int build_material_pack(
    prosper_pt_ctx *ctx, const prosper_MaterialData &m, const std::vector<DeviceTexture> &textures, bool noPacks, bool wide,
    hipStream_t stream, MaterialPack *out)
{
    *out = MaterialPack{nullptr, 0u, 0u, 0u, 0u};
    const uint32_t tb = m.baseColorTextureSampler & 0xFFFFFFu, tm = m.metallicRoughnessTextureSampler & 0xFFFFFFu,
                   tn = m.normalTextureSampler & 0xFFFFFFu;
    const uint32_t sb = m.baseColorTextureSampler >> 24, sm = m.metallicRoughnessTextureSampler >> 24, sn = m.normalTextureSampler >> 24;
    if (noPacks || tb == 0 || tm == 0 || tn == 0 || sb != sm || sb != sn) return PROSPER_PT_OK;
    const DeviceTexture &b = textures[tb], &r = textures[tm], &n = textures[tn];
    if (!b.texels || !r.texels || !n.texels) return PROSPER_PT_OK;
    if (b.width != r.width || b.width != n.width || b.height != r.height || b.height != n.height) return PROSPER_PT_OK;
    if (b.width < 8u || b.height < 8u) return PROSPER_PT_OK; // tiny placeholder textures: nothing to gain
    MaterialPack pk;
    pk.width = b.width;
    pk.height = b.height;
    pk.tilesPerRow = (b.width + kPackTileW - 1u) / kPackTileW;
    // an OPAQUE material never reads base.a: the 8-byte texel
    const bool compact = m.alphaMode == PROSPER_ALPHA_MODE_OPAQUE && !wide;
    pk.sampler = sb | (compact ? kPackCompactBit : 0u);
    const size_t texelCount = (size_t)pk.tilesPerRow * kPackTileW * (((size_t)b.height + kPackTileH - 1u) / kPackTileH) * kPackTileH;
    void *d = nullptr;
    const int rc = device_alloc(ctx, texelCount * (compact ? sizeof(uint2) : sizeof(uint4)), &d);
    if (rc != PROSPER_PT_OK) return rc;
    pk.texels = d;
    launch_pack_material_textures(b, r, n, pk, stream);
    PPT_HIP(hipGetLastError());
    *out = pk;
    return PROSPER_PT_OK;
}

int build_alpha_material(
    prosper_pt_ctx *ctx, const prosper_MaterialData &m, const std::vector<DeviceTexture> &textures,
    const std::vector<prosper_pt_sampler_desc> &samplers, hipStream_t stream, AlphaMaterial *out, uint64_t *boundBytes)
{
    AlphaMaterial am{};
    am.factorA = m.baseColorFactor.w;
    am.cutoff = m.alphaCutoff;
    am.bits = m.alphaMode & 3u;
    *boundBytes = 0;
    const uint32_t tex = m.baseColorTextureSampler & 0xFFFFFFu;
    if (m.alphaMode != PROSPER_ALPHA_MODE_OPAQUE && tex != 0)
    {
        const DeviceTexture &t = textures[tex];
        const prosper_pt_sampler_desc &sd = samplers[m.baseColorTextureSampler >> 24];
        if (!t.texels)
            return fail(PROSPER_PT_ERR_UNSUPPORTED, "the base-colour texture of a MASK / BLEND material has no texels of its own on the device");
        if (t.width > 0xFFFFu || t.height > 0xFFFFu)
            return fail(PROSPER_PT_ERR_UNSUPPORTED, "base-colour texture of a MASK / BLEND material exceeds 65535 texels a side");
        am.texels = t.texels;
        am.width = (uint16_t)t.width;
        am.height = (uint16_t)t.height;
        am.bits |= (sd.wrapS & 3u) << 2 | (sd.wrapT & 3u) << 4 | (sd.magFilter == PROSPER_PT_FILTER_NEAREST ? 64u : 0u);
        // cells of 2 x 2 texels: the table is an eighth of the texture (8 KB for 128^2: it lives in the L1 / L2
        // the texels would have been read through); coarser for textures whose table would pass 2 MB
        uint32_t shift = 1;
        while (((uint64_t)(t.width >> shift) + 1u) * ((t.height >> shift) + 1u) * 2u > (2ull << 20)) ++shift;
        if (ctx->debug.alphaCellShift >= 0) shift = (uint32_t)std::min(15, ctx->debug.alphaCellShift);
        const bool factorOk = std::isfinite(m.baseColorFactor.w) && m.baseColorFactor.w >= 0.0f;
        if (!ctx->debug.noAlphaBounds && factorOk)
        {
            const uint32_t cellsX = (t.width + (1u << shift) - 1u) >> shift, cellsY = (t.height + (1u << shift) - 1u) >> shift;
            void *d = nullptr;
            const int rc = device_alloc(ctx, (size_t)cellsX * cellsY * 2u, &d);
            if (rc != PROSPER_PT_OK) return rc;
            launch_build_alpha_bounds(t, sd.wrapS, sd.wrapT, m.baseColorFactor.w, shift, static_cast<uint16_t *>(d), stream);
            PPT_HIP(hipGetLastError());
            am.bounds = static_cast<const uint16_t *>(d);
            am.bits |= shift << 8;
            *boundBytes = (uint64_t)cellsX * cellsY * 2u;
        }
    }
    *out = am;
    return PROSPER_PT_OK;
}

namespace
{

bool wide_packs(const prosper_pt_ctx *ctx)
{
    // compact packs where the texels outgrow the caches; debug option widePacks = 1 / 0 forces either kind
    if (ctx->debug.widePacks >= 0) return ctx->debug.widePacks != 0;
    return !texel_set_is_big(ctx->materialState->texelBytes);
}

} // namespace

size_t allocation_bytes(prosper_pt_ctx *ctx, const void *p)
{
    const std::lock_guard<std::mutex> lock(ctx->allocMutex);
    for (const DeviceAllocation &a : ctx->sceneAllocations)
        if (a.ptr == p) return a.bytes;
    return 0;
}

// `p` was replaced by an update: nothing new will read it, a frame in flight still may
void retire(prosper_pt_ctx *ctx, const void *p)
{
    if (!p) return;
    MaterialState *ms = ctx->materialState;
    ms->retired.push_back(p);
    ms->retiredBytes += allocation_bytes(ctx, p);
}

// Frees what has been retired once it is worth a device synchronisation (a material slider dragged for a thousand frames
// must not grow the scene without bound; a streamed scene never gets here: it retires a few placeholder texels).
int collect_retired(prosper_pt_ctx *ctx)
{
    MaterialState *ms = ctx->materialState;
    if (ms->retiredBytes < MaterialState::kRetireBytes) return PROSPER_PT_OK;
    PPT_HIP(hipDeviceSynchronize());
    for (const void *p : ms->retired) device_free(ctx, p);
    ms->retired.clear();
    ms->retiredBytes = 0;
    // (the device is idle: the generations a geometry build replaced can go with their events and pinned staging)
    delete_retired_accel(ctx);
    return PROSPER_PT_OK;
}

namespace
{

bool same_pack_inputs(const prosper_MaterialData &a, const prosper_MaterialData &b)
{
    return a.baseColorTextureSampler == b.baseColorTextureSampler && a.metallicRoughnessTextureSampler == b.metallicRoughnessTextureSampler &&
           a.normalTextureSampler == b.normalTextureSampler && a.alphaMode == b.alphaMode;
}

// The pack and the alpha material of material `i` again, from the mirrors, on the upload stream.  `previous`: the
// material's entry before this update (nullptr: its textures' TEXELS changed) - what does not depend on what changed is
// kept: the pack on a material's textures and samplers, the alpha bounds on the base-colour texture, its sampler and
// baseColorFactor.a.
int rebuild_material(prosper_pt_ctx *ctx, uint32_t i, const prosper_MaterialData *previous)
{
    MaterialState *ms = ctx->materialState;
    const prosper_MaterialData &m = ms->materials[i];
    int rc;
    const bool wide = wide_packs(ctx);
    const bool packKindKept = ms->packs[i].texels == nullptr || (((ms->packs[i].sampler & kPackCompactBit) == 0u) == (wide || m.alphaMode != PROSPER_ALPHA_MODE_OPAQUE));
    if (!(previous && same_pack_inputs(*previous, m) && packKindKept))
    {
        MaterialPack pk;
        if ((rc = build_material_pack(ctx, m, ms->textures, ctx->debug.noTexturePacks != 0, wide, ms->uploadStream.get(), &pk))) return rc;
        if ((pk.texels != nullptr) != (ms->packs[i].texels != nullptr)) ms->packedMaterials += pk.texels ? 1u : ~0u;
        retire(ctx, ms->packs[i].texels);
        ms->packs[i] = pk;
    }
    const AlphaMaterial old = ms->alphaMaterials[i];
    const bool boundsKept = previous && previous->baseColorTextureSampler == m.baseColorTextureSampler && previous->alphaMode == m.alphaMode &&
                            std::memcmp(&previous->baseColorFactor.w, &m.baseColorFactor.w, sizeof(float)) == 0;
    if (boundsKept)
    {
        AlphaMaterial am = old; // same texels, same bounds; the cutoff may have moved
        am.cutoff = m.alphaCutoff;
        ms->alphaMaterials[i] = am;
    }
    else
    {
        AlphaMaterial am;
        uint64_t bytes = 0;
        if ((rc = build_alpha_material(ctx, m, ms->textures, ms->samplers, ms->uploadStream.get(), &am, &bytes))) return rc;
        ms->alphaBoundBytes += bytes;
        ms->alphaBoundBytes -= std::min<uint64_t>(ms->alphaBoundBytes, allocation_bytes(ctx, old.bounds));
        retire(ctx, old.bounds);
        ms->alphaMaterials[i] = am;
    }
    if (m.alphaMode != PROSPER_ALPHA_MODE_OPAQUE && std::memcmp(&old, &ms->alphaMaterials[i], sizeof(AlphaMaterial)) != 0)
        ms->pendingAlphaPatch = true;
    return PROSPER_PT_OK;
}

int check_material(const MaterialState *ms, const prosper_MaterialData &m, uint32_t index)
{
    const uint32_t ts[3] = {m.baseColorTextureSampler, m.metallicRoughnessTextureSampler, m.normalTextureSampler};
    for (uint32_t k = 0; k < 3; ++k)
    {
        const uint32_t tex = ts[k] & 0xFFFFFFu, smp = ts[k] >> 24;
        if (tex > 0 && (tex >= ms->textures.size() || smp >= ms->samplers.size()))
            return fail(PROSPER_PT_ERR_SCENE, "material " + std::to_string(index) + " references a missing texture/sampler");
        // (a pack is rebuilt from its three textures' own texels - only when what it depends on changed: an entry that
        //  keeps its textures and samplers keeps its pack, and prosper rewrites the WHOLE table every time)
        if (tex > 0 && !ms->textures[tex].texels && !same_pack_inputs(ms->materials[index], m))
            return fail(
                PROSPER_PT_ERR_UNSUPPORTED, "material " + std::to_string(index) + ": texture " + std::to_string(tex) +
                                                " kept no texels of its own at upload (only packed materials sampled it): update that texture first");
    }
    if (m.alphaMode > PROSPER_ALPHA_MODE_BLEND) return fail(PROSPER_PT_ERR_SCENE, "material alpha mode invalid");
    // the alpha mode decides the opaque flag of the geometry (World.cpp:646-651) and with it the any-hit records; prosper
    // gives a streaming material's placeholder the real mode for the same reason (WorldData.cpp:817-826)
    if (m.alphaMode != ms->materials[index].alphaMode)
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "material " + std::to_string(index) + ": the alpha mode of an uploaded material cannot change (upload the scene again)");
    return PROSPER_PT_OK;
}

} // namespace

int flush_pending_materials(prosper_pt_ctx *ctx, hipStream_t stream)
{
    MaterialState *ms = ctx->materialState;
    if (!ms || !ms->pending) return PROSPER_PT_OK;
    const uint32_t v = ms->versions.next(); // 1, 2, 3, 1, ...: version 0 is the upload's own tables
    int rc;
    if (!ms->dBlocks[v])
    {
        void *d = nullptr;
        if ((rc = device_alloc(ctx, ms->blockBytes, &d))) return rc;
        ms->dBlocks[v] = static_cast<uint8_t *>(d);
    }
    if ((rc = ms->uploadStream.create())) return rc;
    uint8_t *img = nullptr;
    if ((rc = ms->staging.acquire(ms->blockBytes, false, &img))) return rc;
    std::memcpy(img, ms->materials.data(), ms->materials.size() * sizeof(prosper_MaterialData));
    std::memcpy(img + ms->packsOffset, ms->packs.data(), ms->packs.size() * sizeof(MaterialPack));
    std::memcpy(img + ms->alphaOffset, ms->alphaMaterials.data(), ms->alphaMaterials.size() * sizeof(AlphaMaterial));
    std::memcpy(img + ms->texturesOffset, ms->textures.data(), ms->textures.size() * sizeof(DeviceTexture));
    if (!ms->mips.empty()) std::memcpy(img + ms->mipsOffset, ms->mips.data(), ms->mips.size() * sizeof(DeviceTextureMips));
    // the block's last readers (three flushes ago), the texel arrays / packs / bounds the tables point at
    if ((rc = ms->versions.wait_free(v, stream))) return rc;
    if ((rc = ms->uploaded.wait(stream))) return rc;
    // ... and the previous flush, which ran on another render's stream: its rewrite of the any-hit records (they exist
    // once, for every version) must be done before this render reads them.  `ready` is recorded anew below, so this wait is
    // the only thing that orders the render behind the earlier record: without it a frame whose own flush patches nothing
    // could overtake the patch of the flush before (found when a fifth stream changed which streams share a hardware
    // queue: 927 pixels of FlightHelmet's lenses, one frame in six).
    if ((rc = ms->ready.wait(stream))) return rc;
    PPT_HIP(hipMemcpyAsync(ms->dBlocks[v], img, ms->blockBytes, hipMemcpyHostToDevice, stream));
    if ((rc = ms->staging.copy_enqueued(stream))) return rc;
    const AlphaMaterial *dAlpha = reinterpret_cast<const AlphaMaterial *>(ms->dBlocks[v] + ms->alphaOffset);
    if (ms->pendingAlphaPatch && ctx->alphaTriangleCount)
    {
        // the any-hit records carry a copy of their material's AlphaMaterial and exist once: they are rewritten in place,
        // behind every render that may still read them (the one kind of update that waits for the frames in flight)
        if ((rc = ms->versions.wait_all_free(stream))) return rc;
        launch_patch_alpha_records(
            const_cast<AlphaTriangle *>(ctx->scene.alphaTriangles), (uint32_t)ctx->alphaTriangleCount, dAlpha,
            (uint32_t)ms->alphaMaterials.size(), stream);
        PPT_HIP(hipGetLastError());
    }
    if ((rc = ms->ready.record(stream))) return rc;
    // ---- commit ----
    ms->versions.commit(v);
    ctx->scene.materials = reinterpret_cast<const prosper_MaterialData *>(ms->dBlocks[v]);
    ctx->scene.materialPacks = reinterpret_cast<const MaterialPack *>(ms->dBlocks[v] + ms->packsOffset);
    ctx->scene.alphaMaterials = dAlpha;
    ctx->scene.textures = reinterpret_cast<const DeviceTexture *>(ms->dBlocks[v] + ms->texturesOffset);
    if (!ms->mips.empty()) ctx->textureMips = reinterpret_cast<const DeviceTextureMips *>(ms->dBlocks[v] + ms->mipsOffset);
    ctx->scene.batchedTextures = ctx->debug.batchedTextures >= 0 ? (ctx->debug.batchedTextures ? 1u : 0u) : (texel_set_is_big(ms->texelBytes) ? 1u : 0u);
    ctx->packedMaterials = ms->packedMaterials;
    ctx->alphaBoundBytes = ms->alphaBoundBytes;
    ctx->stats.alphaBoundBytes = ms->alphaBoundBytes;
    ctx->stats.deviceBytes = ctx->sceneBytes;
    ms->pending = false;
    ms->pendingAlphaPatch = false;
    ms->updates++;
    return PROSPER_PT_OK;
}

// prosper_pt_compress_texture / prosper_pt_debug_bc7_encode_blocks: the source as the caller holds it, its levels in the
// DeviceTexture tiling, the payload on its way back
struct CompressPassState
{
    DeviceBuffer source, tiled, payload;
    StageEvents<3> events; // around the last compression's stages: prepare, encode, read back
    bool timed = false;
};

extern const PassModule kCompressPasses = pass_module<CompressPassState, &prosper_pt_ctx::compressPasses>();

} // namespace ppt

using namespace ppt;

namespace
{

// What compress() decides for `levels` levels of an extent (src/scene/Texture.cpp:227-237, src/utils/Dds.cpp:100-135)
struct CompressedLayout
{
    uint32_t format = PROSPER_PT_FORMAT_BC7_UNORM;
    uint32_t levels = 1;
    uint64_t bytes = 0;
};
CompressedLayout compressed_layout(uint32_t width, uint32_t height, uint32_t levels)
{
    CompressedLayout out;
    out.levels = levels;
    for (uint32_t l = 0; l < levels; ++l)
        if (std::max(width >> l, 1u) % 4u != 0u || std::max(height >> l, 1u) % 4u != 0u) out.format = PROSPER_PT_FORMAT_RGBA8_UNORM;
    for (uint32_t l = 0; l < levels; ++l)
    {
        const uint64_t w = std::max(width >> l, 1u), h = std::max(height >> l, 1u);
        out.bytes += out.format == PROSPER_PT_FORMAT_BC7_UNORM ? (w / 4u) * (h / 4u) * 16u : w * h * 4u;
    }
    return out;
}

} // namespace

extern "C" {

int prosper_pt_update_textures(prosper_pt_ctx *ctx, const prosper_pt_texture_desc *textures, uint32_t first, uint32_t count)
{
    if (!ctx || (!textures && count)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_update_textures: null argument");
    if (!ctx->haveScene || !ctx->materialState) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    MaterialState *ms = ctx->materialState;
    if ((uint64_t)first + count > ms->textures.size())
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_update_textures: range exceeds the scene's textureCount");
    if (count == 0) return PROSPER_PT_OK;
    size_t stagingBytes = 0;
    const bool withMips = !ms->mips.empty();
    for (uint32_t i = 0; i < count; ++i)
    {
        const int rc = validate_texture(textures[i], first + i, withMips);
        if (rc != PROSPER_PT_OK) return rc;
        stagingBytes += texture_staging_bytes(textures[i], withMips);
    }
    // A material that samples a replaced texture gets its pack rebuilt from its three textures' own texels: a texture whose
    // own copy was released at upload (only packed materials sampled it) must arrive in the same call.
    for (uint32_t m = 0; m < ms->materials.size(); ++m)
    {
        const prosper_MaterialData &md = ms->materials[m];
        const uint32_t t3[3] = {md.baseColorTextureSampler & 0xFFFFFFu, md.metallicRoughnessTextureSampler & 0xFFFFFFu,
                                md.normalTextureSampler & 0xFFFFFFu};
        auto replaced = [&](uint32_t t) { return t >= first && t < first + count; };
        if (!((t3[0] && replaced(t3[0])) || (t3[1] && replaced(t3[1])) || (t3[2] && replaced(t3[2])))) continue;
        for (uint32_t t : t3)
            if (t && !replaced(t) && !ms->textures[t].texels)
                return fail(
                    PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_update_textures: material " + std::to_string(m) + " also samples texture " + std::to_string(t) +
                                                    ", which kept no texels of its own at upload (only packed materials sampled it): update it in the same call");
    }
    PPT_HIP(hipSetDevice(ctx->device));
    int rc = ms->uploadStream.create();
    if (rc == PROSPER_PT_OK) rc = collect_retired(ctx);
    if (rc != PROSPER_PT_OK) return rc;
    // the previous update's copies out of the pinned staging area (a frame ago, as a rule: done long since)
    if ((rc = ms->uploaded.host_wait())) return rc;
    if (stagingBytes > ms->linearStagingBytes)
    {
        // (the outgrown area joins the scene's allocations: kernels of an earlier update may still read it)
        if (ms->linearStaging) ctx->sceneAllocations.push_back({ms->linearStaging, ms->linearStagingBytes});
        ms->linearStaging = nullptr;
        ms->linearStagingBytes = 0;
        PPT_HIP(hipMalloc(&ms->linearStaging, stagingBytes));
        ms->linearStagingBytes = stagingBytes;
    }
    if (stagingBytes > ms->pinnedStaging.bytes)
    {
        // (the stream was synchronised at the end of the previous call: nothing reads the old area any more)
        if ((rc = ms->pinnedStaging.allocate(stagingBytes))) return rc;
    }
    size_t offset = 0;
    std::vector<uint8_t> changed(ms->textures.size(), 0);
    const std::vector<uint8_t> baseColour = base_colour_textures(ms->materials.data(), ms->materials.size(), ms->textures.size());
    for (uint32_t i = 0; i < count; ++i)
    {
        DeviceTexture dt;
        DeviceTextureMips dm{nullptr, 1u, 0u, {}};
        if ((rc = create_device_texture(
                 ctx, textures[i], static_cast<uint8_t *>(ms->linearStaging) + offset, ms->uploadStream.get(), &dt,
                 static_cast<uint8_t *>(ms->pinnedStaging.ptr) + offset, withMips ? &dm : nullptr, baseColour[first + i] != 0)))
        {
            (void)hipStreamSynchronize(ms->uploadStream.get());
            return rc;
        }
        offset += texture_staging_bytes(textures[i], withMips);
        if (withMips)
        {
            // (the old chain like the old level 0: a frame in flight may still read it)
            DeviceTextureMips &oldMips = ms->mips[first + i];
            const DeviceTexture &was = ms->textures[first + i];
            ms->mipTexelBytes += mip_texel_bytes(dt.width, dt.height, dm.levelCount);
            ms->mipTexelBytes -= std::min<uint64_t>(ms->mipTexelBytes, mip_texel_bytes(was.width, was.height, oldMips.levelCount));
            retire(ctx, oldMips.texels);
            oldMips = dm;
        }
        const DeviceTexture &old = ms->textures[first + i];
        ms->texelBytes += (uint64_t)dt.width * dt.height * 4u;
        ms->texelBytes -= std::min<uint64_t>(ms->texelBytes, (uint64_t)old.width * old.height * 4u);
        retire(ctx, old.texels); // (a frame in flight may still read the previous texel array)
        ms->textures[first + i] = dt;
        changed[first + i] = 1;
    }
    // (the caller's memory has been read - into the pinned staging area - when create_device_texture returns: nothing to wait
    //  for here.  The copies out of that area are waited for by the NEXT call, before it overwrites it.)
    // materials that sample a replaced texture: their packs and alpha bounds hold its texels
    for (uint32_t m = 0; m < ms->materials.size(); ++m)
    {
        const prosper_MaterialData &md = ms->materials[m];
        const uint32_t t3[3] = {md.baseColorTextureSampler & 0xFFFFFFu, md.metallicRoughnessTextureSampler & 0xFFFFFFu,
                                md.normalTextureSampler & 0xFFFFFFu};
        if ((t3[0] && changed[t3[0]]) || (t3[1] && changed[t3[1]]) || (t3[2] && changed[t3[2]]))
            if ((rc = rebuild_material(ctx, m, nullptr))) return rc;
    }
    if (const int urc = ms->uploaded.record(ms->uploadStream.get())) return urc;
    ms->pending = true;
    ms->changes++;
    return PROSPER_PT_OK;
}

int prosper_pt_update_materials(prosper_pt_ctx *ctx, const prosper_MaterialData *materials, uint32_t first, uint32_t count)
{
    if (!ctx || (!materials && count)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_update_materials: null argument");
    if (!ctx->haveScene || !ctx->materialState) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    MaterialState *ms = ctx->materialState;
    if ((uint64_t)first + count > ms->materials.size())
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_update_materials: range exceeds the scene's materialCount");
    for (uint32_t i = 0; i < count; ++i)
    {
        const int rc = check_material(ms, materials[i], first + i);
        if (rc != PROSPER_PT_OK) return rc;
    }
    bool any = false;
    for (uint32_t i = 0; i < count; ++i)
    {
        // prosper rewrites the whole buffer when ONE material changed (WorldData.cpp:568-586): the others cost a memcmp
        if (std::memcmp(&ms->materials[first + i], &materials[i], sizeof(prosper_MaterialData)) == 0) continue;
        if (!any)
        {
            PPT_HIP(hipSetDevice(ctx->device));
            int rc = ms->uploadStream.create();
            if (rc == PROSPER_PT_OK) rc = collect_retired(ctx);
            if (rc != PROSPER_PT_OK) return rc;
        }
        any = true;
        const prosper_MaterialData previous = ms->materials[first + i];
        ms->materials[first + i] = materials[i];
        const int rc = rebuild_material(ctx, first + i, &previous);
        if (rc != PROSPER_PT_OK) return rc;
    }
    if (!any) return PROSPER_PT_OK;
    if (const int urc = ms->uploaded.record(ms->uploadStream.get())) return urc;
    ms->pending = true;
    ms->changes++;
    return PROSPER_PT_OK;
}

uint32_t prosper_pt_texture_mip_level_count(uint32_t width, uint32_t height)
{
    return width && height ? mip_level_count(width, height) : 0u;
}

int prosper_pt_check_texture_desc(const prosper_pt_texture_desc *desc, uint32_t create_flags)
{
    if (!desc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_check_texture_desc: null argument");
    return validate_texture(*desc, 0, (create_flags & PROSPER_PT_CREATE_TEXTURE_MIPS) != 0);
}

int prosper_pt_get_texture_mips_info(prosper_pt_ctx *ctx, uint32_t texture, prosper_pt_texture_mips_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_texture_mips_info: null argument");
    if (!(ctx->flags & PROSPER_PT_CREATE_TEXTURE_MIPS))
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_get_texture_mips_info: the context was created without PROSPER_PT_CREATE_TEXTURE_MIPS");
    if (!ctx->haveScene || !ctx->materialState) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    const MaterialState *ms = ctx->materialState;
    if (texture >= ms->textures.size()) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_texture_mips_info: texture out of range");
    out->width = ms->textures[texture].width;
    out->height = ms->textures[texture].height;
    out->levelCount = ms->mips[texture].levelCount;
    out->srgbAveraged = ms->mips[texture].srgb;
    out->mipTexelBytes = ms->mipTexelBytes;
    return PROSPER_PT_OK;
}

int prosper_pt_read_texture_level(prosper_pt_ctx *ctx, uint32_t texture, uint32_t level, void *rgba8, uint64_t bytes, void *stream)
{
    if (!ctx || !rgba8) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_level: null argument");
    if (!ctx->haveScene || !ctx->materialState) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    MaterialState *ms = ctx->materialState;
    if (texture >= ms->textures.size()) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_level: texture out of range");
    const DeviceTexture &t = ms->textures[texture];
    const uint32_t levels = ms->mips.empty() ? 1u : ms->mips[texture].levelCount;
    if (level >= levels || t.width == 0)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_level: the texture has no level " + std::to_string(level));
    const uint32_t w = std::max(t.width >> level, 1u), h = std::max(t.height >> level, 1u);
    if (bytes != (uint64_t)w * h * 4u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_texture_level: the level holds " + std::to_string((uint64_t)w * h * 4u) + " bytes");
    const uint8_t *tiled = level == 0 ? t.texels : ms->mips[texture].texels + (size_t)ms->mips[texture].wordOffset[level] * 4u;
    if (!tiled)
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_read_texture_level: level 0 of this texture lives only in a material pack");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = ms->uploaded.wait(s); // (an update's kernels run on its own stream)
    if (rc != PROSPER_PT_OK) return rc;
    void *linear = nullptr;
    PPT_HIP(hipMalloc(&linear, (size_t)bytes));
    launch_untile_level(tiled, w, h, linear, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(rgba8, linear, (size_t)bytes, hipMemcpyDeviceToHost, s);
    const hipError_t f = hipStreamSynchronize(s);
    (void)hipFree(linear);
    PPT_HIP(e);
    PPT_HIP(f);
    return PROSPER_PT_OK;
}

int prosper_pt_debug_sample_texture_lod(
    prosper_pt_ctx *ctx, uint32_t texture, uint32_t sampler, const float *in6, uint32_t n, float bias, float *out5)
{
    if (!std::isfinite(bias)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_sample_texture_lod: the bias is not finite");
    if (!ctx || (n && (!in6 || !out5))) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_sample_texture_lod: null argument");
    if (!(ctx->flags & PROSPER_PT_CREATE_TEXTURE_MIPS))
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_debug_sample_texture_lod: the context was created without PROSPER_PT_CREATE_TEXTURE_MIPS");
    int rc = check_scene(ctx, "prosper_pt_debug_sample_texture_lod");
    if (rc != PROSPER_PT_OK) return rc;
    const MaterialState *ms = ctx->materialState;
    if (texture == 0 || texture >= ms->textures.size() || sampler >= ms->samplers.size())
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_sample_texture_lod: texture / sampler out of range");
    if (!ms->textures[texture].texels)
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_debug_sample_texture_lod: level 0 of this texture lives only in a material pack");
    if (n == 0) return PROSPER_PT_OK;
    if ((rc = flush_scene_updates(ctx, nullptr, nullptr))) return rc;
    float *dIn = nullptr, *dOut = nullptr;
    const size_t inBytes = (size_t)n * 6u * sizeof(float), outBytes = (size_t)n * 5u * sizeof(float);
    PPT_HIP(hipMalloc((void **)&dIn, inBytes));
    hipError_t e = hipMalloc((void **)&dOut, outBytes);
    if (e == hipSuccess) e = hipMemcpy(dIn, in6, inBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        launch_sample_texture_lod(ctx->scene, ctx->textureMips, texture, sampler, dIn, n, bias, dOut, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out5, dOut, outBytes, hipMemcpyDeviceToHost);
    (void)hipFree(dIn);
    (void)hipFree(dOut);
    if (e != hipSuccess) return fail(PROSPER_PT_ERR_HIP, std::string("prosper_pt_debug_sample_texture_lod: ") + hipGetErrorString(e));
    return mark_versions_read(ctx, nullptr);
}

int prosper_pt_compressed_texture_layout(
    uint32_t width, uint32_t height, uint32_t generateMips, uint32_t *format, uint32_t *levelCount, uint64_t *bytes)
{
    if (!format || !levelCount || !bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_compressed_texture_layout: null argument");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_compressed_texture_layout: empty extent");
    const CompressedLayout layout = compressed_layout(width, height, generateMips ? mip_level_count(width, height) : 1u);
    *format = layout.format;
    *levelCount = layout.levels;
    *bytes = layout.bytes;
    return PROSPER_PT_OK;
}

int prosper_pt_compress_texture(
    prosper_pt_ctx *ctx, const prosper_pt_texture_desc *src, uint32_t flags, void *dst, uint64_t dstBytes, void *stream)
{
    if (!ctx || !src || !dst || !src->texels) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_compress_texture: null argument");
    if (src->width == 0 || src->height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_compress_texture: empty extent");
    if (src->format != PROSPER_PT_FORMAT_RGBA8_UNORM)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_compress_texture: the source must be PROSPER_PT_FORMAT_RGBA8_UNORM");
    if (flags & ~(uint32_t)(PROSPER_PT_COMPRESS_SRGB | PROSPER_PT_COMPRESS_GENERATE_MIPS))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_compress_texture: unknown flags");
    const uint32_t w0 = src->width, h0 = src->height, count = mip_level_count(w0, h0);
    const uint32_t supplied = src->mipLevelCount > 1u ? src->mipLevelCount : 1u;
    if (supplied > count)
        return fail(
            PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_compress_texture: mipLevelCount " + std::to_string(supplied) + " exceeds the " +
                                                 std::to_string(count) + " levels of prosper's chain for the extent");
    const uint32_t levels = supplied > 1u ? supplied : ((flags & PROSPER_PT_COMPRESS_GENERATE_MIPS) ? count : 1u);
    if (levels > kMaxMipLevels) return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_compress_texture: a mip chain of more than 16 levels");
    const CompressedLayout layout = compressed_layout(w0, h0, levels);
    if (dstBytes != layout.bytes)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_compress_texture: the payload holds " + std::to_string(layout.bytes) + " bytes");
    size_t sourceBytes = 0, tiledWords = 0, tiledOffset[kMaxMipLevels] = {};
    for (uint32_t l = 0; l < levels; ++l)
    {
        const uint32_t w = std::max(w0 >> l, 1u), h = std::max(h0 >> l, 1u);
        if (l < supplied) sourceBytes += (size_t)w * h * 4u;
        tiledOffset[l] = tiledWords;
        tiledWords += tiled_level_words(w, h);
    }
    if (tiledWords >= (1ull << 32)) return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_compress_texture: the chain exceeds 2^32 texels");

    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    CompressPassState &st = *ctx->compressPasses;
    int rc;
    if ((rc = grow_to(st.source, sourceBytes, s))) return rc;
    if ((rc = grow_to(st.tiled, tiledWords * 4u, s))) return rc;
    if ((rc = grow_to(st.payload, (size_t)layout.bytes, s))) return rc;
    if ((rc = st.events.create())) return rc;
    st.timed = false;
    // stages between the events: source up + tiling + mip generation, encoding, payload back
    const bool srgb = (flags & PROSPER_PT_COMPRESS_SRGB) != 0;
    const auto enqueue = [&]() -> hipError_t {
        hipError_t e;
        if ((e = hipEventRecord(st.events.events[0], s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(st.source.ptr, src->texels, sourceBytes, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(st.tiled.ptr, 0, tiledWords * 4u, s)) != hipSuccess) return e; // (tile padding)
        size_t sourceOffset = 0, payloadOffset = 0;
        for (uint32_t l = 0; l < levels; ++l)
        {
            const uint32_t w = std::max(w0 >> l, 1u), h = std::max(h0 >> l, 1u);
            uint32_t *level = st.tiled.as<uint32_t>() + tiledOffset[l];
            if (l < supplied)
            {
                launch_retile_rgba8(st.source.as<uint8_t>() + sourceOffset, w, h, (w + kTexTileW - 1u) / kTexTileW, level, s);
                sourceOffset += (size_t)w * h * 4u;
            }
            else
                launch_generate_mip(
                    st.tiled.as<uint32_t>() + tiledOffset[l - 1u], std::max(w0 >> (l - 1u), 1u), std::max(h0 >> (l - 1u), 1u), level, w, h, srgb, s);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(st.events.events[1], s)) != hipSuccess) return e;
        for (uint32_t l = 0; l < levels; ++l)
        {
            const uint32_t w = std::max(w0 >> l, 1u), h = std::max(h0 >> l, 1u);
            const uint32_t *level = st.tiled.as<uint32_t>() + tiledOffset[l];
            uint8_t *out = st.payload.as<uint8_t>() + payloadOffset;
            if (layout.format == PROSPER_PT_FORMAT_BC7_UNORM)
            {
                launch_bc7_encode_level(level, w, h, 0u, out, s);
                payloadOffset += (size_t)(w / 4u) * (h / 4u) * 16u;
            }
            else
            {
                // compress()'s memcpy branch: the raw chain
                launch_untile_level(level, w, h, out, s);
                payloadOffset += (size_t)w * h * 4u;
            }
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(st.events.events[2], s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(dst, st.payload.ptr, (size_t)layout.bytes, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        return hipEventRecord(st.events.events[3], s);
    };
    // (whatever was enqueued is waited for, also after a failure: `src` and `dst` are borrowed for the call only)
    const hipError_t e = enqueue();
    const hipError_t f = hipStreamSynchronize(s);
    PPT_HIP(e);
    PPT_HIP(f);
    st.timed = true;
    return PROSPER_PT_OK;
}

int prosper_pt_get_compress_texture_timing(prosper_pt_ctx *ctx, float *prepareMs, float *encodeMs, float *readbackMs)
{
    if (!ctx || !prepareMs || !encodeMs || !readbackMs) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_compress_texture_timing: null argument");
    const CompressPassState &st = *ctx->compressPasses;
    if (!st.timed) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_compress_texture_timing: no prosper_pt_compress_texture has completed");
    PPT_HIP(hipSetDevice(ctx->device));
    float ms[3];
    const int rc = st.events.elapsed(ms);
    if (rc != PROSPER_PT_OK) return rc;
    *prepareMs = ms[0];
    *encodeMs = ms[1];
    *readbackMs = ms[2];
    return PROSPER_PT_OK;
}

int prosper_pt_debug_bc7_encode_blocks(
    prosper_pt_ctx *ctx, const uint32_t *texels, uint32_t n, uint32_t modeMask, uint32_t *blocks, uint32_t *sse, void *stream)
{
    if (!ctx || (n && (!texels || !blocks || !sse))) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_bc7_encode_blocks: null argument");
    if (modeMask & ~kBc7EncodeModes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_bc7_encode_blocks: modeMask has bits 4, 5 and 6");
    if (n == 0) return PROSPER_PT_OK;
    if (n > (1u << 26)) return fail(PROSPER_PT_ERR_UNSUPPORTED, "prosper_pt_debug_bc7_encode_blocks: more than 2^26 blocks");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    CompressPassState &st = *ctx->compressPasses;
    int rc;
    // blocks and errors side by side: 16 + 4 bytes per block
    if ((rc = grow_to(st.source, (size_t)n * 64u, s))) return rc;
    if ((rc = grow_to(st.payload, (size_t)n * 20u, s))) return rc;
    uint32_t *dBlocks = st.payload.as<uint32_t>(), *dSse = dBlocks + (size_t)n * 4u;
    PPT_HIP(hipMemcpyAsync(st.source.ptr, texels, (size_t)n * 64u, hipMemcpyHostToDevice, s));
    launch_bc7_encode_blocks(st.source.as<uint32_t>(), n, modeMask, dBlocks, dSse, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(blocks, dBlocks, (size_t)n * 16u, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(sse, dSse, (size_t)n * 4u, hipMemcpyDeviceToHost, s);
    const hipError_t f = hipStreamSynchronize(s);
    PPT_HIP(e);
    PPT_HIP(f);
    return PROSPER_PT_OK;
}

} // extern "C"
