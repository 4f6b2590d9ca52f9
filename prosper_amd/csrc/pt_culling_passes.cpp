// pt_culling_passes.cpp — C-ABI of prosper's visibility system (include/prosper_pt/prosper_pt.h): the depth pyramid
// (prosper_pt_hiz_downsample) in the context's two slots and its read-backs, the per-instance uniform scales, the two
// culling phases over the scene's meshlets with their draw lists, and DrawStats.  Kernels: pt_culling.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "pt_context.hpp"
#include "pt_culling.hpp"
#include "pt_culling_state.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

// a new scene: both pyramids and the draw lists describe the old one
static void forget_hiz(prosper_pt_ctx *ctx)
{
    if (!ctx->cullingPasses) return;
    CullingPassState &st = *ctx->cullingPasses;
    for (CullingPassState::HizSlot &slot : st.hiz) slot.valid = false;
    st.keptHiz = -1;
    for (bool &v : st.listValid) v = false;
    st.statsQueued = false;
    st.checked = false;
    st.firstTimed = st.secondTimed = false;
}

extern const PassModule kCullingPasses = pass_module<CullingPassState, &prosper_pt_ctx::cullingPasses>(forget_hiz);

int enqueue_instance_scales(
    prosper_pt_ctx *ctx, AccelState *acc, uint32_t v, const prosper_ModelInstanceTransforms *transforms, uint32_t count, hipStream_t stream)
{
    if (!acc->dScalesV[v])
    {
        void *d = nullptr;
        if (const int rc = device_alloc(ctx, sizeof(float) * (count ? count : 1u), &d)) return rc;
        acc->dScalesV[v] = static_cast<float *>(d);
    }
    launch_instance_scales(transforms, acc->dScalesV[v], count, stream);
    PPT_HIP(hipGetLastError());
    return PROSPER_PT_OK;
}

} // namespace ppt

namespace
{

// the valid pyramid of `slot` and its level `level`, or the refusal
int hiz_level(prosper_pt_ctx *ctx, const char *what, uint32_t slot, uint32_t level, CullingPassState::HizSlot **out)
{
    if (slot > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": slot is 0 or 1");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    CullingPassState::HizSlot &s = ctx->cullingPasses->hiz[slot];
    if (!s.valid) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": the slot holds no pyramid");
    if (level >= s.layout.levelCount) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": level beyond the pyramid's last");
    *out = &s;
    return PROSPER_PT_OK;
}


constexpr uint32_t kArgsWords = 6; // two triples; the DrawListStats follow

// Every loaded mesh's meshlet sections lie inside its geometry buffer: checked on the host mirrors, once per geometry
// generation (the culler reads a meshlet's fourth word and its five bounds words; the other two sections by their start).
int check_meshlet_ranges(prosper_pt_ctx *ctx, const char *what)
{
    CullingPassState &st = *ctx->cullingPasses;
    const GeometryState *gs = ctx->geometry;
    if (!gs) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": no scene");
    if (st.checked && st.checkedGeometry == gs && st.checkedInstalls == gs->installs && st.checkedUpdates == gs->meshUpdates)
        return PROSPER_PT_OK;
    for (size_t i = 0; i < gs->infos.size() && i < gs->metadatas.size(); ++i)
    {
        const prosper_pt_mesh_info &info = gs->infos[i];
        const prosper_GeometryMetadata &md = gs->metadatas[i];
        if (info.meshletCount == 0u) continue;
        const std::string mesh = std::string(what) + ": mesh " + std::to_string(i);
        // (the host's bound on a list counts the meshes that have indices, the generator the meshes that have meshlets)
        if (info.indexCount == 0u) return fail(PROSPER_PT_ERR_SCENE, mesh + " has meshlets and no indices");
        if (md.bufferIndex >= gs->bufferBytes.size() || gs->bufferBytes[md.bufferIndex] == 0u)
            return fail(PROSPER_PT_ERR_SCENE, mesh + " has meshlets and no geometry buffer");
        const uint64_t bytes = gs->bufferBytes[md.bufferIndex], n = info.meshletCount;
        const uint64_t vertexUnit = md.usesShortIndices == 1u ? 2u : 4u;
        if (md.meshletsOffset == 0xFFFFFFFFu || (uint64_t)md.meshletsOffset * 4u + n * 16u > bytes)
            return fail(PROSPER_PT_ERR_SCENE, mesh + ": meshlets leave its geometry buffer");
        if (md.meshletBoundsOffset == 0xFFFFFFFFu || (uint64_t)md.meshletBoundsOffset * 4u + n * 20u > bytes)
            return fail(PROSPER_PT_ERR_SCENE, mesh + ": meshletBounds leave its geometry buffer");
        if (md.meshletVerticesOffset == 0xFFFFFFFFu || (uint64_t)md.meshletVerticesOffset * vertexUnit >= bytes)
            return fail(PROSPER_PT_ERR_SCENE, mesh + ": meshletVertices start past its geometry buffer");
        if (md.meshletTrianglesByteOffset == 0xFFFFFFFFu || (uint64_t)md.meshletTrianglesByteOffset >= bytes)
            return fail(PROSPER_PT_ERR_SCENE, mesh + ": meshletTriangles start past its geometry buffer");
    }
    st.checkedGeometry = gs;
    st.checkedInstalls = gs->installs;
    st.checkedUpdates = gs->meshUpdates;
    st.checked = true;
    // what the generator reads: the meshlet count of every mesh, as of this generation
    st.hostMeshletCounts.assign(gs->infos.size() ? gs->infos.size() : 1u, 0u);
    for (size_t i = 0; i < gs->infos.size(); ++i) st.hostMeshletCounts[i] = gs->infos[i].meshletCount;
    st.countsDirty = true; // (uploaded by the next first phase)
    return PROSPER_PT_OK;
}

// recordGenerateList's host loop: the totals of DrawStats and the bound on the list's length
uint32_t count_totals(const prosper_pt_ctx *ctx, uint32_t mode, prosper_pt_draw_stats *totals)
{
    const GeometryState *gs = ctx->geometry;
    const std::vector<prosper_MaterialData> &materials = ctx->materialState->materials;
    uint32_t upperBound = 0;
    std::vector<bool> modelDrawn(ctx->scene.modelInstanceCount ? ctx->scene.modelInstanceCount : 1u, false);
    *totals = prosper_pt_draw_stats{};
    for (const prosper_DrawInstance &di : gs->drawInstances)
    {
        if (di.meshIndex >= gs->infos.size() || di.materialIndex >= materials.size()) continue;
        const prosper_pt_mesh_info &info = gs->infos[di.meshIndex];
        if (info.indexCount == 0u) continue; // invalid or not yet loaded
        const bool blend = materials[di.materialIndex].alphaMode == PROSPER_ALPHA_MODE_BLEND;
        if ((mode == PROSPER_PT_CULL_MODE_TRANSPARENT) != blend) continue;
        totals->totalMeshCount++;
        totals->totalTriangleCount += info.indexCount / 3u;
        totals->totalMeshletCount += info.meshletCount;
        upperBound += info.meshletCount;
        if (di.modelInstanceIndex < modelDrawn.size() && !modelDrawn[di.modelInstanceIndex])
        {
            totals->totalModelCount++;
            modelDrawn[di.modelInstanceIndex] = true;
        }
    }
    return upperBound;
}

// the culler's parameters that come from the camera and the pyramid of `hizSlot` (PROSPER_PT_NO_HIZ: none)
int set_view(prosper_pt_ctx *ctx, const char *what, const prosper_CameraUniforms *camera, uint32_t hizSlot, DrawListCullerParams &p)
{
    const prosper_vec4 *planes[6] = {&camera->nearPlane, &camera->farPlane, &camera->leftPlane,
                                     &camera->rightPlane, &camera->bottomPlane, &camera->topPlane};
    for (int k = 0; k < 6; ++k) std::memcpy(p.planes[k], planes[k], 16);
    p.eye[0] = camera->eye.x, p.eye[1] = camera->eye.y, p.eye[2] = camera->eye.z;
    std::memcpy(p.worldToCamera, &camera->worldToCamera, 64);
    std::memcpy(p.cameraToClip, &camera->cameraToClip, 64);
    mat4_mul(p.cameraToClip, p.worldToCamera, p.clipFromWorld);
    p.near_ = camera->near_;
    p.maxViewScale = camera->maxViewScale;
    p.resolution[0] = (float)camera->resolution[0];
    p.resolution[1] = (float)camera->resolution[1];
    p.hizMipCount = 0;
    if (hizSlot == PROSPER_PT_NO_HIZ) return PROSPER_PT_OK;
    const CullingPassState::HizSlot &hz = ctx->cullingPasses->hiz[hizSlot];
    if (!hz.valid) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the slot holds no pyramid");
    if (hz.sourceWidth != camera->resolution[0] || hz.sourceHeight != camera->resolution[1])
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": camera->resolution differs from the pyramid's source extent");
    p.hizMipCount = hz.layout.levelCount;
    p.hizResolution[0] = hz.layout.levelW[0];
    p.hizResolution[1] = hz.layout.levelH[0];
    {
        // vec2(resolution) / (2.f * vec2(hizResolution)); volatile: IEEE fp32 products and divides, nothing folded
        volatile float rx = (float)camera->resolution[0], ry = (float)camera->resolution[1];
        volatile float hx = 2.0f * (float)p.hizResolution[0], hy = 2.0f * (float)p.hizResolution[1];
        p.hizUvScale[0] = rx / hx;
        p.hizUvScale[1] = ry / hy;
    }
    for (uint32_t l = 0; l < hz.layout.levelCount; ++l) p.hizLevels[l] = hz.pyramid.as<float>() + hz.layout.levelOffset[l];
    return PROSPER_PT_OK;
}

// one launch of the culler over list `in` into list `out` (and `second`, or -1), then the statistics on their way home
int run_culler(prosper_pt_ctx *ctx, DrawListCullerParams &p, uint32_t in, uint32_t out, int second, uint32_t phase, hipEvent_t after, hipStream_t s)
{
    CullingPassState &st = *ctx->cullingPasses;
    const AccelState *acc = ctx->accel;
    p.geometryBuffers = ctx->scene.geometryBuffers;
    p.metadatas = ctx->scene.geometryMetadatas;
    p.drawInstances = ctx->scene.drawInstances;
    p.transforms = ctx->scene.modelInstanceTransforms;
    p.scales = acc->dScalesV[acc->versions.cur];
    p.inList = st.lists[in].as<uint32_t>();
    p.upperBound = st.upperBound;
    p.capacity = st.capacity;
    p.outList = st.lists[out].as<uint32_t>();
    p.outArgs = st.argsAndStats.as<uint32_t>() + 3u * phase;
    p.outSecondPhase = second >= 0 ? st.lists[second].as<uint32_t>() : nullptr;
    p.stats = reinterpret_cast<DrawListStats *>(st.argsAndStats.as<uint32_t>() + kArgsWords);
    launch_draw_list_culler(p, s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(after, s));
    if (!st.statsHost.ptr)
        if (const int rc = st.statsHost.allocate(sizeof(DrawListStats))) return rc;
    PPT_HIP(hipMemcpyAsync(st.statsHost.ptr, p.stats, sizeof(DrawListStats), hipMemcpyDeviceToHost, s));
    if (const int rc = st.statsDone.record(s)) return rc;
    st.statsQueued = true;
    return PROSPER_PT_OK;
}

int first_phase(prosper_pt_ctx *ctx, const char *what, uint32_t mode, const prosper_CameraUniforms *camera, uint32_t hizSlot, hipStream_t s)
{
    int rc = check_scene(ctx, what);
    if (rc != PROSPER_PT_OK) return rc;
    if (!ctx->accel || !ctx->geometry || !ctx->materialState) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": no scene");
    if ((rc = flush_scene_updates(ctx, s, s)) != PROSPER_PT_OK) return rc;
    if ((rc = check_meshlet_ranges(ctx, what)) != PROSPER_PT_OK) return rc;
    CullingPassState &st = *ctx->cullingPasses;
    DrawListCullerParams p = {};
    if ((rc = set_view(ctx, what, camera, hizSlot, p)) != PROSPER_PT_OK) return rc;
    if (!ctx->accel->dScalesV[ctx->accel->versions.cur]) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + ": the scene version has no scales");
    for (bool &v : st.listValid) v = false;
    st.statsQueued = false;
    prosper_pt_draw_stats totals = {};
    const uint32_t upperBound = count_totals(ctx, mode, &totals);
    // a call on another stream may still read or write the lists: `s` takes up behind it before anything grows or is cleared
    if ((rc = st.done.wait(s)) != PROSPER_PT_OK) return rc;
    if (hizSlot != PROSPER_PT_NO_HIZ && (rc = st.hiz[hizSlot].done.wait(s)) != PROSPER_PT_OK) return rc;
    if (st.capacity < upperBound || !st.lists[0].ptr)
    {
        const size_t bytes = 4u + 8u * (size_t)(upperBound ? upperBound : 1u);
        for (DeviceBuffer &l : st.lists)
            if ((rc = grow_to(l, bytes, s)) != PROSPER_PT_OK) return rc;
        st.capacity = upperBound ? upperBound : 1u;
    }
    if ((rc = grow_to(st.argsAndStats, kArgsWords * 4u + sizeof(DrawListStats), s)) != PROSPER_PT_OK) return rc;
    const size_t countBytes = st.hostMeshletCounts.size() * sizeof(uint32_t);
    if (st.meshletCounts.bytes < countBytes || !st.meshletCounts.ptr)
    {
        if ((rc = grow_to(st.meshletCounts, countBytes, s)) != PROSPER_PT_OK) return rc;
        st.countsDirty = true;
    }
    if (st.countsDirty)
    {
        PPT_HIP(hipMemcpyAsync(st.meshletCounts.ptr, st.hostMeshletCounts.data(), countBytes, hipMemcpyHostToDevice, s));
        st.countsDirty = false;
    }
    for (DeviceBuffer &l : st.lists) PPT_HIP(hipMemsetAsync(l.ptr, 0, 4u, s));
    PPT_HIP(hipMemsetAsync(st.argsAndStats.ptr, 0, kArgsWords * 4u + sizeof(DrawListStats), s));
    st.upperBound = upperBound;
    st.totals = totals;

    DrawListGeneratorParams g = {};
    g.drawInstances = ctx->scene.drawInstances;
    g.materials = ctx->scene.materials;
    g.meshletCounts = st.meshletCounts.as<uint32_t>();
    g.drawInstanceCount = ctx->scene.drawInstanceCount;
    g.matchTransparents = mode == PROSPER_PT_CULL_MODE_TRANSPARENT ? 1u : 0u;
    g.outList = st.lists[PROSPER_PT_DRAW_LIST_GENERATED].as<uint32_t>();
    g.capacity = st.capacity;
    st.firstTimed = st.secondTimed = false;
    if ((rc = st.firstTiming.create()) != PROSPER_PT_OK) return rc;
    PPT_HIP(hipEventRecord(st.firstTiming.events[0], s));
    launch_draw_list_generator(g, s);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(st.firstTiming.events[1], s));
    const bool withHiz = hizSlot != PROSPER_PT_NO_HIZ;
    rc = run_culler(ctx, p, PROSPER_PT_DRAW_LIST_GENERATED, PROSPER_PT_DRAW_LIST_FIRST_PHASE,
                    withHiz ? (int)PROSPER_PT_DRAW_LIST_SECOND_PHASE_INPUT : -1, 0, st.firstTiming.events[2], s);
    st.firstTimed = rc == PROSPER_PT_OK;
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.done.record(s)) != PROSPER_PT_OK) return rc;
    st.listValid[PROSPER_PT_DRAW_LIST_GENERATED] = st.listValid[PROSPER_PT_DRAW_LIST_FIRST_PHASE] = true;
    st.listValid[PROSPER_PT_DRAW_LIST_SECOND_PHASE_INPUT] = withHiz;
    return mark_versions_read(ctx, s);
}

int second_phase(prosper_pt_ctx *ctx, const char *what, const prosper_CameraUniforms *camera, uint32_t hizSlot, hipStream_t s)
{
    int rc = check_scene(ctx, what);
    if (rc != PROSPER_PT_OK) return rc;
    CullingPassState &st = *ctx->cullingPasses;
    if (!st.listValid[PROSPER_PT_DRAW_LIST_FIRST_PHASE] || !st.listValid[PROSPER_PT_DRAW_LIST_SECOND_PHASE_INPUT])
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": no first phase has left a second-phase input");
    if ((rc = flush_scene_updates(ctx, s, s)) != PROSPER_PT_OK) return rc;
    if ((rc = check_meshlet_ranges(ctx, what)) != PROSPER_PT_OK) return rc;
    DrawListCullerParams p = {};
    if ((rc = set_view(ctx, what, camera, hizSlot, p)) != PROSPER_PT_OK) return rc;
    if ((rc = st.done.wait(s)) != PROSPER_PT_OK) return rc;
    if ((rc = st.hiz[hizSlot].done.wait(s)) != PROSPER_PT_OK) return rc;
    st.listValid[PROSPER_PT_DRAW_LIST_SECOND_PHASE] = false;
    PPT_HIP(hipMemsetAsync(st.lists[PROSPER_PT_DRAW_LIST_SECOND_PHASE].ptr, 0, 4u, s));
    PPT_HIP(hipMemsetAsync(st.argsAndStats.as<uint32_t>() + 3u, 0, 12u, s));
    st.secondTimed = false;
    if ((rc = st.secondTiming.create()) != PROSPER_PT_OK) return rc;
    PPT_HIP(hipEventRecord(st.secondTiming.events[0], s));
    rc = run_culler(ctx, p, PROSPER_PT_DRAW_LIST_SECOND_PHASE_INPUT, PROSPER_PT_DRAW_LIST_SECOND_PHASE, -1, 1, st.secondTiming.events[1], s);
    st.secondTimed = rc == PROSPER_PT_OK;
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.done.record(s)) != PROSPER_PT_OK) return rc;
    st.listValid[PROSPER_PT_DRAW_LIST_SECOND_PHASE] = true;
    return mark_versions_read(ctx, s);
}

} // namespace

extern "C" {

int prosper_pt_hiz_downsample(
    prosper_pt_ctx *ctx, uint32_t slot, const float *nonLinearDepth, uint32_t onDevice, uint32_t width, uint32_t height,
    void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (slot > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_hiz_downsample: slot is 0 or 1");
    HizLayout layout = {};
    if (!hiz_layout(width, height, &layout))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_hiz_downsample: width and height are above 1 and at most 4096");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_hiz_downsample: null argument");
    const float *depth = nullptr;
    if (const int drc = resolve_depth(ctx, "prosper_pt_hiz_downsample", nonLinearDepth, onDevice != 0u, width, height, &depth)) return drc;
    CullingPassState::HizSlot &st = ctx->cullingPasses->hiz[slot];
    st.valid = false;
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the previous call into the slot may have run on another stream: `s` takes up behind its kernels, so that a grow
    // (which waits for `s` before it frees) and this call's writes never touch a buffer that call still uses
    int rc = st.done.wait(s);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = grow_to(st.pyramid, layout.floats * sizeof(float), s)) != PROSPER_PT_OK) return rc;
    if ((rc = stage_depth(st.hostDepth, 0, nonLinearDepth, (size_t)width * height, s, &depth)) != PROSPER_PT_OK) return rc;
    launch_hiz_downsample(depth, width, height, st.pyramid.as<float>(), layout, s);
    PPT_HIP(hipGetLastError());
    if ((rc = st.done.record(s)) != PROSPER_PT_OK) return rc;
    st.layout = layout;
    st.sourceWidth = width;
    st.sourceHeight = height;
    st.launches = layout.levelCount > kHizLevelsPerLaunch ? 2u : 1u;
    st.valid = true;
    return PROSPER_PT_OK;
}

int prosper_pt_get_hiz_info(prosper_pt_ctx *ctx, uint32_t slot, prosper_pt_hiz_info *out)
{
    if (slot > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_hiz_info: slot is 0 or 1");
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_hiz_info: null argument");
    const CullingPassState::HizSlot &st = ctx->cullingPasses->hiz[slot];
    prosper_pt_hiz_info info = {};
    if (st.valid)
    {
        info.valid = 1u;
        info.width = st.layout.levelW[0];
        info.height = st.layout.levelH[0];
        info.levelCount = st.layout.levelCount;
        info.sourceWidth = st.sourceWidth;
        info.sourceHeight = st.sourceHeight;
        info.launches = st.launches;
    }
    *out = info;
    return PROSPER_PT_OK;
}

int prosper_pt_get_hiz_device_ptr(
    prosper_pt_ctx *ctx, uint32_t slot, uint32_t level, const float **out, uint32_t *width, uint32_t *height)
{
    if (!out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_hiz_device_ptr: null argument");
    CullingPassState::HizSlot *st = nullptr;
    if (const int rc = hiz_level(ctx, "prosper_pt_get_hiz_device_ptr", slot, level, &st)) return rc;
    *out = st->pyramid.as<float>() + st->layout.levelOffset[level];
    if (width) *width = st->layout.levelW[level];
    if (height) *height = st->layout.levelH[level];
    return PROSPER_PT_OK;
}

int prosper_pt_hiz_wait(prosper_pt_ctx *ctx, uint32_t slot, void *stream)
{
    if (slot > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_hiz_wait: slot is 0 or 1");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_hiz_wait: null argument");
    PPT_HIP(hipSetDevice(ctx->device));
    return ctx->cullingPasses->hiz[slot].done.wait(static_cast<hipStream_t>(stream));
}

int prosper_pt_read_hiz_level(prosper_pt_ctx *ctx, uint32_t slot, uint32_t level, float *host, size_t bytes, void *stream)
{
    if (!host) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_hiz_level: null argument");
    CullingPassState::HizSlot *st = nullptr;
    if (const int rc = hiz_level(ctx, "prosper_pt_read_hiz_level", slot, level, &st)) return rc;
    const size_t need = (size_t)st->layout.levelW[level] * st->layout.levelH[level] * sizeof(float);
    if (bytes < need) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_hiz_level: destination too small");
    return read_back(ctx, static_cast<hipStream_t>(stream), {{host, st->pyramid.as<float>() + st->layout.levelOffset[level], need}}, &st->done);
}

int prosper_pt_cull_meshlets_first_phase(
    prosper_pt_ctx *ctx, uint32_t mode, const prosper_CameraUniforms *camera, uint32_t hizSlot, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (mode > PROSPER_PT_CULL_MODE_TRANSPARENT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cull_meshlets_first_phase: unknown mode");
    if (hizSlot > 1u && hizSlot != PROSPER_PT_NO_HIZ)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cull_meshlets_first_phase: hizSlot is 0, 1 or PROSPER_PT_NO_HIZ");
    if (!ctx || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cull_meshlets_first_phase: null argument");
    return first_phase(ctx, "prosper_pt_cull_meshlets_first_phase", mode, camera, hizSlot, static_cast<hipStream_t>(stream));
}

int prosper_pt_cull_meshlets_second_phase(prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, uint32_t hizSlot, void *stream)
{
    if (hizSlot > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cull_meshlets_second_phase: hizSlot is 0 or 1");
    if (!ctx || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cull_meshlets_second_phase: null argument");
    return second_phase(ctx, "prosper_pt_cull_meshlets_second_phase", camera, hizSlot, static_cast<hipStream_t>(stream));
}

int prosper_pt_cull_gbuffer(prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, void *stream)
{
    if (!ctx || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_cull_gbuffer: null argument");
    CullingPassState &st = *ctx->cullingPasses;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the pyramid the previous call kept, if it is of this extent
    uint32_t previous = PROSPER_PT_NO_HIZ;
    if (st.keptHiz >= 0 && st.hiz[st.keptHiz].valid && st.hiz[st.keptHiz].sourceWidth == camera->resolution[0] &&
        st.hiz[st.keptHiz].sourceHeight == camera->resolution[1])
        previous = (uint32_t)st.keptHiz;
    int rc = first_phase(ctx, "prosper_pt_cull_gbuffer", PROSPER_PT_CULL_MODE_OPAQUE, camera, previous, s);
    if (rc != PROSPER_PT_OK) return rc;
    const uint32_t current = previous == PROSPER_PT_NO_HIZ ? 0u : 1u - previous;
    st.keptHiz = -1;
    if ((rc = prosper_pt_hiz_downsample(ctx, current, nullptr, 1u, camera->resolution[0], camera->resolution[1], stream)) != PROSPER_PT_OK)
        return rc;
    if (previous != PROSPER_PT_NO_HIZ && (rc = second_phase(ctx, "prosper_pt_cull_gbuffer", camera, current, s)) != PROSPER_PT_OK) return rc;
    st.keptHiz = (int32_t)current;
    return PROSPER_PT_OK;
}

int prosper_pt_read_draw_list(
    prosper_pt_ctx *ctx, uint32_t which, uint32_t *count, uint32_t *pairs, uint32_t capacity, uint32_t args3[3], void *stream)
{
    if (which >= PROSPER_PT_DRAW_LIST_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_draw_list: unknown list");
    if (!ctx || !count || (capacity != 0u && !pairs)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_draw_list: null argument");
    CullingPassState &st = *ctx->cullingPasses;
    if (!st.listValid[which]) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_draw_list: the last culling calls did not produce this list");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = st.done.wait(s)) return rc;
    uint32_t n = 0, args[3] = {};
    PPT_HIP(hipMemcpyAsync(&n, st.lists[which].ptr, 4u, hipMemcpyDeviceToHost, s));
    const bool culled = which == PROSPER_PT_DRAW_LIST_FIRST_PHASE || which == PROSPER_PT_DRAW_LIST_SECOND_PHASE;
    if (culled)
        PPT_HIP(hipMemcpyAsync(args, st.argsAndStats.as<uint32_t>() + (which == PROSPER_PT_DRAW_LIST_FIRST_PHASE ? 0u : 3u), 12u, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    if (n > st.capacity) n = st.capacity;
    const uint32_t take = n < capacity ? n : capacity;
    if (take)
    {
        PPT_HIP(hipMemcpyAsync(pairs, st.lists[which].as<uint32_t>() + 1, (size_t)take * 8u, hipMemcpyDeviceToHost, s));
        PPT_HIP(hipStreamSynchronize(s));
    }
    *count = n;
    if (args3) std::memcpy(args3, args, 12u);
    return PROSPER_PT_OK;
}

int prosper_pt_get_draw_list_device_ptr(
    prosper_pt_ctx *ctx, uint32_t which, const uint32_t **list, const uint32_t **args3, uint32_t *capacity)
{
    if (which >= PROSPER_PT_DRAW_LIST_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_draw_list_device_ptr: unknown list");
    if (!ctx || !list) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_draw_list_device_ptr: null argument");
    const CullingPassState &st = *ctx->cullingPasses;
    if (!st.listValid[which]) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_get_draw_list_device_ptr: the last culling calls did not produce this list");
    *list = st.lists[which].as<uint32_t>();
    if (args3)
        *args3 = which == PROSPER_PT_DRAW_LIST_FIRST_PHASE    ? st.argsAndStats.as<uint32_t>()
                 : which == PROSPER_PT_DRAW_LIST_SECOND_PHASE ? st.argsAndStats.as<uint32_t>() + 3
                                                              : nullptr;
    if (capacity) *capacity = st.capacity;
    return PROSPER_PT_OK;
}

int prosper_pt_get_draw_stats(prosper_pt_ctx *ctx, prosper_pt_draw_stats *out, uint32_t wait)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_draw_stats: null argument");
    CullingPassState &st = *ctx->cullingPasses;
    if (!st.statsQueued || !st.listValid[PROSPER_PT_DRAW_LIST_FIRST_PHASE])
        return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_get_draw_stats: no culling call has run on this scene");
    PPT_HIP(hipSetDevice(ctx->device));
    if (wait)
    {
        if (const int rc = st.statsDone.host_wait()) return rc;
    }
    else if (!st.statsDone.passed())
    {
        *out = st.totals; // (the host's totals are known; the two device counts stay zero)
        return PROSPER_PT_NOT_READY;
    }
    prosper_pt_draw_stats r = st.totals;
    r.drawnMeshletCount = st.statsHost.ptr->drawnMeshlets;
    r.rasterizedTriangleCount = st.statsHost.ptr->rasterizedTriangles;
    *out = r;
    return PROSPER_PT_OK;
}

int prosper_pt_get_cull_stage_ms(prosper_pt_ctx *ctx, float ms[3])
{
    if (!ctx || !ms) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_cull_stage_ms: null argument");
    CullingPassState &st = *ctx->cullingPasses;
    ms[0] = ms[1] = ms[2] = 0.0f;
    if (!st.firstTimed || !st.listValid[PROSPER_PT_DRAW_LIST_FIRST_PHASE])
        return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_get_cull_stage_ms: no culling call has run on this scene");
    PPT_HIP(hipSetDevice(ctx->device));
    if (const int rc = st.firstTiming.elapsed(ms)) return rc;
    if (st.secondTimed)
        if (const int rc = st.secondTiming.elapsed(ms + 2)) return rc;
    return PROSPER_PT_OK;
}

int prosper_pt_read_instance_scales(prosper_pt_ctx *ctx, float *host, uint32_t count, void *stream)
{
    if (!ctx || !host) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_instance_scales: null argument");
    int rc = check_scene(ctx, "prosper_pt_read_instance_scales");
    if (rc != PROSPER_PT_OK) return rc;
    if (count != ctx->scene.modelInstanceCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_instance_scales: count is not the scene's model instance count");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = flush_scene_updates(ctx, s, s)) != PROSPER_PT_OK) return rc;
    const AccelState *acc = ctx->accel;
    const float *scales = acc ? acc->dScalesV[acc->versions.cur] : nullptr;
    if (!scales) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_instance_scales: the scene version has no scales");
    if (count) PPT_HIP(hipMemcpyAsync(host, scales, sizeof(float) * count, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return mark_versions_read(ctx, s);
}

} // extern "C"
