// pt_hierarchy.cpp — the hierarchy of an uploaded scene as the caller steers and inspects it: the synchronous rebuild by either
// builder (prosper_pt_rebuild_hierarchy, prosper_pt_build_hierarchy_gpu), when an update asks for a rebuild (decide_rebuild),
// the builder / method / site selection, and the queries and debug read-backs of the tree.  The builds themselves are
// pt_geometry.cpp's.
#include "pt_scene_updates.hpp"

#include <algorithm>
#include <chrono>
#include <exception>
#include <stdexcept>
#include <string>

#include "bvh_build.hpp"
#include "pt_animation.hpp"
#include "pt_bvh_build.hpp"
#include "pt_bvh_ploc_rule.hpp"
#include "pt_geometry.hpp"
#include "pt_scene.hpp"

namespace ppt
{

namespace
{

// The synchronous path: re-split the instances that moved since the last build, re-assemble, upload (what
// prosper_pt_update_transforms did before the refit existed; prosper's own TLAS build is of this kind, on the GPU).
int build_on_host(prosper_pt_ctx *ctx, AccelState *acc)
{
    acc->stale = true; // until the new hierarchy is up
    bool any = false;
    if (acc->flat.size() != (size_t)acc->total) acc->flat.resize((size_t)acc->total); // (a first tree built on the GPU kept no host copy)
    for (size_t r = 0; r < acc->ranges.size(); ++r)
    {
        if (!(acc->movedSinceBuild[r] || !acc->instanced) || !acc->ranges[r].count) continue;
        any = any || acc->movedSinceBuild[r];
        PPT_HIP(hipMemcpy(
            acc->flat.data() + acc->ranges[r].first, acc->dFlat + acc->ranges[r].first,
            sizeof(WorldTriangle) * (size_t)acc->ranges[r].count, hipMemcpyDeviceToHost));
    }
    BvhBuildResult bvh;
    bool instancedNow = acc->instanced;
    const auto tBuild = std::chrono::steady_clock::now();
    try
    {
        if (ctx->debug.failNextUpdate)
        {
            ctx->debug.failNextUpdate = 0;
            throw std::runtime_error("debug option failNextUpdate is set");
        }
        if (acc->instanced)
            bvh = acc->bvh.rebuild(acc->flat.data(), acc->movedSinceBuild, build_options(ctx));
        else if (acc->foreignTree && ctx->debug.flatBvh == 0)
        {
            // the last build ran on the GPU: no subtree is kept, every instance is split as the scene's first build
            // splits it (begin_geometry), with the same way out for a spliced tree that is too deep
            try
            {
                bvh = acc->bvh.build(acc->flat.data(), acc->total, acc->ranges, build_options(ctx));
                instancedNow = true;
            }
            catch (const std::exception &)
            {
                bvh = build_bvh(acc->flat.data(), acc->total, build_options(ctx));
            }
        }
        else
            bvh = build_bvh(acc->flat.data(), acc->total, build_options(ctx));
    }
    catch (const std::exception &ex)
    {
        return fail(PROSPER_PT_ERR_UNSUPPORTED, std::string("BVH rebuild failed: ") + ex.what());
    }
    const double buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tBuild).count();
    GeometryTarget target = context_target(ctx);
    const int rc = upload_hierarchy(ctx, target, bvh);
    if (rc != PROSPER_PT_OK) return rc;
    acc->stale = false;
    acc->instanced = instancedNow;
    acc->foreignTree = false;
    acc->gpuStagesValid = false;
    ctx->stats.nodeCount = bvh.nodes.size();
    ctx->stats.maxDepth = bvh.maxDepth;
    ctx->stats.bvhBuildSeconds = buildSeconds;
    return PROSPER_PT_OK;
}

// The same contract with the tree made on the GPU (pt_bvh_build.hpp): the linear BVH over the device's own
// flat world triangles.  A tree the traversal cannot hold is refused and the scene stays exactly as it was.
int build_on_gpu(prosper_pt_ctx *ctx)
{
    const auto tBuild = std::chrono::steady_clock::now();
    GeometryTarget target = context_target(ctx);
    const int rc = build_hierarchy_on_device(ctx, target);
    if (rc != PROSPER_PT_OK) return rc;
    ctx->stats.bvhBuildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tBuild).count();
    return PROSPER_PT_OK;
}

// What either builder's synchronous rebuild goes through: a pending background geometry is installed first, a staged update
// flushed, the device synchronised; then the build, and what it took.
int rebuild_hierarchy_with(prosper_pt_ctx *ctx, uint32_t builder)
{
    PPT_HIP(hipSetDevice(ctx->device));
    {
        // a background build of streamed-in meshes holds the subtrees: its result is installed first
        const int prc = poll_mesh_build(ctx, true);
        if (prc != PROSPER_PT_OK) return prc;
    }
    AccelState *acc = ctx->accel;
    // (an empty scene has nothing to build on the device and takes the host's path)
    const bool onGpu = builder == PROSPER_PT_BUILDER_GPU && acc->total != 0;
    const auto t0 = std::chrono::steady_clock::now();
    {
        int frc = flush_pending_update(ctx, nullptr); // the moved triangles must be in the flat array
        if (frc == PROSPER_PT_OK) frc = sync_animation_mirrors(ctx);
        if (frc != PROSPER_PT_OK) return frc;
    }
    PPT_HIP(hipDeviceSynchronize()); // renders in flight read the old hierarchy
    const int rc = onGpu ? build_on_gpu(ctx) : build_on_host(ctx, acc);
    if (rc != PROSPER_PT_OK) return rc;
    acc->rebuilds++;
    ctx->stats.deviceBytes = ctx->sceneBytes;
    ctx->stats.buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return PROSPER_PT_OK;
}

float rebuild_cost_ratio(const prosper_pt_ctx *ctx)
{
    return ctx->debug.rebuildCostRatio > 0.0f ? std::max(1.0f, ctx->debug.rebuildCostRatio) : 1.3f;
}

} // namespace

int rebuild_hierarchy(prosper_pt_ctx *ctx) { return rebuild_hierarchy_with(ctx, ctx->hierarchyBuilder); }

RebuildDecision decide_rebuild(const prosper_pt_ctx *ctx, bool moved)
{
    return rebuild_policy(
        moved, ctx->accel->lastCostRatio, rebuild_cost_ratio(ctx), ctx->debug.alwaysRebuild != 0,
        (ctx->gpuHierarchySites & PROSPER_PT_GPU_BUILD_SITE_DRIFT) != 0, ctx->hierarchyBuilder == PROSPER_PT_BUILDER_GPU,
        ctx->meshBuild != nullptr);
}

} // namespace ppt

using namespace ppt;

extern "C" {

int prosper_pt_rebuild_hierarchy(prosper_pt_ctx *ctx)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_rebuild_hierarchy: null argument");
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    return rebuild_hierarchy(ctx);
}

int prosper_pt_build_hierarchy_gpu(prosper_pt_ctx *ctx)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_build_hierarchy_gpu: null argument");
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    return rebuild_hierarchy_with(ctx, PROSPER_PT_BUILDER_GPU);
}

int prosper_pt_set_hierarchy_builder(prosper_pt_ctx *ctx, uint32_t builder)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_hierarchy_builder: null argument");
    if (builder != PROSPER_PT_BUILDER_HOST && builder != PROSPER_PT_BUILDER_GPU)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_hierarchy_builder: unknown builder");
    ctx->hierarchyBuilder = builder;
    return PROSPER_PT_OK;
}

int prosper_pt_set_gpu_hierarchy_method(prosper_pt_ctx *ctx, uint32_t method, uint32_t radius)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_gpu_hierarchy_method: null argument");
    if (method != PROSPER_PT_GPU_HIERARCHY_LINEAR && method != PROSPER_PT_GPU_HIERARCHY_PLOC)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_gpu_hierarchy_method: unknown method");
    if (radius > kPlocMaxRadius) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_gpu_hierarchy_method: the radius is 1 .. 32 (0: the default)");
    ctx->gpuHierarchyMethod = method;
    ctx->gpuHierarchyRadius = radius;
    return PROSPER_PT_OK;
}

int prosper_pt_set_gpu_hierarchy_sites(prosper_pt_ctx *ctx, uint32_t sites)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_gpu_hierarchy_sites: null argument");
    constexpr uint32_t known = PROSPER_PT_GPU_BUILD_SITE_UPLOAD | PROSPER_PT_GPU_BUILD_SITE_MESH_UPDATES | PROSPER_PT_GPU_BUILD_SITE_DRIFT;
    if (sites & ~known) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_gpu_hierarchy_sites: unknown build site");
    ctx->gpuHierarchySites = sites;
    return PROSPER_PT_OK;
}

int prosper_pt_get_gpu_hierarchy_sites(prosper_pt_ctx *ctx, uint32_t *sites)
{
    if (!ctx || !sites) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_gpu_hierarchy_sites: null argument");
    *sites = ctx->gpuHierarchySites;
    return PROSPER_PT_OK;
}

int prosper_pt_get_gpu_hierarchy_method_info(prosper_pt_ctx *ctx, prosper_pt_gpu_hierarchy_method_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_gpu_hierarchy_method_info: null argument");
    *out = prosper_pt_gpu_hierarchy_method_info{};
    out->selectedMethod = ctx->gpuHierarchyMethod;
    out->selectedRadius = ctx->gpuHierarchyRadius ? ctx->gpuHierarchyRadius : kPlocDefaultRadius;
    const AccelState *acc = ctx->haveScene ? ctx->accel : nullptr;
    if (acc && acc->foreignTree)
    {
        out->method = acc->gpuMethod;
        out->radius = acc->gpuRadius;
        out->rounds = acc->gpuRounds;
        out->finishRounds = acc->gpuFinishRounds;
    }
    return PROSPER_PT_OK;
}

int prosper_pt_get_hierarchy_build_info(prosper_pt_ctx *ctx, prosper_pt_hierarchy_build_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_hierarchy_build_info: null argument");
    *out = prosper_pt_hierarchy_build_info{};
    out->selectedBuilder = ctx->hierarchyBuilder;
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    {
        const int prc = ctx->meshBuild ? poll_mesh_build(ctx, false) : PROSPER_PT_OK;
        if (prc != PROSPER_PT_OK) return prc;
    }
    const AccelState *acc = ctx->accel;
    out->builder = acc->foreignTree ? PROSPER_PT_BUILDER_GPU : PROSPER_PT_BUILDER_HOST;
    const uint32_t hostLeaf = ctx->debug.leafSize ? std::min(std::max(ctx->debug.leafSize, 1u), 8u) : kMaxLeafTriangles;
    out->leafSize = acc->foreignTree ? acc->gpuLeafSize : hostLeaf;
    out->nodeCount = acc->nodeCount;
    out->levels = (uint32_t)acc->levelOffsets.size() - 1u;
    out->depths = acc->foreignTree ? acc->gpuDepths : 0u;
    out->stackBound = ctx->stats.maxDepth;
    if (acc->foreignTree && acc->gpuStagesValid)
        for (uint32_t k = 0; k < PROSPER_PT_HIERARCHY_BUILD_STAGES; ++k)
        {
            out->stageMs[k] = acc->gpuStageMs[k];
            out->totalMs += acc->gpuStageMs[k];
        }
    return PROSPER_PT_OK;
}

int prosper_pt_debug_read_hierarchy_arrays(
    prosper_pt_ctx *ctx, void *triangles, size_t triangle_bytes, void *permutation, size_t permutation_bytes)
{
    if (!ctx || !triangles || !permutation) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_read_hierarchy_arrays: null argument");
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    PPT_HIP(hipSetDevice(ctx->device));
    {
        int frc = ctx->meshBuild ? poll_mesh_build(ctx, false) : PROSPER_PT_OK;
        if (frc == PROSPER_PT_OK) frc = flush_pending_update(ctx, nullptr);
        if (frc != PROSPER_PT_OK) return frc;
    }
    const AccelState *acc = ctx->accel;
    const size_t total = (size_t)acc->total;
    if (triangle_bytes < total * sizeof(WorldTriangle) || permutation_bytes < total * sizeof(uint32_t))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_read_hierarchy_arrays: destination too small");
    PPT_HIP(hipDeviceSynchronize());
    if (total)
    {
        PPT_HIP(hipMemcpy(triangles, acc->dFlat, total * sizeof(WorldTriangle), hipMemcpyDeviceToHost));
        PPT_HIP(hipMemcpy(permutation, acc->dPerm, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return PROSPER_PT_OK;
}

int prosper_pt_get_hierarchy_state(prosper_pt_ctx *ctx, prosper_pt_hierarchy_state *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_hierarchy_state: null argument");
    *out = prosper_pt_hierarchy_state{};
    if (ctx->geometry)
    {
        out->meshUpdates = ctx->geometry->meshUpdates;
        out->geometryInstalls = ctx->geometry->installs;
        out->geometryBuildRunning = (ctx->meshBuild || ctx->geometry->dirty) ? 1u : 0u;
    }
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    AccelState *acc = ctx->accel;
    PPT_HIP(hipSetDevice(ctx->device));
    {
        const int frc = flush_pending_update(ctx, nullptr);
        if (frc != PROSPER_PT_OK) return frc;
    }
    {
        const int prc = poll_refit_cost(acc, true);
        if (prc != PROSPER_PT_OK) return prc;
    }
    out->refits = acc->refits;
    out->rebuilds = acc->rebuilds;
    out->costRatio = acc->lastCostRatio;
    out->builtCost = acc->builtCost;
    out->nodeCount = acc->nodeCount;
    out->levels = (uint32_t)acc->levelOffsets.size() - 1u;
    return PROSPER_PT_OK;
}

int prosper_pt_debug_read_nodes(prosper_pt_ctx *ctx, void *out, size_t byte_size)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_read_nodes: null argument");
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    const size_t bytes = (size_t)ctx->accel->nodeCount * sizeof(BvhNode);
    if (byte_size < bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_read_nodes: destination too small");
    PPT_HIP(hipSetDevice(ctx->device));
    {
        const int frc = flush_pending_update(ctx, nullptr);
        if (frc != PROSPER_PT_OK) return frc;
    }
    PPT_HIP(hipDeviceSynchronize());
    PPT_HIP(hipMemcpy(out, ctx->accel->dNodes, bytes, hipMemcpyDeviceToHost));
    return PROSPER_PT_OK;
}

} // extern "C"
