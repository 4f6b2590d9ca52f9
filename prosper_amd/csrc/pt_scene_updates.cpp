// pt_scene_updates.cpp — the updates of an uploaded scene: prosper_pt_update_lights, prosper_pt_update_transforms*,
// prosper_pt_animate.  Each call only STAGES its update; the next consumer of the scene flushes it into the next version on
// its own stream (flush_scene_updates), so the frames in flight go on reading theirs.
#include "pt_scene_updates.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "pt_animation.hpp"
#include "pt_geometry.hpp"
#include "pt_kernels.hpp"
#include "pt_materials.hpp"
#include "pt_pass_support.hpp"
#include "pt_scene.hpp"

namespace ppt
{

namespace
{

// the next light version, ready to be written on `stream`: its block allocated at first need, its last readers waited for
int next_light_version(prosper_pt_ctx *ctx, LightState *ls, hipStream_t stream, uint32_t *out)
{
    const uint32_t v = ls->versions.next();
    int rc;
    if (!ls->dBlocks[v])
    {
        void *d = nullptr;
        if ((rc = device_alloc(ctx, sizeof(LightBlock), &d))) return rc;
        ls->dBlocks[v] = static_cast<LightBlock *>(d);
    }
    if ((rc = ls->versions.wait_free(v, stream))) return rc;
    *out = v;
    return PROSPER_PT_OK;
}

// the staged light set into the next device version, on the stream of the render that is about to read it
int flush_pending_lights(prosper_pt_ctx *ctx, hipStream_t stream)
{
    LightState *ls = ctx->lights;
    if (!ls || !ls->pending) return PROSPER_PT_OK;
    uint32_t v = 0;
    int rc;
    if ((rc = next_light_version(ctx, ls, stream, &v))) return rc;
    const LightBlock *staged = ls->staging.pending_buffer();
    PPT_HIP(hipMemcpyAsync(ls->dBlocks[v], staged, sizeof(LightBlock), hipMemcpyHostToDevice, stream));
    if ((rc = ls->staging.copy_enqueued(stream))) return rc;
    if ((rc = ls->ready.record(stream))) return rc;
    ls->versions.commit(v);
    point_scene_at_lights(ctx->scene, ls->dBlocks[v]);
    ctx->scene.pointLightCount = staged->points.count;
    ctx->scene.spotLightCount = staged->spots.count;
    ls->pending = false;
    ls->updates++;
    return PROSPER_PT_OK;
}

} // namespace

// World::updateScene + the per-frame TLAS rebuild (World.cpp:359-466,749-802,878-928) as a REFIT: the new transforms, the
// world triangles and new boxes for the unchanged tree - no host build, no device-wide synchronisation.  Hits do not
// depend on the hierarchy (hit contract), so the image is the one a fresh upload gives.  Two steps:
//   stage_transforms      the call itself: which instances moved, the table into pinned staging; nothing on the GPU
//   flush_pending_update  run by the next consumer of the scene on ITS stream - a pipelined render's own chain - into the
//                         NEXT scene version: the frames in flight go on reading theirs, nothing waits for them
// What a refit cannot do is keep the tree GOOD when instances travel far: every refit leaves the tree's surface-area
// measure behind, and once that has grown by 30 % over its value at the last build the next update rebuilds
// (pt_rebuild_policy.hpp).
int flush_pending_update(prosper_pt_ctx *ctx, hipStream_t stream)
{
    AccelState *acc = ctx->accel;
    if (!acc) return PROSPER_PT_OK;
    // a staged prosper_pt_animate: the table of the new version is the staged one (or the current one) with the entries
    // the scene's nodes bind evaluated over it, ahead of the refit
    const bool animate = animation_pending(ctx);
    if (!acc->pending && !animate) return PROSPER_PT_OK;
    const uint32_t tableCount = acc->pending ? acc->pendingCount : (uint32_t)acc->transforms.size();
    const uint32_t v = acc->versions.next();
    const size_t transformBytes = sizeof(prosper_ModelInstanceTransforms) * (tableCount ? tableCount : 1);
    const size_t triBytes = sizeof(WorldTriangle) * (size_t)(acc->total ? acc->total : 1);
    void *d = nullptr;
    int rc;
    if (!acc->dTransformsV[v])
    {
        if ((rc = device_alloc(ctx, transformBytes, &d))) return rc;
        acc->dTransformsV[v] = static_cast<prosper_ModelInstanceTransforms *>(d);
    }
    if (!acc->dTrisV[v])
    {
        if ((rc = device_alloc(ctx, triBytes, &d))) return rc;
        acc->dTrisV[v] = static_cast<WorldTriangle *>(d);
    }
    if (!acc->dNodesV[v])
    {
        if ((rc = device_alloc(ctx, acc->nodeCapacityBytes, &d))) return rc;
        acc->dNodesV[v] = static_cast<BvhNode *>(d);
        acc->nodesCurrent[v] = false;
    }
    // Everything is enqueued for version v through LOCAL names; the context switches to v only after the last call has
    // succeeded.  On a failure the previous version stays current and the update stays pending (the next consumer of the
    // scene tries again); what was half-written into v is rewritten by that retry.
    // the version's last readers (three updates ago), and the previous update: it wrote the node array copied below,
    // and it shares the flat triangle array and the bounds scratch with this one
    if ((rc = acc->versions.wait_free(v, stream))) return rc;
    if ((rc = acc->sceneDone.wait(stream))) return rc;
    if (!acc->nodesCurrent[v])
    {
        PPT_HIP(hipMemcpyAsync(acc->dNodesV[v], acc->dNodes, (size_t)acc->nodeCount * sizeof(BvhNode), hipMemcpyDeviceToDevice, stream));
        acc->nodesCurrent[v] = true;
    }
    if (acc->pending)
    {
        PPT_HIP(hipMemcpyAsync(acc->dTransformsV[v], acc->staging.pending_buffer(), sizeof(prosper_ModelInstanceTransforms) * acc->pendingCount, hipMemcpyHostToDevice, stream));
        if ((rc = acc->staging.copy_enqueued(stream))) return rc;
    }
    else if (tableCount)
        PPT_HIP(hipMemcpyAsync(acc->dTransformsV[v], ctx->dTransforms, sizeof(prosper_ModelInstanceTransforms) * tableCount, hipMemcpyDeviceToDevice, stream));
    // The lights its nodes carry go into the next light version, a copy of the current one, ordered like a flushed
    // prosper_pt_update_lights (a staged one is flushed first: it is what the copy starts from).
    LightState *ls = ctx->lights;
    const bool animateLights = animate && ls && animation_moves_lights(ctx);
    uint32_t lv = 0;
    if (animateLights)
    {
        if ((rc = flush_pending_lights(ctx, stream))) return rc;
        if ((rc = next_light_version(ctx, ls, stream, &lv))) return rc;
        if ((rc = ls->ready.wait(stream))) return rc;
        PPT_HIP(hipMemcpyAsync(ls->dBlocks[lv], ls->dBlocks[ls->versions.cur], sizeof(LightBlock), hipMemcpyDeviceToDevice, stream));
        if ((rc = ls->versions.mark_read(stream))) return rc; // (the copy read the current version)
    }
    if (animate && (rc = enqueue_animation(ctx, acc->dTransformsV[v], tableCount, animateLights ? ls->dBlocks[lv] : nullptr, stream))) return rc;
    if (animateLights && (rc = ls->ready.record(stream))) return rc;
    if ((rc = enqueue_instance_scales(ctx, acc, v, acc->dTransformsV[v], tableCount, stream))) return rc;
    // world-space triangles again, in both orders (the shading and any-hit records hold object-space attributes and stay
    // as they are), then the boxes.  (Also when only transforms of instances without geometry changed: a version must be
    // whole.)
    DeviceScene next = ctx->scene;
    next.nodes = acc->dNodesV[v];
    next.triangles = acc->dTrisV[v];
    next.modelInstanceTransforms = acc->dTransformsV[v];
    launch_flatten_triangles(
        next, acc->dOffsets, acc->drawInstanceCount, acc->dFlags, acc->dFlat, nullptr, nullptr, (uint32_t)acc->total, stream,
        acc->dLeafPosition, acc->dTrisV[v]);
    PPT_HIP(hipGetLastError());
    acc->flatStale = true; // (the flat array now holds the new pose whatever happens next)
    if (acc->total && (rc = enqueue_refit(acc, bvh_pad_coefficient(build_options(ctx)), acc->dNodesV[v], acc->dTrisV[v], v, stream))) return rc;
    if (acc->total && acc->foreignTree && (rc = enqueue_nest_boxes(acc, acc->dNodesV[v], stream))) return rc;
    if ((rc = acc->sceneDone.record(stream))) return rc;
    // ---- commit: the new version becomes the scene ----
    acc->versions.commit(v);
    acc->dNodes = acc->dNodesV[v];
    acc->dTris = acc->dTrisV[v];
    ctx->dTransforms = acc->dTransformsV[v];
    ctx->scene = next;
    acc->refits++;
    acc->pending = false;
    acc->stale = false;
    if (animateLights)
    {
        ls->versions.commit(lv);
        point_scene_at_lights(ctx->scene, ls->dBlocks[lv]);
        ls->updates++;
    }
    if (animate) animation_committed(ctx);
    return PROSPER_PT_OK;
}

int check_scene(prosper_pt_ctx *ctx, const char *what)
{
    if (!ctx->haveScene) return fail(PROSPER_PT_ERR_NO_SCENE, std::string(what) + " called before prosper_pt_upload_scene");
    if (ctx->meshBuild)
    {
        const int prc = poll_mesh_build(ctx, false);
        if (prc != PROSPER_PT_OK) return prc;
    }
    if (ctx->accel && ctx->accel->stale && !ctx->accel->pending)
        return fail(PROSPER_PT_ERR_NO_SCENE, "the last prosper_pt_update_transforms failed: update the transforms again (or upload the scene) before tracing");
    return PROSPER_PT_OK;
}

int flush_scene_updates(prosper_pt_ctx *ctx, hipStream_t s, hipStream_t reader)
{
    PPT_HIP(hipSetDevice(ctx->device));
    int rc = flush_pending_update(ctx, s);
    if (rc == PROSPER_PT_OK) rc = flush_pending_lights(ctx, s);
    if (rc == PROSPER_PT_OK) rc = flush_pending_materials(ctx, s);
    // a flush enqueued on another stream than the reader's (a pipelined render's chain, this one's or an earlier one's, or
    // prosper_pt_update_transforms_async) must be done before anything on the reader's stream reads the scene
    if (rc == PROSPER_PT_OK && ctx->lights) rc = ctx->lights->ready.wait(reader);
    if (rc == PROSPER_PT_OK && ctx->materialState) rc = ctx->materialState->ready.wait(reader);
    if (rc == PROSPER_PT_OK && ctx->accel) rc = ctx->accel->sceneDone.wait(reader);
    return rc;
}

// The scene and light versions a render (or a pass over a G-buffer) read are free again behind its last kernel on `s` (the
// accumulate kernel follows the path stages on the caller's stream): VersionRing::mark_read.
int mark_versions_read(prosper_pt_ctx *ctx, hipStream_t s)
{
    int rc = PROSPER_PT_OK;
    if (ctx->accel) rc = ctx->accel->versions.mark_read(s);
    if (rc == PROSPER_PT_OK && ctx->lights) rc = ctx->lights->versions.mark_read(s);
    if (rc == PROSPER_PT_OK && ctx->materialState) rc = ctx->materialState->versions.mark_read(s);
    return rc;
}

int stage_transforms(prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count)
{
    AccelState *acc = ctx->accel;
    if (const int src = sync_animation_mirrors(ctx)) return src; // (the table an animated update left on the device)
    const auto t0 = std::chrono::steady_clock::now();
    // which instances moved (World::updateScene rewrites every transform each frame, World.cpp:359-466; most are unchanged)
    bool any = acc->stale;
    for (size_t r = 0; r < acc->ranges.size(); ++r)
    {
        const uint32_t mi = acc->rangeModelInstance[r];
        if (acc->stale || std::memcmp(&transforms[mi], &acc->transforms[mi], sizeof(prosper_ModelInstanceTransforms)) != 0)
        {
            acc->movedSinceBuild[r] = 1;
            any = true;
        }
    }
    if (!any && std::memcmp(transforms, acc->transforms.data(), sizeof(prosper_ModelInstanceTransforms) * count) == 0) return PROSPER_PT_OK;
    PPT_HIP(hipSetDevice(ctx->device));
    // the measure of the newest refit that has finished (the newest may still be queued behind frames in flight)
    {
        const int prc = poll_refit_cost(acc, false);
        if (prc != PROSPER_PT_OK) return prc;
    }
    // into pinned staging (a pageable source would make the later copy synchronous).  An update that was never consumed
    // is simply replaced: its staging buffer is reused.
    prosper_ModelInstanceTransforms *staged = nullptr;
    if (const int rc = acc->staging.acquire(sizeof(prosper_ModelInstanceTransforms) * (count ? count : 1), acc->pending, &staged)) return rc;
    std::memcpy(staged, transforms, sizeof(prosper_ModelInstanceTransforms) * count);
    acc->pending = true;
    acc->pendingCount = count;
    acc->transforms.assign(transforms, transforms + count);
    ctx->stats.bvhBuildSeconds = 0.0;
    ctx->stats.buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    switch (decide_rebuild(ctx, any))
    {
    case RebuildDecision::Synchronous: return rebuild_hierarchy(ctx);
    // The refits have degraded the tree: the instances that moved since the last build are split again - by the worker
    // thread that also takes up streamed-in meshes, into a new geometry generation, while the frame loop goes on
    // refitting and rendering this one (until round 4 this was a 60-75 ms synchronous rebuild in the middle of the
    // frame loop).  The generation is switched in by the first render after it is done.
    case RebuildDecision::Background: return start_mesh_build(ctx, true);
    case RebuildDecision::None: break;
    }
    return PROSPER_PT_OK;
}

namespace
{

int update_transforms(prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count, hipStream_t stream, bool flushNow)
{
    const int rc = stage_transforms(ctx, transforms, count);
    if (rc != PROSPER_PT_OK || !flushNow) return rc;
    return flush_pending_update(ctx, stream);
}

int check_update_arguments(prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count)
{
    if (!ctx || !transforms) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_update_transforms: null argument");
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    if (count != ctx->accel->transforms.size())
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_update_transforms: count differs from the scene's modelInstanceCount");
    return PROSPER_PT_OK;
}

} // namespace

} // namespace ppt

using namespace ppt;

extern "C" {

int prosper_pt_update_lights(
    prosper_pt_ctx *ctx, const prosper_DirectionalLightParameters *directionalLight,
    const prosper_PointLightsBuffer *pointLights, const prosper_SpotLightsBuffer *spotLights)
{
    if (!ctx || !directionalLight || !pointLights || !spotLights)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_update_lights: null argument");
    if (!ctx->haveScene || !ctx->lights) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    if (pointLights->count > PROSPER_MAX_POINT_LIGHT_COUNT || spotLights->count > PROSPER_MAX_SPOT_LIGHT_COUNT)
        return fail(PROSPER_PT_ERR_SCENE, "light count exceeds 1024");
    LightState *ls = ctx->lights;
    if (const int rc = sync_animation_mirrors(ctx)) return rc; // (an animated update may have moved the lights)
    // prosper rewrites the buffers every frame (World.cpp:531-535) and mostly with what they held: that costs a memcmp
    if (std::memcmp(&ls->mirror->directional, directionalLight, sizeof(*directionalLight)) == 0 &&
        std::memcmp(&ls->mirror->points, pointLights, sizeof(*pointLights)) == 0 &&
        std::memcmp(&ls->mirror->spots, spotLights, sizeof(*spotLights)) == 0)
        return PROSPER_PT_OK;
    PPT_HIP(hipSetDevice(ctx->device));
    LightBlock *staged = nullptr;
    if (const int rc = ls->staging.acquire(sizeof(LightBlock), ls->pending, &staged)) return rc;
    staged->directional = *directionalLight;
    staged->points = *pointLights;
    staged->spots = *spotLights;
    *ls->mirror = *staged;
    ls->pending = true;
    return PROSPER_PT_OK;
}

int prosper_pt_update_transforms(prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count)
{
    const int rc = check_update_arguments(ctx, transforms, count);
    return rc != PROSPER_PT_OK ? rc : update_transforms(ctx, transforms, count, nullptr, false);
}

int prosper_pt_update_transforms_async(
    prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count, uint32_t flags, void *stream)
{
    if (flags & ~(uint32_t)PROSPER_PT_UPDATE_NOW) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_update_transforms_async: unknown flag");
    const int rc = check_update_arguments(ctx, transforms, count);
    return rc != PROSPER_PT_OK ? rc : update_transforms(ctx, transforms, count, static_cast<hipStream_t>(stream), (flags & PROSPER_PT_UPDATE_NOW) != 0);
}

int prosper_pt_animate(prosper_pt_ctx *ctx, float timeS, uint32_t flags, void *stream)
{
    if (flags & ~(uint32_t)PROSPER_PT_UPDATE_NOW) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_animate: unknown flag");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_animate: null argument");
    if (!std::isfinite(timeS)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_animate: timeS is not finite");
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    int rc = stage_animation(ctx, timeS);
    if (rc != PROSPER_PT_OK) return rc;
    // like a staged table (stage_transforms): refits leave the tree's measure behind, and once it has grown too far the
    // instances that moved are split again in the background
    PPT_HIP(hipSetDevice(ctx->device));
    if ((rc = poll_refit_cost(ctx->accel, false))) return rc;
    switch (decide_rebuild(ctx, true))
    {
    case RebuildDecision::Synchronous: return rebuild_hierarchy(ctx); // (it has flushed the animation)
    case RebuildDecision::Background:
        if ((rc = start_mesh_build(ctx, true))) return rc;
        break;
    case RebuildDecision::None: break;
    }
    if (!(flags & PROSPER_PT_UPDATE_NOW)) return PROSPER_PT_OK;
    return flush_pending_update(ctx, static_cast<hipStream_t>(stream));
}

} // extern "C"
