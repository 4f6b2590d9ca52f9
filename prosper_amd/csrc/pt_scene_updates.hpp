// pt_scene_updates.hpp — what the scene's host code shares across its translation units: the upload (pt_scene_upload.cpp), the
// staged updates and their flush (pt_scene_updates.cpp), the synchronous hierarchy rebuild (pt_hierarchy.cpp).  What the pass
// modules use of the updates - check_scene, flush_scene_updates, mark_versions_read - is in pt_pass_support.hpp.  Private to
// the library's translation units.
#pragma once

#include "pt_context.hpp"
#include "pt_rebuild_policy.hpp"

namespace ppt
{

#pragma GCC visibility push(hidden) // (not part of the library's exports)

// ---- pt_scene_upload.cpp ----
// the validated view into a context without a scene (free_scene); on a failure the caller frees what was made
int upload_scene(prosper_pt_ctx *ctx, const prosper_pt_scene_view *v);
// everything of the context that lives as long as its scene; the device is idle
void free_scene(prosper_pt_ctx *ctx);
// the generations a geometry build replaced, with their events and pinned staging; the device is idle
void delete_retired_accel(prosper_pt_ctx *ctx);

// ---- pt_scene_updates.cpp ----
// which instances moved, the table into pinned staging; nothing on the GPU
int stage_transforms(prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count);
// the staged transforms and / or animation time into the next scene version, on the stream of its next consumer
int flush_pending_update(prosper_pt_ctx *ctx, hipStream_t stream);
// the scene reads its lights from `block` (a version of LightState::dBlocks)
inline void point_scene_at_lights(DeviceScene &s, const LightBlock *block)
{
    s.directionalLight = &block->directional;
    s.pointLights = &block->points;
    s.spotLights = &block->spots;
}

// ---- pt_hierarchy.cpp ----
// the synchronous rebuild by the selected builder (prosper_pt_rebuild_hierarchy); flushes a staged update itself
int rebuild_hierarchy(prosper_pt_ctx *ctx);
// rebuild_policy (pt_rebuild_policy.hpp) over the context's state, for an update that has just been staged
RebuildDecision decide_rebuild(const prosper_pt_ctx *ctx, bool moved);

#pragma GCC visibility pop

} // namespace ppt
