// pt_rebuild_policy.hpp — what a scene update does about a tree that refits have degraded: the one statement of the policy
// that prosper_pt_update_transforms* (stage_transforms) and prosper_pt_animate act on (pt_scene_updates.cpp).  A pure function
// over plain values without any include of the runtime, so that tests/rebuild_policy_main.cpp walks its whole table on a CPU.
#pragma once

namespace ppt
{

enum class RebuildDecision
{
    None,        // go on refitting this tree
    Synchronous, // rebuild now, on the calling thread (prosper_pt_rebuild_hierarchy's path)
    Background,  // start a new geometry generation on the worker thread; the frame loop goes on with this one
};

// moved:         the update moves an instance (an animation always does)
// costRatio:     the surface-area measure of the newest finished refit over its value at the last build
// threshold:     the ratio beyond which the tree counts as degraded (debug option rebuildCostRatio; 1.3)
// alwaysRebuild: the debug option - the synchronous path, every time
// driftSite:     site DRIFT of prosper_pt_set_gpu_hierarchy_sites: a background generation from the GPU builder under either
//                selected builder; nothing waits for the device
// gpuBuilder:    prosper_pt_set_hierarchy_builder chose the GPU builder, which is quick enough for the synchronous route (the
//                worker thread is the host builder's) - even while a background build runs
// buildRunning:  a background generation is being built already
inline RebuildDecision rebuild_policy(
    bool moved, float costRatio, float threshold, bool alwaysRebuild, bool driftSite, bool gpuBuilder, bool buildRunning)
{
    if (moved && alwaysRebuild) return RebuildDecision::Synchronous;
    if (!moved || !(costRatio > threshold)) return RebuildDecision::None;
    if (gpuBuilder && !driftSite) return RebuildDecision::Synchronous;
    return buildRunning ? RebuildDecision::None : RebuildDecision::Background;
}

} // namespace ppt
