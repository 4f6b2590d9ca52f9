// pt_animation.hpp — what the scene update (pt_scene_updates.cpp flush_pending_update) and the readers of the host mirrors use
// of the keyframe animation (pt_animation.hip).  Private to the library's translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/prosper_pt/prosper_pt.h"

struct prosper_pt_ctx;

namespace ppt
{

struct AnimationState;
struct LightBlock;

#pragma GCC visibility push(hidden) // (not part of the library's exports)

// Made by prosper_pt_create (false: out of host memory), freed by prosper_pt_destroy.
bool create_animation_state(prosper_pt_ctx *ctx);
void destroy_animation_state(prosper_pt_ctx *ctx);
// a new scene: its nodes are other nodes (the device is idle)
void forget_animations(prosper_pt_ctx *ctx);

// prosper_pt_animate up to the flush: `timeS` is staged, and the ranges of the instances it moves count as moved since the
// last build.  Refused before prosper_pt_set_animations.
int stage_animation(prosper_pt_ctx *ctx, float timeS);
// a prosper_pt_animate waits for the next flush
bool animation_pending(const prosper_pt_ctx *ctx);
// ... and its nodes carry lights: the flush produces the next light version too
bool animation_moves_lights(const prosper_pt_ctx *ctx);
// The staged time into `table` (the next scene version's transform table, already holding its base) and `lights` (the next
// light version, already a copy of the current one; nullptr when no node carries a light), on `stream`: the current
// table is kept as the previous one, the two kernels run, and table, lights and camera record start their way into
// the pinned read-back.  Nothing of the context changes before animation_committed.
int enqueue_animation(prosper_pt_ctx *ctx, prosper_ModelInstanceTransforms *table, uint32_t count, LightBlock *lights, hipStream_t stream);
// every enqueue of the flush has succeeded: the update is consumed
void animation_committed(prosper_pt_ctx *ctx);
// The host mirrors of the transform table and the light buffers (AccelState::transforms, LightState::mirror) take up the
// newest read-back, waiting for it if it is still on its way.  Called before anything reads or replaces a mirror.
int sync_animation_mirrors(prosper_pt_ctx *ctx);

#pragma GCC visibility pop

} // namespace ppt
