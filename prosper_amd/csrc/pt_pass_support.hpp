// pt_pass_support.hpp — what the pass modules (pt_gbuffer_passes.cpp and the others) use of the render path in
// prosper_pt.cpp.  Private to the library's translation units.
#pragma once

#include "pt_context.hpp"

namespace ppt
{

#pragma GCC visibility push(hidden) // (not part of the library's exports)

// What every pass checks of the scene before its arguments' extents: a scene, the meshes a worker finished meanwhile,
// no failed transform update.  `what` names the entry point in the refusal.
int check_scene(prosper_pt_ctx *ctx, const char *what);
// The pending transform, light and material updates are enqueued on `s` and take effect on `reader` - the stream the
// call's kernels read the scene on, `s` itself for a pass - before the call's first kernel: every kernel the call
// launches after this reads the same scene and light version (mark_versions_read after the last one).
int flush_scene_updates(prosper_pt_ctx *ctx, hipStream_t s, hipStream_t reader);
// The scene and light versions a call read are free again behind its last kernel on `s`.
int mark_versions_read(prosper_pt_ctx *ctx, hipStream_t s);
// the camera terms of the path tracer's camera ray (RenderParams eye .. cameraToWorld)
void set_camera_ray_params(RenderParams &p, const prosper_CameraUniforms *camera);
// The context's HDR image for a `width` x `height` image, or for the stripes of it `tile` gives this rank (nullptr:
// the whole image): the caller-owned buffer, or the owned one grown (and cleared) as needed.
int prepare_hdr(prosper_pt_ctx *ctx, uint32_t width, uint32_t height, const prosper_pt_tile_desc *tile, hipStream_t s);
// The global stack-overflow array of `slot` for `gridBlocks` workgroups of 256 lanes of a kernel whose LDS stack holds
// `ldsEntries` entries; *out is nullptr when the tree never needs more.
int ensure_stack_overflow(
    prosper_pt_ctx *ctx, prosper_pt_ctx::RenderSlot &slot, uint32_t ldsEntries, uint32_t gridBlocks, int32_t **out);
// a DeviceBuffer of a pass holds at least `bytes`, grown behind what `s` holds
inline int grow_to(DeviceBuffer &b, size_t bytes, hipStream_t s)
{
    if (b.ptr && b.bytes >= bytes) return PROSPER_PT_OK;
    return grow_buffer(b, GrowWait::Stream, s, bytes, bytes ? bytes : 16u);
}
// the context's HDR image is a whole `width` x `height` image (what a pass works on in place)
inline bool hdr_has_extent(const prosper_pt_ctx *ctx, uint32_t width, uint32_t height)
{
    return ctx->hdr && ctx->localWidth == width && ctx->height == height && ctx->stripeCount <= 1u;
}
// A slot's workspace may be reused once the kernels of its previous user are done: `free` is recorded behind them.
inline void wait_for_slot(prosper_pt_ctx::RenderSlot &slot, hipStream_t stream) { (void)slot.free.wait(stream); }
inline void release_slot(prosper_pt_ctx::RenderSlot &slot, hipStream_t stream) { (void)slot.free.record(stream); }

#pragma GCC visibility pop

} // namespace ppt
