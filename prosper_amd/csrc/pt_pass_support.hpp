// pt_pass_support.hpp — what the pass modules (pt_gbuffer_passes.cpp and the others) share: what they use of the scene's
// updates (pt_scene_updates.cpp) and of the render path in prosper_pt.cpp, and the one way in for a call's image inputs and
// out for its read-backs (pt_pass_support.cpp).
// Private to the library's translation units.
#pragma once

#include <initializer_list>
#include <new>

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

// The largest width or height the image passes take.  Each has its own reason for the same bound: a texel index fits 32
// bits (taa, particles, debug lines, the texture viewer); bloom's compose forms (2 coord + 1) * levelSize + extent in 32 bits.
constexpr uint32_t kMaxExtent = 32768;

// `p` is device memory (a pass that writes through it, or copies from it on the device, takes nothing else)
bool is_device_pointer(const void *p);

// ---- a call's depth input ----
// The depth a pass reads.  NULL: the last traced G-buffer's (gbuffer_last_depth), whose extent must match; a device
// pointer: as it is; a host pointer: *out is nullptr until stage_depth has copied it.  Refuses without touching the
// device, so a caller may ask before its hipSetDevice and flush_scene_updates and stage after them.
int resolve_depth(
    prosper_pt_ctx *ctx, const char *what, const float *depth, bool onDevice, uint32_t width, uint32_t height, const float **out);
// Where resolve_depth left *out nullptr: the copy of the host depth at `offset` of `staging` (grown to hold it, a no-op
// where the caller has grown it for all of a call's inputs), enqueued on `s`.
int stage_depth(DeviceBuffer &staging, size_t offset, const float *host, size_t pixels, hipStream_t s, const float **out);

// ---- a call's illumination input ----
// An in-place pass works on the HDR image as it is, which then must be a whole `width` x `height` image.  The caller
// decides `inPlace`: a NULL illumination, and for taa also a device pointer that is the HDR image itself (bloom and dof
// pass that one on to prepare_hdr, which keeps an HDR image of the same extent).  Touches no device.
int check_in_place_hdr(const prosper_pt_ctx *ctx, const char *what, bool inPlace, uint32_t width, uint32_t height);
// What the kernels read as illumination: in place the HDR image; a device pointer as it is; a host array's copy at the
// front of `staging` (grown to hold it), enqueued on `s`.  For the last two the HDR image is prepared for the extent.
int resolve_illumination(
    prosper_pt_ctx *ctx, const void *illumination, bool inPlace, bool onDevice, DeviceBuffer &staging, uint32_t width, uint32_t height,
    hipStream_t s, const float4 **out);

// ---- a synchronous read-back ----
struct ReadCopy
{
    void *dst;       // host; nullptr: the caller does not want this one
    const void *src; // device
    size_t bytes;
};
// The device is set, `s` waits for `after` (if given: the fence behind the kernels that wrote the sources on whichever
// stream), every copy with a dst and bytes is enqueued on `s`, and `s` is synchronised once.
int read_back(const prosper_pt_ctx *ctx, hipStream_t s, std::initializer_list<ReadCopy> copies, const Fence *after = nullptr);

// ---- a module's description of itself (PassModule, pt_context.hpp) ----
// Its state is made and freed the same way in every module: `member` of the context points to a `State`.
template <class State, State *prosper_pt_ctx::*member> bool create_pass_state(prosper_pt_ctx *ctx)
{
    ctx->*member = new (std::nothrow) State();
    return ctx->*member != nullptr;
}
template <class State, State *prosper_pt_ctx::*member> void destroy_pass_state(prosper_pt_ctx *ctx)
{
    delete (ctx->*member);
    ctx->*member = nullptr;
}
// (Not constexpr, on purpose: hipcc gives these host files a device pass too, which emits every const object that is
// constant-initialised - and the functions a PassModule points to exist on the host only.)
template <class State, State *prosper_pt_ctx::*member>
PassModule pass_module(
    void (*forget_scene)(prosper_pt_ctx *) = nullptr, void (*list_debug_images)(const prosper_pt_ctx *, std::vector<DebugImage> &) = nullptr)
{
    return PassModule{create_pass_state<State, member>, destroy_pass_state<State, member>, forget_scene, list_debug_images};
}

#pragma GCC visibility pop

} // namespace ppt
