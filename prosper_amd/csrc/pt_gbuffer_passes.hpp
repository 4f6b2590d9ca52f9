// pt_gbuffer_passes.hpp — what the other pass modules use of the G-buffer module (pt_gbuffer_passes.cpp): the context's last
// frame, the lighting inputs and refusals of a lit pass, and the pieces of a G-buffer trace that the forward passes
// (pt_forward_passes.cpp) build their launches from.  Private to the library's translation units.
#pragma once

#include "pt_gbuffer_kernels.hpp"
#include "pt_pass_support.hpp"

namespace ppt
{

#pragma GCC visibility push(hidden) // (not part of the library's exports)

// What the last call that wrote a depth left for the passes that read "NULL: the last traced G-buffer's": a G-buffer (a
// trace or a resolve), or a forward frame, which has a depth and a velocity and no attribute targets.  The targets may be
// the caller's or lie in a buffer of the context; the registry of the inspection passes lists only the latter.
struct LastFrame
{
    prosper_pt_gbuffer_targets targets = {};
    uint32_t width = 0, height = 0;
    void *velocity = nullptr; // of the last call that wrote one
    uint32_t velocityWidth = 0, velocityHeight = 0;
    uint32_t derivativesWidth = 0, derivativesHeight = 0; // texture LOD debug; 0: the last traced G-buffer wrote none
    bool forwardDepthOwned = false; // a forward frame's depth lies in the forward module's buffer

    static bool lies_in(const DeviceBuffer &b, const void *p)
    {
        return p && b.ptr && (const uint8_t *)p >= b.as<uint8_t>() && (const uint8_t *)p < b.as<uint8_t>() + b.bytes;
    }
    // after a trace or a resolve into `t` (v nullptr: the call wrote no velocity, the last one stands)
    void set_gbuffer(const prosper_pt_gbuffer_targets &t, void *v, uint32_t w, uint32_t h);
    // after a forward frame
    void set_forward(float *depth, bool depthOwned, void *v, uint32_t w, uint32_t h);
    // `b` is about to be reallocated: what lies in it is forgotten
    void forget_if_in(const DeviceBuffer &b);
    // grow_to for a buffer the last frame may lie in
    int grow(DeviceBuffer &b, size_t bytes, hipStream_t s)
    {
        if (b.ptr && b.bytes >= bytes) return PROSPER_PT_OK;
        forget_if_in(b);
        return grow_to(b, bytes, s);
    }
    // the depth of the last G-buffer or forward frame; NO_SCENE before either
    int depth(const float **out, uint32_t *w, uint32_t *h) const;
};
LastFrame &gbuffer_last_frame(prosper_pt_ctx *ctx);
// LastFrame::depth of the context
int gbuffer_last_depth(prosper_pt_ctx *ctx, const float **depth, uint32_t *width, uint32_t *height);

// prosper_pt_set_texture_lod's state: what the traced G-buffer and the rasteriser's passes sample with
void gbuffer_texture_lod(const prosper_pt_ctx *ctx, bool *enabled, float *bias);
// ... as a launcher takes it: `storage` filled in (without derivatives) and returned, or nullptr while LOD 0 is sampled
const GBufferLodParams *gbuffer_lod_params(const prosper_pt_ctx *ctx, GBufferLodParams &storage);

// What every lit pass refuses of its push constants and camera, in this order: a drawType out of range, an ibl other than 0 or
// 1, ibl = 1 before prosper_pt_generate_ibl (or without a context), a camera clusters cannot be built from
int check_lit_pass(const char *what, const prosper_pt_ctx *ctx, uint32_t drawType, uint32_t ibl, const prosper_CameraUniforms *camera);
// What a pass with a velocity target refuses of it and of the previous transforms, and then of the context and its scene: an
// unaligned target, a count without transforms, a null context, check_scene, a count that is not the scene's
int check_velocity_inputs(
    const char *what, prosper_pt_ctx *ctx, const void *velocity, const prosper_ModelInstanceTransforms *previousTransforms, uint32_t previousTransformCount);
// The lighting inputs of a lit pass on `s` after flush_scene_updates.  `reused` given (the forward passes): the lists of the
// last clustering serve when they were made from the same camera terms, extent and lights (*reused); otherwise, and always
// with `reused` nullptr (deferred shading), the lights are clustered on `s`.  `ibl`: the maps of prosper_pt_generate_ibl.
int clustered_lights(
    prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, bool ibl, hipStream_t s, ClusteredLights *out,
    bool *reused);

// The camera terms a pass needs to rebuild a G-buffer texel's surface (RestirCamera)
RestirCamera gbuffer_camera(const prosper_CameraUniforms *camera);
// The camera ray, the depth's worldToClip and the switches of a G-buffer trace (the forward passes follow the same ray)
GBufferTraceParams gbuffer_trace_params(
    uint32_t drawType, uint32_t frameIndex, bool jitter, bool opaqueOnly, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height);
// the matrices and jitters a velocity target is computed from
void velocity_camera_terms(GBufferVelocityParams &v, const prosper_CameraUniforms *camera);
// the context-owned velocity target, 8 bytes per pixel, grown like hostInputs
int velocity_owned_target(prosper_pt_ctx *ctx, size_t pixels, hipStream_t s, float2 **out);
// the device copy of a call's previous instance transforms, enqueued on `s`
int upload_previous_transforms(
    prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count, hipStream_t s, const prosper_ModelInstanceTransforms **out);

#pragma GCC visibility pop

} // namespace ppt
