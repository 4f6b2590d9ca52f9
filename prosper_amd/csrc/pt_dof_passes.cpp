// pt_dof_passes.cpp — C-ABI of the passes between the shaded G-buffer and the tone map (include/prosper_pt/prosper_pt.h):
// the skybox fill (prosper_pt_skybox_fill) and depth of field (prosper_pt_depth_of_field), with the readbacks of what
// the latter produced.  Kernels: pt_dof.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <cmath>

#include "pt_context.hpp"
#include "pt_dof.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

struct DofPassState
{
    DeviceBuffer hostInputs;    // device copies of a call's host inputs: 16 + 4 bytes per pixel
    DeviceBuffer halfIllumination, halfCoC, tileMinMax, dilatedMinMax;
    DeviceBuffer gather[2], filtered[2];
    DeviceBuffer sampleOffsets; // the octaweb's unit offsets, uploaded once
    DofParams last = {};        // of the last prosper_pt_depth_of_field
    bool valid = false;
    StageEvents<kDofStages> timing;
};

static void list_dof_debug_images(const prosper_pt_ctx *ctx, std::vector<DebugImage> &out)
{
    const DofPassState &st = *ctx->dofPasses;
    const DofParams &p = st.last;
    {
        DebugImage im;
        im.name = "HalfResIllumination";
        im.format = PROSPER_PT_DEBUG_FORMAT_RGBA16F;
        im.valid = st.valid;
        if (st.valid)
        {
            im.width = p.hw, im.height = p.hh;
            im.levelCount = p.levels < kDebugImageMaxLevels ? p.levels : kDebugImageMaxLevels;
            for (uint32_t l = 0; l < im.levelCount; ++l)
            {
                im.level[l] = st.halfIllumination.as<uint8_t>() + (size_t)p.levelOffset[l] * 8u;
                im.levelW[l] = (p.hw >> l) ? (p.hw >> l) : 1u;
                im.levelH[l] = (p.hh >> l) ? (p.hh >> l) : 1u;
            }
        }
        out.push_back(im);
    }
    const struct
    {
        const char *name;
        uint32_t format;
        const DeviceBuffer *buffer;
        bool tiles;
    } images[7] = {{"HalfResCircleOfConfusion", PROSPER_PT_DEBUG_FORMAT_R16F, &st.halfCoC, false},
                   {"tileMinMaxCircleOfConfusion", PROSPER_PT_DEBUG_FORMAT_RG16F, &st.tileMinMax, true},
                   {"dilatedTileMinMaxCoC", PROSPER_PT_DEBUG_FORMAT_RG16F, &st.dilatedMinMax, true},
                   {"halfResFgBokehColorWeight", PROSPER_PT_DEBUG_FORMAT_RGBA16F, &st.gather[0], false},
                   {"halfResBgBokehColorWeight", PROSPER_PT_DEBUG_FORMAT_RGBA16F, &st.gather[1], false},
                   {"halfResFgBokehColorWeightFiltered", PROSPER_PT_DEBUG_FORMAT_RGBA16F, &st.filtered[0], false},
                   {"halfResBgBokehColorWeightFiltered", PROSPER_PT_DEBUG_FORMAT_RGBA16F, &st.filtered[1], false}};
    for (const auto &i : images)
    {
        DebugImage im;
        im.name = i.name;
        im.format = i.format;
        im.valid = st.valid && i.buffer->ptr;
        if (im.valid) im.one_level(i.buffer->ptr, i.tiles ? p.tw : p.hw, i.tiles ? p.th : p.hh);
        out.push_back(im);
    }
}

extern const PassModule kDofPasses = pass_module<DofPassState, &prosper_pt_ctx::dofPasses>(nullptr, list_dof_debug_images);

} // namespace ppt

extern "C" {

// ---- skybox fill (src/render/SkyboxRenderer.cpp) ----

int prosper_pt_skybox_fill(
    prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, const float *nonLinearDepth,
    uint32_t onDevice, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_skybox_fill: null argument");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_skybox_fill: empty extent");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_skybox_fill: null argument");
    const int crc = check_scene(ctx, "prosper_pt_skybox_fill");
    if (crc != PROSPER_PT_OK) return crc;
    if (!hdr_has_extent(ctx, width, height))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_skybox_fill: the HDR image has another extent");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = flush_scene_updates(ctx, s, s);
    if (rc != PROSPER_PT_OK) return rc;
    const size_t pixels = (size_t)width * height;
    const float *depth = nullptr;
    rc = resolve_depth(ctx, "prosper_pt_skybox_fill", nonLinearDepth, onDevice != 0u, width, height, &depth);
    // (behind the 16 bytes per pixel of a depth of field's illumination: hostInputs holds both)
    if (rc == PROSPER_PT_OK) rc = stage_depth(ctx->dofPasses->hostInputs, pixels * 16u, nonLinearDepth, pixels, s, &depth);
    if (rc != PROSPER_PT_OK) return rc;
    RenderParams r = {};
    set_camera_ray_params(r, camera);
    r.width = width;
    r.height = height;
    r.localWidth = width;
    r.stripeCount = 1;
    r.frameCount = 1;
    launch_skybox_fill(ctx->scene, r, depth, ctx->hdr, s);
    PPT_HIP(hipGetLastError());
    return mark_versions_read(ctx, s);
}

// ---- depth of field (src/render/dof/DepthOfField.cpp) ----

void prosper_pt_dof_sample_offsets(float out[242])
{
    if (out) dof_sample_offsets(out);
}

int prosper_pt_depth_of_field(
    prosper_pt_ctx *ctx, const prosper_pt_dof_pc *pc, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height,
    const prosper_pt_dof_inputs *inputs, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!pc || !camera || !inputs) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_depth_of_field: null argument");
    if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_depth_of_field: empty extent");
    if (!std::isfinite(pc->focusDistance) || !std::isfinite(pc->maxBackgroundCoC) || !std::isfinite(pc->maxCoC))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_depth_of_field: non-finite push constant");
    if (!(pc->focusDistance > 0.0f)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_depth_of_field: focusDistance must be positive");
    if (pc->maxBackgroundCoC < 0.0f || pc->maxCoC < 0.0f)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_depth_of_field: negative circle of confusion");
    if (pc->gatherRadius < 1) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_depth_of_field: gatherRadius must be at least 1");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_depth_of_field: null argument");
    const bool inPlace = inputs->illumination == nullptr;
    if (const int rc = check_in_place_hdr(ctx, "prosper_pt_depth_of_field", inPlace, width, height)) return rc;
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DofPassState &st = *ctx->dofPasses;
    const size_t pixels = (size_t)width * height;

    DofParams p = {};
    const size_t mipTexels = dof_set_extents(p, width, height);
    p.focusDistance = pc->focusDistance;
    p.maxBackgroundCoC = pc->maxBackgroundCoC;
    p.maxCoC = pc->maxCoC;
    p.gatherRadius = pc->gatherRadius;
    p.cameraToClip22 = camera->cameraToClip.col[2].z;
    p.cameraToClip32 = camera->cameraToClip.col[3].z;

    st.valid = false;
    const size_t halfTexels = (size_t)p.hw * p.hh, tiles = (size_t)p.tw * p.th;
    int rc = PROSPER_PT_OK;
    if (!inputs->onDevice && (inputs->illumination || inputs->nonLinearDepth)) rc = grow_to(st.hostInputs, pixels * 20u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.halfIllumination, mipTexels * 8u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.halfCoC, halfTexels * 2u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.tileMinMax, tiles * 4u, s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.dilatedMinMax, tiles * 4u, s);
    for (uint32_t k = 0; k < 2u; ++k)
    {
        if (rc == PROSPER_PT_OK) rc = grow_to(st.gather[k], halfTexels * 8u, s);
        if (rc == PROSPER_PT_OK) rc = grow_to(st.filtered[k], halfTexels * 8u, s);
    }
    if (rc == PROSPER_PT_OK && !st.sampleOffsets.ptr)
    {
        float offsets[2 * kDofTaps];
        dof_sample_offsets(offsets);
        rc = grow_buffer(st.sampleOffsets, GrowWait::None, s, sizeof(offsets), sizeof(offsets));
        if (rc == PROSPER_PT_OK) PPT_HIP(hipMemcpy(st.sampleOffsets.ptr, offsets, sizeof(offsets), hipMemcpyHostToDevice));
    }
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = st.timing.create())) return rc;

    DofBuffers b = {};
    const bool onDevice = inputs->onDevice != 0u;
    rc = resolve_depth(ctx, "prosper_pt_depth_of_field", inputs->nonLinearDepth, onDevice, width, height, &b.nonLinearDepth);
    if (rc == PROSPER_PT_OK) rc = stage_depth(st.hostInputs, pixels * 16u, inputs->nonLinearDepth, pixels, s, &b.nonLinearDepth);
    // (an explicit illumination that is the HDR image itself behaves as in place)
    if (rc == PROSPER_PT_OK) rc = resolve_illumination(ctx, inputs->illumination, inPlace, onDevice, st.hostInputs, width, height, s, &b.illumination);
    if (rc != PROSPER_PT_OK) return rc;
    b.out = ctx->hdr;
    b.halfIllumination = st.halfIllumination.as<uint2>();
    b.halfCoC = st.halfCoC.as<uint16_t>();
    b.tileMinMax = st.tileMinMax.as<uint32_t>();
    b.dilatedMinMax = st.dilatedMinMax.as<uint32_t>();
    for (uint32_t k = 0; k < 2u; ++k)
    {
        b.gather[k] = st.gather[k].as<uint2>();
        b.filtered[k] = st.filtered[k].as<uint2>();
    }
    b.sampleOffsets = st.sampleOffsets.as<float>();
    launch_depth_of_field(p, b, st.timing.events, s);
    PPT_HIP(hipGetLastError());
    st.last = p;
    st.valid = true;
    return PROSPER_PT_OK;
}

int prosper_pt_read_dof_stage(prosper_pt_ctx *ctx, uint32_t stage, uint32_t level, void *host, size_t byte_size, void *stream)
{
    if (stage >= PROSPER_PT_DOF_STAGE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_dof_stage: unknown stage");
    if (!ctx || !host) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_dof_stage: null argument");
    const DofPassState &st = *ctx->dofPasses;
    if (!st.valid) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_dof_stage: no depth of field has run yet");
    const DofParams &p = st.last;
    const size_t halfTexels = (size_t)p.hw * p.hh, tiles = (size_t)p.tw * p.th;
    const uint8_t *src = nullptr;
    size_t bytes = 0;
    switch (stage)
    {
    case PROSPER_PT_DOF_HALF_ILLUMINATION:
        if (level >= p.levels) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_dof_stage: no such mip level");
        src = st.halfIllumination.as<uint8_t>() + (size_t)p.levelOffset[level] * 8u;
        bytes = (size_t)((p.hw >> level) ? (p.hw >> level) : 1u) * ((p.hh >> level) ? (p.hh >> level) : 1u) * 8u;
        break;
    case PROSPER_PT_DOF_HALF_COC: src = st.halfCoC.as<uint8_t>(); bytes = halfTexels * 2u; break;
    case PROSPER_PT_DOF_TILE_MIN_MAX: src = st.tileMinMax.as<uint8_t>(); bytes = tiles * 4u; break;
    case PROSPER_PT_DOF_DILATED_TILE_MIN_MAX: src = st.dilatedMinMax.as<uint8_t>(); bytes = tiles * 4u; break;
    case PROSPER_PT_DOF_FG_GATHER: src = st.gather[0].as<uint8_t>(); bytes = halfTexels * 8u; break;
    case PROSPER_PT_DOF_BG_GATHER: src = st.gather[1].as<uint8_t>(); bytes = halfTexels * 8u; break;
    case PROSPER_PT_DOF_FG_FILTERED: src = st.filtered[0].as<uint8_t>(); bytes = halfTexels * 8u; break;
    default: src = st.filtered[1].as<uint8_t>(); bytes = halfTexels * 8u; break;
    }
    if (byte_size != bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_dof_stage: byte_size differs from the stage's");
    return read_back(ctx, static_cast<hipStream_t>(stream), {{host, src, bytes}});
}

int prosper_pt_get_dof_info(prosper_pt_ctx *ctx, prosper_pt_dof_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_dof_info: null argument");
    const DofPassState &st = *ctx->dofPasses;
    prosper_pt_dof_info info = {};
    if (st.valid)
    {
        const DofParams &p = st.last;
        info.valid = 1u;
        info.width = p.width;
        info.height = p.height;
        info.halfWidth = p.hw;
        info.halfHeight = p.hh;
        info.tileWidth = p.tw;
        info.tileHeight = p.th;
        info.mips = p.levels;
        PPT_HIP(hipSetDevice(ctx->device));
        if (const int rc = st.timing.elapsed(&info.setupMs)) return rc;
    }
    *out = info;
    return PROSPER_PT_OK;
}

} // extern "C"
