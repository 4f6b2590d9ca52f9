// host/depth_of_field.cpp — see depth_of_field.hpp.
#include "depth_of_field.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render::dof
{

void DepthOfField::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

prosper_pt_dof_pc DepthOfField::pushConstants(const scene::Camera &cam, uint32_t width, uint32_t height)
{
    (void)height;
    const scene::CameraParameters &camParams = cam.parameters();
    // Setup.cpp:163-177 over the rounded-up half extent
    const uint32_t halfWidth = width / 2u + (width & 1u);
    const float maxBgCoCInUnits =
        (camParams.apertureDiameter * camParams.focalLength) / (camParams.focusDistance - camParams.focalLength);
    const float maxBgCoCInHalfResPixels = (maxBgCoCInUnits / scene::Camera::sensorWidth()) * static_cast<float>(halfWidth);
    // Dilate.cpp:105-121 over the tile extent
    const uint32_t tileWidth = (halfWidth + 7u) / 8u;
    const int32_t maxBgCoCInPixels =
        static_cast<int32_t>(std::ceil((maxBgCoCInUnits / scene::Camera::sensorWidth()) * static_cast<float>(tileWidth)));
    prosper_pt_dof_pc pc = {};
    pc.focusDistance = camParams.focusDistance;
    pc.maxBackgroundCoC = maxBgCoCInHalfResPixels;
    pc.maxCoC = maxBgCoCInHalfResPixels * sMaxFgCoCFactor;
    pc.gatherRadius = std::max(maxBgCoCInPixels * static_cast<int32_t>(std::ceil(sMaxFgCoCFactor)), 1);
    return pc;
}

DepthOfField::Output DepthOfField::record(const scene::Camera &cam, const Input &input, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    m_lastPC = pushConstants(cam, input.width, input.height);
    prosper_pt_dof_inputs in = {};
    in.illumination = input.illumination;
    in.nonLinearDepth = input.depth;
    in.onDevice = input.onDevice ? 1u : 0u;
    if (prosper_pt_depth_of_field(m_ctx, &m_lastPC, &cam.uniforms(), input.width, input.height, &in, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("DepthOfField::record: ") + prosper_pt_last_error());
    Output ret;
    void *ptr = nullptr;
    if (prosper_pt_get_hdr_device_ptr(m_ctx, &ptr, nullptr) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("DepthOfField::record: ") + prosper_pt_last_error());
    ret.combinedIlluminationDoF = static_cast<const float *>(ptr);
    ret.width = input.width;
    ret.height = input.height;
    return ret;
}

} // namespace render::dof

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_depth_of_field
{
    render::dof::DepthOfField pass;
};

extern "C" {

int prosper_host_depth_of_field_create(prosper_pt_ctx *ctx, prosper_host_depth_of_field **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_depth_of_field_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_depth_of_field *r = new (std::nothrow) prosper_host_depth_of_field();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_depth_of_field_destroy(prosper_host_depth_of_field *r) { delete r; }

int prosper_host_depth_of_field_record(
    prosper_host_depth_of_field *r, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const prosper_pt_dof_inputs *inputs, void *stream, prosper_pt_dof_pc *outPushConstants)
{
    if (!r || !camera || !inputs)
    {
        prosper_host_set_error("prosper_host_depth_of_field_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
        render::dof::DepthOfField::Input in;
        in.illumination = inputs->illumination;
        in.depth = inputs->nonLinearDepth;
        in.onDevice = inputs->onDevice != 0;
        in.width = width;
        in.height = height;
        (void)r->pass.record(cam, in, stream);
        if (outPushConstants) *outPushConstants = r->pass.lastPushConstants();
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

} // extern "C"
