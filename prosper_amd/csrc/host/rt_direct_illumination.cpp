// host/rt_direct_illumination.cpp — see rt_direct_illumination.hpp.
#include "rt_direct_illumination.hpp"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render::rtdi
{

namespace
{

// src/render/rtdi/{InitialReservoirs,SpatialReuse,Trace}.cpp: sFramePeriod
constexpr uint32_t sFramePeriod = 4096;

} // namespace

void RtDirectIllumination::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

void RtDirectIllumination::recompileShaders()
{
    PROSPER_ASSERT(m_initialized);
    m_resetAccumulation = true;
}

void RtDirectIllumination::drawUi(bool spatialReuse)
{
    PROSPER_ASSERT(m_initialized);
    m_doSpatialReuse = spatialReuse; // ImGui::Checkbox("Spatial reuse"): does not restart accumulation
}

RtDirectIllumination::Output RtDirectIllumination::record(
    const GBuffer &gbuffer, const scene::Camera &cam, bool resetAccumulation, scene::DrawType drawType,
    uint32_t nextFrame, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    (void)nextFrame;
    // The original's three passes each step a frame counter of their own per record (InitialReservoirs.cpp:105,
    // SpatialReuse.cpp:104, Trace.cpp:151); they agree as long as the spatial pass runs every frame.  One record here
    // runs all three with one index.
    m_frameIndex = (m_frameIndex + 1) % sFramePeriod;

    // Trace.cpp:174-190: a reset or an extent change starts a new history
    resetAccumulation = resetAccumulation || m_resetAccumulation;
    if (resetAccumulation || !m_havePrevious || gbuffer.width != m_previousWidth || gbuffer.height != m_previousHeight)
        m_accumulationDirty = true;

    prosper_pt_restir_trace_pc pc = {};
    pc.drawType = static_cast<uint32_t>(drawType);
    pc.frameIndex = m_frameIndex;
    // Trace.cpp:256-265: skipHistory, accumulate
    pc.flags = (uint32_t)(cam.changedThisFrame() || resetAccumulation || m_accumulationDirty) | ((uint32_t)m_accumulate << 1);
    m_lastPC = pc;

    prosper_pt_restir_inputs in = {};
    in.albedoRoughness = gbuffer.albedoRoughness;
    in.normalMetallic = gbuffer.normalMetallic;
    in.nonLinearDepth = gbuffer.nonLinearDepth;
    in.onDevice = gbuffer.onDevice ? 1u : 0u;
    const uint32_t flags = m_doSpatialReuse ? PROSPER_PT_RESTIR_SPATIAL_REUSE : 0u;
    if (prosper_pt_restir_di_record(m_ctx, &pc, flags, &cam.uniforms(), gbuffer.width, gbuffer.height, &in, stream) !=
        PROSPER_PT_OK)
        throw std::runtime_error(std::string("RtDirectIllumination::record: ") + prosper_pt_last_error());

    m_havePrevious = true; // Trace.cpp:301-303: the illumination is preserved as next frame's history
    m_previousWidth = gbuffer.width;
    m_previousHeight = gbuffer.height;
    m_accumulationDirty = false;
    m_resetAccumulation = false;

    Output ret;
    void *ptr = nullptr;
    if (prosper_pt_get_hdr_device_ptr(m_ctx, &ptr, nullptr) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("RtDirectIllumination::record: ") + prosper_pt_last_error());
    ret.illumination = static_cast<const float *>(ptr);
    ret.width = gbuffer.width;
    ret.height = gbuffer.height;
    return ret;
}

void RtDirectIllumination::releasePreserved()
{
    PROSPER_ASSERT(m_initialized);
    m_havePrevious = false; // Trace.cpp:350-356
}

} // namespace render::rtdi

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_rt_direct_illumination
{
    render::rtdi::RtDirectIllumination pass;
};

extern "C" {

int prosper_host_rt_direct_illumination_create(prosper_pt_ctx *ctx, prosper_host_rt_direct_illumination **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_rt_direct_illumination_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_rt_direct_illumination *r = new (std::nothrow) prosper_host_rt_direct_illumination();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_rt_direct_illumination_destroy(prosper_host_rt_direct_illumination *r) { delete r; }

void prosper_host_rt_direct_illumination_draw_ui(prosper_host_rt_direct_illumination *r, int spatialReuse)
{
    r->pass.drawUi(spatialReuse != 0);
}

void prosper_host_rt_direct_illumination_recompile_shaders(prosper_host_rt_direct_illumination *r)
{
    r->pass.recompileShaders();
}

void prosper_host_rt_direct_illumination_release_preserved(prosper_host_rt_direct_illumination *r)
{
    r->pass.releasePreserved();
}

int prosper_host_rt_direct_illumination_record(
    prosper_host_rt_direct_illumination *r, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const prosper_pt_restir_inputs *gbuffer, int resetAccumulation, uint32_t drawType, uint32_t nextFrame, void *stream,
    prosper_pt_restir_trace_pc *outPushConstants)
{
    if (!r || !camera || !gbuffer)
    {
        prosper_host_set_error("prosper_host_rt_direct_illumination_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (drawType >= (uint32_t)scene::DrawType::Count)
    {
        prosper_host_set_error("prosper_host_rt_direct_illumination_record: drawType out of range");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        render::rtdi::GBuffer g;
        g.albedoRoughness = gbuffer->albedoRoughness;
        g.normalMetallic = gbuffer->normalMetallic;
        g.nonLinearDepth = gbuffer->nonLinearDepth;
        g.onDevice = gbuffer->onDevice != 0;
        g.width = width;
        g.height = height;
        cam.updateResolution(width, height);
        cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
        (void)r->pass.record(g, cam, resetAccumulation != 0, static_cast<scene::DrawType>(drawType), nextFrame, stream);
        cam.endFrame();
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
