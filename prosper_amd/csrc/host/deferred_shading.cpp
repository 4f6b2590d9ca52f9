// host/deferred_shading.cpp — see deferred_shading.hpp.
#include "deferred_shading.hpp"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void DeferredShading::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

DeferredShading::Output DeferredShading::record(
    const scene::Camera &cam, const Input &input, bool applyIbl, scene::DrawType drawType, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    const rtdi::GBuffer &g = input.gbuffer;
    if (input.lightClusters.width != g.width || input.lightClusters.height != g.height)
        throw std::runtime_error("DeferredShading::record: the light clusters were built for another extent");

    // DeferredShading.cpp:216-219
    prosper_pt_deferred_shading_pc pc = {};
    pc.drawType = static_cast<uint32_t>(drawType);
    pc.ibl = applyIbl ? 1u : 0u;
    m_lastPC = pc;

    prosper_pt_restir_inputs in = {};
    in.albedoRoughness = g.albedoRoughness;
    in.normalMetallic = g.normalMetallic;
    in.nonLinearDepth = g.nonLinearDepth;
    in.onDevice = g.onDevice ? 1u : 0u;
    if (prosper_pt_deferred_shading(m_ctx, &pc, 0u, 0u, &cam.uniforms(), g.width, g.height, &in, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("DeferredShading::record: ") + prosper_pt_last_error());

    Output ret;
    void *ptr = nullptr;
    if (prosper_pt_get_hdr_device_ptr(m_ctx, &ptr, nullptr) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("DeferredShading::record: ") + prosper_pt_last_error());
    ret.illumination = static_cast<const float *>(ptr);
    ret.width = g.width;
    ret.height = g.height;
    return ret;
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_deferred_shading
{
    render::DeferredShading pass;
};

extern "C" {

int prosper_host_deferred_shading_create(prosper_pt_ctx *ctx, prosper_host_deferred_shading **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_deferred_shading_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_deferred_shading *r = new (std::nothrow) prosper_host_deferred_shading();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_deferred_shading_destroy(prosper_host_deferred_shading *r) { delete r; }

int prosper_host_deferred_shading_record(
    prosper_host_deferred_shading *r, prosper_host_camera *camera, uint32_t width, uint32_t height,
    const prosper_pt_restir_inputs *gbuffer, int applyIbl, uint32_t drawType, void *stream,
    prosper_pt_deferred_shading_pc *outPushConstants)
{
    if (!r || !camera || !gbuffer)
    {
        prosper_host_set_error("prosper_host_deferred_shading_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (drawType >= (uint32_t)scene::DrawType::Count)
    {
        prosper_host_set_error("prosper_host_deferred_shading_record: drawType out of range");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_pt_ibl_info ibl = {};
    if (applyIbl && (prosper_pt_get_ibl_info(r->pass.context(), &ibl) != PROSPER_PT_OK || !ibl.generated))
    {
        prosper_host_set_error("prosper_host_deferred_shading_record: IBL needs ImageBasedLighting's maps: run ImageBasedLighting::recordGeneration after the scene upload");
        return PROSPER_PT_ERR_UNSUPPORTED;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
        render::rtdi::GBuffer g;
        g.albedoRoughness = gbuffer->albedoRoughness;
        g.normalMetallic = gbuffer->normalMetallic;
        g.nonLinearDepth = gbuffer->nonLinearDepth;
        g.onDevice = gbuffer->onDevice != 0;
        g.width = width;
        g.height = height;
        // Renderer.cpp:430-466: LightClustering::record, then DeferredShading::record over its output
        render::LightClustering clustering;
        clustering.init(r->pass.context());
        const render::LightClusteringOutput clusters = clustering.record(cam, width, height, stream);
        (void)r->pass.record(cam, render::DeferredShading::Input{g, clusters}, applyIbl != 0,
                             static_cast<scene::DrawType>(drawType), stream);
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
