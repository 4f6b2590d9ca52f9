// host/gbuffer_renderer.cpp — see gbuffer_renderer.hpp.
#include "gbuffer_renderer.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void GBufferRenderer::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_culler.init(ctx);
    m_downsampler.init(ctx);
    m_initialized = true;
}

int GBufferRenderer::tryRecord(
    const prosper_CameraUniforms &cam, scene::DrawType drawType, const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount,
    GBufferRendererOutput &out, void *stream) noexcept
{
    PROSPER_ASSERT(m_initialized);
    out = GBufferRendererOutput{};
    prosper_pt_velocity_gbuffer_desc desc = {};
    // what the previous record kept is the previous frame's table; a first call or a changed count sees unmoved instances
    if (transforms && m_previousTransforms.size() == transformCount && transformCount != 0u)
    {
        desc.previousTransforms = m_previousTransforms.data();
        desc.previousTransformCount = transformCount;
    }
    int rc = prosper_pt_raster_gbuffer(m_ctx, (uint32_t)drawType, &cam, &desc, stream);
    if (rc != PROSPER_PT_OK) return rc;
    try
    {
        if (transforms)
            m_previousTransforms.assign(transforms, transforms + transformCount);
        else
            m_previousTransforms.clear();
    }
    catch (const std::bad_alloc &)
    {
        m_previousTransforms.clear();
    }
    prosper_pt_restir_inputs g = {};
    if ((rc = prosper_pt_get_gbuffer_device_ptrs(m_ctx, &g, nullptr, nullptr)) != PROSPER_PT_OK) return rc;
    void *velocity = nullptr;
    if ((rc = prosper_pt_get_velocity_device_ptr(m_ctx, &velocity, nullptr, nullptr)) != PROSPER_PT_OK) return rc;
    out.albedoRoughness = g.albedoRoughness;
    out.normalMetalness = g.normalMetallic;
    out.depth = g.nonLinearDepth;
    out.velocity = velocity;
    return PROSPER_PT_OK;
}

GBufferRendererOutput GBufferRenderer::record(
    const scene::Camera &cam, scene::DrawType drawType, const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount,
    DrawStats *drawStats, void *stream)
{
    GBufferRendererOutput out;
    const int rc = tryRecord(cam.uniforms(), drawType, transforms, transformCount, out, stream);
    if (rc != PROSPER_PT_OK) throw std::runtime_error(std::string("GBufferRenderer::record: ") + prosper_pt_last_error());
    if (drawStats) (void)m_culler.readDrawStats(*drawStats, false);
    return out;
}

void GBufferRenderer::releasePreserved()
{
    PROSPER_ASSERT(m_initialized);
    (void)prosper_pt_raster_release_preserved(m_ctx);
    m_previousTransforms.clear();
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_gbuffer_renderer
{
    render::GBufferRenderer pass;
};

extern "C" {

int prosper_host_gbuffer_renderer_create(prosper_pt_ctx *ctx, prosper_host_gbuffer_renderer **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_gbuffer_renderer_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_gbuffer_renderer *r = new (std::nothrow) prosper_host_gbuffer_renderer();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_gbuffer_renderer_destroy(prosper_host_gbuffer_renderer *r) { delete r; }

int prosper_host_gbuffer_renderer_record(
    prosper_host_gbuffer_renderer *r, prosper_host_camera *camera, uint32_t width, uint32_t height, uint32_t drawType,
    const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount, void *stream, prosper_host_gbuffer_renderer_output *out)
{
    if (!r || !camera || !out)
    {
        prosper_host_set_error("prosper_host_gbuffer_renderer_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (drawType >= (uint32_t)scene::DrawType::Count)
    {
        prosper_host_set_error("prosper_host_gbuffer_renderer_record: drawType out of range");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    scene::Camera &cam = *prosper_host_camera_object(camera);
    cam.updateResolution(width, height);
    cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
    render::GBufferRendererOutput o;
    const int rc = r->pass.tryRecord(cam.uniforms(), static_cast<scene::DrawType>(drawType), transforms, transformCount, o, stream);
    if (rc != PROSPER_PT_OK)
    {
        prosper_host_set_error((std::string("GBufferRenderer::record: ") + prosper_pt_last_error()).c_str());
        return rc;
    }
    *out = prosper_host_gbuffer_renderer_output{o.albedoRoughness, o.normalMetalness, o.velocity, o.depth};
    return PROSPER_PT_OK;
}

int prosper_host_gbuffer_renderer_read_draw_stats(prosper_host_gbuffer_renderer *r, prosper_pt_draw_stats *out, uint32_t wait)
{
    if (!r || !out)
    {
        prosper_host_set_error("prosper_host_gbuffer_renderer_read_draw_stats: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    return prosper_pt_get_draw_stats(r->pass.context(), out, wait);
}

int prosper_host_gbuffer_renderer_release_preserved(prosper_host_gbuffer_renderer *r)
{
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.releasePreserved();
    return PROSPER_PT_OK;
}

} // extern "C"
