// host/skybox_renderer.cpp — see skybox_renderer.hpp.
#include "skybox_renderer.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void SkyboxRenderer::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

void SkyboxRenderer::record(const scene::Camera &cam, const RecordInOut &t, void *stream) const
{
    PROSPER_ASSERT(m_initialized);
    if (prosper_pt_skybox_fill(m_ctx, &cam.uniforms(), t.width, t.height, t.depth, t.onDevice ? 1u : 0u, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("SkyboxRenderer::record: ") + prosper_pt_last_error());
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_skybox_renderer
{
    render::SkyboxRenderer pass;
};

extern "C" {

int prosper_host_skybox_renderer_create(prosper_pt_ctx *ctx, prosper_host_skybox_renderer **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_skybox_renderer_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_skybox_renderer *r = new (std::nothrow) prosper_host_skybox_renderer();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_skybox_renderer_destroy(prosper_host_skybox_renderer *r) { delete r; }

int prosper_host_skybox_renderer_record(
    prosper_host_skybox_renderer *r, prosper_host_camera *camera, uint32_t width, uint32_t height, const float *nonLinearDepth,
    uint32_t onDevice, void *stream)
{
    if (!r || !camera)
    {
        prosper_host_set_error("prosper_host_skybox_renderer_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
        render::SkyboxRenderer::RecordInOut t;
        t.depth = nonLinearDepth;
        t.onDevice = onDevice != 0u;
        t.width = width;
        t.height = height;
        r->pass.record(cam, t, stream);
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

} // extern "C"
