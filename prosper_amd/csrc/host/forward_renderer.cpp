// host/forward_renderer.cpp — see forward_renderer.hpp.
#include "forward_renderer.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void ForwardRenderer::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

int ForwardRenderer::tryRecordOpaque(
    const prosper_CameraUniforms &cam, bool applyIbl, scene::DrawType drawType, const prosper_ModelInstanceTransforms *transforms,
    uint32_t transformCount, OpaqueOutput &out, void *stream) noexcept
{
    PROSPER_ASSERT(m_initialized);
    out = OpaqueOutput{};
    // ForwardRenderer.cpp:658-662
    prosper_pt_forward_pc pc = {};
    pc.drawType = static_cast<uint32_t>(drawType);
    pc.ibl = applyIbl ? 1u : 0u;
    prosper_pt_forward_opaque_desc desc = {};
    // what the previous record kept is the previous frame's table; a first call or a changed count sees unmoved instances
    if (transforms && m_previousTransforms.size() == transformCount && transformCount != 0u)
    {
        desc.previousTransforms = m_previousTransforms.data();
        desc.previousTransformCount = transformCount;
        pc.previousTransformValid = 1u;
    }
    m_lastPC = pc;
    int rc = prosper_pt_set_texture_lod(m_ctx, m_textureLod ? 1 : 0, m_lodBias);
    if (rc != PROSPER_PT_OK) return rc;
    if ((rc = prosper_pt_raster_forward(m_ctx, &pc, &cam, &desc, stream)) != PROSPER_PT_OK) return rc;
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
    void *hdr = nullptr, *velocity = nullptr;
    float *depth = nullptr;
    if ((rc = prosper_pt_get_hdr_device_ptr(m_ctx, &hdr, nullptr)) != PROSPER_PT_OK) return rc;
    if ((rc = prosper_pt_get_velocity_device_ptr(m_ctx, &velocity, nullptr, nullptr)) != PROSPER_PT_OK) return rc;
    if ((rc = prosper_pt_get_forward_depth_device_ptr(m_ctx, &depth, nullptr, nullptr)) != PROSPER_PT_OK) return rc;
    out.illumination = hdr;
    out.velocity = velocity;
    out.depth = depth;
    return PROSPER_PT_OK;
}

ForwardRenderer::OpaqueOutput ForwardRenderer::recordOpaque(
    const scene::Camera &cam, const LightClusteringOutput *lightClusters, bool applyIbl, scene::DrawType drawType, void *stream,
    const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount)
{
    PROSPER_ASSERT(m_initialized);
    const prosper_CameraUniforms &u = cam.uniforms();
    if (lightClusters && (lightClusters->width != u.resolution[0] || lightClusters->height != u.resolution[1]))
        throw std::runtime_error("ForwardRenderer::recordOpaque: the light clusters were built for another extent");
    OpaqueOutput out;
    if (tryRecordOpaque(u, applyIbl, drawType, transforms, transformCount, out, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("ForwardRenderer::recordOpaque: ") + prosper_pt_last_error());
    return out;
}

void ForwardRenderer::releasePreserved()
{
    PROSPER_ASSERT(m_initialized);
    (void)prosper_pt_raster_release_preserved(m_ctx);
    m_previousTransforms.clear();
}

void ForwardRenderer::recordTransparent(
    const scene::Camera &cam, const TransparentInOut &t, const LightClusteringOutput *lightClusters, scene::DrawType drawType,
    bool applyIbl, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    if (lightClusters && (lightClusters->width != t.width || lightClusters->height != t.height))
        throw std::runtime_error("ForwardRenderer::recordTransparent: the light clusters were built for another extent");

    // ForwardRenderer.cpp:658-662
    prosper_pt_forward_pc pc = {};
    pc.drawType = static_cast<uint32_t>(drawType);
    pc.ibl = applyIbl ? 1u : 0u;
    m_lastPC = pc;

    if (prosper_pt_set_texture_lod(m_ctx, m_textureLod ? 1 : 0, m_lodBias) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("ForwardRenderer::recordTransparent: ") + prosper_pt_last_error());
    if (prosper_pt_forward_transparent(
            m_ctx, &pc, t.rayFlags, t.frameIndex, &cam.uniforms(), t.width, t.height, t.depth, t.onDevice ? 1u : 0u, stream) !=
        PROSPER_PT_OK)
        throw std::runtime_error(std::string("ForwardRenderer::recordTransparent: ") + prosper_pt_last_error());
}

void ForwardRenderer::recordTransparentRaster(
    const scene::Camera &cam, const TransparentInOut &t, const LightClusteringOutput *lightClusters, bool applyIbl, scene::DrawType drawType,
    void *stream)
{
    PROSPER_ASSERT(m_initialized);
    const prosper_CameraUniforms &u = cam.uniforms();
    if (t.width != u.resolution[0] || t.height != u.resolution[1])
        throw std::runtime_error("ForwardRenderer::recordTransparentRaster: the targets' extent is not the camera's resolution");
    if (lightClusters && (lightClusters->width != t.width || lightClusters->height != t.height))
        throw std::runtime_error("ForwardRenderer::recordTransparentRaster: the light clusters were built for another extent");

    // ForwardRenderer.cpp:658-662
    prosper_pt_forward_pc pc = {};
    pc.drawType = static_cast<uint32_t>(drawType);
    pc.ibl = applyIbl ? 1u : 0u;
    m_lastPC = pc;

    if (prosper_pt_set_texture_lod(m_ctx, m_textureLod ? 1 : 0, m_lodBias) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("ForwardRenderer::recordTransparentRaster: ") + prosper_pt_last_error());
    if (prosper_pt_raster_forward_transparent(m_ctx, &pc, &u, t.depth, t.onDevice ? 1u : 0u, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("ForwardRenderer::recordTransparentRaster: ") + prosper_pt_last_error());
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_forward_renderer
{
    render::ForwardRenderer pass;
};

extern "C" {

int prosper_host_forward_renderer_create(prosper_pt_ctx *ctx, prosper_host_forward_renderer **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_forward_renderer_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_forward_renderer *r = new (std::nothrow) prosper_host_forward_renderer();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_forward_renderer_destroy(prosper_host_forward_renderer *r) { delete r; }

int prosper_host_forward_renderer_set_texture_lod(prosper_host_forward_renderer *r, int enabled, float lodBias)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_forward_renderer_set_texture_lod: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    r->pass.setTextureLod(enabled != 0);
    r->pass.setLodBias(lodBias);
    return PROSPER_PT_OK;
}

int prosper_host_forward_renderer_record_transparent(
    prosper_host_forward_renderer *r, prosper_host_camera *camera, uint32_t width, uint32_t height, const float *nonLinearDepth,
    uint32_t onDevice, uint32_t rayFlags, uint32_t frameIndex, int applyIbl, uint32_t drawType, void *stream,
    prosper_pt_forward_pc *outPushConstants)
{
    if (!r || !camera)
    {
        prosper_host_set_error("prosper_host_forward_renderer_record_transparent: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (drawType >= (uint32_t)scene::DrawType::Count)
    {
        prosper_host_set_error("prosper_host_forward_renderer_record_transparent: drawType out of range");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
        render::ForwardRenderer::TransparentInOut t;
        t.depth = nonLinearDepth;
        t.onDevice = onDevice != 0u;
        t.width = width;
        t.height = height;
        t.rayFlags = rayFlags;
        t.frameIndex = frameIndex;
        r->pass.recordTransparent(cam, t, nullptr, static_cast<scene::DrawType>(drawType), applyIbl != 0, stream);
        if (outPushConstants) *outPushConstants = r->pass.lastPushConstants();
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

int prosper_host_forward_renderer_record_transparent_raster(
    prosper_host_forward_renderer *r, prosper_host_camera *camera, uint32_t width, uint32_t height, const float *nonLinearDepth,
    uint32_t onDevice, int applyIbl, uint32_t drawType, void *stream, prosper_pt_forward_pc *outPushConstants)
{
    if (!r || !camera)
    {
        prosper_host_set_error("prosper_host_forward_renderer_record_transparent_raster: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (drawType >= (uint32_t)scene::DrawType::Count)
    {
        prosper_host_set_error("prosper_host_forward_renderer_record_transparent_raster: drawType out of range");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
        render::ForwardRenderer::TransparentInOut t;
        t.depth = nonLinearDepth;
        t.onDevice = onDevice != 0u;
        t.width = width;
        t.height = height;
        r->pass.recordTransparentRaster(cam, t, nullptr, applyIbl != 0, static_cast<scene::DrawType>(drawType), stream);
        if (outPushConstants) *outPushConstants = r->pass.lastPushConstants();
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

int prosper_host_forward_renderer_record_opaque(
    prosper_host_forward_renderer *r, prosper_host_camera *camera, uint32_t width, uint32_t height, int applyIbl, uint32_t drawType,
    const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount, void *stream, prosper_host_forward_renderer_output *out)
{
    if (!r || !camera || !out)
    {
        prosper_host_set_error("prosper_host_forward_renderer_record_opaque: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (drawType >= (uint32_t)scene::DrawType::Count)
    {
        prosper_host_set_error("prosper_host_forward_renderer_record_opaque: drawType out of range");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    scene::Camera &cam = *prosper_host_camera_object(camera);
    cam.updateResolution(width, height);
    cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
    render::ForwardRenderer::OpaqueOutput o;
    const int rc = r->pass.tryRecordOpaque(cam.uniforms(), applyIbl != 0, static_cast<scene::DrawType>(drawType), transforms, transformCount, o, stream);
    if (rc != PROSPER_PT_OK)
    {
        prosper_host_set_error((std::string("ForwardRenderer::recordOpaque: ") + prosper_pt_last_error()).c_str());
        return rc;
    }
    *out = prosper_host_forward_renderer_output{o.illumination, o.velocity, o.depth};
    return PROSPER_PT_OK;
}

int prosper_host_forward_renderer_release_preserved(prosper_host_forward_renderer *r)
{
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.releasePreserved();
    return PROSPER_PT_OK;
}

} // extern "C"
