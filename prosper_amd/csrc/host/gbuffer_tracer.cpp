// host/gbuffer_tracer.cpp — see gbuffer_tracer.hpp.
#include "gbuffer_tracer.hpp"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void GBufferTracer::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

// the context's texture-LOD state is this pass's before each of its records (another user of the context may have set it)
void GBufferTracer::applyTextureLod(const char *what) const
{
    if (prosper_pt_set_texture_lod(m_ctx, m_textureLod ? 1 : 0, m_lodBias) != PROSPER_PT_OK)
        throw std::runtime_error(std::string(what) + ": " + prosper_pt_last_error());
}

rtdi::GBuffer GBufferTracer::record(
    const scene::Camera &cam, uint32_t width, uint32_t height, scene::DrawType drawType, uint32_t frameIndex, bool jitter,
    void *stream)
{
    PROSPER_ASSERT(m_initialized);
    applyTextureLod("GBufferTracer::record");
    const uint32_t flags = (jitter ? PROSPER_PT_GBUFFER_JITTER : 0u) | (m_opaqueOnly ? PROSPER_PT_GBUFFER_OPAQUE_ONLY : 0u);
    if (prosper_pt_trace_gbuffer(
            m_ctx, static_cast<uint32_t>(drawType), frameIndex, flags, &cam.uniforms(), width, height, nullptr, stream) !=
        PROSPER_PT_OK)
        throw std::runtime_error(std::string("GBufferTracer::record: ") + prosper_pt_last_error());
    prosper_pt_restir_inputs in = {};
    if (prosper_pt_get_gbuffer_device_ptrs(m_ctx, &in, nullptr, nullptr) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("GBufferTracer::record: ") + prosper_pt_last_error());
    rtdi::GBuffer ret;
    ret.albedoRoughness = in.albedoRoughness;
    ret.normalMetallic = in.normalMetallic;
    ret.nonLinearDepth = in.nonLinearDepth;
    ret.onDevice = true;
    ret.width = width;
    ret.height = height;
    return ret;
}

GBufferTracer::VelocityGBuffer GBufferTracer::recordVelocity(
    const scene::Camera &cam, uint32_t width, uint32_t height, scene::DrawType drawType, uint32_t frameIndex,
    const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    applyTextureLod("GBufferTracer::recordVelocity");
    prosper_pt_velocity_gbuffer_desc desc = {};
    if (transforms && m_previousTransforms.size() == transformCount && transformCount != 0u)
    {
        desc.previousTransforms = m_previousTransforms.data();
        desc.previousTransformCount = transformCount;
    }
    if (prosper_pt_trace_gbuffer_velocity(
            m_ctx, static_cast<uint32_t>(drawType), frameIndex, m_opaqueOnly ? PROSPER_PT_GBUFFER_OPAQUE_ONLY : 0u, &cam.uniforms(),
            width, height, &desc, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("GBufferTracer::recordVelocity: ") + prosper_pt_last_error());
    if (transforms)
        m_previousTransforms.assign(transforms, transforms + transformCount);
    else
        m_previousTransforms.clear();
    prosper_pt_restir_inputs in = {};
    void *velocity = nullptr;
    if (prosper_pt_get_gbuffer_device_ptrs(m_ctx, &in, nullptr, nullptr) != PROSPER_PT_OK ||
        prosper_pt_get_velocity_device_ptr(m_ctx, &velocity, nullptr, nullptr) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("GBufferTracer::recordVelocity: ") + prosper_pt_last_error());
    VelocityGBuffer ret;
    ret.gbuffer.albedoRoughness = in.albedoRoughness;
    ret.gbuffer.normalMetallic = in.normalMetallic;
    ret.gbuffer.nonLinearDepth = in.nonLinearDepth;
    ret.gbuffer.onDevice = true;
    ret.gbuffer.width = width;
    ret.gbuffer.height = height;
    ret.velocity = velocity;
    return ret;
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_gbuffer_tracer
{
    render::GBufferTracer pass;
};

extern "C" {

int prosper_host_gbuffer_tracer_create(prosper_pt_ctx *ctx, prosper_host_gbuffer_tracer **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_gbuffer_tracer_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_gbuffer_tracer *r = new (std::nothrow) prosper_host_gbuffer_tracer();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_gbuffer_tracer_destroy(prosper_host_gbuffer_tracer *r) { delete r; }

int prosper_host_gbuffer_tracer_set_opaque_only(prosper_host_gbuffer_tracer *r, int opaqueOnly)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_gbuffer_tracer_set_opaque_only: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    r->pass.setOpaqueOnly(opaqueOnly != 0);
    return PROSPER_PT_OK;
}

int prosper_host_gbuffer_tracer_set_texture_lod(prosper_host_gbuffer_tracer *r, int enabled, float lodBias)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_gbuffer_tracer_set_texture_lod: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    r->pass.setTextureLod(enabled != 0);
    r->pass.setLodBias(lodBias);
    return PROSPER_PT_OK;
}

float prosper_host_renderer_lod_bias(int applyTaa) { return render::GBufferTracer::lodBias(applyTaa != 0); }

int prosper_host_gbuffer_tracer_record(
    prosper_host_gbuffer_tracer *r, prosper_host_camera *camera, uint32_t width, uint32_t height, uint32_t drawType,
    uint32_t frameIndex, int jitter, void *stream, prosper_pt_restir_inputs *outGBuffer)
{
    if (!r || !camera || !outGBuffer)
    {
        prosper_host_set_error("prosper_host_gbuffer_tracer_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (drawType >= (uint32_t)scene::DrawType::Count)
    {
        prosper_host_set_error("prosper_host_gbuffer_tracer_record: drawType out of range");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer();
        const render::rtdi::GBuffer g =
            r->pass.record(cam, width, height, static_cast<scene::DrawType>(drawType), frameIndex, jitter != 0, stream);
        *outGBuffer = prosper_pt_restir_inputs{};
        outGBuffer->albedoRoughness = g.albedoRoughness;
        outGBuffer->normalMetallic = g.normalMetallic;
        outGBuffer->nonLinearDepth = g.nonLinearDepth;
        outGBuffer->onDevice = 1;
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

int prosper_host_gbuffer_tracer_record_velocity(
    prosper_host_gbuffer_tracer *r, prosper_host_camera *camera, uint32_t width, uint32_t height, uint32_t drawType,
    uint32_t frameIndex, const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount, void *stream,
    prosper_pt_restir_inputs *outGBuffer, void **outVelocity)
{
    if (!r || !camera || !outGBuffer || !outVelocity)
    {
        prosper_host_set_error("prosper_host_gbuffer_tracer_record_velocity: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (drawType >= (uint32_t)scene::DrawType::Count)
    {
        prosper_host_set_error("prosper_host_gbuffer_tracer_record_velocity: drawType out of range");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer();
        const render::GBufferTracer::VelocityGBuffer g = r->pass.recordVelocity(
            cam, width, height, static_cast<scene::DrawType>(drawType), frameIndex, transforms, transformCount, stream);
        *outGBuffer = prosper_pt_restir_inputs{};
        outGBuffer->albedoRoughness = g.gbuffer.albedoRoughness;
        outGBuffer->normalMetallic = g.gbuffer.normalMetallic;
        outGBuffer->nonLinearDepth = g.gbuffer.nonLinearDepth;
        outGBuffer->onDevice = 1;
        *outVelocity = const_cast<void *>(g.velocity);
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

} // extern "C"
