// host/temporal_anti_aliasing.cpp — see temporal_anti_aliasing.hpp.
#include "temporal_anti_aliasing.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void TemporalAntiAliasing::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

prosper_pt_taa_pc TemporalAntiAliasing::pushConstants() const
{
    prosper_pt_taa_pc pc = {};
    pc.catmullRom = m_catmullRom ? 1u : 0u;
    pc.colorClipping = static_cast<uint32_t>(m_colorClipping);
    pc.velocitySampling = static_cast<uint32_t>(m_velocitySampling);
    pc.luminanceWeighting = m_luminanceWeighting ? 1u : 0u;
    return pc;
}

TemporalAntiAliasing::Output TemporalAntiAliasing::record(const Input &input, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    const prosper_pt_taa_pc pc = pushConstants();
    prosper_pt_taa_inputs in = {};
    in.illumination = input.illumination;
    in.velocity = input.velocity;
    in.nonLinearDepth = input.nonLinearDepth;
    in.onDevice = input.onDevice ? 1u : 0u;
    if (prosper_pt_taa_resolve(m_ctx, &pc, input.width, input.height, &in, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("TemporalAntiAliasing::record: ") + prosper_pt_last_error());
    Output ret;
    void *ptr = nullptr;
    if (prosper_pt_get_hdr_device_ptr(m_ctx, &ptr, nullptr) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("TemporalAntiAliasing::record: ") + prosper_pt_last_error());
    ret.resolvedIllumination = static_cast<const float *>(ptr);
    ret.width = input.width;
    ret.height = input.height;
    return ret;
}

void TemporalAntiAliasing::releasePreserved()
{
    PROSPER_ASSERT(m_initialized);
    prosper_pt_taa_release_history(m_ctx);
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_taa
{
    render::TemporalAntiAliasing pass;
};

extern "C" {

int prosper_host_taa_create(prosper_pt_ctx *ctx, prosper_host_taa **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_taa_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_taa *r = new (std::nothrow) prosper_host_taa();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_taa_destroy(prosper_host_taa *r) { delete r; }

void prosper_host_taa_draw_ui(
    prosper_host_taa *r, uint32_t catmullRom, uint32_t colorClipping, uint32_t velocitySampling, uint32_t luminanceWeighting)
{
    if (!r) return;
    r->pass.setCatmullRom(catmullRom != 0u);
    r->pass.setColorClipping(static_cast<render::TemporalAntiAliasing::ColorClippingType>(colorClipping));
    r->pass.setVelocitySampling(static_cast<render::TemporalAntiAliasing::VelocitySamplingType>(velocitySampling));
    r->pass.setLuminanceWeighting(luminanceWeighting != 0u);
}

int prosper_host_taa_record(
    prosper_host_taa *r, uint32_t width, uint32_t height, const prosper_pt_taa_inputs *inputs, void *stream,
    prosper_pt_taa_pc *outPushConstants)
{
    if (!r || !inputs)
    {
        prosper_host_set_error("prosper_host_taa_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        render::TemporalAntiAliasing::Input in;
        in.illumination = inputs->illumination;
        in.velocity = inputs->velocity;
        in.nonLinearDepth = inputs->nonLinearDepth;
        in.onDevice = inputs->onDevice != 0u;
        in.width = width;
        in.height = height;
        (void)r->pass.record(in, stream);
        if (outPushConstants) *outPushConstants = r->pass.pushConstants();
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

void prosper_host_taa_release_preserved(prosper_host_taa *r)
{
    if (r) r->pass.releasePreserved();
}

} // extern "C"
