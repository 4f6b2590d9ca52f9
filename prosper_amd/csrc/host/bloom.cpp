// host/bloom.cpp — see bloom.hpp.
#include "bloom.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render::bloom
{

void Bloom::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

void Bloom::setBlendFactors(float mip0, float mip1, float mip2)
{
    m_blendFactors[0] = mip0;
    m_blendFactors[1] = mip1;
    m_blendFactors[2] = mip2;
}

prosper_pt_bloom_pc Bloom::pushConstants() const
{
    prosper_pt_bloom_pc pc = {};
    pc.threshold = m_threshold;
    for (int k = 0; k < 3; ++k) pc.blendFactors[k] = m_blendFactors[k];
    pc.resolutionScale = static_cast<uint32_t>(m_resolutionScale);
    pc.biquadratic = m_biquadraticSampling ? 1u : 0u;
    return pc;
}

prosper_pt_bloom_fft_pc Bloom::fftPushConstants() const
{
    prosper_pt_bloom_fft_pc pc = {};
    pc.threshold = m_threshold;
    pc.resolutionScale = static_cast<uint32_t>(m_resolutionScale);
    pc.biquadratic = m_biquadraticSampling ? 1u : 0u;
    pc.regenerateKernel = m_regenerateKernel ? 1u : 0u;
    return pc;
}

void Bloom::releasePreserved()
{
    PROSPER_ASSERT(m_initialized);
    prosper_pt_bloom_fft_release_kernel(m_ctx);
}

Bloom::Output Bloom::record(const Input &input, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    int rc;
    if (m_technique == Technique::Fft)
    {
        const prosper_pt_bloom_fft_pc pc = fftPushConstants();
        rc = prosper_pt_bloom_fft(m_ctx, &pc, input.width, input.height, input.illumination, input.onDevice ? 1u : 0u, stream);
    }
    else
    {
        releasePreserved(); // Bloom.cpp:117
        const prosper_pt_bloom_pc pc = pushConstants();
        rc = prosper_pt_bloom(m_ctx, &pc, input.width, input.height, input.illumination, input.onDevice ? 1u : 0u, stream);
    }
    if (rc != PROSPER_PT_OK) throw std::runtime_error(std::string("Bloom::record: ") + prosper_pt_last_error());
    Output ret;
    void *ptr = nullptr;
    if (prosper_pt_get_hdr_device_ptr(m_ctx, &ptr, nullptr) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("Bloom::record: ") + prosper_pt_last_error());
    ret.illuminationWithBloom = static_cast<const float *>(ptr);
    ret.width = input.width;
    ret.height = input.height;
    return ret;
}

} // namespace render::bloom

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_bloom
{
    render::bloom::Bloom pass;
};

extern "C" {

int prosper_host_bloom_create(prosper_pt_ctx *ctx, prosper_host_bloom **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_bloom_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_bloom *r = new (std::nothrow) prosper_host_bloom();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_bloom_destroy(prosper_host_bloom *r) { delete r; }

void prosper_host_bloom_draw_ui(
    prosper_host_bloom *r, float threshold, float blendFactor0, float blendFactor1, float blendFactor2, uint32_t biquadratic,
    uint32_t resolutionScale)
{
    if (!r) return;
    r->pass.setThreshold(threshold);
    r->pass.setBlendFactors(blendFactor0, blendFactor1, blendFactor2);
    r->pass.setBiquadraticSampling(biquadratic != 0u);
    r->pass.setResolutionScale(static_cast<render::bloom::ResolutionScale>(resolutionScale));
}

void prosper_host_bloom_set_technique(prosper_host_bloom *r, uint32_t technique, uint32_t regenerateKernel)
{
    if (!r || technique > static_cast<uint32_t>(render::bloom::Technique::Fft)) return; // an unknown technique changes nothing
    r->pass.setTechnique(static_cast<render::bloom::Technique>(technique));
    r->pass.setRegenerateKernel(regenerateKernel != 0u);
}

void prosper_host_bloom_release_preserved(prosper_host_bloom *r)
{
    if (r) r->pass.releasePreserved();
}

void prosper_host_bloom_fft_push_constants(prosper_host_bloom *r, prosper_pt_bloom_fft_pc *out)
{
    if (r && out) *out = r->pass.fftPushConstants();
}

int prosper_host_bloom_record(
    prosper_host_bloom *r, uint32_t width, uint32_t height, const void *illumination, uint32_t onDevice, void *stream,
    prosper_pt_bloom_pc *outPushConstants)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_bloom_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        render::bloom::Bloom::Input in;
        in.illumination = illumination;
        in.onDevice = onDevice != 0u;
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

} // extern "C"
