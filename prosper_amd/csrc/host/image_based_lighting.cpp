// host/image_based_lighting.cpp — see image_based_lighting.hpp.
#include "image_based_lighting.hpp"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void ImageBasedLighting::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

bool ImageBasedLighting::isGenerated() const
{
    PROSPER_ASSERT(m_initialized);
    prosper_pt_ibl_info info = {};
    if (prosper_pt_get_ibl_info(m_ctx, &info) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("ImageBasedLighting::isGenerated: ") + prosper_pt_last_error());
    return info.generated != 0;
}

// ImageBasedLighting.cpp recordGeneration: the irradiance, radiance and BRDF LUT passes on `stream`
void ImageBasedLighting::recordGeneration(void *stream)
{
    PROSPER_ASSERT(m_initialized);
    if (prosper_pt_generate_ibl(m_ctx, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("ImageBasedLighting::recordGeneration: ") + prosper_pt_last_error());
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_image_based_lighting
{
    render::ImageBasedLighting pass;
};

extern "C" {

int prosper_host_image_based_lighting_create(prosper_pt_ctx *ctx, prosper_host_image_based_lighting **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_image_based_lighting_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_image_based_lighting *r = new (std::nothrow) prosper_host_image_based_lighting();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_image_based_lighting_destroy(prosper_host_image_based_lighting *r) { delete r; }

int prosper_host_image_based_lighting_is_generated(prosper_host_image_based_lighting *r)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_image_based_lighting_is_generated: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        return r->pass.isGenerated() ? 1 : 0;
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
}

int prosper_host_image_based_lighting_record_generation(prosper_host_image_based_lighting *r, void *stream)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_image_based_lighting_record_generation: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        r->pass.recordGeneration(stream);
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

} // extern "C"
