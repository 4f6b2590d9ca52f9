// host/hierarchical_depth_downsampler.cpp — see hierarchical_depth_downsampler.hpp.
#include "hierarchical_depth_downsampler.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void HierarchicalDepthDownsampler::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

int HierarchicalDepthDownsampler::tryRecord(const Input &in, uint32_t nextFrame, void *stream, Output &out) const noexcept
{
    PROSPER_ASSERT(m_initialized);
    // 1 px wide/tall inputs won't behave well (HierarchicalDepthDownsampler.cpp:112): the call refuses them
    out = Output{};
    out.slot = nextFrame & 1u;
    int rc = prosper_pt_hiz_downsample(m_ctx, out.slot, in.nonLinearDepth, in.onDevice ? 1u : 0u, in.width, in.height, stream);
    if (rc != PROSPER_PT_OK) return rc;
    prosper_pt_hiz_info info = {};
    if ((rc = prosper_pt_get_hiz_info(m_ctx, out.slot, &info)) != PROSPER_PT_OK) return rc;
    out.mipCount = info.levelCount;
    for (uint32_t l = 0; l < out.mipCount; ++l)
        if ((rc = prosper_pt_get_hiz_device_ptr(m_ctx, out.slot, l, &out.mips[l], &out.mipWidth[l], &out.mipHeight[l])) != PROSPER_PT_OK)
            return rc;
    return PROSPER_PT_OK;
}

HierarchicalDepthDownsampler::Output HierarchicalDepthDownsampler::record(const Input &in, uint32_t nextFrame, void *stream) const
{
    Output out;
    if (tryRecord(in, nextFrame, stream, out) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("HierarchicalDepthDownsampler::record: ") + prosper_pt_last_error());
    return out;
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_hiz_downsampler
{
    render::HierarchicalDepthDownsampler pass;
};

extern "C" {

int prosper_host_hiz_downsampler_create(prosper_pt_ctx *ctx, prosper_host_hiz_downsampler **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_hiz_downsampler_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_hiz_downsampler *r = new (std::nothrow) prosper_host_hiz_downsampler();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_hiz_downsampler_destroy(prosper_host_hiz_downsampler *r) { delete r; }

int prosper_host_hiz_downsampler_record(
    prosper_host_hiz_downsampler *r, const float *nonLinearDepth, uint32_t onDevice, uint32_t width, uint32_t height,
    uint32_t nextFrame, uint32_t *mipCount, const float **mips, void *stream)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_hiz_downsampler_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    render::HierarchicalDepthDownsampler::Input in;
    in.nonLinearDepth = nonLinearDepth;
    in.onDevice = onDevice != 0u;
    in.width = width;
    in.height = height;
    render::HierarchicalDepthDownsampler::Output out;
    const int rc = r->pass.tryRecord(in, nextFrame, stream, out);
    if (rc != PROSPER_PT_OK)
    {
        // the library's own code, not a blanket one: a refused extent is INVALID_ARGUMENT, no G-buffer NO_SCENE
        prosper_host_set_error((std::string("HierarchicalDepthDownsampler::record: ") + prosper_pt_last_error()).c_str());
        return rc;
    }
    if (mipCount) *mipCount = out.mipCount;
    if (mips)
        for (uint32_t l = 0; l < out.mipCount; ++l) mips[l] = out.mips[l];
    return PROSPER_PT_OK;
}

} // extern "C"
