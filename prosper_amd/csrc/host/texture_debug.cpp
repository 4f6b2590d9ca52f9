// host/texture_debug.cpp — see texture_debug.hpp.
#include "texture_debug.hpp"

#include <cstring>
#include <new>
#include <stdexcept>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void TextureDebug::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

void TextureDebug::record(
    uint32_t outWidth, uint32_t outHeight, std::optional<std::array<float, 2>> cursorUv, void *deviceRgba8, uint8_t *hostRgba8,
    size_t byteSize, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    if (!textureSelected()) throw std::logic_error("TextureDebug::record: no texture is selected");
    const uint32_t count = prosper_pt_debug_resource_count(m_ctx);
    uint32_t index = count;
    prosper_pt_debug_resource resource = {};
    for (uint32_t i = 0; i < count && index == count; ++i)
        if (prosper_pt_get_debug_resource(m_ctx, i, &resource) == PROSPER_PT_OK && m_target == resource.name) index = i;
    if (index == count) throw std::runtime_error("TextureDebug::record: the registry has no image called " + m_target);

    TargetSettings &s = m_targetSettings[m_target];
    // TextureDebug.cpp: the slider's range is the image's mips
    const int32_t lastLevel = resource.levelCount ? (int32_t)resource.levelCount - 1 : 0;
    s.lod = s.lod < 0 ? 0 : (s.lod > lastLevel ? lastLevel : s.lod);

    prosper_pt_texture_debug_pc pc = {};
    pc.inRes[0] = (int32_t)resource.width, pc.inRes[1] = (int32_t)resource.height;
    pc.outRes[0] = (int32_t)outWidth, pc.outRes[1] = (int32_t)outHeight;
    pc.range[0] = s.range[0], pc.range[1] = s.range[1];
    pc.lod = (uint32_t)s.lod;
    pc.flags = (uint32_t)s.channelType | (s.absBeforeRange ? PROSPER_PT_TEXTURE_DEBUG_ABS_BEFORE_RANGE : 0u) |
               (m_zoom ? PROSPER_PT_TEXTURE_DEBUG_ZOOM : 0u) | (cursorUv ? PROSPER_PT_TEXTURE_DEBUG_MAGNIFIER : 0u);
    if (cursorUv) pc.cursorUv[0] = (*cursorUv)[0], pc.cursorUv[1] = (*cursorUv)[1];
    if (prosper_pt_texture_debug(m_ctx, index, &pc, s.useBilinearSampler ? 1u : 0u, deviceRgba8, hostRgba8, byteSize, stream) !=
        PROSPER_PT_OK)
        throw std::runtime_error(std::string("TextureDebug::record: ") + prosper_pt_last_error());
    m_lastPC = pc;
}

std::array<float, 4> TextureDebug::peekedValue() const
{
    std::array<float, 4> v = {};
    if (prosper_pt_get_texture_debug_peek(m_ctx, v.data()) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("TextureDebug::peekedValue: ") + prosper_pt_last_error());
    return v;
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_texture_debug
{
    render::TextureDebug pass;
};

extern "C" {

int prosper_host_texture_debug_create(prosper_pt_ctx *ctx, prosper_host_texture_debug **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_texture_debug_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_texture_debug *r = new (std::nothrow) prosper_host_texture_debug();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_texture_debug_destroy(prosper_host_texture_debug *r) { delete r; }

void prosper_host_texture_debug_set_target(prosper_host_texture_debug *r, const char *name)
{
    if (r) r->pass.setTarget(name ? name : "");
}

int prosper_host_texture_debug_texture_selected(const prosper_host_texture_debug *r) { return r && r->pass.textureSelected() ? 1 : 0; }

void prosper_host_texture_debug_set_settings(
    prosper_host_texture_debug *r, const char *name, float rangeLo, float rangeHi, int32_t lod, uint32_t channelType,
    int absBeforeRange, int useBilinearSampler)
{
    if (!r || !name) return;
    render::TextureDebug::TargetSettings &s = r->pass.settings(name);
    s.range[0] = rangeLo, s.range[1] = rangeHi;
    s.lod = lod;
    s.channelType = (render::TextureDebug::ChannelType)(channelType > 4u ? 4u : channelType);
    s.absBeforeRange = absBeforeRange != 0;
    s.useBilinearSampler = useBilinearSampler != 0;
}

void prosper_host_texture_debug_set_zoom(prosper_host_texture_debug *r, int zoom)
{
    if (r) r->pass.setZoom(zoom != 0);
}

int prosper_host_texture_debug_record(
    prosper_host_texture_debug *r, uint32_t outWidth, uint32_t outHeight, const float *cursorUv, void *deviceRgba8,
    uint8_t *hostRgba8, size_t byteSize, void *stream, prosper_pt_texture_debug_pc *outPushConstants)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_texture_debug_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        std::optional<std::array<float, 2>> cursor;
        if (cursorUv) cursor = std::array<float, 2>{cursorUv[0], cursorUv[1]};
        r->pass.record(outWidth, outHeight, cursor, deviceRgba8, hostRgba8, byteSize, stream);
        if (outPushConstants) *outPushConstants = r->pass.lastPushConstants();
    }
    catch (const std::logic_error &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

int prosper_host_texture_debug_peeked_value(prosper_host_texture_debug *r, float out[4])
{
    if (!r || !out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    try
    {
        const std::array<float, 4> v = r->pass.peekedValue();
        std::memcpy(out, v.data(), sizeof(float) * 4);
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

} // extern "C"
