// host/texture_readback.cpp — see texture_readback.hpp.
#include "texture_readback.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render
{

void TextureReadback::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

void TextureReadback::startFrame()
{
    // TextureReadback.cpp:65-72
    if (m_framesUntilReady > 0)
        m_framesUntilReady--;
    else if (m_framesUntilReady == 0)
    {
        if (!m_polled) throw std::logic_error("Forgot to call readback() on subsequent frames after queueing readback");
        m_polled = false; // polled, and the copy had not finished: ask again this frame
    }
}

void TextureReadback::record(uint32_t resource, float pxX, float pxY, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    if (m_framesUntilReady != -1) throw std::logic_error("Readback already queued and unread");
    if (prosper_pt_texture_readback(m_ctx, resource, pxX, pxY, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("TextureReadback::record: ") + prosper_pt_last_error());
    m_framesUntilReady = MAX_FRAMES_IN_FLIGHT;
    m_polled = false;
}

std::optional<std::array<float, 4>> TextureReadback::readback()
{
    PROSPER_ASSERT(m_initialized);
    if (m_framesUntilReady < 0) throw std::logic_error("No readback in flight");
    if (m_framesUntilReady > 0) return {};
    m_polled = true;
    std::array<float, 4> value = {};
    const int rc = prosper_pt_try_texture_readback(m_ctx, value.data());
    if (rc == PROSPER_PT_NOT_READY) return {};
    if (rc != PROSPER_PT_OK) throw std::runtime_error(std::string("TextureReadback::readback: ") + prosper_pt_last_error());
    m_framesUntilReady = -1;
    return value;
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_texture_readback
{
    render::TextureReadback pass;
};

extern "C" {

int prosper_host_texture_readback_create(prosper_pt_ctx *ctx, prosper_host_texture_readback **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_texture_readback_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_texture_readback *r = new (std::nothrow) prosper_host_texture_readback();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_texture_readback_destroy(prosper_host_texture_readback *r) { delete r; }

int prosper_host_texture_readback_start_frame(prosper_host_texture_readback *r)
{
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    try
    {
        r->pass.startFrame();
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    return PROSPER_PT_OK;
}

int prosper_host_texture_readback_record(prosper_host_texture_readback *r, uint32_t resource, float pxX, float pxY, void *stream)
{
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    try
    {
        r->pass.record(resource, pxX, pxY, stream);
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

int prosper_host_texture_readback_readback(prosper_host_texture_readback *r, float out[4], uint32_t *outReady)
{
    if (!r || !out || !outReady) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *outReady = 0u;
    try
    {
        const auto value = r->pass.readback();
        if (value)
        {
            for (int i = 0; i < 4; ++i) out[i] = (*value)[i];
            *outReady = 1u;
        }
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

int32_t prosper_host_texture_readback_frames_until_ready(const prosper_host_texture_readback *r)
{
    return r ? r->pass.framesUntilReady() : -1;
}

} // extern "C"
