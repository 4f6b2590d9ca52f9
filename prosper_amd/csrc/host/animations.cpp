// host/animations.cpp — see animations.hpp.
#include "animations.hpp"

#include <cstring>
#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace scene
{

void Animations::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

void Animations::load(const prosper_pt_animation_desc &desc)
{
    PROSPER_ASSERT(m_initialized);
    if (prosper_pt_set_animations(m_ctx, &desc) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("Animations::load: ") + prosper_pt_last_error());
    prosper_pt_animation_state st = {};
    if (prosper_pt_get_animation_state(m_ctx, &st) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("Animations::load: ") + prosper_pt_last_error());
    m_endTimeS = st.endTimeS;
    m_nodeCount = st.nodeCount;
    m_animatedNodeCount = st.animatedNodeCount;
}

void Animations::updateAnimations(float timeS, bool now, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    if (prosper_pt_animate(m_ctx, timeS, now ? (uint32_t)PROSPER_PT_UPDATE_NOW : 0u, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("Animations::updateAnimations: ") + prosper_pt_last_error());
}

bool Animations::cameraTransform(CameraTransform &out) const
{
    PROSPER_ASSERT(m_initialized);
    prosper_pt_animation_state st = {};
    if (prosper_pt_get_animation_state(m_ctx, &st) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("Animations::cameraTransform: ") + prosper_pt_last_error());
    if (!st.cameraValid) return false;
    std::memcpy(out.eye, st.eye, sizeof(out.eye));
    std::memcpy(out.target, st.target, sizeof(out.target));
    std::memcpy(out.up, st.up, sizeof(out.up));
    return true;
}

} // namespace scene

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_animations
{
    scene::Animations animations;
};

extern "C" {

int prosper_host_animations_create(prosper_pt_ctx *ctx, const prosper_pt_animation_desc *desc, prosper_host_animations **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx || !desc)
    {
        prosper_host_set_error("prosper_host_animations_create: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_animations *r = new (std::nothrow) prosper_host_animations();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->animations.init(ctx);
    try
    {
        r->animations.load(*desc);
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        delete r;
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_animations_destroy(prosper_host_animations *r) { delete r; }

int prosper_host_animations_update(prosper_host_animations *r, float timeS)
{
    if (!r)
    {
        prosper_host_set_error("prosper_host_animations_update: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        r->animations.updateAnimations(timeS);
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    return PROSPER_PT_OK;
}

float prosper_host_animations_end_time(const prosper_host_animations *r) { return r ? r->animations.endTimeS() : 0.0f; }

} // extern "C"
