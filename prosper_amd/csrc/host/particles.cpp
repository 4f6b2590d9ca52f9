// host/particles.cpp — see particles.hpp.
#include "particles.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace render::particles
{

void Particles::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

bool Particles::record(const scene::Camera &cam, const InOutTargets &t, float deltaTimeS, void *stream)
{
    PROSPER_ASSERT(m_initialized);

    prosper_pt_particles_pc pc = {};
    pc.maxParticleCount = m_maxParticleCount;
    pc.sourceDrawInstanceIndex = m_sourceDrawInstanceIndex;
    pc.reset = m_resetParticles ? 1u : 0u; // Particles.cpp:116-124
    pc.deltaTimeS = deltaTimeS;
    pc.simulateFrameIndex = m_simulateFrameIndex + 1u;      // Simulate.cpp:61
    pc.renderFrameIndex = (m_renderFrameIndex + 1u) % 64u;  // Render.cpp:98

    if (prosper_pt_particles(m_ctx, &pc, PROSPER_PT_PARTICLES_ALL, &cam.uniforms(), t.width, t.height, t.depth, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("Particles::record: ") + prosper_pt_last_error());
    m_simulateFrameIndex = pc.simulateFrameIndex;
    m_renderFrameIndex = pc.renderFrameIndex;
    m_lastPC = pc;

    bool initRecorded = false;
    if (m_resetParticles)
    {
        prosper_pt_particles_info info = {};
        if (prosper_pt_get_particles_info(m_ctx, &info) != PROSPER_PT_OK)
            throw std::runtime_error(std::string("Particles::record: ") + prosper_pt_last_error());
        initRecorded = info.initRecorded != 0u;
        // Particles.cpp:126-135
        if (initRecorded) m_resetParticles = false;
    }
    return initRecorded;
}

} // namespace render::particles

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_particles
{
    render::particles::Particles pass;
};

extern "C" {

int prosper_host_particles_create(prosper_pt_ctx *ctx, prosper_host_particles **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_particles_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_particles *r = new (std::nothrow) prosper_host_particles();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_particles_destroy(prosper_host_particles *r) { delete r; }

void prosper_host_particles_set_source(prosper_host_particles *r, uint32_t sourceDrawInstanceIndex)
{
    if (r) r->pass.setSourceDrawInstance(sourceDrawInstanceIndex);
}

void prosper_host_particles_set_max_particle_count(prosper_host_particles *r, uint32_t maxParticleCount)
{
    if (r) r->pass.setMaxParticleCount(maxParticleCount);
}

int prosper_host_particles_record(
    prosper_host_particles *r, prosper_host_camera *camera, uint32_t width, uint32_t height, float *nonLinearDepth,
    float deltaTimeS, void *stream, prosper_pt_particles_pc *outPushConstants, uint32_t *outInitRecorded)
{
    if (!r || !camera)
    {
        prosper_host_set_error("prosper_host_particles_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
        render::particles::Particles::InOutTargets t;
        t.depth = nonLinearDepth;
        t.width = width;
        t.height = height;
        const bool initRecorded = r->pass.record(cam, t, deltaTimeS, stream);
        if (outPushConstants) *outPushConstants = r->pass.lastPushConstants();
        if (outInitRecorded) *outInitRecorded = initRecorded ? 1u : 0u;
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

} // extern "C"
