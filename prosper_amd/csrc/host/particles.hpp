// host/particles.hpp — render::particles::Particles of the headless host layer.
//
// Same role as prosper's particles::Particles (reference: src/render/particles/Particles.hpp, Particles.cpp:106-152;
// Renderer.cpp:530-538 runs it between bloom and TAA): decay, init while a reset is pending, simulate and render over the
// illumination and the depth, through prosper_pt_particles.  The pool and its freelist belong to the
// context; this class keeps what prosper's keeps on the host: the pending reset and the two frame indices.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"
#include "rt_reference.hpp"

namespace render::particles
{

class Particles
{
  public:
    Particles() noexcept = default;
    Particles(const Particles &) = delete;
    Particles &operator=(const Particles &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    struct InOutTargets
    {
        float *depth{nullptr}; // non-linear depth on the device, read and written; nullptr: the last traced G-buffer's
        uint32_t width{0};     // of the context's HDR image, the illumination
        uint32_t height{0};
    };
    // The camera's current uniforms (the caller has run Camera::updateBuffer).  Returns whether init was recorded; a
    // pending reset stays pending until it was.  Throws std::runtime_error on failure.
    bool record(const scene::Camera &cam, const InOutTargets &inOutTargets, float deltaTimeS, void *stream);

    // Particles::drawUi's "Reset particles" button
    void requestReset() { m_resetParticles = true; }
    void setSourceDrawInstance(uint32_t index) { m_sourceDrawInstanceIndex = index; }
    // 0: prosper's 500 000
    void setMaxParticleCount(uint32_t count) { m_maxParticleCount = count; }

    [[nodiscard]] bool resetPending() const { return m_resetParticles; }
    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }
    [[nodiscard]] const prosper_pt_particles_pc &lastPushConstants() const { return m_lastPC; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    bool m_resetParticles{true};
    uint32_t m_simulateFrameIndex{0};
    uint32_t m_renderFrameIndex{0};
    uint32_t m_sourceDrawInstanceIndex{0};
    uint32_t m_maxParticleCount{0};
    prosper_pt_particles_pc m_lastPC{};
};

} // namespace render::particles
