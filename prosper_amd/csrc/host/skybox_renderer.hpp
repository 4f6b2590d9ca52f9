// host/skybox_renderer.hpp — render::SkyboxRenderer of the headless host layer.
//
// Same role as prosper's pass (reference: src/render/SkyboxRenderer.hpp, SkyboxRenderer.cpp): `record` draws the sky
// into the illumination wherever the depth is the far plane's, through prosper_pt_skybox_fill over the context's HDR
// image.  There is no velocity target.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"
#include "rt_reference.hpp"

namespace render
{

class SkyboxRenderer
{
  public:
    SkyboxRenderer() noexcept = default;
    SkyboxRenderer(const SkyboxRenderer &) = delete;
    SkyboxRenderer &operator=(const SkyboxRenderer &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    struct RecordInOut
    {
        const float *depth{nullptr}; // non-linear depth; nullptr: the last traced G-buffer's
        bool onDevice{true};
        uint32_t width{0}; // of the context's HDR image, the illumination
        uint32_t height{0};
    };
    // The camera's current uniforms (the caller has run Camera::updateBuffer).  Throws std::runtime_error on failure.
    void record(const scene::Camera &cam, const RecordInOut &inOutTargets, void *stream) const;

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
};

} // namespace render
