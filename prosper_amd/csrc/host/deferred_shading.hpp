// host/deferred_shading.hpp — render::DeferredShading of the headless host layer.
//
// Same surface as prosper's pass (reference: src/render/DeferredShading.hpp:18-66, DeferredShading.cpp:121-251):
// `record` shades the G-buffer over the light clusters into the context's HDR image through prosper_pt_deferred_shading
// and returns the DeferredShadingPC it pushed.  prosper_pt_deferred_shading clusters the lights itself, with the same
// camera and extent as LightClustering::record and so the same lists; Input::lightClusters is checked against the
// G-buffer's extent.  applyIbl adds evalIBL over ImageBasedLighting's maps, which recordGeneration must have made for
// the current scene (Renderer.cpp:380-382 runs it before the first frame that applies IBL).
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"
#include "light_clustering.hpp"
#include "rt_direct_illumination.hpp"
#include "rt_reference.hpp"

namespace render
{

class DeferredShading
{
  public:
    DeferredShading() noexcept = default;
    DeferredShading(const DeferredShading &) = delete;
    DeferredShading &operator=(const DeferredShading &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    struct Input
    {
        const rtdi::GBuffer &gbuffer;
        const LightClusteringOutput &lightClusters;
    };
    struct Output
    {
        const float *illumination{nullptr}; // device pointer, RGBA32F, width*height texels (the context's HDR image)
        uint32_t width{0};
        uint32_t height{0};
    };
    // The camera's current uniforms (the caller has run Camera::updateBuffer).  Throws std::runtime_error on failure.
    [[nodiscard]] Output record(
        const scene::Camera &cam, const Input &input, bool applyIbl, scene::DrawType drawType, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }
    [[nodiscard]] const prosper_pt_deferred_shading_pc &lastPushConstants() const { return m_lastPC; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    prosper_pt_deferred_shading_pc m_lastPC{};
};

} // namespace render
