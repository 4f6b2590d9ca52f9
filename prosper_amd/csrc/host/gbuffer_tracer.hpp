// host/gbuffer_tracer.hpp — render::GBufferTracer of the headless host layer.
//
// A ray-traced stand-in for the output of prosper's raster pass (reference: src/render/GBufferRenderer.hpp,
// GBufferRenderer::record): the albedo/roughness, normal/metallic and depth images RtDirectIllumination reads, traced
// over the context's scene by prosper_pt_trace_gbuffer into context-owned device buffers.  The raster pass itself
// (meshlet culling, velocity, TAA jitter) stays out of scope.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"
#include "rt_direct_illumination.hpp"
#include "rt_reference.hpp"

namespace render
{

class GBufferTracer
{
  public:
    GBufferTracer() noexcept = default;
    GBufferTracer(const GBufferTracer &) = delete;
    GBufferTracer &operator=(const GBufferTracer &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    // Traces the G-buffer for the camera's current uniforms (the caller has run Camera::updateBuffer) at the camera's
    // resolution `width` x `height`.  `jitter`: the path tracer's jittered sample of (px, py, frameIndex) instead of
    // the pixel centre.  The returned device pointers stay valid until the next record with a larger extent or the
    // context's destruction.  Throws std::runtime_error on failure.
    [[nodiscard]] rtdi::GBuffer record(
        const scene::Camera &cam, uint32_t width, uint32_t height, scene::DrawType drawType, uint32_t frameIndex,
        bool jitter, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
};

} // namespace render
