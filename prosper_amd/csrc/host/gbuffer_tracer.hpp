// host/gbuffer_tracer.hpp — render::GBufferTracer of the headless host layer.
//
// A ray-traced stand-in for the output of prosper's raster pass (reference: src/render/GBufferRenderer.hpp,
// GBufferRenderer::record): the albedo/roughness, normal/metallic and depth images RtDirectIllumination reads, traced
// over the context's scene by prosper_pt_trace_gbuffer into context-owned device buffers, and with `recordVelocity` the
// velocity image TemporalAntiAliasing reads, sampled through the camera's TAA jitter (prosper_pt_trace_gbuffer_velocity;
// DESIGN.md f10).  The meshlet culling GBufferRenderer::record runs around its draws is render::MeshletCuller
// (meshlet_culler.hpp; prosper_pt_cull_gbuffer is the whole sequence); the mesh-shader draws themselves stay
// out of scope.
#pragma once

#include <cstdint>
#include <vector>

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

    // BLEND surfaces are left out of both records (PROSPER_PT_GBUFFER_OPAQUE_ONLY), as prosper's G-buffer leaves them to
    // ForwardRenderer::recordTransparent.  Off by default.
    void setOpaqueOnly(bool opaqueOnly) { m_opaqueOnly = opaqueOnly; }
    [[nodiscard]] bool opaqueOnly() const { return m_opaqueOnly; }

    // Material textures sampled through their mip chains by both records (prosper_pt_set_texture_lod; the context must
    // have been created with PROSPER_PT_CREATE_TEXTURE_MIPS), with the bias prosper writes beside its material buffer
    // each frame: lodBias(applyTaa), Renderer::lodBias() (Renderer.cpp:709-715).  Off, bias 0 by default.
    void setTextureLod(bool enabled) { m_textureLod = enabled; }
    void setLodBias(float lodBias) { m_lodBias = lodBias; }
    [[nodiscard]] bool textureLod() const { return m_textureLod; }
    [[nodiscard]] float lodBias() const { return m_lodBias; }
    [[nodiscard]] static float lodBias(bool applyTaa) { return applyTaa ? -1.0f : 0.0f; }

    // Traces the G-buffer for the camera's current uniforms (the caller has run Camera::updateBuffer) at the camera's
    // resolution `width` x `height`.  `jitter`: the path tracer's jittered sample of (px, py, frameIndex) instead of
    // the pixel centre.  The returned device pointers stay valid until the next record with a larger extent or the
    // context's destruction.  Throws std::runtime_error on failure.
    [[nodiscard]] rtdi::GBuffer record(
        const scene::Camera &cam, uint32_t width, uint32_t height, scene::DrawType drawType, uint32_t frameIndex,
        bool jitter, void *stream);

    struct VelocityGBuffer
    {
        rtdi::GBuffer gbuffer;
        const void *velocity{nullptr}; // device pointer, width * height float2
    };
    // The same through the pixel centres of the camera's (jittered) projection, with the velocity target.  `transforms`
    // (optional, `transformCount` = the scene's model instances): the instance transforms of this frame.  They are kept,
    // and what the previous call kept is handed on as the previous frame's transforms (World keeps the previous
    // frame's transform buffer the same way); the first call and a call after a changed count see unmoved instances.
    // Without `transforms` the instances count as unmoved and nothing is kept.
    [[nodiscard]] VelocityGBuffer recordVelocity(
        const scene::Camera &cam, uint32_t width, uint32_t height, scene::DrawType drawType, uint32_t frameIndex,
        const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    bool m_opaqueOnly{false};
    bool m_textureLod{false};
    float m_lodBias{0.0f};
    void applyTextureLod(const char *what) const;
    std::vector<prosper_ModelInstanceTransforms> m_previousTransforms;
};

} // namespace render
