// host/forward_renderer.hpp — render::ForwardRenderer of the headless host layer: only its transparent pass.
//
// Same role as prosper's ForwardRenderer::recordTransparent (reference: src/render/ForwardRenderer.hpp:62-72,
// ForwardRenderer.cpp:222-256; Renderer.cpp:493-500 runs it between the skybox and bloom): the BLEND surfaces drawn over
// the illumination against the depth, through prosper_pt_forward_transparent over the context's HDR image (DESIGN.md
// f12).  prosper draws them with Options{transparents, drawType}, i.e. ibl = 0; `applyIbl` is there for the push constant's
// other value.  The culling recordTransparent runs first is render::MeshletCuller in Mode::Transparent (meshlet_culler.hpp,
// DESIGN.md f17).  The opaque passes of ForwardRenderer (recordOpaque: the forward path's mesh-shader raster) stay out of
// scope like the raster G-buffer.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"
#include "light_clustering.hpp"
#include "rt_reference.hpp"

namespace render
{

class ForwardRenderer
{
  public:
    ForwardRenderer() noexcept = default;
    ForwardRenderer(const ForwardRenderer &) = delete;
    ForwardRenderer &operator=(const ForwardRenderer &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    struct TransparentInOut
    {
        const float *depth{nullptr}; // non-linear depth; nullptr: the last traced G-buffer's
        bool onDevice{true};
        uint32_t width{0}; // of the context's HDR image, the illumination
        uint32_t height{0};
        // the ray the G-buffer was traced with: 0, PROSPER_PT_TRANSPARENT_JITTER (with frameIndex) or
        // PROSPER_PT_TRANSPARENT_CAMERA_JITTER
        uint32_t rayFlags{0};
        uint32_t frameIndex{0};
    };
    // The camera's current uniforms (the caller has run Camera::updateBuffer).  `lightClusters` (optional) is checked
    // against the extent; the pass reuses the context's clustering when it was made for this camera and these lights,
    // and clusters itself otherwise.  Throws std::runtime_error on failure.
    void recordTransparent(
        const scene::Camera &cam, const TransparentInOut &inOutTargets, const LightClusteringOutput *lightClusters,
        scene::DrawType drawType, bool applyIbl, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }
    [[nodiscard]] const prosper_pt_forward_pc &lastPushConstants() const { return m_lastPC; }

    // Every layer's material sampled through the textures' mip chains (prosper_pt_set_texture_lod, which the pass sets
    // before each record; the context must have been created with PROSPER_PT_CREATE_TEXTURE_MIPS), with the bias
    // prosper's forward pass is given each frame: GBufferTracer::lodBias(applyTaa).  Off, bias 0 by default.
    void setTextureLod(bool enabled) { m_textureLod = enabled; }
    void setLodBias(float lodBias) { m_lodBias = lodBias; }
    [[nodiscard]] bool textureLod() const { return m_textureLod; }
    [[nodiscard]] float lodBias() const { return m_lodBias; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    prosper_pt_forward_pc m_lastPC{};
    bool m_textureLod{false};
    float m_lodBias{0.0f};
};

} // namespace render
