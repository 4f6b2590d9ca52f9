// host/forward_renderer.hpp — render::ForwardRenderer of the headless host layer: its opaque and its transparent pass.
//
// Same role as prosper's pass (reference: src/render/ForwardRenderer.hpp, ForwardRenderer.cpp):
//   recordOpaque       (ForwardRenderer.cpp:134-217; Renderer.cpp:404-483 with m_renderDeferred == false) culls the scene's
//                      meshlets in two phases around its own depth, draws them and leaves illumination, velocity and depth.
//                      Here the draws are the compute rasteriser's and the forward shade over its visibility image
//                      (prosper_pt_raster_forward), one chain of launches on the caller's stream.  The
//                      illumination is the context's HDR image, the depth and the velocity the context's last ones, so
//                      every pass that reads "the last G-buffer's depth" reads this frame's.
//   recordTransparent  (ForwardRenderer.cpp:222-256; Renderer.cpp:493-500 runs it between the skybox and bloom) the BLEND
//                      surfaces drawn over the illumination against the depth, through prosper_pt_forward_transparent over
//                      the context's HDR image.  prosper draws them with Options{transparents, drawType},
//                      i.e. ibl = 0; `applyIbl` is there for the push constant's other value.  The culling it runs first is
//                      render::MeshletCuller in Mode::Transparent (meshlet_culler.hpp).
//   recordTransparentRaster  the same step of the raster frame: that culling and the draw of its list as one chain
//                      (prosper_pt_raster_forward_transparent).
#pragma once

#include <cstdint>
#include <vector>

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

    struct OpaqueOutput
    {
        const void *illumination{nullptr}; // device pointers: width * height float4 (the context's HDR image), float2, float
        const void *velocity{nullptr};
        const float *depth{nullptr};
    };
    // Records the opaque image for the camera's current uniforms (the caller has run Camera::updateBuffer) at the camera's
    // resolution.  `lightClusters` (optional) is checked against that extent; the pass reuses the context's clustering when
    // it was made for this camera and these lights, and clusters itself otherwise.  `transforms` (optional,
    // `transformCount` = the scene's model instances): this frame's instance transforms; they are kept, and what the
    // previous call kept is the previous frame's (the velocity's), as GBufferRenderer::record keeps them.  Throws
    // std::runtime_error on failure.
    [[nodiscard]] OpaqueOutput recordOpaque(
        const scene::Camera &cam, const LightClusteringOutput *lightClusters, bool applyIbl, scene::DrawType drawType, void *stream,
        const prosper_ModelInstanceTransforms *transforms = nullptr, uint32_t transformCount = 0);
    // the same without exceptions: the library's return code (prosper_pt_last_error has the text)
    [[nodiscard]] int tryRecordOpaque(
        const prosper_CameraUniforms &cam, bool applyIbl, scene::DrawType drawType, const prosper_ModelInstanceTransforms *transforms,
        uint32_t transformCount, OpaqueOutput &out, void *stream) noexcept;
    // forgets the previous frame: the kept pyramid and the kept transforms
    void releasePreserved();

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

    // recordTransparent over the meshlet draw lists (ForwardRenderer.cpp:222-260): the TRANSPARENT list culled
    // once without a pyramid, its fragments listed per pixel and resolved front to back over the illumination, through
    // prosper_pt_raster_forward_transparent - the raster frame's transparents, where recordTransparent above is the traced
    // frame's.  inOut.rayFlags and frameIndex are not read (the rasteriser's pixel is the camera's, jitter included); the
    // extent must be the camera's resolution.  The call waits on the host once (for the lists' size).  Arguments and
    // failures otherwise as recordTransparent.
    void recordTransparentRaster(
        const scene::Camera &cam, const TransparentInOut &inOutTargets, const LightClusteringOutput *lightClusters, bool applyIbl,
        scene::DrawType drawType, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }
    [[nodiscard]] const prosper_pt_forward_pc &lastPushConstants() const { return m_lastPC; }

    // Every surface's and layer's material sampled through the textures' mip chains (prosper_pt_set_texture_lod, which both
    // passes set before each record; the context must have been created with PROSPER_PT_CREATE_TEXTURE_MIPS), with the bias
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
    std::vector<prosper_ModelInstanceTransforms> m_previousTransforms;
};

} // namespace render
