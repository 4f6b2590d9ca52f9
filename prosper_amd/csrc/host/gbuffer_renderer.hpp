// host/gbuffer_renderer.hpp — render::GBufferRenderer of the headless host layer.
//
// Same role as prosper's pass (reference: src/render/GBufferRenderer.hpp, GBufferRenderer.cpp:146-231): record culls the
// scene's meshlets in two phases around its own depth, draws them and leaves albedoRoughness, normalMetalness, velocity and
// depth.  Here the draws are the compute rasteriser's and its resolve (prosper_pt_raster_gbuffer), one chain
// of launches on the caller's stream.  Device pointers stand in for the reference's image handles; the images are the
// context's own G-buffer targets, so every pass that reads "the last G-buffer" reads this one.  `world` is the scene the
// context holds and `renderArea` the camera's resolution: neither is a parameter.  `nextFrame` is the context's slot
// bookkeeping (the pyramid kept for the next record), which releasePreserved forgets.
#pragma once

#include <cstdint>
#include <vector>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"
#include "hierarchical_depth_downsampler.hpp"
#include "meshlet_culler.hpp"
#include "rt_reference.hpp"

namespace render
{

struct GBufferRendererOutput
{
    const void *albedoRoughness{nullptr}; // device pointers: width * height float4, float4, float2, float
    const void *normalMetalness{nullptr};
    const void *velocity{nullptr};
    const float *depth{nullptr};
};

class GBufferRenderer
{
  public:
    GBufferRenderer() noexcept = default;
    GBufferRenderer(const GBufferRenderer &) = delete;
    GBufferRenderer &operator=(const GBufferRenderer &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    // Records the G-buffer for the camera's current uniforms (the caller has run Camera::updateBuffer).  `transforms`
    // (optional, `transformCount` = the scene's model instances): this frame's instance transforms; they are kept, and
    // what the previous call kept is the previous frame's (the velocity's), as GBufferTracer::recordVelocity keeps them.
    // `drawStats` receives the host's totals; its device counts come with readDrawStats.  Throws std::runtime_error.
    [[nodiscard]] GBufferRendererOutput record(
        const scene::Camera &cam, scene::DrawType drawType, const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount,
        DrawStats *drawStats, void *stream);
    // the same without exceptions: the library's return code (prosper_pt_last_error has the text)
    [[nodiscard]] int tryRecord(
        const prosper_CameraUniforms &cam, scene::DrawType drawType, const prosper_ModelInstanceTransforms *transforms, uint32_t transformCount,
        GBufferRendererOutput &out, void *stream) noexcept;
    bool readDrawStats(DrawStats &drawStats, bool wait) const { return m_culler.readDrawStats(drawStats, wait); }
    // forgets the previous frame: the kept pyramid and the kept transforms
    void releasePreserved();

    [[nodiscard]] const MeshletCuller &meshletCuller() const { return m_culler; }
    [[nodiscard]] const HierarchicalDepthDownsampler &hierarchicalDepthDownsampler() const { return m_downsampler; }
    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    MeshletCuller m_culler;
    HierarchicalDepthDownsampler m_downsampler;
    std::vector<prosper_ModelInstanceTransforms> m_previousTransforms;
};

} // namespace render
