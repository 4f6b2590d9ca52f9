// host/image_based_lighting.hpp — render::ImageBasedLighting of the headless host layer.
//
// Same surface as prosper's pass (reference: src/render/ImageBasedLighting.hpp, ImageBasedLighting.cpp):
// `recordGeneration` generates the irradiance cube, the prefiltered radiance cube and the specular BRDF LUT from the
// scene's sky through prosper_pt_generate_ibl, into the context-owned maps that DeferredShading::record reads with
// applyIbl.  `isGenerated` is false again after a scene upload (the maps describe the old sky).
#pragma once

#include "../../../include/prosper_pt/prosper_pt.h"

namespace render
{

class ImageBasedLighting
{
  public:
    ImageBasedLighting() noexcept = default;
    ImageBasedLighting(const ImageBasedLighting &) = delete;
    ImageBasedLighting &operator=(const ImageBasedLighting &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    // Throws std::runtime_error on failure.
    [[nodiscard]] bool isGenerated() const;
    void recordGeneration(void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
};

} // namespace render
