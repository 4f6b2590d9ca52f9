// host/light_clustering.hpp — render::LightClustering of the headless host layer.
//
// Same surface as prosper's pass (reference: src/render/LightClustering.hpp:22-64, LightClustering.cpp:155-251):
// `record` builds the per-cluster point / spot light lists of the camera's view through prosper_pt_cluster_lights into
// context-owned device buffers.  The pass has no UI and its kernel is compiled ahead of time (no recompileShaders).
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"

namespace render
{

// LightClusteringOutput: the pointer grid's extent; the buffers themselves belong to the context
// (prosper_pt_read_light_clusters reads them)
struct LightClusteringOutput
{
    uint32_t width{0}; // the render extent the grid was sized from
    uint32_t height{0};
    uint32_t dims[3]{}; // ceil(width / 32), ceil(height / 32), zSlices + 1
};

class LightClustering
{
  public:
    static const uint32_t clusterDim = 32;
    static const uint32_t zSlices = 16;

    LightClustering() noexcept = default;
    LightClustering(const LightClustering &) = delete;
    LightClustering &operator=(const LightClustering &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    // Clusters the context's lights for the camera's current uniforms (the caller has run Camera::updateBuffer) over a
    // `width` x `height` render extent.  Throws std::runtime_error on failure.
    [[nodiscard]] LightClusteringOutput record(const scene::Camera &cam, uint32_t width, uint32_t height, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
};

} // namespace render
