// host/rt_direct_illumination.hpp — render::rtdi::RtDirectIllumination of the headless host layer.
//
// Same surface as prosper's pass (reference: src/render/rtdi/RtDirectIllumination.hpp:19-58): `record` runs the
// initial reservoirs, the optional spatial reuse and the trace (RtDirectIllumination.cpp:70-115) through one
// prosper_pt_restir_di_record where the original records three passes; the "Spatial reuse" checkbox of drawUi
// (:62-67) becomes a plain argument.  The Trace sub-pass's accumulation state (src/render/rtdi/Trace.cpp:146-345)
// lives here: its frame index, the history restart on an extent change, and its accumulate switch, which prosper
// leaves off.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "rt_reference.hpp"

namespace render::rtdi
{

// GBufferRendererOutput (src/render/GBufferRenderer.hpp): the three images the passes read
struct GBuffer
{
    const void *albedoRoughness{nullptr}; // width*height float4
    const void *normalMetallic{nullptr};  // width*height float4 (octNormal.xy, metallic, octNormal.z)
    const float *nonLinearDepth{nullptr}; // width*height
    bool onDevice{true};                  // false: host memory, copied by record()
    uint32_t width{0};
    uint32_t height{0};
};

class RtDirectIllumination
{
  public:
    RtDirectIllumination() noexcept = default;
    RtDirectIllumination(const RtDirectIllumination &) = delete;
    RtDirectIllumination &operator=(const RtDirectIllumination &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);
    // The kernels are compiled ahead of time; like a successful recompile of the resampling shaders in the original
    // this only restarts accumulation (RtDirectIllumination.cpp:34-58).
    void recompileShaders();
    void drawUi(bool spatialReuse);
    [[nodiscard]] bool spatialReuse() const { return m_doSpatialReuse; }

    struct Output
    {
        const float *illumination{nullptr}; // device pointer, RGBA32F, width*height texels
        uint32_t width{0};
        uint32_t height{0};
    };
    // Throws std::runtime_error on failure.  `nextFrame` selects per-frame descriptor sets in the original; the
    // passes themselves count frames (Trace.cpp:151), as here.
    [[nodiscard]] Output record(
        const GBuffer &gbuffer, const scene::Camera &cam, bool resetAccumulation, scene::DrawType drawType,
        uint32_t nextFrame, void *stream);
    void releasePreserved();

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }
    [[nodiscard]] const prosper_pt_restir_trace_pc &lastPushConstants() const { return m_lastPC; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};

    bool m_doSpatialReuse{true};
    bool m_resetAccumulation{true};

    // Trace (src/render/rtdi/Trace.hpp:92-94)
    bool m_accumulationDirty{true};
    bool m_accumulate{false};
    uint32_t m_frameIndex{0};
    bool m_havePrevious{false};
    uint32_t m_previousWidth{0}, m_previousHeight{0};
    prosper_pt_restir_trace_pc m_lastPC{};
};

} // namespace render::rtdi
