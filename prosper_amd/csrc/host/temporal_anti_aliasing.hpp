// host/temporal_anti_aliasing.hpp — render::TemporalAntiAliasing of the headless host layer.
//
// Same surface as prosper's pass (reference: src/render/TemporalAntiAliasing.hpp, TemporalAntiAliasing.cpp:160-325):
// `record` resolves the illumination with the velocity, the depth and the preserved previous resolve through
// prosper_pt_taa_resolve and returns the context's HDR image; `releasePreserved` drops the previous resolve.  What
// drawUi edits in prosper are plain setters, with prosper's defaults (TemporalAntiAliasing.hpp: Variance, Closest,
// Catmull-Rom, luminance weighting).
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"

namespace render
{

class TemporalAntiAliasing
{
  public:
    enum class ColorClippingType : uint32_t
    {
        None = 0,
        MinMax = 1,
        Variance = 2,
    };
    enum class VelocitySamplingType : uint32_t
    {
        Center = 0,
        Largest = 1,
        Closest = 2,
    };

    TemporalAntiAliasing() noexcept = default;
    TemporalAntiAliasing(const TemporalAntiAliasing &) = delete;
    TemporalAntiAliasing &operator=(const TemporalAntiAliasing &) = delete;

    // `ctx` is borrowed; it outlives the pass.
    void init(prosper_pt_ctx *ctx);
    void recompileShaders() {} // kernels are compiled ahead of time

    // drawUi
    void setColorClipping(ColorClippingType type) { m_colorClipping = type; }
    void setVelocitySampling(VelocitySamplingType type) { m_velocitySampling = type; }
    void setCatmullRom(bool on) { m_catmullRom = on; }
    void setLuminanceWeighting(bool on) { m_luminanceWeighting = on; }

    struct Input
    {
        const void *illumination{nullptr};   // RGBA32F; nullptr: the context's HDR image, in place
        const void *velocity{nullptr};       // float2
        const float *nonLinearDepth{nullptr}; // nullptr: the last traced G-buffer's
        bool onDevice{true};
        uint32_t width{0};
        uint32_t height{0};
    };
    struct Output
    {
        const float *resolvedIllumination{nullptr}; // device pointer, RGBA32F (the context's HDR image)
        uint32_t width{0};
        uint32_t height{0};
    };
    // what record pushes with the current settings
    [[nodiscard]] prosper_pt_taa_pc pushConstants() const;
    // Throws std::runtime_error on failure.
    [[nodiscard]] Output record(const Input &input, void *stream);
    void releasePreserved();

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    ColorClippingType m_colorClipping{ColorClippingType::Variance};
    VelocitySamplingType m_velocitySampling{VelocitySamplingType::Closest};
    bool m_catmullRom{true};
    bool m_luminanceWeighting{true};
};

} // namespace render
