// host/bloom.hpp — render::bloom::Bloom of the headless host layer.
//
// Same surface as prosper's pass (reference: src/render/bloom/Bloom.hpp, Bloom.cpp:15-141): `record` runs separate,
// reduce, blur and compose over the illumination through prosper_pt_bloom and returns the context's HDR image.  Only
// the multi-resolution blur exists here.  What drawUi edits in prosper (Separate.cpp:81, Compose.cpp:85-87,
// Bloom.cpp:61-62) are plain setters, with prosper's defaults (Separate.hpp:46, Compose.hpp:48-49, Bloom.hpp:57).
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"

namespace render::bloom
{

enum class ResolutionScale : uint32_t
{
    Half = 0,
    Quarter = 1,
};

class Bloom
{
  public:
    Bloom() noexcept = default;
    Bloom(const Bloom &) = delete;
    Bloom &operator=(const Bloom &) = delete;

    // `ctx` is borrowed; it outlives the pass.
    void init(prosper_pt_ctx *ctx);
    void recompileShaders() {} // kernels are compiled ahead of time
    void startFrame() {}       // (prosper's resets the blur pass's descriptor allocations)

    // drawUi
    void setThreshold(float threshold) { m_threshold = threshold; }
    void setBlendFactors(float mip0, float mip1, float mip2);
    void setBiquadraticSampling(bool on) { m_biquadraticSampling = on; }
    void setResolutionScale(ResolutionScale scale) { m_resolutionScale = scale; }

    struct Input
    {
        const void *illumination{nullptr}; // RGBA32F; nullptr: the context's HDR image, in place
        bool onDevice{true};
        uint32_t width{0};
        uint32_t height{0};
    };
    struct Output
    {
        const float *illuminationWithBloom{nullptr}; // device pointer, RGBA32F (the context's HDR image)
        uint32_t width{0};
        uint32_t height{0};
    };
    // what record pushes with the current settings
    [[nodiscard]] prosper_pt_bloom_pc pushConstants() const;
    // Throws std::runtime_error on failure.
    [[nodiscard]] Output record(const Input &input, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    ResolutionScale m_resolutionScale{ResolutionScale::Half};
    float m_threshold{1.f};
    bool m_biquadraticSampling{true};
    float m_blendFactors[3]{.9f, .04f, .04f};
};

} // namespace render::bloom
