// host/bloom.hpp — render::bloom::Bloom of the headless host layer.
//
// Same surface as prosper's pass (reference: src/render/bloom/Bloom.hpp, Bloom.cpp:15-141): `record` switches on the
// technique as Bloom.cpp:83-124 does - separate, reduce, blur and compose through prosper_pt_bloom, or separate, the
// kernel's DFT, the convolution and compose through prosper_pt_bloom_fft - and returns the context's HDR image.  What
// drawUi edits in prosper (Bloom.cpp:60-62, Separate.cpp:81, GenerateKernel.cpp:65, Compose.cpp:85-87) are plain
// setters, with prosper's defaults (Separate.hpp:46, Compose.hpp:48-49, Bloom.hpp:57-58).
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

enum class Technique : uint32_t
{
    MultiResolutionBlur = 0,
    Fft = 1,
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
    void setTechnique(Technique technique) { m_technique = technique; }
    // GenerateKernel's "Re-generate kernel" checkbox: while set, every Fft record remakes the kernel's DFT
    void setRegenerateKernel(bool on) { m_regenerateKernel = on; }
    // drops the kernel's DFT the context keeps; the next Fft record remakes it
    void releasePreserved();

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
    [[nodiscard]] prosper_pt_bloom_fft_pc fftPushConstants() const; // with Technique::Fft
    // Throws std::runtime_error on failure.
    [[nodiscard]] Output record(const Input &input, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    ResolutionScale m_resolutionScale{ResolutionScale::Half};
    Technique m_technique{Technique::MultiResolutionBlur};
    bool m_regenerateKernel{false};
    float m_threshold{1.f};
    bool m_biquadraticSampling{true};
    float m_blendFactors[3]{.9f, .04f, .04f};
};

} // namespace render::bloom
