// host/hierarchical_depth_downsampler.hpp — render::HierarchicalDepthDownsampler of the headless host layer.
//
// Same role as prosper's pass (reference: src/render/HierarchicalDepthDownsampler.hpp, .cpp): `record` makes the depth
// pyramid of a non-linear depth through prosper_pt_hiz_downsample and hands back what stands in for the image handle: the
// device pointers of its levels.  The reference keeps two storage sets, the G-buffer's pyramid before and after the second
// culling phase, picked by `nextFrame`; here that index picks one of the context's two slots.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"

namespace render
{

class HierarchicalDepthDownsampler
{
  public:
    static constexpr uint32_t sMaxMips = 12;

    HierarchicalDepthDownsampler() noexcept = default;
    HierarchicalDepthDownsampler(const HierarchicalDepthDownsampler &) = delete;
    HierarchicalDepthDownsampler &operator=(const HierarchicalDepthDownsampler &) = delete;

    // `ctx` is borrowed; it outlives the pass.
    void init(prosper_pt_ctx *ctx);

    struct Input
    {
        const float *nonLinearDepth{nullptr}; // nullptr: the last traced G-buffer's
        bool onDevice{true};
        uint32_t width{0};
        uint32_t height{0};
    };
    // the pyramid in place of the reference's ImageHandle: R32F levels on the device, finest first
    struct Output
    {
        uint32_t slot{0};
        uint32_t mipCount{0};
        const float *mips[sMaxMips]{};
        uint32_t mipWidth[sMaxMips]{}, mipHeight[sMaxMips]{};
    };
    // Throws std::runtime_error on failure.
    [[nodiscard]] Output record(const Input &inNonLinearDepth, uint32_t nextFrame, void *stream) const;
    // The same without exceptions: the library's return code (prosper_pt_last_error has the text), `out` filled on success.
    [[nodiscard]] int tryRecord(const Input &inNonLinearDepth, uint32_t nextFrame, void *stream, Output &out) const noexcept;

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
};

} // namespace render
