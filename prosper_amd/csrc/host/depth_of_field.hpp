// host/depth_of_field.hpp — render::dof::DepthOfField of the headless host layer.
//
// Same surface as prosper's pass (reference: src/render/dof/DepthOfField.hpp, DepthOfField.cpp:46-110): `record` runs
// the seven passes over the illumination and the depth through prosper_pt_depth_of_field and returns the context's HDR
// image.  The push constants are computed from the camera's parameters as the passes compute them
// (dof/Setup.cpp:163-177, dof/Dilate.cpp:105-127): only aperture, focus distance and focal length drive them.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"
#include "rt_reference.hpp"

namespace render::dof
{

class DepthOfField
{
  public:
    static constexpr float sMaxFgCoCFactor = 2.f;

    DepthOfField() noexcept = default;
    DepthOfField(const DepthOfField &) = delete;
    DepthOfField &operator=(const DepthOfField &) = delete;

    // `ctx` is borrowed; it outlives the pass.
    void init(prosper_pt_ctx *ctx);

    struct Input
    {
        const void *illumination{nullptr}; // RGBA32F; nullptr: the context's HDR image, in place
        const float *depth{nullptr};       // non-linear depth; nullptr: the last traced G-buffer's
        bool onDevice{true};
        uint32_t width{0};
        uint32_t height{0};
    };
    struct Output
    {
        const float *combinedIlluminationDoF{nullptr}; // device pointer, RGBA32F (the context's HDR image)
        uint32_t width{0};
        uint32_t height{0};
    };
    // SetupPC and DilatePC for a width x height illumination, from the camera's parameters
    [[nodiscard]] static prosper_pt_dof_pc pushConstants(const scene::Camera &cam, uint32_t width, uint32_t height);
    // The camera's current uniforms (the caller has run Camera::updateBuffer).  Throws std::runtime_error on failure.
    [[nodiscard]] Output record(const scene::Camera &cam, const Input &input, void *stream);

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }
    [[nodiscard]] const prosper_pt_dof_pc &lastPushConstants() const { return m_lastPC; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    prosper_pt_dof_pc m_lastPC{};
};

} // namespace render::dof
