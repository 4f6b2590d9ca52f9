// host/debug_renderer.hpp — scene::DebugLines and render::DebugRenderer of the headless host layer.
//
// Same role as prosper's scene::DebugLines (reference: src/scene/DebugGeometry.hpp, DebugGeometry.cpp) and
// render::DebugRenderer (src/render/DebugRenderer.cpp; Renderer.cpp:502 runs it between the transparents and bloom):
// a host-side list of world-space lines, drawn depth-tested over the illumination and the depth through
// prosper_pt_debug_lines.  Prosper keeps the lines in a mapped buffer per frame in flight; here the list
// is host memory and the call copies it.
#pragma once

#include <cstdint>
#include <vector>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"
#include "rt_reference.hpp"

namespace scene
{

struct DebugLines
{
    static constexpr uint32_t sMaxLineCount = 100'000;
    // A line is two positions and a color
    static constexpr uint32_t sLineFloats = 9;
    std::vector<float> buffer; // sMaxLineCount lines once the first one was added
    uint32_t count{0};

    void reset() { count = 0; }
    // The reference writes past its mapped buffer's end when it is full; here the line is dropped and false returned.
    bool addLine(const float p0[3], const float p1[3], const float color[3]);
};

} // namespace scene

namespace render
{

class DebugRenderer
{
  public:
    DebugRenderer() noexcept = default;
    DebugRenderer(const DebugRenderer &) = delete;
    DebugRenderer &operator=(const DebugRenderer &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    struct RecordInOut
    {
        uint32_t width{0}; // of the context's HDR image (the illumination) and the last traced G-buffer's depth
        uint32_t height{0};
    };
    // The camera's current uniforms (the caller has run Camera::updateBuffer).  Throws std::runtime_error on failure.
    void record(const scene::Camera &cam, const scene::DebugLines &lines, const RecordInOut &inOutTargets, void *stream);

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
};

} // namespace render
