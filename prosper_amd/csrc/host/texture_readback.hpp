// host/texture_readback.hpp — render::TextureReadback of the headless host layer.
//
// Same role as prosper's TextureReadback (reference: src/render/TextureReadback.{hpp,cpp}; Renderer.cpp:510-514 records
// it on the depth, App.cpp:583-631 turns the texel into the focus distance): one texel of one image, queued in a frame and
// handed out MAX_FRAMES_IN_FLIGHT frames later.  The frame counting is the reference's m_framesUntilReady; below it sits
// the library's non-blocking prosper_pt_try_texture_readback, so a value whose copy has not finished after those frames
// is simply not there yet.
#pragma once

#include <array>
#include <cstdint>
#include <optional>

#include "../../../include/prosper_pt/prosper_pt.h"

namespace render
{

constexpr int32_t MAX_FRAMES_IN_FLIGHT = 2;

class TextureReadback
{
  public:
    TextureReadback() noexcept = default;
    TextureReadback(const TextureReadback &) = delete;
    TextureReadback &operator=(const TextureReadback &) = delete;

    // `ctx` is the context that owns the images (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    // Throws std::logic_error where the reference asserts: a frame started with a finished readback nobody asked for.
    void startFrame();
    // Queues the texel of registry entry `resource` under (pxX, pxY).  Throws std::logic_error when one is queued and
    // unread, std::runtime_error when the library refuses.
    void record(uint32_t resource, float pxX, float pxY, void *stream);
    // Empty until MAX_FRAMES_IN_FLIGHT frames have started since record (and the copy has finished); then the value, once.
    // Throws std::logic_error without a readback in flight.
    std::optional<std::array<float, 4>> readback();

    [[nodiscard]] int32_t framesUntilReady() const { return m_framesUntilReady; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    int32_t m_framesUntilReady{-1};
    bool m_polled{false}; // readback() was called since the counter reached 0
};

} // namespace render
