// host/texture_debug.hpp — render::TextureDebug of the headless host layer.
//
// Same role as prosper's TextureDebug (reference: src/render/TextureDebug.{hpp,cpp}, res/shader/texture_debug.comp;
// Renderer.cpp:621 lets its output replace the final composite): views one of the context's registry images through
// per-name settings - range, LOD, channel, abs, sampler - plus the zoom toggle and the cursor's magnifier, through
// prosper_pt_texture_debug.  Prosper picks the target in an ImGui combo over its resource pool's debug
// names; here setTarget names a registry entry and textureSelected() says whether one is named.
#pragma once

#include <array>
#include <cstdint>
#include <optional>
#include <string>
#include <unordered_map>

#include "../../../include/prosper_pt/prosper_pt.h"

namespace render
{

class TextureDebug
{
  public:
    enum class ChannelType : uint8_t
    {
        R,
        G,
        B,
        A,
        RGB,
    };
    struct TargetSettings
    {
        float range[2]{0.f, 1.f};
        int32_t lod{0};
        ChannelType channelType{ChannelType::RGB};
        bool absBeforeRange{false};
        bool useBilinearSampler{false};
    };

    TextureDebug() noexcept = default;
    TextureDebug(const TextureDebug &) = delete;
    TextureDebug &operator=(const TextureDebug &) = delete;

    // `ctx` is the context that owns the images (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    // the combo: an empty name deselects
    void setTarget(const std::string &name) { m_target = name; }
    [[nodiscard]] bool textureSelected() const { return !m_target.empty(); }
    [[nodiscard]] const std::string &target() const { return m_target; }
    // the settings of a name, made with the defaults at first use and kept per name, as the reference's hash map
    TargetSettings &settings(const std::string &name) { return m_targetSettings[name]; }
    void setZoom(bool zoom) { m_zoom = zoom; }

    // The selected entry as outWidth x outHeight RGBA8 into device and / or host memory; `cursorUv` (the cursor inside the
    // output, if it is) turns the magnifier's peek and marker on.  The LOD is clamped to the entry's last level, as the
    // reference's slider is.  Throws std::logic_error without a selection, std::runtime_error when the name is not in
    // the registry or the library refuses (an entry that is not valid: prosper clears to black there).
    void record(
        uint32_t outWidth, uint32_t outHeight, std::optional<std::array<float, 2>> cursorUv, void *deviceRgba8,
        uint8_t *hostRgba8, size_t byteSize, void *stream);
    // the peeked value of the last record that had a cursor (waits for it)
    [[nodiscard]] std::array<float, 4> peekedValue() const;
    [[nodiscard]] const prosper_pt_texture_debug_pc &lastPushConstants() const { return m_lastPC; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    std::string m_target;
    std::unordered_map<std::string, TargetSettings> m_targetSettings;
    bool m_zoom{false};
    prosper_pt_texture_debug_pc m_lastPC{};
};

} // namespace render
