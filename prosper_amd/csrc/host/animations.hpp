// host/animations.hpp — scene::Animations of the headless host layer.
//
// The part of prosper's World a frame loop calls for a moving scene (reference: src/scene/World.hpp updateAnimations /
// updateScene, src/scene/Animations.hpp): `load` hands the scene's node tree and channels to the library once
// (prosper_pt_set_animations), `updateAnimations(timeS)` stages the frame's time (prosper_pt_animate) - the sampling, the
// scene-graph walk and the refit run on the GPU at the head of the next render - and `endTimeS` is Scene::endTimeS.  The
// camera transform World::updateScene returns comes back with `cameraTransform`.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"

namespace scene
{

struct CameraTransform
{
    float eye[3]{0.f, 0.f, 0.f};
    float target[3]{0.f, 0.f, -1.f};
    float up[3]{0.f, 1.f, 0.f};
};

class Animations
{
  public:
    Animations() noexcept = default;
    Animations(const Animations &) = delete;
    Animations &operator=(const Animations &) = delete;

    // `ctx` is borrowed; it outlives the object.
    void init(prosper_pt_ctx *ctx);
    // The uploaded scene's nodes and channels (borrowed for the call).  Throws std::runtime_error on a refusal.
    void load(const prosper_pt_animation_desc &desc);
    // World::updateAnimations + updateScene for the next frame.  `stream` is used only with `now` (PROSPER_PT_UPDATE_NOW).
    // Throws std::runtime_error on failure.
    void updateAnimations(float timeS, bool now = false, void *stream = nullptr);
    [[nodiscard]] float endTimeS() const { return m_endTimeS; }
    [[nodiscard]] uint32_t nodeCount() const { return m_nodeCount; }
    [[nodiscard]] uint32_t animatedNodeCount() const { return m_animatedNodeCount; }
    // false while the scene has no camera node or no update has run; enqueues a staged update and waits for its record
    [[nodiscard]] bool cameraTransform(CameraTransform &out) const;

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    float m_endTimeS{0.f};
    uint32_t m_nodeCount{0};
    uint32_t m_animatedNodeCount{0};
};

} // namespace scene
