// host/meshlet_culler.hpp — render::MeshletCuller and render::DrawStats of the headless host layer.
//
// Same role as prosper's pass (reference: src/render/MeshletCuller.hpp, MeshletCuller.cpp, DrawStats.hpp): recordFirstPhase
// generates the draw list of a Mode and culls it against the camera and, where a hierarchical depth is given, against that
// pyramid, which also yields the second phase's input; recordSecondPhase culls that input against another pyramid.  Both go
// through prosper_pt_cull_meshlets_first_phase / _second_phase.  Device pointers stand in for the
// reference's buffer handles, a slot of the context (render::HierarchicalDepthDownsampler::Output::slot) for its
// hierarchical depth image.  The context holds one set of lists: an output is valid until the next culling call.
#pragma once

#include <cstdint>

#include "../../../include/prosper_pt/prosper_pt.h"
#include "camera.hpp"

namespace render
{

// DrawStats.hpp
struct DrawStats
{
    uint32_t drawnMeshletCount{0};
    uint32_t rasterizedTriangleCount{0};
    uint32_t totalTriangleCount{0};
    uint32_t totalMeshletCount{0};
    uint32_t totalMeshCount{0};
    uint32_t totalModelCount{0};
};

struct MeshletCullerFirstPhaseOutput
{
    const uint32_t *dataBuffer{nullptr};       // uint count; { drawInstanceIndex, meshletIndex }[]
    const uint32_t *argumentBuffer{nullptr};   // groupsX, groupsY, groupsZ
    const uint32_t *secondPhaseInput{nullptr}; // nullptr: no hierarchical depth was given
    uint32_t capacity{0};                      // pairs each list has room for
};

struct MeshletCullerSecondPhaseOutput
{
    const uint32_t *dataBuffer{nullptr};
    const uint32_t *argumentBuffer{nullptr};
    uint32_t capacity{0};
};

class MeshletCuller
{
  public:
    static constexpr uint32_t sNoHierarchicalDepth = PROSPER_PT_NO_HIZ;

    MeshletCuller() noexcept = default;
    MeshletCuller(const MeshletCuller &) = delete;
    MeshletCuller &operator=(const MeshletCuller &) = delete;

    // `ctx` is the context the scene was uploaded to (borrowed; it outlives the pass).
    void init(prosper_pt_ctx *ctx);

    enum class Mode : uint8_t
    {
        Opaque,
        Transparent,
    };
    // Creates and culls meshlet draw lists from full scene data.  Also creates input for the second phase if
    // `inHierarchicalDepth` (a pyramid slot) is given.  The camera's current uniforms (the caller has run
    // Camera::updateBuffer).  `drawStats` receives the host's totals; its two device counts are zero until readDrawStats.
    // Throws std::runtime_error on failure.
    [[nodiscard]] MeshletCullerFirstPhaseOutput recordFirstPhase(
        Mode mode, const scene::Camera &cam, uint32_t inHierarchicalDepth, DrawStats &drawStats, void *stream) const;
    // Culls the first phase's second-phase input.  Intended to use with depth drawn with the first pass outputs.
    [[nodiscard]] MeshletCullerSecondPhaseOutput recordSecondPhase(const scene::Camera &cam, uint32_t inHierarchicalDepth, void *stream) const;
    // The statistics of the phases recorded so far, the device counts included; `wait` false: false while those have not
    // landed (never blocks).  Prosper reads its counts back a frame later the same way.
    bool readDrawStats(DrawStats &drawStats, bool wait) const;
    // the same without exceptions: the library's return code (prosper_pt_last_error has the text)
    [[nodiscard]] int tryRecordFirstPhase(
        Mode mode, const prosper_CameraUniforms &cam, uint32_t inHierarchicalDepth, MeshletCullerFirstPhaseOutput &out, void *stream) const noexcept;
    [[nodiscard]] int tryRecordSecondPhase(
        const prosper_CameraUniforms &cam, uint32_t inHierarchicalDepth, MeshletCullerSecondPhaseOutput &out, void *stream) const noexcept;

    [[nodiscard]] prosper_pt_ctx *context() const { return m_ctx; }

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
};

} // namespace render
