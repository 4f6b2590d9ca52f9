// host/mesh_preparer.hpp — scene::MeshPreparer of the headless host layer.
//
// Same role as the body of loadNextMesh in prosper's DeferredLoadingContext.cpp for a primitive whose cache is missing or
// stale (reference: src/scene/DeferredLoadingContext.cpp:836-870): the primitive's accessors in, the cache header's
// fields and the blob out - tangents generated where the primitive has uvs and none of its own, meshlets, packed
// streams.  Below it sit prosper_pt_prepare_mesh and its read-backs: tangents, packing and meshlet bounds run on the GPU
// (DESIGN.md f22).  Writing the cache file stays with the caller, as writeCache is a step of its own in the reference.
#pragma once

#include <cstdint>
#include <vector>

#include "../../../include/prosper_pt/prosper_pt.h"

namespace scene
{

struct MeshPrepareOptions
{
    bool generateTangents{true}; // prosper's condition: acts on a primitive with uvs and no tangents
    bool generateMeshlets{true};
};

class MeshPreparer
{
  public:
    MeshPreparer() noexcept = default;
    MeshPreparer(const MeshPreparer &) = delete;
    MeshPreparer &operator=(const MeshPreparer &) = delete;

    // `ctx` is the context whose staging the preparation uses (borrowed; it outlives the preparer).
    void init(prosper_pt_ctx *ctx);

    // -> the cache header's fields.  Throws std::runtime_error when the library refuses.
    prosper_pt_prepared_mesh prepare(const prosper_pt_mesh_source &source, const MeshPrepareOptions &options = {}, void *stream = nullptr);
    // the blob of the last prepare(), blobByteCount / 4 words
    std::vector<uint32_t> blob() const;
    // the float32 tangents, 4 per vertex, of the last prepare() if it generated any; empty otherwise
    std::vector<float> tangents() const;

  private:
    bool m_initialized{false};
    prosper_pt_ctx *m_ctx{nullptr};
    prosper_pt_prepared_mesh m_last{};
    bool m_prepared{false};
    bool m_generated{false};
};

} // namespace scene
