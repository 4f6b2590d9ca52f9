// host/mesh_preparer.cpp — see mesh_preparer.hpp.
#include "mesh_preparer.hpp"

#include <stdexcept>
#include <string>

#include "host_common.hpp"

namespace scene
{

void MeshPreparer::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

prosper_pt_prepared_mesh MeshPreparer::prepare(const prosper_pt_mesh_source &source, const MeshPrepareOptions &options, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    const uint32_t flags = (options.generateTangents ? (uint32_t)PROSPER_PT_PREPARE_GENERATE_TANGENTS : 0u) |
                           (options.generateMeshlets ? (uint32_t)PROSPER_PT_PREPARE_MESHLETS : 0u);
    prosper_pt_prepared_mesh out = {};
    if (prosper_pt_prepare_mesh(m_ctx, &source, flags, &out, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("MeshPreparer::prepare: ") + prosper_pt_last_error());
    m_last = out;
    m_prepared = true;
    m_generated = options.generateTangents && !source.tangents && source.texCoord0s;
    return out;
}

std::vector<uint32_t> MeshPreparer::blob() const
{
    PROSPER_ASSERT(m_prepared);
    std::vector<uint32_t> out(m_last.blobByteCount / 4u);
    if (prosper_pt_read_prepared_mesh(m_ctx, out.data(), m_last.blobByteCount) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("MeshPreparer::blob: ") + prosper_pt_last_error());
    return out;
}

std::vector<float> MeshPreparer::tangents() const
{
    PROSPER_ASSERT(m_prepared);
    std::vector<float> out;
    if (!m_generated) return out;
    out.resize((size_t)m_last.vertexCount * 4u);
    if (prosper_pt_read_prepared_tangents(m_ctx, out.data(), (uint64_t)out.size() * 4u) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("MeshPreparer::tangents: ") + prosper_pt_last_error());
    return out;
}

} // namespace scene
