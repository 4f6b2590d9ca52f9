// host/meshlet_culler.cpp — see meshlet_culler.hpp.
#include "meshlet_culler.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"
#include "rt_reference.hpp"

namespace render
{

namespace
{

DrawStats from_c(const prosper_pt_draw_stats &s)
{
    DrawStats d;
    d.drawnMeshletCount = s.drawnMeshletCount;
    d.rasterizedTriangleCount = s.rasterizedTriangleCount;
    d.totalTriangleCount = s.totalTriangleCount;
    d.totalMeshletCount = s.totalMeshletCount;
    d.totalMeshCount = s.totalMeshCount;
    d.totalModelCount = s.totalModelCount;
    return d;
}

} // namespace

void MeshletCuller::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

int MeshletCuller::tryRecordFirstPhase(
    Mode mode, const prosper_CameraUniforms &cam, uint32_t inHierarchicalDepth, MeshletCullerFirstPhaseOutput &out, void *stream) const noexcept
{
    PROSPER_ASSERT(m_initialized);
    out = MeshletCullerFirstPhaseOutput{};
    const uint32_t m = mode == Mode::Transparent ? PROSPER_PT_CULL_MODE_TRANSPARENT : PROSPER_PT_CULL_MODE_OPAQUE;
    int rc = prosper_pt_cull_meshlets_first_phase(m_ctx, m, &cam, inHierarchicalDepth, stream);
    if (rc != PROSPER_PT_OK) return rc;
    rc = prosper_pt_get_draw_list_device_ptr(m_ctx, PROSPER_PT_DRAW_LIST_FIRST_PHASE, &out.dataBuffer, &out.argumentBuffer, &out.capacity);
    if (rc != PROSPER_PT_OK) return rc;
    if (inHierarchicalDepth != sNoHierarchicalDepth)
        rc = prosper_pt_get_draw_list_device_ptr(m_ctx, PROSPER_PT_DRAW_LIST_SECOND_PHASE_INPUT, &out.secondPhaseInput, nullptr, nullptr);
    return rc;
}

int MeshletCuller::tryRecordSecondPhase(
    const prosper_CameraUniforms &cam, uint32_t inHierarchicalDepth, MeshletCullerSecondPhaseOutput &out, void *stream) const noexcept
{
    PROSPER_ASSERT(m_initialized);
    out = MeshletCullerSecondPhaseOutput{};
    const int rc = prosper_pt_cull_meshlets_second_phase(m_ctx, &cam, inHierarchicalDepth, stream);
    if (rc != PROSPER_PT_OK) return rc;
    return prosper_pt_get_draw_list_device_ptr(m_ctx, PROSPER_PT_DRAW_LIST_SECOND_PHASE, &out.dataBuffer, &out.argumentBuffer, &out.capacity);
}

MeshletCullerFirstPhaseOutput MeshletCuller::recordFirstPhase(
    Mode mode, const scene::Camera &cam, uint32_t inHierarchicalDepth, DrawStats &drawStats, void *stream) const
{
    MeshletCullerFirstPhaseOutput out;
    if (tryRecordFirstPhase(mode, cam.uniforms(), inHierarchicalDepth, out, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("MeshletCuller::recordFirstPhase: ") + prosper_pt_last_error());
    // recordGenerateList adds its totals to the caller's statistics as it records
    (void)readDrawStats(drawStats, false);
    return out;
}

MeshletCullerSecondPhaseOutput MeshletCuller::recordSecondPhase(const scene::Camera &cam, uint32_t inHierarchicalDepth, void *stream) const
{
    MeshletCullerSecondPhaseOutput out;
    if (tryRecordSecondPhase(cam.uniforms(), inHierarchicalDepth, out, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("MeshletCuller::recordSecondPhase: ") + prosper_pt_last_error());
    return out;
}

bool MeshletCuller::readDrawStats(DrawStats &drawStats, bool wait) const
{
    PROSPER_ASSERT(m_initialized);
    prosper_pt_draw_stats s = {};
    const int rc = prosper_pt_get_draw_stats(m_ctx, &s, wait ? 1u : 0u);
    if (rc == PROSPER_PT_OK)
    {
        drawStats = from_c(s);
        return true;
    }
    if (rc != PROSPER_PT_NOT_READY) throw std::runtime_error(std::string("MeshletCuller::readDrawStats: ") + prosper_pt_last_error());
    // the host's totals are known as soon as the phase is recorded: they come with the device counts still zero
    drawStats = from_c(s);
    return false;
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_meshlet_culler
{
    render::MeshletCuller pass;
};

extern "C" {

int prosper_host_meshlet_culler_create(prosper_pt_ctx *ctx, prosper_host_meshlet_culler **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_meshlet_culler_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_meshlet_culler *r = new (std::nothrow) prosper_host_meshlet_culler();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_meshlet_culler_destroy(prosper_host_meshlet_culler *r) { delete r; }

int prosper_host_meshlet_culler_record_first_phase(
    prosper_host_meshlet_culler *r, uint32_t mode, prosper_host_camera *camera, uint32_t width, uint32_t height,
    uint32_t inHierarchicalDepth, prosper_host_meshlet_culler_output *out, void *stream)
{
    if (!r || !camera || !out || mode > 1u)
    {
        prosper_host_set_error("prosper_host_meshlet_culler_record_first_phase: null argument or unknown mode");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    scene::Camera &cam = *prosper_host_camera_object(camera);
    cam.updateResolution(width, height);
    cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
    render::MeshletCullerFirstPhaseOutput o;
    const auto m = mode == 1u ? render::MeshletCuller::Mode::Transparent : render::MeshletCuller::Mode::Opaque;
    const int rc = r->pass.tryRecordFirstPhase(m, cam.uniforms(), inHierarchicalDepth, o, stream);
    if (rc != PROSPER_PT_OK)
    {
        prosper_host_set_error((std::string("MeshletCuller::recordFirstPhase: ") + prosper_pt_last_error()).c_str());
        return rc;
    }
    *out = prosper_host_meshlet_culler_output{o.dataBuffer, o.argumentBuffer, o.secondPhaseInput, o.capacity, 0u};
    return PROSPER_PT_OK;
}

int prosper_host_meshlet_culler_record_second_phase(
    prosper_host_meshlet_culler *r, prosper_host_camera *camera, uint32_t width, uint32_t height, uint32_t inHierarchicalDepth,
    prosper_host_meshlet_culler_output *out, void *stream)
{
    if (!r || !camera || !out)
    {
        prosper_host_set_error("prosper_host_meshlet_culler_record_second_phase: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    scene::Camera &cam = *prosper_host_camera_object(camera);
    cam.updateResolution(width, height);
    cam.updateBuffer();
    render::MeshletCullerSecondPhaseOutput o;
    const int rc = r->pass.tryRecordSecondPhase(cam.uniforms(), inHierarchicalDepth, o, stream);
    if (rc != PROSPER_PT_OK)
    {
        prosper_host_set_error((std::string("MeshletCuller::recordSecondPhase: ") + prosper_pt_last_error()).c_str());
        return rc;
    }
    *out = prosper_host_meshlet_culler_output{o.dataBuffer, o.argumentBuffer, nullptr, o.capacity, 0u};
    return PROSPER_PT_OK;
}

int prosper_host_meshlet_culler_read_draw_stats(prosper_host_meshlet_culler *r, prosper_pt_draw_stats *out, uint32_t wait)
{
    if (!r || !out)
    {
        prosper_host_set_error("prosper_host_meshlet_culler_read_draw_stats: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        render::DrawStats d;
        const bool landed = r->pass.readDrawStats(d, wait != 0u);
        *out = prosper_pt_draw_stats{d.drawnMeshletCount, d.rasterizedTriangleCount, d.totalTriangleCount,
                                     d.totalMeshletCount, d.totalMeshCount,          d.totalModelCount};
        return landed ? PROSPER_PT_OK : PROSPER_PT_NOT_READY;
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_NO_SCENE;
    }
}

} // extern "C"
