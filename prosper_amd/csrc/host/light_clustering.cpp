// host/light_clustering.cpp — see light_clustering.hpp.
#include "light_clustering.hpp"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "rt_reference.hpp"
#include "host_common.hpp"

namespace render
{

void LightClustering::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

LightClusteringOutput LightClustering::record(const scene::Camera &cam, uint32_t width, uint32_t height, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    if (prosper_pt_cluster_lights(m_ctx, &cam.uniforms(), width, height, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("LightClustering::record: ") + prosper_pt_last_error());
    LightClusteringOutput ret;
    ret.width = width;
    ret.height = height;
    if (prosper_pt_get_light_cluster_dims(m_ctx, &ret.dims[0], &ret.dims[1], &ret.dims[2]) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("LightClustering::record: ") + prosper_pt_last_error());
    return ret;
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_light_clustering
{
    render::LightClustering pass;
};

extern "C" {

int prosper_host_light_clustering_create(prosper_pt_ctx *ctx, prosper_host_light_clustering **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_light_clustering_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_light_clustering *r = new (std::nothrow) prosper_host_light_clustering();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_light_clustering_destroy(prosper_host_light_clustering *r) { delete r; }

int prosper_host_light_clustering_record(
    prosper_host_light_clustering *r, prosper_host_camera *camera, uint32_t width, uint32_t height, void *stream)
{
    if (!r || !camera)
    {
        prosper_host_set_error("prosper_host_light_clustering_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer();
        (void)r->pass.record(cam, width, height, stream);
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

} // extern "C"
