// host/debug_renderer.cpp — see debug_renderer.hpp.
#include "debug_renderer.hpp"

#include <new>
#include <stdexcept>
#include <string>

#include "../../../include/prosper_pt/prosper_host.h"
#include "host_common.hpp"

namespace scene
{

bool DebugLines::addLine(const float p0[3], const float p1[3], const float color[3])
{
    if (count >= sMaxLineCount) return false;
    if (buffer.empty()) buffer.resize((size_t)sMaxLineCount * sLineFloats);
    float *lineData = buffer.data() + (size_t)count * sLineFloats;
    for (int i = 0; i < 3; ++i)
    {
        lineData[i] = p0[i];
        lineData[3 + i] = p1[i];
        lineData[6 + i] = color[i];
    }
    count++;
    return true;
}

} // namespace scene

namespace render
{

void DebugRenderer::init(prosper_pt_ctx *ctx)
{
    PROSPER_ASSERT(!m_initialized);
    PROSPER_ASSERT(ctx != nullptr);
    m_ctx = ctx;
    m_initialized = true;
}

void DebugRenderer::record(const scene::Camera &cam, const scene::DebugLines &lines, const RecordInOut &t, void *stream)
{
    PROSPER_ASSERT(m_initialized);
    const float *data = lines.count ? lines.buffer.data() : nullptr;
    if (prosper_pt_debug_lines(m_ctx, data, lines.count, &cam.uniforms(), t.width, t.height, stream) != PROSPER_PT_OK)
        throw std::runtime_error(std::string("DebugRenderer::record: ") + prosper_pt_last_error());
}

} // namespace render

// ---- plain-C shims (include/prosper_pt/prosper_host.h) ----

struct prosper_host_debug_lines
{
    scene::DebugLines lines;
};

struct prosper_host_debug_renderer
{
    render::DebugRenderer pass;
};

extern "C" {

int prosper_host_debug_lines_create(prosper_host_debug_lines **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = new (std::nothrow) prosper_host_debug_lines();
    return *out ? PROSPER_PT_OK : PROSPER_PT_ERR_INVALID_ARGUMENT;
}

void prosper_host_debug_lines_destroy(prosper_host_debug_lines *l) { delete l; }

void prosper_host_debug_lines_reset(prosper_host_debug_lines *l)
{
    if (l) l->lines.reset();
}

int prosper_host_debug_lines_add_line(prosper_host_debug_lines *l, const float *p0, const float *p1, const float *color)
{
    if (!l || !p0 || !p1 || !color)
    {
        prosper_host_set_error("prosper_host_debug_lines_add_line: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    if (!l->lines.addLine(p0, p1, color))
    {
        prosper_host_set_error("prosper_host_debug_lines_add_line: the list holds sMaxLineCount lines");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    return PROSPER_PT_OK;
}

uint32_t prosper_host_debug_lines_count(const prosper_host_debug_lines *l) { return l ? l->lines.count : 0u; }

const float *prosper_host_debug_lines_data(const prosper_host_debug_lines *l)
{
    return l && l->lines.count ? l->lines.buffer.data() : nullptr;
}

int prosper_host_debug_renderer_create(prosper_pt_ctx *ctx, prosper_host_debug_renderer **out)
{
    if (!out) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!ctx)
    {
        prosper_host_set_error("prosper_host_debug_renderer_create: null context");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    prosper_host_debug_renderer *r = new (std::nothrow) prosper_host_debug_renderer();
    if (!r) return PROSPER_PT_ERR_INVALID_ARGUMENT;
    r->pass.init(ctx);
    *out = r;
    return PROSPER_PT_OK;
}

void prosper_host_debug_renderer_destroy(prosper_host_debug_renderer *r) { delete r; }

int prosper_host_debug_renderer_record(
    prosper_host_debug_renderer *r, prosper_host_camera *camera, const prosper_host_debug_lines *lines, uint32_t width,
    uint32_t height, void *stream)
{
    if (!r || !camera || !lines)
    {
        prosper_host_set_error("prosper_host_debug_renderer_record: null argument");
        return PROSPER_PT_ERR_INVALID_ARGUMENT;
    }
    try
    {
        scene::Camera &cam = *prosper_host_camera_object(camera);
        cam.updateResolution(width, height);
        cam.updateBuffer(); // App::drawFrame does this before Renderer::render (App.cpp:556)
        render::DebugRenderer::RecordInOut t;
        t.width = width;
        t.height = height;
        r->pass.record(cam, lines->lines, t, stream);
    }
    catch (const std::exception &e)
    {
        prosper_host_set_error(e.what());
        return PROSPER_PT_ERR_HIP;
    }
    return PROSPER_PT_OK;
}

} // extern "C"
