// pt_pass_support.cpp — the one way in for a pass's depth and illumination inputs and the one way out for its read-backs
// (pt_pass_support.hpp).  The refusals here are the entry points' own: same code, same text, and none of them after a
// HIP call the entry point did not make before.
#include <string>

#include "pt_gbuffer_passes.hpp"
#include "pt_pass_support.hpp"

namespace ppt
{

bool is_device_pointer(const void *p)
{
    hipPointerAttribute_t a = {};
    if (hipPointerGetAttributes(&a, p) != hipSuccess)
    {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

int resolve_depth(
    prosper_pt_ctx *ctx, const char *what, const float *depth, bool onDevice, uint32_t width, uint32_t height, const float **out)
{
    *out = onDevice ? depth : nullptr;
    if (depth) return PROSPER_PT_OK;
    uint32_t gw = 0, gh = 0;
    if (const int rc = gbuffer_last_depth(ctx, out, &gw, &gh)) return rc;
    if (gw != width || gh != height)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the last traced G-buffer has another extent");
    return PROSPER_PT_OK;
}

int stage_depth(DeviceBuffer &staging, size_t offset, const float *host, size_t pixels, hipStream_t s, const float **out)
{
    if (*out) return PROSPER_PT_OK;
    if (const int rc = grow_to(staging, offset + pixels * 4u, s)) return rc;
    float *copy = reinterpret_cast<float *>(staging.as<uint8_t>() + offset);
    PPT_HIP(hipMemcpyAsync(copy, host, pixels * 4u, hipMemcpyHostToDevice, s));
    *out = copy;
    return PROSPER_PT_OK;
}

int check_in_place_hdr(const prosper_pt_ctx *ctx, const char *what, bool inPlace, uint32_t width, uint32_t height)
{
    if (inPlace && !hdr_has_extent(ctx, width, height))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, std::string(what) + ": the HDR image has another extent");
    return PROSPER_PT_OK;
}

int resolve_illumination(
    prosper_pt_ctx *ctx, const void *illumination, bool inPlace, bool onDevice, DeviceBuffer &staging, uint32_t width, uint32_t height,
    hipStream_t s, const float4 **out)
{
    if (!inPlace)
    {
        *out = static_cast<const float4 *>(illumination);
        if (!onDevice)
        {
            const size_t bytes = (size_t)width * height * 16u;
            if (const int rc = grow_to(staging, bytes, s)) return rc;
            PPT_HIP(hipMemcpyAsync(staging.ptr, illumination, bytes, hipMemcpyHostToDevice, s));
            *out = staging.as<float4>();
        }
        return prepare_hdr(ctx, width, height, nullptr, s);
    }
    *out = ctx->hdr;
    return PROSPER_PT_OK;
}

int read_back(const prosper_pt_ctx *ctx, hipStream_t s, std::initializer_list<ReadCopy> copies, const Fence *after)
{
    PPT_HIP(hipSetDevice(ctx->device));
    if (after)
        if (const int rc = after->wait(s)) return rc;
    for (const ReadCopy &c : copies)
        if (c.dst && c.bytes) PPT_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

} // namespace ppt
