// pt_raster_surface.hpp — the surface of a pixel of the rasteriser's visibility image: the pixel's own ray
// as gbuffer_trace_kernel<true, true, kLod> forms it, the Hit on a geometry triangle, and the traced kernel's
// evaluate_surface from that Hit.  Device code shared by raster_resolve_kernel (pt_gbuffer_kernels.hip) and by the MASK
// discard of the raster kernels (pt_raster.hip), which therefore can never disagree: same ray, same uv, same LOD state.
#pragma once

#include "pt_device.hpp"

namespace ppt
{

// the ray through the pixel's centre minus currentJitter * 0.5
PPT_D Ray raster_pixel_ray(const RenderParams &r, const float currentJitter[2], uint32_t px, uint32_t py)
{
    f2 uv = f2{((float)px + 0.5f) / (float)r.width, ((float)py + 0.5f) / (float)r.height};
    uv = f2{uv.x - currentJitter[0] * 0.5f, uv.y - currentJitter[1] * 0.5f};
    return pinhole_camera_ray(r, uv);
}

// The Hit of `ray` on geometry triangle `prim` of draw instance `di`: bu = V / det, bv = W / det from edge_functions on the
// world-space triangle the traversal tests (flatten_triangles_kernel's: the index buffer's vertices through
// modelToWorld) - unclamped, no pass / range / box-guard rejection, the traversal's own `* (1 / det)`
PPT_D Hit raster_hit(const DeviceScene &s, const Ray &ray, uint32_t di, uint32_t prim)
{
    const prosper_DrawInstance inst = s.drawInstances[di];
    const prosper_GeometryMetadata m = s.geometryMetadatas[inst.meshIndex];
    const prosper_mat3x4 modelToWorld = s.modelInstanceTransforms[inst.modelInstanceIndex].modelToWorld;
    const f3 w0 = mul_point_mat3x4(load_r16g16b16a16(s, m.bufferIndex, m.positionsOffset, load_index(s, m, prim * 3u + 0u)), modelToWorld);
    const f3 w1 = mul_point_mat3x4(load_r16g16b16a16(s, m.bufferIndex, m.positionsOffset, load_index(s, m, prim * 3u + 1u)), modelToWorld);
    const f3 w2 = mul_point_mat3x4(load_r16g16b16a16(s, m.bufferIndex, m.positionsOffset, load_index(s, m, prim * 3u + 2u)), modelToWorld);
    const EdgeFunctions e = edge_functions(ray.o, ray.d, w0, w1, w2);
    const float inv = 1.0f / e.det;
    Hit hit;
    hit.drawInstance = di;
    hit.primitive = prim;
    hit.bary = f2{e.V * inv, e.W * inv};
    hit.t = __builtin_fmaf(e.W, dot(w2 - ray.o, ray.d), __builtin_fmaf(e.V, dot(w1 - ray.o, ray.d), e.U * dot(w0 - ray.o, ray.d))) * inv;
    return hit;
}

// evaluate_surface from that Hit; kLod: through the mip chains with the uv differences towards the rays of the pixels
// (px + 1, py) and (px, py + 1), as the traced kernel takes them.  `used` (may be nullptr): the derivatives sampled with.
template <bool kLod>
PPT_D Surface raster_pixel_surface(
    const DeviceScene &s, const RenderParams &r, const float currentJitter[2], const DeviceTextureMips *mips, float bias, uint32_t px,
    uint32_t py, const Ray &ray, const Hit &hit, UvDerivatives *used)
{
    LaneCounters cnt = {};
    if constexpr (kLod)
    {
        const SurfaceLod lod{mips, bias, ray.o, raster_pixel_ray(r, currentJitter, px + 1u, py).d, raster_pixel_ray(r, currentJitter, px, py + 1u).d, used};
        return evaluate_surface<false, false, true>(s, ray.d, hit, cnt, &lod);
    }
    else
        return evaluate_surface<false>(s, ray.d, hit, cnt);
}

} // namespace ppt
