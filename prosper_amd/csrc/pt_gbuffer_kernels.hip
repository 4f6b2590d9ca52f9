// pt_gbuffer_kernels.hip — gfx950 kernels of the passes over a G-buffer (host side: pt_gbuffer_passes.cpp,
// pt_forward_passes.cpp).
//
//   restir_di_*         ReSTIR-DI initial reservoirs, spatial reuse and trace over a G-buffer
//   gbuffer_trace       the ray-traced G-buffer those passes read
//   light_clustering    per-cluster point / spot light lists (LightClustering)
//   deferred_shading    unshadowed shading of the G-buffer over those lists (DeferredShading), with evalIBL over the
//                       maps of pt_ibl.hip in its _ibl variant
#include "pt_gbuffer_kernels.hpp"

#include <type_traits>

#include "pt_device.hpp"
#include "pt_ibl.hpp"
#include "pt_raster_surface.hpp"
#include "pt_render_common.hpp"

namespace ppt
{

// ------------------------------------------------------------------------------------------
// ReSTIR-DI (src/render/rtdi/RtDirectIllumination.cpp:70-115): three passes over the G-buffer, one lane per pixel,
// 256-lane blocks over 16x16 tiles (a wave per 8x8 quarter) dealt to the XCDs in contiguous bands (restir_tile).
//   restir_di_initial_kernel   RIS over 5 uniformly drawn lights      (restir_di/initial_reservoirs.comp)
//   restir_di_spatial_kernel   resamples 5 neighbour reservoirs        (restir_di/spatial_reuse.comp)
//   restir_di_trace_kernel     the reservoir's light, one shadow ray   (rt/direct_illumination/main.rgen:44-165,
//                              a second client of the traversal; src/render/rtdi/Trace.cpp:297)
// ------------------------------------------------------------------------------------------

// scene/material.glsl:20-32
PPT_D f3 signed_oct_decode(f3 n)
{
    f3 o;
    o.x = n.x - n.y;
    o.y = (n.x + n.y) - 1.0f;
    o.z = n.z * 2.0f - 1.0f;
    o.z = o.z * ((1.0f - fabs_(o.x)) - fabs_(o.y));
    return normalize(o);
}

struct RestirParams
{
    uint32_t drawType, frameIndex, flags, width, height;
    float eye[3];
    float clipToWorld[16]; // column-major
    float cameraToClip22, cameraToClip32; // linearizeDepth (scene/camera.glsl:11-22)
};

// Block b and b + 8 run on the same XCD: the tiles [x * perXcd, (x + 1) * perXcd) go to XCD x, so the neighbours the
// spatial pass reads mostly sit in the L2 of the XCD that reads them.  False past the last tile.
PPT_D bool restir_pixel(uint32_t width, uint32_t height, uint32_t &px, uint32_t &py)
{
    const uint32_t tilesX = (width + 15u) / 16u, tilesY = (height + 15u) / 16u;
    const uint32_t numTiles = tilesX * tilesY;
    const uint32_t perXcd = (numTiles + 7u) / 8u;
    const uint32_t tile = (blockIdx.x % 8u) * perXcd + (blockIdx.x / 8u);
    if (tile >= numTiles) return false;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    px = (tile % tilesX) * 16u + (wave & 1u) * 8u + (lane & 7u);
    py = (tile / tilesX) * 16u + (wave >> 1) * 8u + (lane >> 3);
    return true;
}
PPT_D bool restir_pixel(const RestirParams &p, uint32_t &px, uint32_t &py) { return restir_pixel(p.width, p.height, px, py); }

// scene/camera.glsl:11-22
PPT_D float linearize_depth(const RestirParams &p, float nonLinearDepth)
{
    return -p.cameraToClip32 / (nonLinearDepth + p.cameraToClip22);
}

// The VisibleSurface of a G-buffer texel, as all three passes build it (main.rgen:113-129,
// initial_reservoirs.comp:70-87, spatial_reuse.comp:145-162): uv = px / size (no half-pixel offset), worldPos through
// clipToWorld, the signed-octahedral normal, alpha = -1.
PPT_D Surface restir_surface(
    const RestirParams &p, uint32_t px, uint32_t py, float depth, const float4 &ar, const float4 &nm)
{
    const f2 uv = f2{(float)px / (float)p.width, (float)py / (float)p.height};
    Surface sf;
    {
        // worldPos, scene/camera.glsl:27-33
        const float *m = p.clipToWorld;
        const float x = uv.x * 2.0f - 1.0f, y = uv.y * 2.0f - 1.0f;
        const float vx = __builtin_fmaf(m[8], depth, __builtin_fmaf(m[4], y, __builtin_fmaf(m[0], x, m[12])));
        const float vy = __builtin_fmaf(m[9], depth, __builtin_fmaf(m[5], y, __builtin_fmaf(m[1], x, m[13])));
        const float vz = __builtin_fmaf(m[10], depth, __builtin_fmaf(m[6], y, __builtin_fmaf(m[2], x, m[14])));
        const float vw = __builtin_fmaf(m[11], depth, __builtin_fmaf(m[7], y, __builtin_fmaf(m[3], x, m[15])));
        sf.positionWS = f3{vx, vy, vz} * (1.0f / vw);
    }
    sf.invViewRayWS = normalize(f3{p.eye[0], p.eye[1], p.eye[2]} - sf.positionWS);
    sf.material.albedo = f3{ar.x, ar.y, ar.z};
    sf.material.roughness = ar.w;
    sf.material.normal = signed_oct_decode(f3{nm.x, nm.y, nm.w});
    sf.material.metallic = nm.z;
    sf.material.alpha = -1.0f;
    sf.normalWS = sf.material.normal;
    sf.uv = f2{0.0f, 0.0f};
    sf.NoV = saturate(dot(sf.normalWS, sf.invViewRayWS));
    return sf;
}

// pHatLight, restir_di/resampling_phat.glsl: luminance (common/math.glsl:15) of the unshadowed contribution
PPT_D float restir_p_hat(const DeviceScene &s, const Surface &sf, uint32_t lightIndex)
{
    f3 l, irradiance;
    float d;
    sample_light(s, sf.positionWS, lightIndex, l, d, irradiance);
    return dot(f3{0.299f, 0.587f, 0.114f}, irradiance * eval_brdf_times_nol(l, sf));
}

// restir_di/reservoir.glsl packReservoir
PPT_D float2 pack_reservoir(int32_t lightIndex, float weight)
{
    return make_float2(u2f((uint32_t)lightIndex), weight);
}

// initial_reservoirs.comp:31-60 initialLightCandidate.  The pHat of the pick is kept rather than evaluated again: the
// same function of the same light, the same bits.
__global__ __launch_bounds__(256) void restir_di_initial_kernel(
    DeviceScene s, RestirParams p, const float4 *__restrict__ albedoRoughness, const float4 *__restrict__ normalMetallic,
    const float *__restrict__ nonLinearDepth, float2 *__restrict__ outReservoirs)
{
    uint32_t px, py;
    if (!restir_pixel(p, px, py) || px >= p.width || py >= p.height) return;
    const size_t i = (size_t)py * p.width + px;
    const Surface sf = restir_surface(p, px, py, nonLinearDepth[i], albedoRoughness[i], normalMetallic[i]);
    Rng rng{px, py, p.frameIndex}; // :72

    const int32_t lightCount = 1 + (int32_t)(s.pointLightCount + s.spotLightCount);
    int32_t chosen = -1;
    float chosenPHat = 0.0f;
    float sumResamplingWeights = 0.0f;
    for (int k = 0; k < 5; ++k)
    {
        int32_t lightIndex = (int32_t)(rng.rnd01() * (float)lightCount);
        lightIndex = lightIndex < lightCount - 1 ? lightIndex : lightCount - 1;
        const float pHat = restir_p_hat(s, sf, (uint32_t)lightIndex);
        // misWeight 1 / 5, unbiasedContributionWeight = lightCount
        const float resamplingWeight = (0.2f * pHat) * (float)lightCount;
        sumResamplingWeights += resamplingWeight;
        if (rng.rnd01() < resamplingWeight / sumResamplingWeights)
        {
            chosen = lightIndex;
            chosenPHat = pHat;
        }
    }
    outReservoirs[i] = pack_reservoir(chosen, chosen >= 0 ? sumResamplingWeights / chosenPHat : 0.0f);
}

// spatial_reuse.comp:33-134 resampleReservoirSpatially.  The five slots are unrolled so that their reservoirs stay in
// registers; every random number is drawn in the GLSL's order (all the disc offsets first, then the accept tests).
__global__ __launch_bounds__(256) void restir_di_spatial_kernel(
    DeviceScene s, RestirParams p, const float4 *__restrict__ albedoRoughness, const float4 *__restrict__ normalMetallic,
    const float *__restrict__ nonLinearDepth, const float2 *__restrict__ inReservoirs, float2 *__restrict__ outReservoirs)
{
    uint32_t px, py;
    if (!restir_pixel(p, px, py) || px >= p.width || py >= p.height) return;
    const size_t i = (size_t)py * p.width + px;
    const float depth = nonLinearDepth[i];
    const Surface sf = restir_surface(p, px, py, depth, albedoRoughness[i], normalMetallic[i]);
    const float linearDepth = linearize_depth(p, depth);
    Rng rng{px, py, p.frameIndex}; // :147, the same stream the initial pass of this frame started

    int32_t sampleIndex[5];
    float sampleWeight[5];
    uint32_t validSampleCount = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k)
    {
        sampleIndex[k] = -1;
        sampleWeight[k] = 0.0f;
        for (int kill = 0; kill < 5; ++kill)
        {
            // uniformSampleDisk (common/sampling.glsl:8-13) * spatialRadius * 2 - spatialRadius, truncated
            const f2 u = rng.rnd2d01();
            const float r = sqrt_(u.x);
            float sn, cs;
            sincos_(kTwoPi * u.y, sn, cs);
            const int32_t ox = (int32_t)(((r * cs) * 30.0f) * 2.0f - 30.0f);
            const int32_t oy = (int32_t)(((r * sn) * 30.0f) * 2.0f - 30.0f);
            const int32_t qx = (int32_t)px + ox, qy = (int32_t)py + oy;
            if (qx <= 0 || qy <= 0 || qx >= (int32_t)p.width || qy >= (int32_t)p.height) continue;
            const size_t q = (size_t)qy * p.width + (size_t)qx;
            // 10 % depth difference (a NaN passes)
            if (fabs_(1.0f - linearize_depth(p, nonLinearDepth[q]) / linearDepth) > 0.1f) continue;
            const float4 nm = normalMetallic[q];
            if (dot(signed_oct_decode(f3{nm.x, nm.y, nm.w}), sf.normalWS) < 0.9f) continue;
            const float2 packed = inReservoirs[q];
            sampleIndex[k] = (int32_t)f2u(packed.x);
            sampleWeight[k] = packed.y;
            validSampleCount++;
            break;
        }
    }

    int32_t chosen = -1;
    float chosenPHat = 0.0f;
    float sumResamplingWeights = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k)
    {
        if (sampleIndex[k] < 0) continue;
        const float pHat = restir_p_hat(s, sf, (uint32_t)sampleIndex[k]);
        const float resamplingWeight = pHat * sampleWeight[k];
        sumResamplingWeights += resamplingWeight;
        if (rng.rnd01() < resamplingWeight / sumResamplingWeights)
        {
            chosen = sampleIndex[k];
            chosenPHat = pHat;
        }
    }
    float weight = 0.0f;
    if (chosen >= 0)
    {
        const float misWeight = 1.0f / (float)validSampleCount;
        weight = (misWeight * sumResamplingWeights) / chosenPHat;
    }
    outReservoirs[i] = pack_reservoir(chosen, weight);
}

__global__ __launch_bounds__(256) void restir_di_trace_kernel(
    DeviceScene s, RestirParams p, const float4 *__restrict__ albedoRoughness, const float4 *__restrict__ normalMetallic,
    const float *__restrict__ nonLinearDepth, const float2 *__restrict__ reservoirs, float4 *__restrict__ hdr,
    int32_t *__restrict__ stackOverflow)
{
    __shared__ int32_t ldsStack[kTraversalStackDepth * 256];
    uint32_t px, py;
    if (!restir_pixel(p, px, py)) return;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const TraversalStack stack{(lds_int32 *)ldsStack + wave * (kTraversalStackDepth * 64u) + lane,
                               stackOverflow + blockIdx.x * 256u + threadIdx.x, kTraversalStackDepth, gridDim.x * 256u, 64u};
    if (px >= p.width || py >= p.height) return;
    const size_t i = (size_t)py * p.width + px;

    // main.rgen:113-129
    const Surface sf = restir_surface(p, px, py, nonLinearDepth[i], albedoRoughness[i], normalMetallic[i]);

    if (p.drawType != PROSPER_DRAW_TYPE_DEFAULT)
    {
        const f3 c = p.drawType == PROSPER_DRAW_TYPE_POSITION ? sf.positionWS : sf.material.albedo;
        hdr[i] = make_float4(c.x, c.y, c.z, 1.0f);
        return;
    }
    // evaluateDirectLightingReSTIR, main.rgen:88-109
    const float2 packed = reservoirs[i];
    const int32_t lightIndex = (int32_t)f2u(packed.x);
    f3 color = f3{0.0f, 0.0f, 0.0f};
    if (!(sf.material.alpha == 0.0f || lightIndex < 0))
    {
        f3 l, irradiance;
        float d;
        sample_light(s, sf.positionWS, (uint32_t)lightIndex, l, d, irradiance);
        if (dot(l, sf.normalWS) > 0.0f)
        {
            LaneCounters cnt = {};
            Hit sh;
            const bool occluded = trace<true, false>(s, sf.positionWS, l, 0.1f, d, pcg(px ^ py), stack, sh, cnt);
            irradiance = irradiance * (occluded ? 0.0f : 1.0f);
            color = (irradiance * eval_brdf_times_nol(l, sf)) * packed.y;
        }
    }
    if ((p.flags & 1u) || !(p.flags & 2u))
        hdr[i] = make_float4(color.x, color.y, color.z, 1.0f);
    else
    {
        const float4 h = hdr[i];
        const float count = h.w + 1.0f;
        const float inv = 1.0f / count;
        hdr[i] = make_float4(
            __builtin_fmaf(color.x - h.x, inv, h.x), __builtin_fmaf(color.y - h.y, inv, h.y),
            __builtin_fmaf(color.z - h.z, inv, h.z), count);
    }
}

uint32_t restir_grid_blocks(uint32_t width, uint32_t height)
{
    const uint32_t numTiles = ((width + 15u) / 16u) * ((height + 15u) / 16u);
    return ((numTiles + 7u) / 8u) * 8u;
}

static RestirParams restir_params(
    uint32_t drawType, uint32_t frameIndex, uint32_t flags, uint32_t width, uint32_t height, const RestirCamera &cam)
{
    RestirParams p;
    p.drawType = drawType;
    p.frameIndex = frameIndex;
    p.flags = flags;
    p.width = width;
    p.height = height;
    for (int k = 0; k < 3; ++k) p.eye[k] = cam.eye[k];
    for (int k = 0; k < 16; ++k) p.clipToWorld[k] = cam.clipToWorld[k];
    p.cameraToClip22 = cam.cameraToClip22;
    p.cameraToClip32 = cam.cameraToClip32;
    return p;
}

void launch_restir_di_initial(
    const DeviceScene &s, uint32_t frameIndex, uint32_t width, uint32_t height, const RestirCamera &cam,
    const void *albedoRoughness, const void *normalMetallic, const float *nonLinearDepth, void *outReservoirs,
    hipStream_t stream)
{
    if (width == 0 || height == 0) return;
    hipLaunchKernelGGL(
        restir_di_initial_kernel, dim3(restir_grid_blocks(width, height)), dim3(256), 0, stream, s,
        restir_params(0, frameIndex, 0, width, height, cam), static_cast<const float4 *>(albedoRoughness),
        static_cast<const float4 *>(normalMetallic), nonLinearDepth, static_cast<float2 *>(outReservoirs));
}

void launch_restir_di_spatial(
    const DeviceScene &s, uint32_t frameIndex, uint32_t width, uint32_t height, const RestirCamera &cam,
    const void *albedoRoughness, const void *normalMetallic, const float *nonLinearDepth, const void *inReservoirs,
    void *outReservoirs, hipStream_t stream)
{
    if (width == 0 || height == 0) return;
    hipLaunchKernelGGL(
        restir_di_spatial_kernel, dim3(restir_grid_blocks(width, height)), dim3(256), 0, stream, s,
        restir_params(0, frameIndex, 0, width, height, cam), static_cast<const float4 *>(albedoRoughness),
        static_cast<const float4 *>(normalMetallic), nonLinearDepth, static_cast<const float2 *>(inReservoirs),
        static_cast<float2 *>(outReservoirs));
}

void launch_restir_di_trace(
    const DeviceScene &s, uint32_t drawType, uint32_t frameIndex, uint32_t flags, uint32_t width, uint32_t height,
    const RestirCamera &cam, const void *albedoRoughness, const void *normalMetallic, const float *nonLinearDepth,
    const void *reservoirs, float4 *hdr, int32_t *stackOverflow, hipStream_t stream)
{
    if (width == 0 || height == 0) return;
    hipLaunchKernelGGL(
        restir_di_trace_kernel, dim3(restir_grid_blocks(width, height)), dim3(256), 0, stream, s,
        restir_params(drawType, frameIndex, flags, width, height, cam), static_cast<const float4 *>(albedoRoughness),
        static_cast<const float4 *>(normalMetallic), nonLinearDepth, static_cast<const float2 *>(reservoirs), hdr,
        stackOverflow);
}

// ------------------------------------------------------------------------------------------
// Ray-traced G-buffer: the three targets of gbuffer.frag (albedoRoughness, normalMetallic, depth) from the path tracer's
// primary hit, one lane per pixel on the ReSTIR passes' tile / XCD mapping.  The ray is trace_path's camera ray without
// depth of field: the jittered sample of the pixel (main.rgen:229-231) or its centre.  The rng draws the jitter either
// way, so the any-hit seed pcg(x ^ z) is the path tracer's in both modes.
// ------------------------------------------------------------------------------------------

// gbuffer.frag:41-58 signedOctEncode
PPT_D f3 signed_oct_encode(f3 n)
{
    const float sum = (fabs_(n.x) + fabs_(n.y)) + fabs_(n.z);
    const float x = n.x / sum, y = n.y / sum, z = n.z / sum;
    f3 o;
    o.y = y * 0.5f + 0.5f;
    o.x = x * 0.5f + o.y;
    o.y = x * -0.5f + o.y;
    o.z = saturate(z * 3.40282e+38f);
    return o;
}

// The xy of (cameraToClip * worldToCamera * (p, 1)) / w, both matrices column-major (gbuffer.frag:74-75 over
// forward.mesh:74-88); `direction`: worldToCamera as mat4(mat3(.)) (skybox.vert:16-24).  w comes from the matrices.
PPT_D f2 project_ndc(const float *c, const float *m, f3 p, bool direction)
{
    float cam[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const float t = direction ? (k == 3 ? 1.0f : 0.0f) : m[12 + k];
        const bool lastRow = direction && k == 3; // (0, 0, 0, 1)
        cam[k] = lastRow ? 1.0f : __builtin_fmaf(m[8 + k], p.z, __builtin_fmaf(m[4 + k], p.y, __builtin_fmaf(m[k], p.x, t)));
    }
    const float x = __builtin_fmaf(c[12], cam[3], __builtin_fmaf(c[8], cam[2], __builtin_fmaf(c[4], cam[1], c[0] * cam[0])));
    const float y = __builtin_fmaf(c[13], cam[3], __builtin_fmaf(c[9], cam[2], __builtin_fmaf(c[5], cam[1], c[1] * cam[0])));
    const float w = __builtin_fmaf(c[15], cam[3], __builtin_fmaf(c[11], cam[2], __builtin_fmaf(c[7], cam[1], c[3] * cam[0])));
    return f2{x / w, y / w};
}

// gbuffer.frag:76-84 / skybox.frag:22-29: the motion in NDC with both jitters taken out, y up, clamped as the SNORM
// target clamps it
PPT_D float2 ndc_velocity(const GBufferVelocityParams &v, f3 position, f3 previousPosition, bool direction)
{
    const f2 pos = project_ndc(v.cameraToClip, v.worldToCamera, position, direction);
    const f2 prev = project_ndc(v.previousCameraToClip, v.previousWorldToCamera, previousPosition, direction);
    const float vx = (pos.x - v.currentJitter[0]) - (prev.x - v.previousJitter[0]);
    const float vy = -((pos.y - v.currentJitter[1]) - (prev.y - v.previousJitter[1]));
    return make_float2(fmin_(fmax_(vx, -1.0f), 1.0f), fmin_(fmax_(vy, -1.0f), 1.0f));
}

struct GBufferNoVelocity
{
};
struct GBufferNoLod
{
};

// kVelocity: the primary ray goes through the point the (jittered) projection puts on the pixel centre, and a fourth
// target takes the velocity, on hits and on the sky.  The plain instantiation reads nothing of `v`.
// kOpaqueOnly (PROSPER_PT_GBUFFER_OPAQUE_ONLY): BLEND candidates are always rejected, as prosper keeps BLEND geometry out of its G-buffer
// (draw_list_generator.comp:43-54); forward_transparent_kernel draws them afterwards.
// kLod (prosper_pt_set_texture_lod): the material is sampled through the textures' mip chains, with the uv
// forward differences towards the pixels (px + 1, py) and (px, py + 1) - the pinhole rays through them, with this
// pixel's own jitter offset, met with the hit triangle's plane.  The ray, the hit and everything but the sampled
// material are the plain instantiation's.
template <bool kVelocity, bool kOpaqueOnly = false, bool kLod = false>
__global__ __launch_bounds__(256) void gbuffer_trace_kernel(
    DeviceScene s, GBufferTraceParams g, float4 *__restrict__ albedoRoughness, float4 *__restrict__ normalMetallic,
    float *__restrict__ nonLinearDepth, int32_t *__restrict__ stackOverflow,
    std::conditional_t<kVelocity, GBufferVelocityParams, GBufferNoVelocity> v, std::conditional_t<kLod, GBufferLodParams, GBufferNoLod> lodp)
{
    __shared__ int32_t ldsStack[kTraversalStackDepth * 256];
    uint32_t px, py;
    if (!restir_pixel(g.r.width, g.r.height, px, py)) return;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const TraversalStack stack{(lds_int32 *)ldsStack + wave * (kTraversalStackDepth * 64u) + lane,
                               stackOverflow + blockIdx.x * 256u + threadIdx.x, kTraversalStackDepth, gridDim.x * 256u, 64u};
    if (px >= g.r.width || py >= g.r.height) return;
    const size_t i = (size_t)py * g.r.width + px;

    Rng rng{px, py, g.frameIndex};
    const f2 j = rng.rnd2d01();
    f2 uv = g.jitter ? f2{((float)px + j.x) / (float)g.r.width, ((float)py + j.y) / (float)g.r.height}
                     : f2{((float)px + 0.5f) / (float)g.r.width, ((float)py + 0.5f) / (float)g.r.height};
    // ndc_jittered = ndc_unjittered + currentJitter: the unjittered ray half a jitter back lands on the pixel centre
    if constexpr (kVelocity) uv = f2{uv.x - v.currentJitter[0] * 0.5f, uv.y - v.currentJitter[1] * 0.5f};
    const Ray ray = pinhole_camera_ray(g.r, uv);
    LaneCounters cnt = {};
    Hit hit;
    if (!trace<false, false, kOpaqueOnly ? kBlendReject : kBlendStochastic>(s, ray.o, ray.d, ray.tMin, ray.tMax, pcg(rng.x ^ rng.z), stack, hit, cnt))
    {
        // the clear values of GBufferRenderer.cpp:487-516
        albedoRoughness[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        normalMetallic[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        nonLinearDepth[i] = 0.0f;
        if constexpr (kVelocity) v.velocity[i] = ndc_velocity(v, ray.d, ray.d, true);
        if constexpr (kLod)
            if (lodp.derivatives) lodp.derivatives[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    Surface sf;
    if constexpr (kLod)
    {
        // the neighbours' uv by the expressions above with px + 1 / py + 1
        const float w = (float)g.r.width, h = (float)g.r.height;
        const float ox = g.jitter ? j.x : 0.5f, oy = g.jitter ? j.y : 0.5f;
        f2 uvX = f2{((float)(px + 1u) + ox) / w, ((float)py + oy) / h};
        f2 uvY = f2{((float)px + ox) / w, ((float)(py + 1u) + oy) / h};
        if constexpr (kVelocity)
        {
            uvX = f2{uvX.x - v.currentJitter[0] * 0.5f, uvX.y - v.currentJitter[1] * 0.5f};
            uvY = f2{uvY.x - v.currentJitter[0] * 0.5f, uvY.y - v.currentJitter[1] * 0.5f};
        }
        UvDerivatives used;
        const SurfaceLod lod{lodp.mips, lodp.bias, ray.o, pinhole_camera_ray(g.r, uvX).d, pinhole_camera_ray(g.r, uvY).d, &used};
        sf = evaluate_surface<false, false, true>(s, ray.d, hit, cnt, &lod);
        if (lodp.derivatives) lodp.derivatives[i] = make_float4(used.dudx, used.dvdx, used.dudy, used.dvdy);
    }
    else
        sf = evaluate_surface<false>(s, ray.d, hit, cnt);
    if constexpr (kVelocity)
    {
        f3 previous = sf.positionWS;
        if (v.previousTransforms)
        {
            // the interpolated model-space vertex evaluate_surface transforms, through the instance's previous transform
            const float4 *rec = reinterpret_cast<const float4 *>(s.shadeTriangles + (s.triangleOffsets[hit.drawInstance] + hit.primitive));
            const float4 q6 = rec[6], q7 = rec[7];
            const f3 p0 = unpack_half3(__builtin_bit_cast(uint32_t, q6.x), __builtin_bit_cast(uint32_t, q6.y));
            const f3 p1 = unpack_half3(__builtin_bit_cast(uint32_t, q6.z), __builtin_bit_cast(uint32_t, q6.w));
            const f3 p2 = unpack_half3(__builtin_bit_cast(uint32_t, q7.x), __builtin_bit_cast(uint32_t, q7.y));
            const float a = (1.0f - hit.bary.x) - hit.bary.y, b = hit.bary.x, c = hit.bary.y;
            const f3 model = f3{bary1(p0.x, p1.x, p2.x, a, b, c), bary1(p0.y, p1.y, p2.y, a, b, c), bary1(p0.z, p1.z, p2.z, a, b, c)};
            previous = mul_point_mat3x4(model, v.previousTransforms[s.drawInstances[hit.drawInstance].modelInstanceIndex].modelToWorld);
        }
        v.velocity[i] = ndc_velocity(v, sf.positionWS, previous, false);
    }
    if (g.drawType != PROSPER_DRAW_TYPE_DEFAULT && g.drawType != PROSPER_DRAW_TYPE_MESHLET_ID)
    {
        // gbuffer.frag:83-99
        const f3 c = debug_color(s, g.drawType, hit, sf);
        albedoRoughness[i] = make_float4(c.x, c.y, c.z, 1.0f);
        normalMetallic[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    else
    {
        const f3 enc = signed_oct_encode(sf.normalWS);
        albedoRoughness[i] = make_float4(sf.material.albedo.x, sf.material.albedo.y, sf.material.albedo.z, sf.material.roughness);
        normalMetallic[i] = make_float4(enc.x, enc.y, sf.material.metallic, enc.z);
    }
    // posNDC.z of gbuffer.vert / gbuffer.frag: (worldToClip * (positionWS, 1)).z / .w
    const float *m = g.worldToClip;
    const f3 p = sf.positionWS;
    const float cz = __builtin_fmaf(m[10], p.z, __builtin_fmaf(m[6], p.y, __builtin_fmaf(m[2], p.x, m[14])));
    const float cw = __builtin_fmaf(m[11], p.z, __builtin_fmaf(m[7], p.y, __builtin_fmaf(m[3], p.x, m[15])));
    nonLinearDepth[i] = cz / cw;
}

// The winning triangle of a visibility key (pt_raster.hpp RasterParams::keys): the draw instance whose meshlet range holds
// the ordinal, the meshlet in it, the meshlet-local triangle, and the geometry triangle through the triangle map.  False
// for the clear value and for a key that names nothing the tables hold.  One copy for the resolve and the forward pass.
PPT_D bool raster_decode_key(
    const DeviceScene &s, const RasterResolveTables &r, unsigned long long key, uint32_t &di, uint32_t &mi, uint32_t &local, uint32_t &prim)
{
    bool covered = key != 0ull;
    if (covered)
    {
        const uint32_t low = ~(uint32_t)key, ordinal = low >> 7;
        local = low & 127u;
        // the last draw instance whose base is not above the ordinal
        uint32_t lo = 0, hi = r.drawInstanceCount;
        while (hi - lo > 1u)
        {
            const uint32_t mid = (lo + hi) >> 1;
            if (r.meshletBase[mid] <= ordinal)
                lo = mid;
            else
                hi = mid;
        }
        di = lo;
        covered = r.drawInstanceCount != 0u && r.meshletBase[di] <= ordinal;
        if (covered)
        {
            mi = ordinal - r.meshletBase[di];
            const uint32_t mesh = s.drawInstances[di].meshIndex;
            covered = mesh < r.meshCount && mi < r.meshMeshletBase[mesh + 1u] - r.meshMeshletBase[mesh];
            if (covered)
            {
                const uint32_t gm = r.meshMeshletBase[mesh] + mi;
                covered = local < r.meshletTriStart[gm + 1u] - r.meshletTriStart[gm];
                if (covered) prim = r.triMap[r.meshletTriStart[gm] + local];
            }
        }
    }
    return covered;
}

// The velocity of a covered pixel of the visibility image, as gbuffer_trace_kernel<true> takes it: the interpolated
// model-space vertex evaluate_surface transforms, through the instance's previous transform where there is one
PPT_D float2 raster_surface_velocity(const DeviceScene &s, const GBufferVelocityParams &v, uint32_t modelInstanceIndex, const Hit &hit, const Surface &sf)
{
    f3 previous = sf.positionWS;
    if (v.previousTransforms)
    {
        const float4 *rec = reinterpret_cast<const float4 *>(s.shadeTriangles + (s.triangleOffsets[hit.drawInstance] + hit.primitive));
        const float4 q6 = rec[6], q7 = rec[7];
        const f3 p0 = unpack_half3(__builtin_bit_cast(uint32_t, q6.x), __builtin_bit_cast(uint32_t, q6.y));
        const f3 p1 = unpack_half3(__builtin_bit_cast(uint32_t, q6.z), __builtin_bit_cast(uint32_t, q6.w));
        const f3 p2 = unpack_half3(__builtin_bit_cast(uint32_t, q7.x), __builtin_bit_cast(uint32_t, q7.y));
        const float a = (1.0f - hit.bary.x) - hit.bary.y, b = hit.bary.x, c = hit.bary.y;
        const f3 model = f3{bary1(p0.x, p1.x, p2.x, a, b, c), bary1(p0.y, p1.y, p2.y, a, b, c), bary1(p0.z, p1.z, p2.z, a, b, c)};
        previous = mul_point_mat3x4(model, v.previousTransforms[modelInstanceIndex].modelToWorld);
    }
    return ndc_velocity(v, sf.positionWS, previous, false);
}

// The resolve of the rasteriser's visibility image (pt_raster.hip) into the G-buffer targets: one lane per
// pixel.  Nothing is interpolated in screen space: for the winning triangle the lane forms the pixel's own ray exactly as
// gbuffer_trace_kernel<true, true, kLod> does, takes bu = V / det, bv = W / det from edge_functions on the world-space
// triangle the traversal tests (flatten_triangles_kernel's: the index buffer's vertices through modelToWorld) - unclamped,
// no pass / range / box-guard rejection, the traversal's own `* (1 / det)` - and from that Hit runs the traced kernel's
// code.  The depth is the rasteriser's, from the key.  MeshletID and PrimitiveID are the mesh shader's (gbuffer.frag:88-93,
// forward.mesh:144): the meshlet's index and the meshlet-local triangle.
template <bool kLod>
__global__ __launch_bounds__(256) void raster_resolve_kernel(
    DeviceScene s, GBufferTraceParams g, RasterResolveTables r, float4 *__restrict__ albedoRoughness, float4 *__restrict__ normalMetallic,
    float *__restrict__ nonLinearDepth, GBufferVelocityParams v, std::conditional_t<kLod, GBufferLodParams, GBufferNoLod> lodp)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)g.r.width * g.r.height) return;
    const uint32_t px = (uint32_t)(i % g.r.width), py = (uint32_t)(i / g.r.width);
    const Ray ray = raster_pixel_ray(g.r, v.currentJitter, px, py);
    const unsigned long long key = r.keys[i];
    uint32_t di = 0, mi = 0, local = 0, prim = 0;
    const bool covered = raster_decode_key(s, r, key, di, mi, local, prim);
    if (!covered)
    {
        // the clear values of GBufferRenderer.cpp:487-516; the sky's velocity as the traced entry computes it
        albedoRoughness[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        normalMetallic[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        nonLinearDepth[i] = 0.0f;
        v.velocity[i] = ndc_velocity(v, ray.d, ray.d, true);
        if constexpr (kLod)
            if (lodp.derivatives) lodp.derivatives[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const prosper_DrawInstance inst = s.drawInstances[di];
    const Hit hit = raster_hit(s, ray, di, prim);
    Surface sf;
    if constexpr (kLod)
    {
        UvDerivatives used;
        sf = raster_pixel_surface<true>(s, g.r, v.currentJitter, lodp.mips, lodp.bias, px, py, ray, hit, &used);
        if (lodp.derivatives) lodp.derivatives[i] = make_float4(used.dudx, used.dvdx, used.dudy, used.dvdy);
    }
    else
        sf = raster_pixel_surface<false>(s, g.r, v.currentJitter, nullptr, 0.0f, px, py, ray, hit, nullptr);
    v.velocity[i] = raster_surface_velocity(s, v, inst.modelInstanceIndex, hit, sf);
    if (g.drawType == PROSPER_DRAW_TYPE_MESHLET_ID || g.drawType == PROSPER_DRAW_TYPE_PRIMITIVE_ID)
    {
        const f3 c = uint_to_color(g.drawType == PROSPER_DRAW_TYPE_MESHLET_ID ? mi : local);
        albedoRoughness[i] = make_float4(c.x, c.y, c.z, 1.0f);
        normalMetallic[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    else if (g.drawType != PROSPER_DRAW_TYPE_DEFAULT)
    {
        const f3 c = debug_color(s, g.drawType, hit, sf);
        albedoRoughness[i] = make_float4(c.x, c.y, c.z, 1.0f);
        normalMetallic[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    else
    {
        const f3 enc = signed_oct_encode(sf.normalWS);
        albedoRoughness[i] = make_float4(sf.material.albedo.x, sf.material.albedo.y, sf.material.albedo.z, sf.material.roughness);
        normalMetallic[i] = make_float4(enc.x, enc.y, sf.material.metallic, enc.z);
    }
    nonLinearDepth[i] = u2f((uint32_t)(key >> 32));
}

void launch_raster_resolve(
    const DeviceScene &s, const GBufferTraceParams &g, const RasterResolveTables &r, const GBufferVelocityParams &v, void *albedoRoughness,
    void *normalMetallic, float *nonLinearDepth, hipStream_t stream, const GBufferLodParams *lod)
{
    const size_t pixels = (size_t)g.r.width * g.r.height;
    if (pixels == 0) return;
    const dim3 grid((uint32_t)((pixels + 255u) / 256u));
    if (lod)
        hipLaunchKernelGGL(raster_resolve_kernel<true>, grid, dim3(256), 0, stream, s, g, r, static_cast<float4 *>(albedoRoughness),
                           static_cast<float4 *>(normalMetallic), nonLinearDepth, v, *lod);
    else
        hipLaunchKernelGGL(raster_resolve_kernel<false>, grid, dim3(256), 0, stream, s, g, r, static_cast<float4 *>(albedoRoughness),
                           static_cast<float4 *>(normalMetallic), nonLinearDepth, v, GBufferNoLod{});
}

void launch_gbuffer_trace(
    const DeviceScene &s, const GBufferTraceParams &g, void *albedoRoughness, void *normalMetallic, float *nonLinearDepth,
    int32_t *stackOverflow, hipStream_t stream, const GBufferLodParams *lod)
{
    if (g.r.width == 0 || g.r.height == 0) return;
    const dim3 grid(restir_grid_blocks(g.r.width, g.r.height));
    if (lod)
    {
        const auto kernel = g.opaqueOnly ? gbuffer_trace_kernel<false, true, true> : gbuffer_trace_kernel<false, false, true>;
        hipLaunchKernelGGL(
            kernel, grid, dim3(256), 0, stream, s, g, static_cast<float4 *>(albedoRoughness), static_cast<float4 *>(normalMetallic),
            nonLinearDepth, stackOverflow, GBufferNoVelocity{}, *lod);
        return;
    }
    const auto kernel = g.opaqueOnly ? gbuffer_trace_kernel<false, true> : gbuffer_trace_kernel<false, false>;
    hipLaunchKernelGGL(
        kernel, grid, dim3(256), 0, stream, s, g, static_cast<float4 *>(albedoRoughness), static_cast<float4 *>(normalMetallic),
        nonLinearDepth, stackOverflow, GBufferNoVelocity{}, GBufferNoLod{});
}

void launch_gbuffer_trace_velocity(
    const DeviceScene &s, const GBufferTraceParams &g, const GBufferVelocityParams &v, void *albedoRoughness, void *normalMetallic,
    float *nonLinearDepth, int32_t *stackOverflow, hipStream_t stream, const GBufferLodParams *lod)
{
    if (g.r.width == 0 || g.r.height == 0) return;
    const dim3 grid(restir_grid_blocks(g.r.width, g.r.height));
    if (lod)
    {
        const auto kernel = g.opaqueOnly ? gbuffer_trace_kernel<true, true, true> : gbuffer_trace_kernel<true, false, true>;
        hipLaunchKernelGGL(
            kernel, grid, dim3(256), 0, stream, s, g, static_cast<float4 *>(albedoRoughness), static_cast<float4 *>(normalMetallic),
            nonLinearDepth, stackOverflow, v, *lod);
        return;
    }
    const auto kernel = g.opaqueOnly ? gbuffer_trace_kernel<true, true> : gbuffer_trace_kernel<true, false>;
    hipLaunchKernelGGL(
        kernel, grid, dim3(256), 0, stream, s, g, static_cast<float4 *>(albedoRoughness), static_cast<float4 *>(normalMetallic),
        nonLinearDepth, stackOverflow, v, GBufferNoLod{});
}

// ------------------------------------------------------------------------------------------
// Clustered lighting (src/render/LightClustering.cpp, src/render/DeferredShading.cpp):
//   light_clustering_kernel   one 256-lane block per cluster builds its point / spot lists (light_clustering.comp)
//   deferred_shading_kernel   one lane per pixel shades the G-buffer texel over its cluster's lists
//                             (deferred_shading.comp, scene/light_clusters.glsl), unshadowed
// The three rules the GLSL leaves open: ascending light order in a list, the fixed slot
// clusterLinearIndex * 256 of the index buffer, and the 128 lowest indices of each type kept on overflow.
// ------------------------------------------------------------------------------------------

static_assert(PROSPER_MAX_POINT_LIGHT_COUNT <= 256u * 32u, "a lane's share of the point lights must fit a 32-bit mask");

// light_clustering.comp clusterFrustum: six planes (xyz, w), signedDistance = dot(xyz, p) - w
struct ClusterFrustum
{
    f4 planes[6];
};

// scene/light_clusters.glsl sliceStart
PPT_D float slice_start(const ClusterParams &c, uint32_t slice)
{
    const float sliceFrac = (float)slice / (float)kClusterZSlices;
    return c.near_ * pow_(c.far_ / c.near_, sliceFrac);
}

PPT_D ClusterFrustum cluster_frustum(const ClusterParams &c, uint32_t cx, uint32_t cy, uint32_t cz)
{
    const float tileScaleX = c.resolution[0] / (float)(2u * kClusterDim);
    const float tileScaleY = c.resolution[1] / (float)(2u * kClusterDim);
    const float tileBiasX = tileScaleX - (float)cx, tileBiasY = tileScaleY - (float)cy;
    // c1 = (m00 * sx, 0, -bx, 0), c2 = (0, m11 * sy, -by, 0), c4 = (0, 0, -1, 0); the projection's Y is already flipped
    const float c1x = c.cameraToClip00 * tileScaleX, c1z = -tileBiasX;
    const float c2y = c.cameraToClip11 * tileScaleY, c2z = -tileBiasY;
    ClusterFrustum f;
    f.planes[0] = f4{-c1x, 0.0f, -1.0f - c1z, 0.0f};
    f.planes[1] = f4{c1x, 0.0f, -1.0f + c1z, 0.0f};
    f.planes[2] = f4{0.0f, -c2y, -1.0f - c2z, 0.0f};
    f.planes[3] = f4{0.0f, c2y, -1.0f + c2z, 0.0f};
    f.planes[4] = f4{0.0f, 0.0f, -1.0f, cz == 0 ? 0.0f : slice_start(c, cz)};
    f.planes[5] = f4{0.0f, 0.0f, 1.0f, -slice_start(c, cz + 1u)};
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        const f4 p = f.planes[i];
        const float inv = 1.0f / sqrt_(__builtin_fmaf(p.z, p.z, __builtin_fmaf(p.y, p.y, p.x * p.x)));
        f.planes[i] = f4{p.x * inv, p.y * inv, p.z * inv, p.w * inv};
    }
    return f;
}

// isPointVisible: the light's sphere (worldToCamera * position, radianceAndRadius.w) against the six planes
PPT_D bool point_light_visible(const ClusterParams &c, const ClusterFrustum &f, const prosper_PointLight &light)
{
    const float *m = c.worldToCamera;
    const prosper_vec4 q = light.position;
    const float x = __builtin_fmaf(m[12], q.w, __builtin_fmaf(m[8], q.z, __builtin_fmaf(m[4], q.y, m[0] * q.x)));
    const float y = __builtin_fmaf(m[13], q.w, __builtin_fmaf(m[9], q.z, __builtin_fmaf(m[5], q.y, m[1] * q.x)));
    const float z = __builtin_fmaf(m[14], q.w, __builtin_fmaf(m[10], q.z, __builtin_fmaf(m[6], q.y, m[2] * q.x)));
    const float r = light.radianceAndRadius.w;
    bool visible = true;
#pragma unroll
    for (int i = 0; i < 6; ++i)
    {
        const f4 p = f.planes[i];
        visible = visible && __builtin_fmaf(p.z, z, __builtin_fmaf(p.y, y, p.x * x)) - p.w >= -r;
    }
    return visible;
}

__global__ __launch_bounds__(256) void light_clustering_kernel(
    DeviceScene s, ClusterParams c, uint2 *__restrict__ pointers, uint16_t *__restrict__ indices,
    uint32_t *__restrict__ dropped)
{
    __shared__ uint32_t waveTotals[4];
    const uint32_t cx = blockIdx.x, cy = blockIdx.y, cz = blockIdx.z;
    const uint32_t cluster = (cz * c.dimY + cy) * c.dimX + cx;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const ClusterFrustum f = cluster_frustum(c, cx, cy, cz);

    // contiguous chunks of roundedUpQuotient(count, 256) lights per lane, as the GLSL splits them
    const uint32_t totalPoints = s.pointLightCount;
    const uint32_t perLane = (totalPoints + 255u) / 256u;
    uint32_t mask = 0, count = 0;
    for (uint32_t k = 0; k < perLane; ++k)
    {
        const uint32_t pi = tid * perLane + k;
        if (pi >= totalPoints) break;
        if (point_light_visible(c, f, s.pointLights->lights[pi]))
        {
            mask |= 1u << k;
            ++count;
        }
    }
    // block-wide exclusive prefix of the lanes' counts: lane order is light order, so the list is ascending
    uint32_t inclusive = count;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1)
    {
        const uint32_t t = __shfl_up(inclusive, off, 64);
        if (lane >= off) inclusive += t;
    }
    if (lane == 63u) waveTotals[wave] = inclusive;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; ++w) base += waveTotals[w];
    const uint32_t visiblePoints = (waveTotals[0] + waveTotals[1]) + (waveTotals[2] + waveTotals[3]);
    const uint32_t keptPoints = visiblePoints < kClusterMaxPoints ? visiblePoints : kClusterMaxPoints;
    // isSpotVisible is always true: every spot, the lowest kClusterMaxSpots of them
    const uint32_t totalSpots = s.spotLightCount;
    const uint32_t keptSpots = totalSpots < kClusterMaxSpots ? totalSpots : kClusterMaxSpots;
    uint16_t *slot = indices + (size_t)cluster * kClusterSlot;

    uint32_t pos = base + inclusive - count;
    for (uint32_t k = 0; mask != 0u; ++k, mask >>= 1)
    {
        if (!(mask & 1u)) continue;
        if (pos < kClusterMaxPoints) slot[pos] = (uint16_t)(tid * perLane + k);
        ++pos;
    }
    for (uint32_t i = tid; i < keptSpots; i += 256u) slot[keptPoints + i] = (uint16_t)i;

    if (tid == 0)
    {
        const uint32_t kept = keptPoints + keptSpots;
        // packClusterPointer; an empty cluster's offset is 0, as the GLSL writes it
        pointers[cluster] = make_uint2(kept > 0u ? cluster * kClusterSlot : 0u, (keptPoints << 16) | keptSpots);
        // per cluster, not one global atomic counter: 34 680 clusters at 1920x1080 would serialise on its address
        dropped[cluster] = (visiblePoints - keptPoints) + (totalSpots - keptSpots);
    }
}

void launch_light_clustering(
    const DeviceScene &s, const ClusterParams &c, void *pointers, uint16_t *indices, uint32_t *dropped, hipStream_t stream)
{
    if (c.dimX == 0 || c.dimY == 0) return;
    hipLaunchKernelGGL(
        light_clustering_kernel, dim3(c.dimX, c.dimY, kClusterZSlices + 1u), dim3(256), 0, stream, s, c,
        static_cast<uint2 *>(pointers), indices, dropped);
}

// deferred_shading.comp: the G-buffer texel's VisibleSurface (restir_surface), the sun, then its cluster's point and
// spot lists, each summed from zero and added in that order.  Debug draw types write the position or the G-buffer's
// albedo without lighting (the GLSL's lighting of those texels is overwritten).
struct DeferredParams
{
    RestirParams r;
    float near_, far_;
    uint32_t clustersX, clustersY;
};

// evalIBL (scene/skybox.glsl:48-83), as written: the split-sum specular over the prefiltered radiance and the BRDF LUT
// plus the diffuse irradiance, without AO.
PPT_D f3 eval_ibl(const IblMaps &m, const Surface &sf)
{
    const f3 f0 = fresnel_zero(sf);
    const float NoV = saturate(dot(sf.normalWS, sf.invViewRayWS));
    // schlickFresnelWithRoughness (brdf.glsl:28-31)
    const float p = pow5(1.0f - NoV);
    const float r1 = 1.0f - sf.material.roughness;
    const f3 F = f3{__builtin_fmaf(fmax_(r1, f0.x) - f0.x, p, f0.x), __builtin_fmaf(fmax_(r1, f0.y) - f0.y, p, f0.y),
                    __builtin_fmaf(fmax_(r1, f0.z) - f0.z, p, f0.z)};
    const f3 kD = (f3{1.0f, 1.0f, 1.0f} - F) * (1.0f - sf.material.metallic);
    const f3 diffuse = sample_cube_bordered(m.irradiance, kIblIrradianceSize, sf.normalWS) * sf.material.albedo;
    const f3 R = reflect(-sf.invViewRayWS, sf.normalWS);
    const f3 prefiltered = sample_radiance_trilinear(m.radiance, R, sf.material.roughness);
    const f2 envBrdf = sample_brdf_lut(m.lut, NoV, sf.material.roughness);
    const f3 specular = prefiltered * (F * envBrdf.x + f3{envBrdf.y, envBrdf.y, envBrdf.y});
    return kD * diffuse + specular;
}

// What deferred_shading.comp:40-60 and forward.frag:69-81 both sum over a surface, in their order: the sun, then the
// point and the spot lights of clusterIndex(px, zCam) (scene/light_clusters.glsl), each list summed from zero, then with
// IBL evalIBL.  zCam: the surface's camera-space z (negative in front of the camera).
struct ClusterGrid
{
    float near_, far_;
    uint32_t clustersX, clustersY;
};
template <bool IBL>
PPT_D f3 shade_clustered(
    const DeviceScene &s, const Surface &sf, uint32_t px, uint32_t py, float zCam, const ClusterGrid &d,
    const uint2 *__restrict__ pointers, const uint16_t *__restrict__ indices, const IblMaps *ibl)
{
    // evalDirectionalLight (scene/lighting.glsl:8-12)
    const prosper_DirectionalLightParameters sun = *s.directionalLight;
    const f3 sunL = -normalize(f3{sun.direction.x, sun.direction.y, sun.direction.z});
    f3 color = f3{0.0f, 0.0f, 0.0f} + f3{sun.irradiance.x, sun.irradiance.y, sun.irradiance.z} * eval_brdf_times_nol(sunL, sf);

    // clusterIndex: slice = uint(16 * log(-z / near) / log(far / near)); nearer than near (or NaN) is slice 0, past
    // the last slice (16) a cluster without lights
    const float ratio = -zCam / d.near_;
    float slice = ratio > 0.0f ? ((float)kClusterZSlices * log2_(ratio)) / log2_(d.far_ / d.near_) : 0.0f;
    if (!(slice >= 0.0f)) slice = 0.0f;
    uint32_t offset = 0, pointCount = 0, spotCount = 0;
    if (slice < (float)(kClusterZSlices + 1u))
    {
        const uint32_t cluster = ((uint32_t)slice * d.clustersY + py / kClusterDim) * d.clustersX + px / kClusterDim;
        const uint2 packed = pointers[cluster];
        offset = packed.x;
        pointCount = packed.y >> 16;
        spotCount = packed.y & 0xFFFFu;
    }
    f3 points = f3{0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0; k < pointCount; ++k)
    {
        f3 l, irradiance;
        float dist;
        eval_point_light(s.pointLights->lights[indices[offset + k]], sf.positionWS, l, dist, irradiance);
        points = points + irradiance * eval_brdf_times_nol(l, sf);
    }
    color = color + points;
    f3 spots = f3{0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0; k < spotCount; ++k)
    {
        f3 l, irradiance;
        float dist;
        eval_spot_light(s.spotLights->lights[indices[offset + pointCount + k]], sf.positionWS, l, dist, irradiance);
        spots = spots + irradiance * eval_brdf_times_nol(l, sf);
    }
    color = color + spots;
    if constexpr (IBL) color = color + eval_ibl(*ibl, sf);
    return color;
}

// The body of both shading kernels; IBL adds evalIBL after the spot lights (deferred_shading.comp:59-60).
template <bool IBL>
PPT_D void deferred_shade(
    const DeviceScene &s, const DeferredParams &d, const float4 *__restrict__ albedoRoughness,
    const float4 *__restrict__ normalMetallic, const float *__restrict__ nonLinearDepth,
    const uint2 *__restrict__ pointers, const uint16_t *__restrict__ indices, float4 *__restrict__ hdr, const IblMaps *ibl)
{
    uint32_t px, py;
    if (!restir_pixel(d.r, px, py) || px >= d.r.width || py >= d.r.height) return;
    const size_t i = (size_t)py * d.r.width + px;
    const float depth = nonLinearDepth[i];
    const Surface sf = restir_surface(d.r, px, py, depth, albedoRoughness[i], normalMetallic[i]);
    if (d.r.drawType != PROSPER_DRAW_TYPE_DEFAULT)
    {
        const f3 c = d.r.drawType == PROSPER_DRAW_TYPE_POSITION ? sf.positionWS : sf.material.albedo;
        hdr[i] = make_float4(c.x, c.y, c.z, 1.0f);
        return;
    }
    const float linearDepth = linearize_depth(d.r, depth);
    const f3 color = shade_clustered<IBL>(s, sf, px, py, linearDepth, ClusterGrid{d.near_, d.far_, d.clustersX, d.clustersY}, pointers, indices, ibl);
    hdr[i] = make_float4(color.x, color.y, color.z, 1.0f);
}

__global__ __launch_bounds__(256) void deferred_shading_kernel(
    DeviceScene s, DeferredParams d, const float4 *__restrict__ albedoRoughness,
    const float4 *__restrict__ normalMetallic, const float *__restrict__ nonLinearDepth,
    const uint2 *__restrict__ pointers, const uint16_t *__restrict__ indices, float4 *__restrict__ hdr)
{
    deferred_shade<false>(s, d, albedoRoughness, normalMetallic, nonLinearDepth, pointers, indices, hdr, nullptr);
}

__global__ __launch_bounds__(256) void deferred_shading_ibl_kernel(
    DeviceScene s, DeferredParams d, const float4 *__restrict__ albedoRoughness,
    const float4 *__restrict__ normalMetallic, const float *__restrict__ nonLinearDepth,
    const uint2 *__restrict__ pointers, const uint16_t *__restrict__ indices, float4 *__restrict__ hdr, IblMaps ibl)
{
    deferred_shade<true>(s, d, albedoRoughness, normalMetallic, nonLinearDepth, pointers, indices, hdr, &ibl);
}

void launch_deferred_shading(
    const DeviceScene &s, uint32_t drawType, uint32_t width, uint32_t height, const RestirCamera &cam, const ClusteredLights &l,
    const void *albedoRoughness, const void *normalMetallic, const float *nonLinearDepth, float4 *hdr, hipStream_t stream)
{
    if (width == 0 || height == 0) return;
    DeferredParams d;
    d.r = restir_params(drawType, 0, 0, width, height, cam);
    d.near_ = l.params.near_;
    d.far_ = l.params.far_;
    d.clustersX = l.params.dimX;
    d.clustersY = l.params.dimY;
    const dim3 grid(restir_grid_blocks(width, height));
    const float4 *ar = static_cast<const float4 *>(albedoRoughness), *nm = static_cast<const float4 *>(normalMetallic);
    const uint2 *ptrs = static_cast<const uint2 *>(l.pointers);
    const IblMaps maps = {l.irradiance, l.radiance, l.lut};
    if (l.irradiance)
        hipLaunchKernelGGL(deferred_shading_ibl_kernel, grid, dim3(256), 0, stream, s, d, ar, nm, nonLinearDepth, ptrs, l.indices, hdr, maps);
    else
        hipLaunchKernelGGL(deferred_shading_kernel, grid, dim3(256), 0, stream, s, d, ar, nm, nonLinearDepth, ptrs, l.indices, hdr);
}

// ------------------------------------------------------------------------------------------
// Forward transparent pass (src/render/ForwardRenderer.cpp recordTransparent, forward.frag): the BLEND
// surfaces the opaque-only G-buffer left out, lit forward over the light clusters and blended over the HDR image in
// place.  One lane per pixel on the G-buffer's pixel mapping, along the G-buffer's own ray of that pixel.  Layers are
// peeled front to back: each closest-hit traversal (kBlendPeel) returns the nearest front-facing BLEND triangle behind
// the last one by the key (t, drawInstance, primitive); C += T a src, T *= 1 - a, and the end is C + T dst - in exact
// arithmetic prosper's blend state applied back to front.  No layer cap, no memory beyond the traversal stack.
// ------------------------------------------------------------------------------------------

// What the forward passes keep of a layer (prosper_pt_read_transparent_layers, prosper_pt_read_forward_surfaces,
// prosper_pt_read_raster_transparent_layers): one copy for the three kernels
PPT_D void store_layer_record(prosper_pt_transparent_layer *out, const Hit &hit, const Surface &sf, float depth)
{
    const f3 q = sf.positionWS;
    prosper_pt_transparent_layer L;
    L.drawInstance = hit.drawInstance;
    L.primitive = hit.primitive;
    L.positionWS[0] = q.x; L.positionWS[1] = q.y; L.positionWS[2] = q.z;
    L.nonLinearDepth = depth;
    L.albedo[0] = sf.material.albedo.x; L.albedo[1] = sf.material.albedo.y; L.albedo[2] = sf.material.albedo.z;
    L.roughness = sf.material.roughness;
    L.normal[0] = sf.normalWS.x; L.normal[1] = sf.normalWS.y; L.normal[2] = sf.normalWS.z;
    L.metallic = sf.material.metallic;
    L.alpha = sf.material.alpha;
    L.reserved = 0u;
    *out = L;
}

// forward.frag:69-83 for a layer whose view vector is set: the clustered lights (and evalIBL) at its own camera-space z
// (forward.mesh:75: the third component of worldToCamera * (position, 1)), and the source alpha in *a
template <bool IBL>
PPT_D f3 shade_forward_layer(
    const DeviceScene &s, const Surface &sf, uint32_t px, uint32_t py, const float *w, const ClusterGrid &grid, const uint2 *__restrict__ pointers,
    const uint16_t *__restrict__ indices, const IblMaps *ibl, float *a)
{
    const f3 q = sf.positionWS;
    const float zCam = __builtin_fmaf(w[10], q.z, __builtin_fmaf(w[6], q.y, __builtin_fmaf(w[2], q.x, w[14])));
    const f3 src = shade_clustered<IBL>(s, sf, px, py, zCam, grid, pointers, indices, ibl);
    *a = sf.material.alpha > 0.0f ? sf.material.alpha : 1.0f; // forward.frag:83
    return src;
}

// One step of the front-to-back blend: C += T a src, T *= 1 - a
PPT_D void blend_layer_under(f3 &C, float &T, f3 src, float a)
{
    C = C + src * (T * a);
    T = T * (1.0f - a);
}

// kLayers: the debug mode of prosper_pt_read_transparent_layers - the first p.debugLayers layers of a pixel are kept
// kLod (prosper_pt_set_texture_lod): every peeled layer samples its material through the mip chains, with
// the uv forward differences of gbuffer_trace_kernel<.., .., true> - the same two neighbour rays for all layers of the
// pixel, met with each layer's own triangle plane.
template <bool IBL, bool kLayers, bool kLod = false>
__global__ __launch_bounds__(256) void forward_transparent_kernel(
    DeviceScene s, TransparentParams p, const float *__restrict__ nonLinearDepth, const uint2 *__restrict__ pointers,
    const uint16_t *__restrict__ indices, float4 *__restrict__ hdr, int32_t *__restrict__ stackOverflow,
    uint32_t *__restrict__ stats, uint32_t *__restrict__ layerCounts, prosper_pt_transparent_layer *__restrict__ layers,
    IblMaps ibl, std::conditional_t<kLod, GBufferLodParams, GBufferNoLod> lodp)
{
    __shared__ int32_t ldsStack[kTraversalStackDepth * 256];
    const GBufferTraceParams &g = p.g;
    uint32_t px, py;
    if (!restir_pixel(g.r.width, g.r.height, px, py)) return;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const TraversalStack stack{(lds_int32 *)ldsStack + wave * (kTraversalStackDepth * 64u) + lane,
                               stackOverflow + blockIdx.x * 256u + threadIdx.x, kTraversalStackDepth, gridDim.x * 256u, 64u};
    uint32_t count = 0;
    if (px < g.r.width && py < g.r.height)
    {
        const size_t i = (size_t)py * g.r.width + px;
        // the G-buffer's ray of this pixel (gbuffer_trace_kernel): centre, the path tracer's sample, or the centre half a
        // camera jitter back
        f2 uv = f2{((float)px + 0.5f) / (float)g.r.width, ((float)py + 0.5f) / (float)g.r.height};
        [[maybe_unused]] float ox = 0.5f, oy = 0.5f; // the pixel's own offset, for the neighbours' rays (kLod)
        if (g.jitter)
        {
            Rng rng{px, py, g.frameIndex};
            const f2 j = rng.rnd2d01();
            uv = f2{((float)px + j.x) / (float)g.r.width, ((float)py + j.y) / (float)g.r.height};
            ox = j.x;
            oy = j.y;
        }
        if (p.cameraJitter) uv = f2{uv.x - p.currentJitter[0] * 0.5f, uv.y - p.currentJitter[1] * 0.5f};
        const Ray ray = pinhole_camera_ray(g.r, uv);
        [[maybe_unused]] SurfaceLod lod = {};
        if constexpr (kLod)
        {
            f2 uvX = f2{((float)(px + 1u) + ox) / (float)g.r.width, ((float)py + oy) / (float)g.r.height};
            f2 uvY = f2{((float)px + ox) / (float)g.r.width, ((float)(py + 1u) + oy) / (float)g.r.height};
            if (p.cameraJitter)
            {
                uvX = f2{uvX.x - p.currentJitter[0] * 0.5f, uvX.y - p.currentJitter[1] * 0.5f};
                uvY = f2{uvY.x - p.currentJitter[0] * 0.5f, uvY.y - p.currentJitter[1] * 0.5f};
            }
            lod = SurfaceLod{lodp.mips, lodp.bias, ray.o, pinhole_camera_ray(g.r, uvX).d, pinhole_camera_ray(g.r, uvY).d, nullptr};
        }
        const float stored = nonLinearDepth[i];
        // Nothing behind the opaque surface can pass the depth test: the traversal ends a little past it (0.1 %, far more
        // than the depth's rounding), and the exact test below decides.  A depth that gives no positive distance (the sky's
        // 0 on an infinite far plane, a NaN) bounds nothing.
        float tMax = ray.tMax;
        {
            const float zCam = -p.cameraToClip32 / (stored + p.cameraToClip22);
            const float cosFwd = dot(ray.d, f3{g.r.fwd[0], g.r.fwd[1], g.r.fwd[2]});
            const float bound = (-zCam / cosFwd) * 1.001f;
            if (stored != 0.0f && bound > 0.0f && bound < tMax) tMax = bound;
        }
        const f3 eye = f3{g.r.eye[0], g.r.eye[1], g.r.eye[2]};
        const bool debugView = g.drawType != PROSPER_DRAW_TYPE_DEFAULT && g.drawType != PROSPER_DRAW_TYPE_MESHLET_ID;
        const ClusterGrid grid{p.near_, p.far_, p.clustersX, p.clustersY};

        f3 C = f3{0.0f, 0.0f, 0.0f};
        float T = 1.0f, nearestAlpha = 0.0f;
        Hit after;
        after.drawInstance = 0u;
        after.primitive = 0u;
        after.bary = f2{0.0f, 0.0f};
        after.t = -1.0f; // every candidate's t is > tMin = 0
        LaneCounters cnt = {};
        while (T != 0.0f)
        {
            Hit hit;
            if (!trace<false, false, kBlendPeel>(s, ray.o, ray.d, ray.tMin, tMax, 0u, stack, hit, cnt, &after)) break;
            after = hit;
            Surface sf;
            if constexpr (kLod)
                sf = evaluate_surface<false, false, true>(s, ray.d, hit, cnt, &lod);
            else
                sf = evaluate_surface<false>(s, ray.d, hit, cnt);
            if (sf.material.alpha == 0.0f) continue; // forward.frag:57
            // posNDC.z as gbuffer_trace_kernel computes it; eGreater on reverse Z, no depth write
            const float *m = g.worldToClip;
            const f3 q = sf.positionWS;
            const float cz = __builtin_fmaf(m[10], q.z, __builtin_fmaf(m[6], q.y, __builtin_fmaf(m[2], q.x, m[14])));
            const float cw = __builtin_fmaf(m[11], q.z, __builtin_fmaf(m[7], q.y, __builtin_fmaf(m[3], q.x, m[15])));
            const float depth = cz / cw;
            if (!(depth > stored)) continue;
            // forward.frag:52,67
            sf.invViewRayWS = normalize(eye - sf.positionWS);
            sf.NoV = saturate(dot(sf.normalWS, sf.invViewRayWS));
            if constexpr (kLayers)
            {
                if (count < p.debugLayers) store_layer_record(layers + (i * p.debugLayers + count), hit, sf, depth);
            }
            f3 src;
            float a;
            if (debugView)
            {
                src = debug_color(s, g.drawType, hit, sf);
                a = 1.0f;
            }
            else
                src = shade_forward_layer<IBL>(s, sf, px, py, p.worldToCamera, grid, pointers, indices, &ibl, &a);
            if (count == 0) nearestAlpha = a;
            ++count;
            blend_layer_under(C, T, src, a);
        }
        if constexpr (kLayers) layerCounts[i] = count;
        if (count > 0)
        {
            const float4 dst = hdr[i];
            // VkUtils.hpp:93-106: colour srcAlpha / oneMinusSrcAlpha; alpha oneMinusSrcAlpha / zero, i.e. the last drawn
            // (nearest) layer's a (1 - a)
            hdr[i] = make_float4(
                C.x + dst.x * T, C.y + dst.y * T, C.z + dst.z * T, nearestAlpha * (1.0f - nearestAlpha));
        }
    }
    // prosper_pt_get_transparent_info: one set of atomics per wave
    const uint64_t covered = __ballot(count > 0);
    if (covered != 0ull)
    {
        uint32_t sum = count, deepest = count;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
        {
            sum += __shfl_xor(sum, off, 64);
            const uint32_t o = __shfl_xor(deepest, off, 64);
            deepest = o > deepest ? o : deepest;
        }
        if (lane == 0)
        {
            atomicAdd(&stats[0], (uint32_t)__popcll(covered));
            atomicMax(&stats[1], deepest);
            atomicAdd(reinterpret_cast<unsigned long long *>(stats + 2), (unsigned long long)sum);
        }
    }
}

void launch_forward_transparent(
    const DeviceScene &s, const TransparentParams &p, const float *nonLinearDepth, const ClusteredLights &l, float4 *hdr,
    int32_t *stackOverflow, uint32_t *stats, uint32_t *layerCounts, prosper_pt_transparent_layer *layers, hipStream_t stream,
    const GBufferLodParams *lod)
{
    if (p.g.r.width == 0 || p.g.r.height == 0) return;
    const dim3 grid(restir_grid_blocks(p.g.r.width, p.g.r.height));
    const IblMaps maps = {l.irradiance, l.radiance, l.lut};
    const uint2 *ptrs = static_cast<const uint2 *>(l.pointers);
    const bool ibl = l.irradiance != nullptr, debug = p.debugLayers != 0u;
    if (lod)
    {
        const auto kernel = ibl ? (debug ? forward_transparent_kernel<true, true, true> : forward_transparent_kernel<true, false, true>)
                                : (debug ? forward_transparent_kernel<false, true, true> : forward_transparent_kernel<false, false, true>);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s, p, nonLinearDepth, ptrs, l.indices, hdr, stackOverflow, stats, layerCounts, layers, maps, *lod);
        return;
    }
    const auto kernel = ibl ? (debug ? forward_transparent_kernel<true, true> : forward_transparent_kernel<true, false>)
                            : (debug ? forward_transparent_kernel<false, true> : forward_transparent_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s, p, nonLinearDepth, ptrs, l.indices, hdr, stackOverflow, stats, layerCounts, layers, maps, GBufferNoLod{});
}

// ------------------------------------------------------------------------------------------
// Forward opaque pass (src/render/ForwardRenderer.cpp recordOpaque, forward.frag): the pixel's winning
// triangle of the visibility image shaded directly over the light clusters - raster_resolve_kernel's surface, which is
// never stored, then forward_transparent_kernel's shading of it.  One lane per pixel on the G-buffer passes' mapping
// (restir_pixel: a wave is an aligned 8 x 8 block, which never straddles an edge of the 32 x 32 clusters: its lanes' lists
// differ only where the block spans two depth slices).  It stands here, not beside the resolve, because it needs
// shade_clustered.
//   covered    illumination (colour, material alpha or 1), velocity and depth as the resolve writes them; the debug draw
//              types write what the resolve writes to albedoRoughness (forward.frag:99-116)
//   uncovered  the clear values (0, 0, 0, 0) and 0 (ForwardRenderer.cpp:574-604), the sky's velocity
// kSurfaces (prosper_pt_set_forward_debug_surfaces): the pixel's surface is also stored, one record per pixel.
// ------------------------------------------------------------------------------------------
template <bool IBL, bool kLod, bool kSurfaces>
__global__ __launch_bounds__(256) void forward_opaque_kernel(
    DeviceScene s, GBufferTraceParams g, RasterResolveTables r, GBufferVelocityParams v, ClusterGrid grid, const uint2 *__restrict__ pointers,
    const uint16_t *__restrict__ indices, float4 *__restrict__ hdr, float *__restrict__ nonLinearDepth, uint32_t *__restrict__ shadedPixels,
    prosper_pt_transparent_layer *__restrict__ surfaces, IblMaps ibl, std::conditional_t<kLod, GBufferLodParams, GBufferNoLod> lodp)
{
    uint32_t px, py;
    if (!restir_pixel(g.r.width, g.r.height, px, py)) return;
    bool covered = false;
    if (px < g.r.width && py < g.r.height)
    {
        const size_t i = (size_t)py * g.r.width + px;
        const Ray ray = raster_pixel_ray(g.r, v.currentJitter, px, py);
        const unsigned long long key = r.keys[i];
        uint32_t di = 0, mi = 0, local = 0, prim = 0;
        covered = raster_decode_key(s, r, key, di, mi, local, prim);
        if (!covered)
        {
            hdr[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            nonLinearDepth[i] = 0.0f;
            v.velocity[i] = ndc_velocity(v, ray.d, ray.d, true);
            if constexpr (kSurfaces)
            {
                prosper_pt_transparent_layer L = {};
                L.drawInstance = 0xFFFFFFFFu;
                surfaces[i] = L;
            }
        }
        else
        {
            const prosper_DrawInstance inst = s.drawInstances[di];
            const Hit hit = raster_hit(s, ray, di, prim);
            Surface sf;
            if constexpr (kLod)
                sf = raster_pixel_surface<true>(s, g.r, v.currentJitter, lodp.mips, lodp.bias, px, py, ray, hit, nullptr);
            else
                sf = raster_pixel_surface<false>(s, g.r, v.currentJitter, nullptr, 0.0f, px, py, ray, hit, nullptr);
            // forward.frag:94-97: the velocity is written whatever the draw type
            v.velocity[i] = raster_surface_velocity(s, v, inst.modelInstanceIndex, hit, sf);
            const float depth = u2f((uint32_t)(key >> 32));
            nonLinearDepth[i] = depth;
            const f3 q = sf.positionWS;
            if constexpr (kSurfaces) store_layer_record(surfaces + i, hit, sf, depth);
            if (g.drawType == PROSPER_DRAW_TYPE_MESHLET_ID || g.drawType == PROSPER_DRAW_TYPE_PRIMITIVE_ID)
            {
                // forward.frag:99-107 over forward.mesh:144
                const f3 c = uint_to_color(g.drawType == PROSPER_DRAW_TYPE_MESHLET_ID ? mi : local);
                hdr[i] = make_float4(c.x, c.y, c.z, 1.0f);
            }
            else if (g.drawType != PROSPER_DRAW_TYPE_DEFAULT)
            {
                const f3 c = debug_color(s, g.drawType, hit, sf);
                hdr[i] = make_float4(c.x, c.y, c.z, 1.0f);
            }
            else
            {
                // forward.frag:52,67
                sf.invViewRayWS = normalize(f3{g.r.eye[0], g.r.eye[1], g.r.eye[2]} - q);
                sf.NoV = saturate(dot(sf.normalWS, sf.invViewRayWS));
                float a; // forward.frag:83,118
                const f3 color = shade_forward_layer<IBL>(s, sf, px, py, v.worldToCamera, grid, pointers, indices, &ibl, &a);
                hdr[i] = make_float4(color.x, color.y, color.z, a);
            }
        }
    }
    // prosper_pt_get_forward_opaque_info: one atomic per wave, dealt over kForwardCountSlots counters a cache line apart (32 400
    // waves at 1920x1080 on one address serialise: measured)
    const uint64_t mask = __ballot(covered);
    if (mask != 0ull && (threadIdx.x & 63u) == 0u)
        atomicAdd(shadedPixels + (blockIdx.x % kForwardCountSlots) * kForwardCountStride, (uint32_t)__popcll(mask));
}

void launch_forward_opaque(
    const DeviceScene &s, const GBufferTraceParams &g, const RasterResolveTables &r, const GBufferVelocityParams &v, const ClusteredLights &l,
    float4 *hdr, float *nonLinearDepth, uint32_t *shadedPixels, prosper_pt_transparent_layer *surfaces, hipStream_t stream,
    const GBufferLodParams *lod)
{
    if (g.r.width == 0 || g.r.height == 0) return;
    const dim3 grid(restir_grid_blocks(g.r.width, g.r.height));
    const ClusterGrid cg{l.params.near_, l.params.far_, l.params.dimX, l.params.dimY};
    const IblMaps maps = {l.irradiance, l.radiance, l.lut};
    const uint2 *ptrs = static_cast<const uint2 *>(l.pointers);
    const bool ibl = l.irradiance != nullptr, debug = surfaces != nullptr;
    if (lod)
    {
        const auto kernel = ibl ? (debug ? forward_opaque_kernel<true, true, true> : forward_opaque_kernel<true, true, false>)
                                : (debug ? forward_opaque_kernel<false, true, true> : forward_opaque_kernel<false, true, false>);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s, g, r, v, cg, ptrs, l.indices, hdr, nonLinearDepth, shadedPixels, surfaces, maps, *lod);
        return;
    }
    const auto kernel = ibl ? (debug ? forward_opaque_kernel<true, false, true> : forward_opaque_kernel<true, false, false>)
                            : (debug ? forward_opaque_kernel<false, false, true> : forward_opaque_kernel<false, false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s, g, r, v, cg, ptrs, l.indices, hdr, nonLinearDepth, shadedPixels, surfaces, maps, GBufferNoLod{});
}

// ------------------------------------------------------------------------------------------
// Rasterised transparent pass (ForwardRenderer::recordTransparent over the meshlet draw lists): the resolve
// of the per-pixel fragment lists the raster kernels filled (pt_raster.hip).  One lane per pixel on forward_opaque_kernel's
// mapping, for its reason.  Front to back the lane SELECTS the greatest key of its list below the previous one - over
// global memory, no per-lane array, O(n^2) in the layers of one pixel - rebuilds the layer's surface as forward_opaque_kernel
// rebuilds the winner's, shades it and blends it under what is nearer with forward_transparent_kernel's own arithmetic.
// A pixel without a list keeps its four floats.  kLayers: the first t.debugLayers shaded layers of a pixel are kept.
// stats: kForwardCountSlots sets a cache line apart of { pixels with a list, layers shaded, the longest list }.
// ------------------------------------------------------------------------------------------
template <bool IBL, bool kLod, bool kLayers>
__global__ __launch_bounds__(256) void raster_transparent_kernel(
    DeviceScene s, GBufferTraceParams g, RasterResolveTables r, RasterLayerLists t, GBufferVelocityParams v, ClusterGrid grid,
    const uint2 *__restrict__ pointers, const uint16_t *__restrict__ indices, float4 *__restrict__ hdr, uint32_t *__restrict__ stats,
    uint32_t debugLayers, uint32_t *__restrict__ layerCounts, prosper_pt_transparent_layer *__restrict__ layers, IblMaps ibl,
    std::conditional_t<kLod, GBufferLodParams, GBufferNoLod> lodp)
{
    uint32_t px, py;
    if (!restir_pixel(g.r.width, g.r.height, px, py)) return;
    uint32_t n = 0, shaded = 0;
    if (px < g.r.width && py < g.r.height)
    {
        const size_t i = (size_t)py * g.r.width + px;
        n = t.counts[i];
        const uint32_t first = t.offsets[i];
        // (a list never leaves the buffer: the scan's total bounds offset + count)
        if (first > t.total || n > t.total - first) n = 0u;
        if (n != 0u)
        {
            const unsigned long long *list = t.fragments + first;
            const Ray ray = raster_pixel_ray(g.r, v.currentJitter, px, py);
            const f3 eye = f3{g.r.eye[0], g.r.eye[1], g.r.eye[2]};
            f3 C = f3{0.0f, 0.0f, 0.0f};
            float T = 1.0f, nearestAlpha = 0.0f;
            unsigned long long previous = ~0ull; // (above every key: a depth is at most 1)
            for (uint32_t k = 0; k < n && T != 0.0f; ++k)
            {
                unsigned long long key = 0ull;
                for (uint32_t j = 0; j < n; ++j)
                {
                    const unsigned long long c = list[j];
                    if (c < previous && c > key) key = c;
                }
                if (key == 0ull) break; // (keys of one pixel are unique: never taken before k == n)
                previous = key;
                uint32_t di = 0, mi = 0, local = 0, prim = 0;
                if (!raster_decode_key(s, r, key, di, mi, local, prim)) continue;
                const Hit hit = raster_hit(s, ray, di, prim);
                Surface sf;
                if constexpr (kLod)
                    sf = raster_pixel_surface<true>(s, g.r, v.currentJitter, lodp.mips, lodp.bias, px, py, ray, hit, nullptr);
                else
                    sf = raster_pixel_surface<false>(s, g.r, v.currentJitter, nullptr, 0.0f, px, py, ray, hit, nullptr);
                // forward.frag:52,67
                sf.invViewRayWS = normalize(eye - sf.positionWS);
                sf.NoV = saturate(dot(sf.normalWS, sf.invViewRayWS));
                if constexpr (kLayers)
                    if (shaded < debugLayers) store_layer_record(layers + (i * debugLayers + shaded), hit, sf, u2f((uint32_t)(key >> 32)));
                f3 src;
                float a = 1.0f;
                if (g.drawType == PROSPER_DRAW_TYPE_MESHLET_ID || g.drawType == PROSPER_DRAW_TYPE_PRIMITIVE_ID)
                    src = uint_to_color(g.drawType == PROSPER_DRAW_TYPE_MESHLET_ID ? mi : local); // forward.frag:99-107 over forward.mesh:144
                else if (g.drawType != PROSPER_DRAW_TYPE_DEFAULT)
                    src = debug_color(s, g.drawType, hit, sf);
                else
                    src = shade_forward_layer<IBL>(s, sf, px, py, v.worldToCamera, grid, pointers, indices, &ibl, &a);
                if (shaded == 0u) nearestAlpha = a;
                ++shaded;
                blend_layer_under(C, T, src, a);
            }
            if (shaded > 0u)
            {
                const float4 dst = hdr[i];
                // VkUtils.hpp:93-106, as forward_transparent_kernel ends
                hdr[i] = make_float4(C.x + dst.x * T, C.y + dst.y * T, C.z + dst.z * T, nearestAlpha * (1.0f - nearestAlpha));
            }
        }
        if constexpr (kLayers) layerCounts[i] = shaded;
    }
    // prosper_pt_get_raster_transparent_info: one set of atomics per wave, dealt over kForwardCountSlots sets a cache line apart
    const uint64_t listed = __ballot(n != 0u);
    if (listed != 0ull)
    {
        uint32_t sum = shaded, deepest = n;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
        {
            sum += __shfl_xor(sum, off, 64);
            const uint32_t o = __shfl_xor(deepest, off, 64);
            deepest = o > deepest ? o : deepest;
        }
        if ((threadIdx.x & 63u) == 0u)
        {
            uint32_t *slot = stats + (blockIdx.x % kForwardCountSlots) * kForwardCountStride;
            atomicAdd(slot + 0, (uint32_t)__popcll(listed));
            atomicAdd(slot + 1, sum);
            atomicMax(slot + 2, deepest);
        }
    }
}

void launch_raster_transparent(
    const DeviceScene &s, const GBufferTraceParams &g, const RasterResolveTables &r, const RasterLayerLists &t, const GBufferVelocityParams &v,
    const ClusteredLights &l, float4 *hdr, uint32_t *stats, uint32_t debugLayers, uint32_t *layerCounts, prosper_pt_transparent_layer *layers,
    hipStream_t stream, const GBufferLodParams *lod)
{
    if (g.r.width == 0 || g.r.height == 0) return;
    const dim3 grid(restir_grid_blocks(g.r.width, g.r.height));
    const ClusterGrid cg{l.params.near_, l.params.far_, l.params.dimX, l.params.dimY};
    const IblMaps maps = {l.irradiance, l.radiance, l.lut};
    const uint2 *ptrs = static_cast<const uint2 *>(l.pointers);
    const bool ibl = l.irradiance != nullptr, debug = debugLayers != 0u;
    if (lod)
    {
        const auto kernel = ibl ? (debug ? raster_transparent_kernel<true, true, true> : raster_transparent_kernel<true, true, false>)
                                : (debug ? raster_transparent_kernel<false, true, true> : raster_transparent_kernel<false, true, false>);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s, g, r, t, v, cg, ptrs, l.indices, hdr, stats, debugLayers, layerCounts, layers, maps, *lod);
        return;
    }
    const auto kernel = ibl ? (debug ? raster_transparent_kernel<true, false, true> : raster_transparent_kernel<true, false, false>)
                            : (debug ? raster_transparent_kernel<false, false, true> : raster_transparent_kernel<false, false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s, g, r, t, v, cg, ptrs, l.indices, hdr, stats, debugLayers, layerCounts, layers, maps, GBufferNoLod{});
}

} // namespace ppt
