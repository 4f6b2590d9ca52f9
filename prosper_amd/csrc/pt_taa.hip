// pt_taa.hip — gfx950 kernels of the temporal anti-aliasing resolve (src/render/TemporalAntiAliasing.cpp,
// res/shader/taa_resolve.comp).
//
//   taa_resolve_kernel<index>   taa_resolve.comp specialised as prosper's pipeline `index` (specializationIndex): the
//                               illumination, the velocity, the depth and the previous resolve into the new one
//   taa_expand_kernel           the new resolve (RGBA16F) into the HDR image (RGBA32F) after an in-place resolve
//
// Images have no sampler here; the lookups are written out.  A nearest lookup at (px + offset + .5) / res is the texel
// px + offset clamped to the edge, formed from the integers.  A block of 32 x 8 texels stages its illumination tile with
// a one-texel halo in LDS - clamped to the edge as it is loaded, so the tile IS the clamped neighbourhood - and the
// centre read, the min/max loop and the moment loops read it from there; the velocity and the depth tile are staged the
// same way for the samplings that look at the neighbourhood.  The history taps depend on the velocity and stay loads.
#include "pt_taa.hpp"

#include <utility>

#include "pt_device.hpp"

namespace ppt
{

const float kTaaHalton23[8][2] = {
    {0.5f, 0.3333333333333333f},   {0.25f, 0.6666666666666666f},  {0.75f, 0.1111111111111111f},  {0.125f, 0.4444444444444444f},
    {0.625f, 0.7777777777777778f}, {0.375f, 0.2222222222222222f}, {0.875f, 0.5555555555555556f}, {0.0625f, 0.8888888888888888f}};

namespace taa
{

constexpr uint32_t kTileW = 32, kTileH = 8;                 // texels a block resolves, one per lane
constexpr uint32_t kHaloW = kTileW + 2, kHaloH = kTileH + 2; // ... and stages
constexpr uint32_t kHaloTexels = kHaloW * kHaloH;

enum : uint32_t
{
    kClipNone = 0,
    kClipMinMax = 1,
    kClipVariance = 2,
    kVelocityCenter = 0,
    kVelocityLargest = 1,
    kVelocityClosest = 2,
};

struct Rgb
{
    float r, g, b;
};

PPT_D Rgb texel_rgb(uint2 p) { return Rgb{half_to_float(p.x & 0xFFFFu), half_to_float(p.x >> 16), half_to_float(p.y & 0xFFFFu)}; }
PPT_D int32_t clamp_i(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// bilinearSampler over the previous resolve: clamp to edge
PPT_D Rgb texel_edge(const uint2 *__restrict__ img, int32_t w, int32_t h, int32_t x, int32_t y)
{
    return texel_rgb(img[(size_t)clamp_i(y, 0, h - 1) * (uint32_t)w + (uint32_t)clamp_i(x, 0, w - 1)]);
}
PPT_D Rgb mix2(Rgb a, Rgb b, float t)
{
    const float s = 1.0f - t;
    return Rgb{s * a.r + t * b.r, s * a.g + t * b.g, s * a.b + t * b.b};
}
// the four texels of a bilinear footprint blended with float weights, a and b the fractions along x and y
PPT_D Rgb blend4(Rgb t00, Rgb t10, Rgb t01, Rgb t11, float a, float b)
{
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    return Rgb{((w00 * t00.r + w10 * t10.r) + w01 * t01.r) + w11 * t11.r, ((w00 * t00.g + w10 * t10.g) + w01 * t01.g) + w11 * t11.g,
               ((w00 * t00.b + w10 * t10.b) + w01 * t01.b) + w11 * t11.b};
}
PPT_D Rgb edge_bilinear(const uint2 *__restrict__ img, int32_t w, int32_t h, int32_t ix, float fx, int32_t iy, float fy)
{
    return blend4(texel_edge(img, w, h, ix, iy), texel_edge(img, w, h, ix + 1, iy), texel_edge(img, w, h, ix, iy + 1),
                  texel_edge(img, w, h, ix + 1, iy + 1), fx, fy);
}

// optimizedCatmullRom's weights along one axis for the fraction f (taa_resolve.comp:95-107), c = sharpness / 100
struct CatmullAxis
{
    float w0, w12, w3, t; // t = w2 / w12: the fraction of the centre tap between the texels i and i + 1
};
PPT_D CatmullAxis catmull_axis(float f)
{
    constexpr float c = 70.0f / 100.0f;
    constexpr float k2c = 2.0f * c, k2mc = 2.0f - c, k3mc = 3.0f - c, k3m2c = 3.0f - 2.0f * c;
    const float f2 = f * f, f3 = f * f2;
    const float w0 = (-c * f3 + k2c * f2) - c * f;
    const float w1 = (k2mc * f3 - k3mc * f2) + 1.0f;
    const float w2 = (-k2mc * f3 + k3m2c * f2) + c * f;
    const float w3 = c * f3 - c * f2;
    CatmullAxis a;
    a.w0 = w0;
    a.w12 = w1 + w2;
    a.w3 = w3;
    a.t = w2 / a.w12;
    return a;
}

// The previous resolve at the footprint (ix, fx), (iy, fy): the five taps of optimizedCatmullRom in texel space.  The
// centre tap blends the texels i, i + 1 of both axes, an outer tap is the single texel i - 1 or i + 2 of its axis.
PPT_D Rgb catmull_rom(const uint2 *__restrict__ img, int32_t w, int32_t h, int32_t ix, float fx, int32_t iy, float fy)
{
    const CatmullAxis ax = catmull_axis(fx), ay = catmull_axis(fy);
    const Rgb up = mix2(texel_edge(img, w, h, ix, iy - 1), texel_edge(img, w, h, ix + 1, iy - 1), ax.t);     // (tc12.x, tc0.y)
    const Rgb left = mix2(texel_edge(img, w, h, ix - 1, iy), texel_edge(img, w, h, ix - 1, iy + 1), ay.t);   // (tc0.x, tc12.y)
    const Rgb centre = edge_bilinear(img, w, h, ix, ax.t, iy, ay.t);
    const Rgb right = mix2(texel_edge(img, w, h, ix + 2, iy), texel_edge(img, w, h, ix + 2, iy + 1), ay.t);  // (tc3.x, tc12.y)
    const Rgb down = mix2(texel_edge(img, w, h, ix, iy + 2), texel_edge(img, w, h, ix + 1, iy + 2), ax.t);   // (tc12.x, tc3.y)
    const float k0 = ax.w12 * ay.w0, k1 = ax.w0 * ay.w12, k2 = ax.w12 * ay.w12, k3 = ax.w3 * ay.w12, k4 = ax.w12 * ay.w3;
    const float a = (((k0 + k1) + k2) + k3) + k4;
    return Rgb{((((up.r * k0 + left.r * k1) + centre.r * k2) + right.r * k3) + down.r * k4) / a,
               ((((up.g * k0 + left.g * k1) + centre.g * k2) + right.g * k3) + down.g * k4) / a,
               ((((up.b * k0 + left.b * k1) + centre.b * k2) + right.b * k3) + down.b * k4) / a};
}

PPT_D float luminance(Rgb c) { return (0.299f * c.r + 0.587f * c.g) + 0.114f * c.b; }

PPT_D void store_resolved(const TaaBuffers &b, size_t i, Rgb v)
{
    const uint2 packed = make_uint2(float_to_half(v.r) | (float_to_half(v.g) << 16), float_to_half(v.b) | (0x3C00u << 16));
    b.resolved[i] = packed;
    // the HDR image holds what the stored texel holds
    if (b.hdr) b.hdr[i] = make_float4(half_to_float(packed.x & 0xFFFFu), half_to_float(packed.x >> 16), half_to_float(packed.y & 0xFFFFu), 1.0f);
}

template <uint32_t kIndex>
__global__ __launch_bounds__(256) void taa_resolve_kernel(uint32_t width, uint32_t height, TaaBuffers b)
{
    constexpr bool kIgnoreHistory = (kIndex & 1u) != 0u, kCatmullRom = ((kIndex >> 1) & 1u) != 0u, kLuminanceWeighting = ((kIndex >> 6) & 1u) != 0u;
    constexpr uint32_t kClipping = (kIndex >> 2) & 3u, kVelocity = (kIndex >> 4) & 3u;
    constexpr bool kStageIllumination = !kIgnoreHistory && kClipping != kClipNone;
    constexpr bool kStageVelocity = !kIgnoreHistory && kVelocity != kVelocityCenter;
    constexpr bool kStageDepth = !kIgnoreHistory && kVelocity == kVelocityClosest;
    __shared__ float4 sIllumination[kStageIllumination ? kHaloTexels : 1u];
    __shared__ float2 sVelocity[kStageVelocity ? kHaloTexels : 1u];
    __shared__ float sDepth[kStageDepth ? kHaloTexels : 1u];

    const int32_t w = (int32_t)width, h = (int32_t)height;
    const uint32_t tid = threadIdx.x, lx = tid & (kTileW - 1u), ly = tid / kTileW;
    const int32_t x0 = (int32_t)(blockIdx.x * kTileW), y0 = (int32_t)(blockIdx.y * kTileH);
    const int32_t x = x0 + (int32_t)lx, y = y0 + (int32_t)ly;

    if (kStageIllumination || kStageVelocity)
    {
        // tile texel (hx, hy) is the image texel (x0 - 1 + hx, y0 - 1 + hy) clamped to the edge
        for (uint32_t k = tid; k < kHaloTexels; k += 256u)
        {
            const int32_t gx = clamp_i(x0 - 1 + (int32_t)(k % kHaloW), 0, w - 1), gy = clamp_i(y0 - 1 + (int32_t)(k / kHaloW), 0, h - 1);
            const size_t g = (size_t)gy * width + (uint32_t)gx;
            if (kStageIllumination) sIllumination[k] = b.illumination[g];
            if (kStageVelocity) sVelocity[k] = b.velocity[g];
            if (kStageDepth) sDepth[k] = b.nonLinearDepth[g];
        }
        __syncthreads();
    }
    if (x >= w || y >= h) return;

    const size_t i = (size_t)y * width + (uint32_t)x;
    const uint32_t centre = (ly + 1u) * kHaloW + lx + 1u;
    const float4 in = kStageIllumination ? sIllumination[centre] : b.illumination[i];
    const Rgb illumination = Rgb{in.x, in.y, in.z};
    if (kIgnoreHistory)
    {
        store_resolved(b, i, illumination);
        return;
    }

    // sampleVelocity
    float2 velocity;
    if (kVelocity == kVelocityCenter)
        velocity = b.velocity[i];
    else if (kVelocity == kVelocityLargest)
    {
        float best = 0.0f;
        velocity = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int32_t ox = -1; ox <= 1; ++ox)
#pragma unroll
            for (int32_t oy = -1; oy <= 1; ++oy)
            {
                const float2 v = sVelocity[(uint32_t)((int32_t)centre + oy * (int32_t)kHaloW + ox)];
                const float lenSqr = v.x * v.x + v.y * v.y;
                if (best < lenSqr)
                {
                    velocity = v;
                    best = lenSqr;
                }
            }
    }
    else
    {
        float closest = 0.0f;
        uint32_t at = centre;
#pragma unroll
        for (int32_t ox = -1; ox <= 1; ++ox)
#pragma unroll
            for (int32_t oy = -1; oy <= 1; ++oy)
            {
                const uint32_t k = (uint32_t)((int32_t)centre + oy * (int32_t)kHaloW + ox);
                const float depth = sDepth[k];
                if (depth > closest)
                {
                    closest = depth;
                    at = k;
                }
            }
        velocity = sVelocity[at];
    }

    const float resX = (float)width, resY = (float)height;
    const float u = ((float)x + 0.5f) / resX, v = ((float)y + 0.5f) / resY;
    const float ru = u - velocity.x * 0.5f, rv = v - velocity.y * -0.5f;
    // any(notEqual(reprojectedUv, saturate(reprojectedUv))): 0 and 1 are inside, a NaN is not
    if (!(ru == saturate(ru)) || !(rv == saturate(rv)))
    {
        store_resolved(b, i, illumination);
        return;
    }

    const float cx = ru * resX - 0.5f, cy = rv * resY - 0.5f;
    const float wx = __builtin_floorf(cx), wy = __builtin_floorf(cy);
    const float fx = cx - wx, fy = cy - wy;
    const int32_t ix = (int32_t)wx, iy = (int32_t)wy;
    Rgb previous = kCatmullRom ? catmull_rom(b.history, w, h, ix, fx, iy, fy) : edge_bilinear(b.history, w, h, ix, fx, iy, fy);

    // clipColor
    if (kClipping == kClipMinMax)
    {
        Rgb lo = Rgb{9999.0f, 9999.0f, 9999.0f}, hi = Rgb{-9999.0f, -9999.0f, -9999.0f};
#pragma unroll
        for (int32_t ox = -1; ox <= 1; ++ox)
#pragma unroll
            for (int32_t oy = -1; oy <= 1; ++oy)
            {
                const float4 c = sIllumination[(uint32_t)((int32_t)centre + oy * (int32_t)kHaloW + ox)];
                lo = Rgb{fmin_(lo.r, c.x), fmin_(lo.g, c.y), fmin_(lo.b, c.z)};
                hi = Rgb{fmax_(hi.r, c.x), fmax_(hi.g, c.y), fmax_(hi.b, c.z)};
            }
        previous = Rgb{clamp_(previous.r, lo.r, hi.r), clamp_(previous.g, lo.g, hi.g), clamp_(previous.b, lo.b, hi.b)};
    }
    else if (kClipping == kClipVariance)
    {
        Rgb m1 = Rgb{0.0f, 0.0f, 0.0f}, m2 = Rgb{0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int32_t ox = -1; ox <= 1; ++ox)
#pragma unroll
            for (int32_t oy = -1; oy <= 1; ++oy)
            {
                const float4 c = sIllumination[(uint32_t)((int32_t)centre + oy * (int32_t)kHaloW + ox)];
                m1 = Rgb{m1.r + c.x, m1.g + c.y, m1.b + c.z};
                m2 = Rgb{m2.r + c.x * c.x, m2.g + c.y * c.y, m2.b + c.z * c.z};
            }
        const Rgb mu = Rgb{m1.r / 9.0f, m1.g / 9.0f, m1.b / 9.0f};
        // (the GLSL's argument goes negative on a flat neighbourhood: the max is the stated deviation)
        const Rgb sigma = Rgb{__builtin_sqrtf(fmax_(m2.r / 9.0f - mu.r * mu.r, 0.0f)), __builtin_sqrtf(fmax_(m2.g / 9.0f - mu.g * mu.g, 0.0f)),
                              __builtin_sqrtf(fmax_(m2.b / 9.0f - mu.b * mu.b, 0.0f))};
        previous = Rgb{clamp_(previous.r, mu.r - sigma.r, mu.r + sigma.r), clamp_(previous.g, mu.g - sigma.g, mu.g + sigma.g),
                       clamp_(previous.b, mu.b - sigma.b, mu.b + sigma.b)};
    }

    float currentWeight = 0.1f;
    float historyWeight = 1.0f - currentWeight;
    if (kLuminanceWeighting)
    {
        currentWeight *= 1.0f / (1.0f + luminance(illumination));
        historyWeight *= 1.0f / (1.0f + luminance(previous));
    }
    const float norm = fmax_(currentWeight + historyWeight, 0.00001f);
    store_resolved(b, i, Rgb{(illumination.r * currentWeight + previous.r * historyWeight) / norm,
                             (illumination.g * currentWeight + previous.g * historyWeight) / norm,
                             (illumination.b * currentWeight + previous.b * historyWeight) / norm});
}

__global__ __launch_bounds__(256) void taa_expand_kernel(uint32_t texels, const uint2 *__restrict__ resolved, float4 *__restrict__ hdr)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= texels) return;
    const uint2 p = resolved[i];
    hdr[i] = make_float4(half_to_float(p.x & 0xFFFFu), half_to_float(p.x >> 16), half_to_float(p.y & 0xFFFFu), half_to_float(p.y >> 16));
}

using ResolveKernel = void (*)(uint32_t, uint32_t, TaaBuffers);

// The pipelines TemporalAntiAliasing.cpp:67-110 creates: every index whose clipping and sampling fields name a type.
// IGNORE_HISTORY leaves nothing of the other constants in the shader, so its indices share one kernel.
template <uint32_t kIndex> constexpr ResolveKernel resolve_kernel_of()
{
    if constexpr (((kIndex >> 2) & 3u) == 3u || ((kIndex >> 4) & 3u) == 3u)
        return nullptr;
    else if constexpr ((kIndex & 1u) != 0u)
        return taa_resolve_kernel<1u>;
    else
        return taa_resolve_kernel<kIndex>;
}
template <uint32_t... kIndices> ResolveKernel resolve_kernel(uint32_t index, std::integer_sequence<uint32_t, kIndices...>)
{
    static const ResolveKernel table[] = {resolve_kernel_of<kIndices>()...};
    return index < sizeof...(kIndices) ? table[index] : nullptr;
}

} // namespace taa

using namespace taa;

bool launch_taa_resolve(
    uint32_t specializationIndex, uint32_t width, uint32_t height, const TaaBuffers &b, hipEvent_t *events, hipStream_t stream)
{
    const ResolveKernel kernel = resolve_kernel(specializationIndex, std::make_integer_sequence<uint32_t, kTaaSpecializations>());
    if (!kernel) return false;
    uint32_t e = 0;
    auto mark = [&]() {
        if (events) (void)hipEventRecord(events[e++], stream);
    };
    const bool inPlace = static_cast<const void *>(b.illumination) == static_cast<const void *>(b.hdr);
    TaaBuffers r = b;
    if (inPlace) r.hdr = nullptr;
    mark();
    hipLaunchKernelGGL(kernel, dim3((width + kTileW - 1u) / kTileW, (height + kTileH - 1u) / kTileH), dim3(256), 0, stream, width, height, r);
    mark();
    if (inPlace)
    {
        const uint32_t texels = width * height;
        hipLaunchKernelGGL(taa_expand_kernel, dim3((texels + 255u) / 256u), dim3(256), 0, stream, texels, b.resolved, b.hdr);
    }
    mark();
    return true;
}

} // namespace ppt
