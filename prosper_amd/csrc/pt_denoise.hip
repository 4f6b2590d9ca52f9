// pt_denoise.hip — gfx950 kernels of the spatiotemporal denoiser of the path-traced image.  prosper has
// no denoiser: the rule is this library's own, stated operation for operation in prosper_amd/denoise.py, and these
// kernels meet it bit for bit (float32, no contraction, only + - * / sqrt min max floor abs and comparisons).
//
//   denoise_temporal_kernel   the guide of this frame (view depth, its gradient, the decoded normal), the reprojected
//                             history blended with this frame's colour and luminance moments, the history length
//   denoise_variance_kernel   the variance: temporal where the history is 4 frames or longer, else re-estimated over 7 x 7
//   denoise_atrous_kernel     one edge-avoiding a-trous pass (5 x 5 B3, step 1 << i); the last one stores the HDR image
//   denoise_finish_kernel     the store to the HDR image when no a-trous pass runs
//
// One lane per pixel, blocks of 32 x 8 texels as in pt_taa.hip.  What a tap reads is three 16-byte records (colour +
// variance, z + gradient + flag, normal).  The a-trous passes at steps 1 and 2 stage the block's tile with a halo of 4
// texels in LDS (30 KB) and read every tap from there: measured 0.080 against 0.149 ms a pass on C2 at 1920 x 1080
// (DESIGN.md f28).  Elsewhere the taps are straight global loads: neighbouring lanes read neighbouring texels of the same
// tap offset, so every tap is a coalesced row segment and the reuse lands in L2.
#include "pt_denoise.hpp"

#include "pt_device.hpp"

namespace ppt
{

namespace denoise
{

constexpr uint32_t kTileW = 32, kTileH = 8;
constexpr float kMinAlbedo = 1.0f / 64.0f;

struct V3
{
    float x, y, z;
};

PPT_D float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
PPT_D float luminance(V3 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }
PPT_D bool finite3(V3 c) { return is_finite(c.x) && is_finite(c.y) && is_finite(c.z); }

// signedOctDecode (scene/material.glsl:20-32) of normalMetallic's x, y and w, with the dot product and the
// normalisation in the pinned order of this pass (no fused multiply-add)
PPT_D V3 decode_normal(float4 nm)
{
    V3 o;
    o.x = nm.x - nm.y;
    o.y = (nm.x + nm.y) - 1.0f;
    o.z = nm.w * 2.0f - 1.0f;
    o.z = o.z * ((1.0f - fabs_(o.x)) - fabs_(o.y));
    const float inv = 1.0f / __builtin_sqrtf(dot3(o, o));
    return V3{o.x * inv, o.y * inv, o.z * inv};
}

// linearize_depth's distance along the view direction: -viewZ, positive in front of the camera, which looks down -z
PPT_D float view_depth(const DenoiseParams &p, float nonLinearDepth) { return p.cameraToClip32 / (nonLinearDepth + p.cameraToClip22); }

// the forward or the backward difference, whichever is smaller in magnitude (ties: forward); 0 without a neighbour
PPT_D float depth_gradient(bool hasForward, float zForward, bool hasBackward, float zBackward, float z)
{
    const float f = zForward - z, k = z - zBackward;
    if (hasForward && hasBackward) return fabs_(k) < fabs_(f) ? k : f;
    if (hasForward) return f;
    if (hasBackward) return k;
    return 0.0f;
}

PPT_D bool is_geometry(float4 guideA) { return f2u(guideA.w) != 0u; }

// w_n F(x_z + xl) of the tap at the offset (ox, oy) texels from the centre (zp, gx, gy, np)
PPT_D float edge_weight(const DenoiseParams &p, float zp, float gx, float gy, V3 np, float4 qa, float4 qb, int32_t ox, int32_t oy, float xl)
{
    const float tx = gx * (float)ox, ty = gy * (float)oy;
    const float xz = fabs_(qa.x - ((zp + tx) + ty)) / (p.sigmaDepth * (fabs_(tx) + fabs_(ty)) + 1e-3f * zp);
    float wn = fmax_(0.0f, dot3(np, V3{qb.x, qb.y, qb.z}));
    for (uint32_t k = 0; k < p.normalPowerLog2; ++k) wn = wn * wn;
    const float t = fmax_(0.0f, 1.0f - (xz + xl) * 0.125f);
    const float t2 = t * t, t4 = t2 * t2;
    return wn * (t4 * t4);
}

__global__ __launch_bounds__(256) void denoise_temporal_kernel(DenoiseParams p, DenoiseBuffers b)
{
    const int32_t w = (int32_t)p.width, h = (int32_t)p.height;
    const int32_t x = (int32_t)(blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1u))), y = (int32_t)(blockIdx.y * kTileH + threadIdx.x / kTileW);
    const bool feedbackTemporal = p.feedbackIteration >= p.iterations;
    bool geometry = false, hasHistory = false;
    if (x < w && y < h)
    {
        const size_t i = (size_t)y * p.width + (uint32_t)x;
        const float depth = b.nonLinearDepth[i];
        geometry = depth != 0.0f;
        if (!geometry)
        {
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            b.temporal[i] = zero;
            b.next.moments[i] = zero;
            b.next.guideA[i] = zero;
            b.next.guideB[i] = zero;
            if (feedbackTemporal) b.next.colour[i] = zero;
        }
        else
        {
            const float z = view_depth(p, depth);
            float zl = 0.0f, zr = 0.0f, zu = 0.0f, zd = 0.0f;
            bool hl = false, hr = false, hu = false, hd = false;
            if (x > 0)
            {
                const float q = b.nonLinearDepth[i - 1u];
                hl = q != 0.0f;
                zl = view_depth(p, q);
            }
            if (x + 1 < w)
            {
                const float q = b.nonLinearDepth[i + 1u];
                hr = q != 0.0f;
                zr = view_depth(p, q);
            }
            if (y > 0)
            {
                const float q = b.nonLinearDepth[i - p.width];
                hu = q != 0.0f;
                zu = view_depth(p, q);
            }
            if (y + 1 < h)
            {
                const float q = b.nonLinearDepth[i + p.width];
                hd = q != 0.0f;
                zd = view_depth(p, q);
            }
            const float gx = depth_gradient(hr, zr, hl, zl, z), gy = depth_gradient(hd, zd, hu, zu, z);
            const V3 n = decode_normal(b.normalMetallic[i]);

            const float4 in = b.illumination[i];
            V3 c = V3{in.x, in.y, in.z};
            if (p.demodulate)
            {
                const float4 a = b.albedoRoughness[i];
                c = V3{c.x / fmax_(a.x, kMinAlbedo), c.y / fmax_(a.y, kMinAlbedo), c.z / fmax_(a.z, kMinAlbedo)};
            }
            const bool sample = finite3(c);
            const float l = luminance(c);

            // TAA's reprojection; the four taps of the bilinear footprint that lie inside and agree in depth and normal
            float sw = 0.0f, m1 = 0.0f, m2 = 0.0f;
            V3 prev = V3{0.0f, 0.0f, 0.0f};
            uint32_t length = 0u;
            if (!p.ignoreHistory)
            {
                const float2 velocity = b.velocity[i];
                const float resX = (float)p.width, resY = (float)p.height;
                const float u = ((float)x + 0.5f) / resX, v = ((float)y + 0.5f) / resY;
                const float ru = u - velocity.x * 0.5f, rv = v - velocity.y * -0.5f;
                const float cx = ru * resX - 0.5f, cy = rv * resY - 0.5f;
                // (a NaN fails; beyond this range no tap lies inside)
                if (cx >= -1.0f && cx <= resX && cy >= -1.0f && cy <= resY)
                {
                    const float wx = __builtin_floorf(cx), wy = __builtin_floorf(cy);
                    const float fx = cx - wx, fy = cy - wy;
                    const int32_t ix = (int32_t)wx, iy = (int32_t)wy;
                    const float weights[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
#pragma unroll
                    for (int32_t k = 0; k < 4; ++k)
                    {
                        const int32_t qx = ix + (k & 1), qy = iy + (k >> 1);
                        if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
                        const size_t q = (size_t)qy * p.width + (uint32_t)qx;
                        const float4 qa = b.previous.guideA[q];
                        if (!is_geometry(qa)) continue;
                        if (!(fabs_(qa.x - z) <= p.depthTolerance * fmax_(z, qa.x))) continue;
                        const float4 qb = b.previous.guideB[q];
                        if (!(dot3(V3{qb.x, qb.y, qb.z}, n) >= p.normalThreshold)) continue;
                        const float4 qc = b.previous.colour[q], qm = b.previous.moments[q];
                        const float wk = weights[k];
                        sw = sw + wk;
                        prev = V3{prev.x + wk * qc.x, prev.y + wk * qc.y, prev.z + wk * qc.z};
                        m1 = m1 + wk * qm.x;
                        m2 = m2 + wk * qm.y;
                        const uint32_t ql = f2u(qm.z);
                        length = ql > length ? ql : length;
                    }
                }
            }
            hasHistory = sw > 0.0f;
            V3 colour;
            if (hasHistory)
            {
                prev = V3{prev.x / sw, prev.y / sw, prev.z / sw};
                m1 = m1 / sw;
                m2 = m2 / sw;
                if (sample)
                {
                    length = length + 1u < p.maxHistoryLength ? length + 1u : p.maxHistoryLength;
                    const float alpha = fmax_(1.0f / (float)length, p.minAlpha), keep = 1.0f - alpha;
                    colour = V3{keep * prev.x + alpha * c.x, keep * prev.y + alpha * c.y, keep * prev.z + alpha * c.z};
                    m1 = keep * m1 + alpha * l;
                    m2 = keep * m2 + alpha * (l * l);
                }
                else
                {
                    // an invalid sample: the history as it is, the length not incremented
                    length = length < p.maxHistoryLength ? length : p.maxHistoryLength;
                    colour = prev;
                }
            }
            else if (sample)
            {
                length = 1u;
                colour = c;
                m1 = l;
                m2 = l * l;
            }
            else
            {
                length = 0u;
                colour = V3{0.0f, 0.0f, 0.0f};
                m1 = 0.0f;
                m2 = 0.0f;
            }
            const float4 out = make_float4(colour.x, colour.y, colour.z, fmax_(m2 - m1 * m1, 0.0f));
            b.temporal[i] = out;
            if (feedbackTemporal) b.next.colour[i] = out;
            b.next.moments[i] = make_float4(m1, m2, u2f(length), 0.0f);
            b.next.guideA[i] = make_float4(z, gx, gy, u2f(1u));
            b.next.guideB[i] = make_float4(n.x, n.y, n.z, 0.0f);
        }
    }
    // the counts of the info: one atomic per wave and counter (no lane has left: lane 0 of every wave is here)
    const unsigned long long with = __ballot(geometry && hasHistory), without = __ballot(geometry && !hasHistory);
    if ((threadIdx.x & 63u) == 0u)
    {
        if (with) atomicAdd(&b.counts[0], (uint32_t)__popcll(with));
        if (without) atomicAdd(&b.counts[1], (uint32_t)__popcll(without));
    }
}

__global__ __launch_bounds__(256) void denoise_variance_kernel(DenoiseParams p, DenoiseBuffers b)
{
    const int32_t w = (int32_t)p.width, h = (int32_t)p.height;
    const int32_t x = (int32_t)(blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1u))), y = (int32_t)(blockIdx.y * kTileH + threadIdx.x / kTileW);
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * p.width + (uint32_t)x;
    const float4 pa = b.next.guideA[i];
    if (!is_geometry(pa)) return;
    const float4 pm = b.next.moments[i];
    const uint32_t length = f2u(pm.z);
    if (length >= 4u) return; // the temporal variance stands
    const float4 pb = b.next.guideB[i];
    const V3 np = V3{pb.x, pb.y, pb.z};
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int32_t dy = -3; dy <= 3; ++dy)
        for (int32_t dx = -3; dx <= 3; ++dx)
        {
            float wk = 1.0f; // the centre
            float4 qm = pm;
            if (dx != 0 || dy != 0)
            {
                const int32_t qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
                const size_t q = (size_t)qy * p.width + (uint32_t)qx;
                const float4 qa = b.next.guideA[q];
                if (!is_geometry(qa)) continue;
                wk = edge_weight(p, pa.x, pa.y, pa.z, np, qa, b.next.guideB[q], dx, dy, 0.0f);
                qm = b.next.moments[q];
            }
            sw = sw + wk;
            s1 = s1 + wk * qm.x;
            s2 = s2 + wk * qm.y;
        }
    const float m1 = s1 / sw, m2 = s2 / sw;
    b.temporal[i].w = fmax_(m2 - m1 * m1, 0.0f) * (4.0f / (float)(length > 1u ? length : 1u));
}

// the stored texel: the filtered colour times the albedo it was divided by, the input's alpha; a sky texel as it came in
PPT_D void store_result(const DenoiseParams &p, const DenoiseBuffers &b, size_t i, bool geometry, float4 colour)
{
    const float4 in = b.illumination[i];
    if (!geometry)
    {
        if (static_cast<const void *>(b.hdr) != static_cast<const void *>(b.illumination)) b.hdr[i] = in;
        return;
    }
    if (p.demodulate)
    {
        const float4 a = b.albedoRoughness[i];
        colour = make_float4(colour.x * fmax_(a.x, kMinAlbedo), colour.y * fmax_(a.y, kMinAlbedo), colour.z * fmax_(a.z, kMinAlbedo), 0.0f);
    }
    b.hdr[i] = make_float4(colour.x, colour.y, colour.z, in.w);
}

// kLds (steps 1 and 2): the block's tile with a halo of 4 texels - 40 x 16 records of colour, guide A and guide B - is staged
// in LDS and every tap is read from there; a texel outside the image is staged with the flag 0, which skips it like the
// bounds test of the global path does.  The arithmetic is the same, operation for operation.
constexpr int32_t kHalo = 4, kLdsW = (int32_t)kTileW + 2 * kHalo, kLdsH = (int32_t)kTileH + 2 * kHalo, kLdsTexels = kLdsW * kLdsH;

template <bool kLds>
__global__ __launch_bounds__(256) void denoise_atrous_kernel(
    DenoiseParams p, DenoiseBuffers b, const float4 *in, float4 *out, float4 *feedback, int32_t step, uint32_t last)
{
    __shared__ float4 sC[kLds ? kLdsTexels : 1], sA[kLds ? kLdsTexels : 1], sB[kLds ? kLdsTexels : 1];
    const int32_t w = (int32_t)p.width, h = (int32_t)p.height;
    const int32_t lx = (int32_t)(threadIdx.x & (kTileW - 1u)), ly = (int32_t)(threadIdx.x / kTileW);
    const int32_t x0 = (int32_t)(blockIdx.x * kTileW), y0 = (int32_t)(blockIdx.y * kTileH);
    const int32_t x = x0 + lx, y = y0 + ly;
    if (kLds)
    {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int32_t k = (int32_t)threadIdx.x; k < kLdsTexels; k += 256)
        {
            const int32_t gx = x0 - kHalo + k % kLdsW, gy = y0 - kHalo + k / kLdsW;
            const bool inside = gx >= 0 && gy >= 0 && gx < w && gy < h;
            const size_t g = (size_t)(inside ? gy : 0) * p.width + (uint32_t)(inside ? gx : 0);
            sA[k] = inside ? b.next.guideA[g] : zero;
            sC[k] = inside ? in[g] : zero;
            sB[k] = inside ? b.next.guideB[g] : zero;
        }
        __syncthreads();
    }
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * p.width + (uint32_t)x;
    // guide A of the texel (ox, oy) away and where its other records are; outside the image: the flag 0
    const auto guide_a = [&](int32_t ox, int32_t oy, size_t &q) -> float4 {
        if (kLds)
        {
            q = (size_t)((ly + kHalo + oy) * kLdsW + lx + kHalo + ox);
            return sA[q];
        }
        const int32_t qx = x + ox, qy = y + oy;
        if (qx < 0 || qy < 0 || qx >= w || qy >= h) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        q = (size_t)qy * p.width + (uint32_t)qx;
        return b.next.guideA[q];
    };
    const auto colour = [&](size_t q) -> float4 { return kLds ? sC[q] : in[q]; };
    const auto guide_b = [&](size_t q) -> float4 { return kLds ? sB[q] : b.next.guideB[q]; };
    size_t centre = 0;
    const float4 pa = guide_a(0, 0, centre);
    const float4 pc = colour(centre);
    float4 result = pc; // (a sky texel passes through; it is nobody's tap)
    const bool geometry = is_geometry(pa);
    if (geometry)
    {
        // the centre's terms, once
        float gw = 0.0f, gv = 0.0f;
        for (int32_t dy = -1; dy <= 1; ++dy)
            for (int32_t dx = -1; dx <= 1; ++dx)
            {
                size_t q = 0;
                if (!is_geometry(guide_a(dx, dy, q))) continue;
                const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
                gw = gw + k;
                gv = gv + k * colour(q).w;
            }
        const float denomL = p.sigmaLuminance * __builtin_sqrtf(gv / gw) + 1e-4f;
        const float lp = luminance(V3{pc.x, pc.y, pc.z});
        const float4 pb = guide_b(centre);
        const V3 np = V3{pb.x, pb.y, pb.z};

        float sw = 0.0f, sv = 0.0f;
        V3 sc = V3{0.0f, 0.0f, 0.0f};
        for (int32_t dy = -2; dy <= 2; ++dy)
            for (int32_t dx = -2; dx <= 2; ++dx)
            {
                const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
                const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f);
                float wk = hx * hy; // the centre: w_n = F = 1
                float4 qc = pc;
                if (dx != 0 || dy != 0)
                {
                    const int32_t ox = step * dx, oy = step * dy;
                    size_t q = 0;
                    const float4 qa = guide_a(ox, oy, q);
                    if (!is_geometry(qa)) continue;
                    qc = colour(q);
                    const float xl = fabs_(luminance(V3{qc.x, qc.y, qc.z}) - lp) / denomL;
                    wk = wk * edge_weight(p, pa.x, pa.y, pa.z, np, qa, guide_b(q), ox, oy, xl);
                }
                sw = sw + wk;
                sc = V3{sc.x + wk * qc.x, sc.y + wk * qc.y, sc.z + wk * qc.z};
                sv = sv + (wk * wk) * qc.w;
            }
        result = make_float4(sc.x / sw, sc.y / sw, sc.z / sw, sv / (sw * sw));
    }
    out[i] = result;
    if (feedback) feedback[i] = result;
    if (last) store_result(p, b, i, geometry, result);
}

__global__ __launch_bounds__(256) void denoise_finish_kernel(DenoiseParams p, DenoiseBuffers b)
{
    const uint32_t texels = p.width * p.height, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= texels) return;
    store_result(p, b, i, is_geometry(b.next.guideA[i]), b.temporal[i]);
}

} // namespace denoise

using namespace denoise;

void launch_denoise(const DenoiseParams &p, const DenoiseBuffers &b, hipEvent_t *events, hipStream_t stream)
{
    uint32_t e = 0;
    auto mark = [&]() {
        if (events) (void)hipEventRecord(events[e++], stream);
    };
    const dim3 grid((p.width + kTileW - 1u) / kTileW, (p.height + kTileH - 1u) / kTileH), block(256);
    (void)hipMemsetAsync(b.counts, 0, 2u * sizeof(uint32_t), stream);
    mark();
    hipLaunchKernelGGL(denoise_temporal_kernel, grid, block, 0, stream, p, b);
    mark();
    hipLaunchKernelGGL(denoise_variance_kernel, grid, block, 0, stream, p, b);
    mark();
    const float4 *in = b.temporal;
    for (uint32_t k = 0; k < kDenoiseMaxIterations; ++k)
    {
        if (k < p.iterations)
        {
            float4 *out = b.pingPong[k & 1u];
            // steps 1 and 2 reach no further than the halo: those passes read their taps from LDS
            const auto kernel = (1 << k) * 2 <= kHalo ? denoise_atrous_kernel<true> : denoise_atrous_kernel<false>;
            hipLaunchKernelGGL(kernel, grid, block, 0, stream, p, b, in, out, k == p.feedbackIteration ? b.next.colour : nullptr,
                               (int32_t)(1u << k), k + 1u == p.iterations ? 1u : 0u);
            in = out;
        }
        mark();
    }
    if (p.iterations == 0u)
    {
        const uint32_t texels = p.width * p.height;
        hipLaunchKernelGGL(denoise_finish_kernel, dim3((texels + 255u) / 256u), block, 0, stream, p, b);
    }
    mark();
}

} // namespace ppt
