// pt_debug_view.hip — gfx950 kernels of prosper's inspection passes.
//
//   debug_lines_raster_kernel   debug_lines.vert + clipping + line rasterisation + the depth test: one wave per line,
//                               its lanes take consecutive major-axis steps; a 64-bit atomic maximum per fragment
//   debug_lines_resolve_kernel  colour and depth where a key was left; zeroes the key
//   texture_readback_kernel     texture_readback.comp: one nearest clamp-to-edge texel of a registry image
//   texture_debug_kernel        texture_debug.comp as it is compiled: one lane per output texel of the viewer
//
// Vulkan leaves the fragments of a non-strict line to the implementation, so the rule here is the library's own and
// tests/debug_view_reference.py restates it operation by operation (float32, -ffp-contract=off: the only fused
// operations are the fmaf chains of the two matrix products, and the viewer's bilinear blend).
#include "pt_debug_view.hpp"

#include "pt_math.hpp"

namespace ppt
{

namespace
{

#define PPT_DV __device__ __forceinline__

// row `row` of m * (x, y, z, 1), as pt_particles.hip's clip_row
PPT_DV float row_point(const float *m, uint32_t row, float x, float y, float z)
{
    return __builtin_fmaf(m[8 + row], z, __builtin_fmaf(m[4 + row], y, __builtin_fmaf(m[row], x, m[12 + row])));
}

// row `row` of m * v
PPT_DV float row_vec(const float *m, uint32_t row, const float *v)
{
    return __builtin_fmaf(m[12 + row], v[3], __builtin_fmaf(m[8 + row], v[2], __builtin_fmaf(m[4 + row], v[1], m[row] * v[0])));
}

PPT_DV bool finite_(float v) { return fabs_(v) <= 3.402823466e+38f; }

// the distance of a clip-space point to plane k of Vulkan's volume: -w <= x, y <= w, 0 <= z <= w
PPT_DV float plane_distance(const float *c, uint32_t k)
{
    switch (k)
    {
    case 0: return c[3] + c[0];
    case 1: return c[3] - c[0];
    case 2: return c[3] + c[1];
    case 3: return c[3] - c[1];
    case 4: return c[2];
    default: return c[3] - c[2];
    }
}

// What a line's walk needs: the same in every lane of its wave
struct LineWalk
{
    bool clippedAway; // a non-finite endpoint or an empty interval: never walked
    bool xMajor;
    int32_t first, step; // major-axis pixel of step 0, +1 or -1
    uint32_t steps;      // <= max(width, height)
    float m0, dm;        // major coordinate of the start, and end - start
    float n0, dn;        // minor
    float z0, dz;        // z / w
};

// clip endpoint -> framebuffer x, y and depth; false: not usable
PPT_DV bool to_screen(const float *c, float width, float height, float &sx, float &sy, float &sz)
{
    const float w = c[3];
    if (!(w > 0.0f)) return false;
    sx = ((c[0] / w) * 0.5f + 0.5f) * width;
    sy = ((c[1] / w) * 0.5f + 0.5f) * height;
    sz = c[2] / w;
    if (!(finite_(sx) && finite_(sy) && finite_(sz))) return false;
    // the clipped point lies in the viewport up to rounding: the walk below is derived from the bounded point
    sx = clamp_(sx, 0.0f, width);
    sy = clamp_(sy, 0.0f, height);
    sz = clamp_(sz, 0.0f, 1.0f);
    return true;
}

PPT_DV LineWalk set_up_line(const DebugLinesParams &p, uint32_t line)
{
    LineWalk lw = {};
    lw.clippedAway = true;
    const float *l = p.lines + (size_t)line * kDebugLineFloats;
    float c0[4], c1[4];
    {
        float v0[4], v1[4];
        for (uint32_t r = 0; r < 4u; ++r)
        {
            v0[r] = row_point(p.worldToCamera, r, l[0], l[1], l[2]);
            v1[r] = row_point(p.worldToCamera, r, l[3], l[4], l[5]);
        }
        for (uint32_t r = 0; r < 4u; ++r)
        {
            c0[r] = row_vec(p.cameraToClip, r, v0);
            c1[r] = row_vec(p.cameraToClip, r, v1);
        }
    }
    for (uint32_t r = 0; r < 4u; ++r)
        if (!(finite_(c0[r]) && finite_(c1[r]))) return lw;

    // Liang-Barsky in homogeneous space
    float t0 = 0.0f, t1 = 1.0f;
    for (uint32_t k = 0; k < 6u; ++k)
    {
        const float d0 = plane_distance(c0, k), d1 = plane_distance(c1, k);
        if (d0 < 0.0f && d1 < 0.0f) return lw;
        if (d0 < 0.0f)
            t0 = fmax_(t0, d0 / (d0 - d1));
        else if (d1 < 0.0f)
            t1 = fmin_(t1, d0 / (d0 - d1));
    }
    if (!(t0 <= t1)) return lw;
    float a[4], b[4];
    for (uint32_t r = 0; r < 4u; ++r)
    {
        const float d = c1[r] - c0[r];
        a[r] = t0 > 0.0f ? c0[r] + t0 * d : c0[r];
        b[r] = t1 < 1.0f ? c0[r] + t1 * d : c1[r];
    }
    const float width = (float)p.width, height = (float)p.height;
    float ax, ay, az, bx, by, bz;
    if (!to_screen(a, width, height, ax, ay, az) || !to_screen(b, width, height, bx, by, bz)) return lw;
    lw.clippedAway = false;

    const float dx = bx - ax, dy = by - ay;
    lw.xMajor = fabs_(dx) >= fabs_(dy);
    const float m1 = lw.xMajor ? bx : by;
    lw.m0 = lw.xMajor ? ax : ay;
    lw.dm = lw.xMajor ? dx : dy;
    lw.n0 = lw.xMajor ? ay : ax;
    lw.dn = lw.xMajor ? dy : dx;
    lw.z0 = az;
    lw.dz = bz - az;
    // the pixel centres k + 0.5 in [m0, m1) going up, in (m1, m0] going down: half-open from start to end
    int32_t steps = 0;
    if (m1 > lw.m0)
    {
        lw.first = (int32_t)__builtin_ceilf(lw.m0 - 0.5f);
        lw.step = 1;
        steps = (int32_t)__builtin_ceilf(m1 - 0.5f) - lw.first;
    }
    else if (m1 < lw.m0)
    {
        lw.first = (int32_t)__builtin_floorf(lw.m0 - 0.5f);
        lw.step = -1;
        steps = lw.first - (int32_t)__builtin_floorf(m1 - 0.5f);
    }
    const int32_t most = (int32_t)(p.width > p.height ? p.width : p.height);
    steps = steps < 0 ? 0 : steps;
    lw.steps = (uint32_t)(steps > most ? most : steps);
    return lw;
}

} // namespace

__global__ __launch_bounds__(256) void debug_lines_raster_kernel(DebugLinesParams p)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t line = blockIdx.x * kDebugLinesPerBlock + (threadIdx.x >> 6);
    if (line >= p.count) return;
    const LineWalk lw = set_up_line(p, line);
    if (lw.clippedAway)
    {
        if (lane == 0u) atomicAdd(&p.stats->linesClippedAway, 1u);
        return;
    }
    const int32_t majorExtent = (int32_t)(lw.xMajor ? p.width : p.height);
    const int32_t minorExtent = (int32_t)(lw.xMajor ? p.height : p.width);
    // BOUNDED: lw.steps comes from the clipped endpoints clamped to the viewport and is capped at max(width, height),
    // whatever the line's endpoints were; a lane takes every 64th step, so it loops at most max(width, height) / 64 + 1 times.
    for (uint32_t j = lane; j < lw.steps; j += 64u)
    {
        const int32_t k = lw.first + lw.step * (int32_t)j;
        if (k < 0 || k >= majorExtent) continue;
        const float t = (((float)k + 0.5f) - lw.m0) / lw.dm;
        int32_t q = (int32_t)__builtin_floorf(lw.n0 + t * lw.dn);
        q = q < 0 ? 0 : (q > minorExtent - 1 ? minorExtent - 1 : q);
        const float depth = clamp_(lw.z0 + t * lw.dz, 0.0f, 1.0f);
        const size_t pixel = lw.xMajor ? (size_t)q * p.width + (size_t)k : (size_t)k * p.width + (size_t)q;
        if (!(depth > p.nonLinearDepth[pixel])) continue; // reverse-Z eGreater against the stored depth: equal loses
        // the nearest fragment wins, among equal depths the higher line index (a passing depth is > 0: the key is not 0)
        atomicMax(p.keys + pixel, ((unsigned long long)f2u(depth) << 32) | (unsigned long long)line);
    }
}

__global__ __launch_bounds__(256) void debug_lines_resolve_kernel(DebugLinesParams p)
{
    const size_t pixel = (size_t)blockIdx.x * 256u + threadIdx.x;
    bool wrote = false;
    if (pixel < (size_t)p.width * p.height)
    {
        const unsigned long long key = p.keys[pixel];
        if (key != 0ull)
        {
            const uint32_t line = (uint32_t)key;
            if (line < p.count)
            {
                const float *c = p.lines + (size_t)line * kDebugLineFloats + 6u;
                p.hdr[pixel] = make_float4(c[0], c[1], c[2], 1.0f);
                p.nonLinearDepth[pixel] = u2f((uint32_t)(key >> 32));
                wrote = true;
            }
            p.keys[pixel] = 0ull;
        }
    }
    const unsigned long long mask = __ballot(wrote);
    if (mask != 0ull && (int32_t)(threadIdx.x & 63u) == (int32_t)__ffsll((long long)mask) - 1)
        atomicAdd(&p.stats->fragmentsWritten, (uint32_t)__popcll(mask));
}

// ---- texture readback ----

// Texel `i` of an image of `format` as Vulkan returns it: missing components are (0, 0, 1), fp16 decodes exactly,
// UNORM codes are divided by 65535 or 255
static PPT_DV float4 load_texel(const void *image, uint32_t format, size_t i)
{
    switch (format)
    {
    case PROSPER_PT_DEBUG_FORMAT_RGBA32F: return static_cast<const float4 *>(image)[i];
    case PROSPER_PT_DEBUG_FORMAT_RG32F:
    {
        const float2 v = static_cast<const float2 *>(image)[i];
        return make_float4(v.x, v.y, 0.0f, 1.0f);
    }
    case PROSPER_PT_DEBUG_FORMAT_R32F: return make_float4(static_cast<const float *>(image)[i], 0.0f, 0.0f, 1.0f);
    case PROSPER_PT_DEBUG_FORMAT_RGBA16F:
    {
        const uint2 v = static_cast<const uint2 *>(image)[i];
        return make_float4(half_to_float(v.x & 0xFFFFu), half_to_float(v.x >> 16), half_to_float(v.y & 0xFFFFu), half_to_float(v.y >> 16));
    }
    case PROSPER_PT_DEBUG_FORMAT_RG16F:
    {
        const uint32_t v = static_cast<const uint32_t *>(image)[i];
        return make_float4(half_to_float(v & 0xFFFFu), half_to_float(v >> 16), 0.0f, 1.0f);
    }
    case PROSPER_PT_DEBUG_FORMAT_R16F: return make_float4(half_to_float(static_cast<const uint16_t *>(image)[i]), 0.0f, 0.0f, 1.0f);
    case PROSPER_PT_DEBUG_FORMAT_RG16_UNORM:
    {
        const uint32_t v = static_cast<const uint32_t *>(image)[i];
        return make_float4((float)(v & 0xFFFFu) / 65535.0f, (float)(v >> 16) / 65535.0f, 0.0f, 1.0f);
    }
    default: // RGBA8_UNORM
    {
        const uint32_t v = static_cast<const uint32_t *>(image)[i];
        return make_float4((float)(v & 0xFFu) / 255.0f, (float)((v >> 8) & 0xFFu) / 255.0f, (float)((v >> 16) & 0xFFu) / 255.0f,
                           (float)(v >> 24) / 255.0f);
    }
    }
}

// clamp(floor(u * extent), 0, extent - 1) of u = px / extent; the caller passes finite coordinates
static PPT_DV uint32_t nearest_texel(float px, uint32_t extent)
{
    const float e = (float)extent;
    const float t = __builtin_floorf((px / e) * e);
    if (!(t >= 0.0f)) return 0u;
    return t >= e ? extent - 1u : (uint32_t)t;
}

__global__ void texture_readback_kernel(TextureReadbackParams p)
{
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const uint32_t x = nearest_texel(p.pxX, p.width), y = nearest_texel(p.pxY, p.height);
    *p.out = load_texel(p.image, p.format, (size_t)y * p.width + x);
}

void launch_texture_readback(const TextureReadbackParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(texture_readback_kernel, dim3(1), dim3(64), 0, stream, p);
}

// ---- texture debug (texture_debug.comp as it is compiled: the magnifier's warp is commented out there and stays out) ----

// the shader's flag bits
PPT_DV uint32_t viewer_channel(uint32_t flags) { return flags & 7u; }
PPT_DV bool viewer_abs(uint32_t flags) { return (flags >> 3) & 1u; }
PPT_DV bool viewer_zoom(uint32_t flags) { return (flags >> 4) & 1u; }
PPT_DV bool viewer_magnifier(uint32_t flags) { return (flags >> 5) & 1u; }

// aspectCorrectedUv / unAspectCorrectedUv: in = inRes() at the lod, out = outRes
PPT_DV void aspect_corrected_uv(float &u, float &v, int32_t inW, int32_t inH, int32_t outW, int32_t outH, bool undo)
{
    if (inW == outW && inH == outH) return;
    const float inAspect = (float)inW / (float)inH;
    const float outAspect = (float)outW / (float)outH;
    const bool tall = inAspect > outAspect;
    const float scale = tall ? inAspect / outAspect : outAspect / inAspect;
    const float shift = (scale - 1.0f) * 0.5f;
    float &c = tall ? v : u;
    c = undo ? (c + shift) / scale : c * scale - shift;
}

// textureLod with clamp-to-edge over one level: nearest is clamp(floor(u * W), 0, W - 1); bilinear takes u * W - 0.5,
// its floor, and the unquantised float32 fraction, blended in the order of pt_ibl.hpp's LUT lookup
static PPT_DV float4 viewer_sample(const TextureDebugParams &p, float u, float v, bool bilinear)
{
    const int32_t w = (int32_t)p.levelW, h = (int32_t)p.levelH;
    const auto clampi = [](int32_t i, int32_t n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); };
    if (!bilinear)
    {
        const int32_t x = clampi(f2i(__builtin_floorf(u * (float)w)), w), y = clampi(f2i(__builtin_floorf(v * (float)h)), h);
        return load_texel(p.image, p.format, (size_t)y * p.levelW + (size_t)x);
    }
    const float cu = u * (float)w - 0.5f, cv = v * (float)h - 0.5f;
    const float fu = __builtin_floorf(cu), fv = __builtin_floorf(cv);
    const float a = cu - fu, b = cv - fv;
    const int32_t i0 = f2i(fu), j0 = f2i(fv);
    const int32_t ia = clampi(i0, w), ib = clampi(i0 + 1, w), ja = clampi(j0, h), jb = clampi(j0 + 1, h);
    const float4 t00 = load_texel(p.image, p.format, (size_t)ja * p.levelW + (size_t)ia);
    const float4 t10 = load_texel(p.image, p.format, (size_t)ja * p.levelW + (size_t)ib);
    const float4 t01 = load_texel(p.image, p.format, (size_t)jb * p.levelW + (size_t)ia);
    const float4 t11 = load_texel(p.image, p.format, (size_t)jb * p.levelW + (size_t)ib);
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    const auto blend = [&](float c00, float c10, float c01, float c11) {
        return __builtin_fmaf(w11, c11, __builtin_fmaf(w01, c01, __builtin_fmaf(w10, c10, w00 * c00)));
    };
    return make_float4(blend(t00.x, t10.x, t01.x, t11.x), blend(t00.y, t10.y, t01.y, t11.y), blend(t00.z, t10.z, t01.z, t11.z),
                       blend(t00.w, t10.w, t01.w, t11.w));
}

// tone_map_kernel's float -> UNORM8 (NaN stores 0)
PPT_DV uint32_t viewer_unorm8(float x) { return (uint32_t)__builtin_rintf(clamp_(x, 0.0f, 1.0f) * 255.0f); }

__global__ __launch_bounds__(256) void texture_debug_kernel(TextureDebugParams p)
{
    const uint32_t outW = (uint32_t)p.pc.outRes[0], outH = (uint32_t)p.pc.outRes[1];
    const size_t texel = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (texel >= (size_t)outW * outH) return;
    const uint32_t ox = (uint32_t)(texel % outW), oy = (uint32_t)(texel / outW);
    const int32_t inW = (int32_t)p.levelW, inH = (int32_t)p.levelH; // inRes() = max(inRes / (1 << lod), 1): the level's extent
    const uint32_t flags = p.pc.flags;
    const float fOutW = (float)outW, fOutH = (float)outH;

    float u = ((float)ox + 0.5f) / fOutW, v = ((float)oy + 0.5f) / fOutH;
    aspect_corrected_uv(u, v, inW, inH, (int32_t)outW, (int32_t)outH, false);
    if (viewer_zoom(flags)) u = u * 0.25f + 0.375f, v = v * 0.25f + 0.375f;

    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (u >= 0.0f && v >= 0.0f && u <= 1.0f && v <= 1.0f)
    {
        const float4 s = viewer_sample(p, u, v, p.bilinear != 0u);
        const uint32_t channel = viewer_channel(flags);
        if (channel > 3u)
            r = s.x, g = s.y, b = s.z;
        else
            r = g = b = channel == 0u ? s.x : (channel == 1u ? s.y : (channel == 2u ? s.z : s.w));
    }
    if (viewer_abs(flags)) r = fabs_(r), g = fabs_(g), b = fabs_(b);
    const float lo = p.pc.range[0], span = p.pc.range[1] - p.pc.range[0];
    r = (r - lo) / span, g = (g - lo) / span, b = (b - lo) / span;

    if (viewer_magnifier(flags))
    {
        // the sample point snapped to the nearest input texel centre
        float su = p.pc.cursorUv[0], sv = p.pc.cursorUv[1];
        aspect_corrected_uv(su, sv, inW, inH, (int32_t)outW, (int32_t)outH, false);
        if (viewer_zoom(flags)) su = su * 0.25f + 0.375f, sv = sv * 0.25f + 0.375f;
        su = (__builtin_floorf(su * (float)inW) + 0.5f) / (float)inW;
        sv = (__builtin_floorf(sv * (float)inH) + 0.5f) / (float)inH;
        if (texel == 0u)
        {
            if (su >= 0.0f && sv >= 0.0f && su < 1.0f && sv < 1.0f)
                *p.peek = viewer_sample(p, su, sv, false);
            else
                *p.peek = make_float4(kInf, kInf, kInf, kInf);
        }
        // the cursor snapped in output resolution
        float cu = su, cv = sv;
        if (viewer_zoom(flags)) cu = (cu - 0.375f) * 4.0f, cv = (cv - 0.375f) * 4.0f;
        aspect_corrected_uv(cu, cv, inW, inH, (int32_t)outW, (int32_t)outH, true);
        const float dx = fabs_(cu * fOutW - (float)ox), dy = fabs_(cv * fOutH - (float)oy);
        if (dx < 3.0f && dy < 3.0f) r = g = b = 0.0f;
        if (dx < 2.0f && dy < 2.0f) r = g = b = 1.0f;
    }
    p.out[texel] = viewer_unorm8(r) | (viewer_unorm8(g) << 8) | (viewer_unorm8(b) << 16) | (255u << 24);
}

void launch_texture_debug(const TextureDebugParams &p, hipStream_t stream)
{
    const size_t texels = (size_t)p.pc.outRes[0] * (size_t)p.pc.outRes[1];
    if (texels == 0u) return;
    hipLaunchKernelGGL(texture_debug_kernel, dim3((uint32_t)((texels + 255u) / 256u)), dim3(256), 0, stream, p);
}

void launch_debug_lines(const DebugLinesParams &p, hipStream_t stream)
{
    if (p.count == 0u || p.width == 0u || p.height == 0u) return;
    const uint32_t blocks = (p.count + kDebugLinesPerBlock - 1u) / kDebugLinesPerBlock;
    hipLaunchKernelGGL(debug_lines_raster_kernel, dim3(blocks), dim3(256), 0, stream, p);
    const size_t pixels = (size_t)p.width * p.height;
    hipLaunchKernelGGL(debug_lines_resolve_kernel, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), 0, stream, p);
}

} // namespace ppt
