// pt_dof.hip — gfx950 kernels of the skybox fill (SkyboxRenderer, skybox.vert / .frag) and of depth of field
// (src/render/dof/*, res/shader/dof/*: seven compute passes after Abadie's "A Life of a Bokeh").
//
//   skybox_fill_kernel    (sample_skybox(primary ray of the pixel centre), 1) wherever the depth is the miss value 0
//   dof_setup_kernel      setup.comp: half-resolution colour (bilateral mean of four) and circle of confusion (min of four)
//   dof_reduce_kernel     reduce.comp, levels 1-6: one block per 64 x 64 source tile, every level from the unrounded one below
//   dof_reduce_tail_kernel  levels 7 and up: one block, each level from the stored one below
//   dof_flatten_kernel    flatten.comp: min / max CoC of every 8 x 8 tile, one wave per tile
//   dof_dilate_kernel     dilate.comp: the tiles' min / max spread over the tiles their circles reach
//   dof_gather_kernel     gather.comp, foreground or background: 121 octaweb taps per texel, one wave per tile
//   dof_filter_kernel     filter.comp: 3 x 3 median by luminance
//   dof_combine_kernel    combine.comp: both layers over the full-resolution image
//
// Images have no sampler here: a nearest lookup is a clamped index, the trilinear lookup of the gather is written out.
#include "pt_dof.hpp"

#include <cmath>

#include "pt_device.hpp"

namespace ppt
{

constexpr float kDofPi = 3.14159265f;               // PI of common/math.glsl, which sampleAlpha uses
constexpr float kDofSinglePixelRadius = 0.7071f;    // DOF_SINGLE_PIXEL_RADIUS

PPT_D f4 unpack_rgba16f(uint2 p)
{
    return f4{half_to_float(p.x & 0xFFFFu), half_to_float(p.x >> 16), half_to_float(p.y & 0xFFFFu), half_to_float(p.y >> 16)};
}
PPT_D uint2 pack_rgba16f(float r, float g, float b, float a)
{
    return make_uint2(float_to_half(r) | (float_to_half(g) << 16), float_to_half(b) | (float_to_half(a) << 16));
}
PPT_D uint32_t level_width(const DofParams &p, uint32_t l) { return (p.hw >> l) ? (p.hw >> l) : 1u; }
PPT_D uint32_t level_height(const DofParams &p, uint32_t l) { return (p.hh >> l) ? (p.hh >> l) : 1u; }
PPT_D uint32_t min_u(uint32_t a, uint32_t b) { return a < b ? a : b; }
PPT_D int32_t clamp_i(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bilateral.glsl: the weight of a sample whose CoC is `sampleCoC` in an output of CoC `outputCoC`
PPT_D float bilateral_weight(float outputCoC, float sampleCoC) { return saturate(1.0f - (outputCoC - sampleCoC)); }

// bilateralFilter of bilateral.glsl over (rgb, coc) inputs in the order 01, 11, 10, 00
PPT_D f4 bilateral_filter(f4 v01, f4 v11, f4 v10, f4 v00)
{
    const float cocOut = fmin_(fmin_(v01.w, v11.w), fmin_(v10.w, v00.w));
    const float w01 = bilateral_weight(cocOut, v01.w), w11 = bilateral_weight(cocOut, v11.w);
    const float w10 = bilateral_weight(cocOut, v10.w), w00 = bilateral_weight(cocOut, v00.w);
    const float norm = ((w01 + w11) + w10) + w00;
    return f4{(((w01 * v01.x + w11 * v11.x) + w10 * v10.x) + w00 * v00.x) / norm,
              (((w01 * v01.y + w11 * v11.y) + w10 * v10.y) + w00 * v00.y) / norm,
              (((w01 * v01.z + w11 * v11.z) + w10 * v10.z) + w00 * v00.z) / norm,
              (((w01 * v01.w + w11 * v11.w) + w10 * v10.w) + w00 * v00.w) / norm};
}

// ---- skybox fill ----

__global__ __launch_bounds__(256) void skybox_fill_kernel(
    DeviceScene s, RenderParams r, const float *__restrict__ nonLinearDepth, float4 *__restrict__ hdr)
{
    const uint32_t px = blockIdx.x * 64u + (threadIdx.x & 63u), py = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (px >= r.width || py >= r.height) return;
    const size_t i = (size_t)py * r.width + px;
    if (nonLinearDepth[i] != 0.0f) return;
    const f2 uv = f2{((float)px + 0.5f) / (float)r.width, ((float)py + 0.5f) / (float)r.height};
    const f3 c = sample_skybox(s, pinhole_camera_ray(r, uv).d);
    hdr[i] = make_float4(c.x, c.y, c.z, 1.0f);
}

// ---- setup ----

PPT_D float circle_of_confusion(const DofParams &p, float nonLinearDepth)
{
    // linearize_depth of the G-buffer passes; the camera looks down -z
    const float viewZ = -p.cameraToClip32 / (nonLinearDepth + p.cameraToClip22);
    return fmax_((1.0f - p.focusDistance / (-viewZ)) * p.maxBackgroundCoC, -p.maxCoC);
}

__global__ __launch_bounds__(256) void dof_setup_kernel(DofParams p, DofBuffers b)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= p.hw || y >= p.hh) return;
    const uint32_t x0 = min_u(2u * x, p.width - 1u), x1 = min_u(2u * x + 1u, p.width - 1u);
    const uint32_t y0 = min_u(2u * y, p.height - 1u), y1 = min_u(2u * y + 1u, p.height - 1u);
    const size_t i01 = (size_t)y1 * p.width + x0, i11 = (size_t)y1 * p.width + x1;
    const size_t i10 = (size_t)y0 * p.width + x1, i00 = (size_t)y0 * p.width + x0;
    const float4 c01 = b.illumination[i01], c11 = b.illumination[i11], c10 = b.illumination[i10], c00 = b.illumination[i00];
    const f4 v01 = f4{c01.x, c01.y, c01.z, circle_of_confusion(p, b.nonLinearDepth[i01])};
    const f4 v11 = f4{c11.x, c11.y, c11.z, circle_of_confusion(p, b.nonLinearDepth[i11])};
    const f4 v10 = f4{c10.x, c10.y, c10.z, circle_of_confusion(p, b.nonLinearDepth[i10])};
    const f4 v00 = f4{c00.x, c00.y, c00.z, circle_of_confusion(p, b.nonLinearDepth[i00])};
    const f4 o = bilateral_filter(v01, v11, v10, v00);
    const size_t i = (size_t)y * p.hw + x;
    b.halfIllumination[i] = pack_rgba16f(o.x, o.y, o.z, 1.0f);
    b.halfCoC[i] = (uint16_t)float_to_half(fmin_(fmin_(v01.w, v11.w), fmin_(v10.w, v00.w)));
}

// ---- reduce ----

struct Rgb
{
    float r, g, b;
};
// the mean of four (every stored alpha is 1, so bilateralFilter weighs them equally)
PPT_D Rgb mean4(Rgb a, Rgb b, Rgb c, Rgb d)
{
    return Rgb{(((a.r + b.r) + c.r) + d.r) * 0.25f, (((a.g + b.g) + c.g) + d.g) * 0.25f, (((a.b + b.b) + c.b) + d.b) * 0.25f};
}
PPT_D void store_level(const DofParams &p, uint2 *mips, uint32_t l, uint32_t x, uint32_t y, Rgb v)
{
    if (l >= p.levels || x >= level_width(p, l) || y >= level_height(p, l)) return;
    mips[p.levelOffset[l] + (size_t)y * level_width(p, l) + x] = pack_rgba16f(v.r, v.g, v.b, 1.0f);
}

// One block per 64 x 64 tile of virtual level-0 texels (the source clamped to its edge).  Level k is the mean of four
// unrounded level k - 1 texels, texels past that level's extent included; only texels inside level k's extent are stored.
__global__ __launch_bounds__(256) void dof_reduce_kernel(DofParams p, uint2 *__restrict__ mips)
{
    __shared__ Rgb l1[32 * 32], l2[16 * 16], l3[8 * 8], l4[4 * 4], l5[2 * 2];
    const uint32_t tid = threadIdx.x;
    const uint32_t bx = blockIdx.x, by = blockIdx.y;
    for (uint32_t k = tid; k < 1024u; k += 256u)
    {
        const uint32_t lx = k & 31u, ly = k >> 5;
        const uint32_t sx = bx * 64u + 2u * lx, sy = by * 64u + 2u * ly;
        Rgb t[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q)
        {
            const uint32_t cx = min_u(sx + (q & 1u), p.hw - 1u), cy = min_u(sy + (q >> 1), p.hh - 1u);
            const f4 c = unpack_rgba16f(mips[(size_t)cy * p.hw + cx]);
            t[q] = Rgb{c.x, c.y, c.z};
        }
        const Rgb v = mean4(t[0], t[1], t[2], t[3]);
        l1[k] = v;
        store_level(p, mips, 1u, bx * 32u + lx, by * 32u + ly, v);
    }
    __syncthreads();
    {
        const uint32_t lx = tid & 15u, ly = tid >> 4;
        const Rgb v = mean4(l1[(2u * ly) * 32u + 2u * lx], l1[(2u * ly) * 32u + 2u * lx + 1u], l1[(2u * ly + 1u) * 32u + 2u * lx],
                            l1[(2u * ly + 1u) * 32u + 2u * lx + 1u]);
        l2[tid] = v;
        store_level(p, mips, 2u, bx * 16u + lx, by * 16u + ly, v);
    }
    __syncthreads();
    if (tid < 64u)
    {
        const uint32_t lx = tid & 7u, ly = tid >> 3;
        const Rgb v = mean4(l2[(2u * ly) * 16u + 2u * lx], l2[(2u * ly) * 16u + 2u * lx + 1u], l2[(2u * ly + 1u) * 16u + 2u * lx],
                            l2[(2u * ly + 1u) * 16u + 2u * lx + 1u]);
        l3[tid] = v;
        store_level(p, mips, 3u, bx * 8u + lx, by * 8u + ly, v);
    }
    __syncthreads();
    if (tid < 16u)
    {
        const uint32_t lx = tid & 3u, ly = tid >> 2;
        const Rgb v = mean4(l3[(2u * ly) * 8u + 2u * lx], l3[(2u * ly) * 8u + 2u * lx + 1u], l3[(2u * ly + 1u) * 8u + 2u * lx],
                            l3[(2u * ly + 1u) * 8u + 2u * lx + 1u]);
        l4[tid] = v;
        store_level(p, mips, 4u, bx * 4u + lx, by * 4u + ly, v);
    }
    __syncthreads();
    if (tid < 4u)
    {
        const uint32_t lx = tid & 1u, ly = tid >> 1;
        const Rgb v = mean4(l4[(2u * ly) * 4u + 2u * lx], l4[(2u * ly) * 4u + 2u * lx + 1u], l4[(2u * ly + 1u) * 4u + 2u * lx],
                            l4[(2u * ly + 1u) * 4u + 2u * lx + 1u]);
        l5[tid] = v;
        store_level(p, mips, 5u, bx * 2u + lx, by * 2u + ly, v);
    }
    __syncthreads();
    if (tid == 0u) store_level(p, mips, 6u, bx, by, mean4(l5[0], l5[1], l5[2], l5[3]));
}

// Levels 7 and up, one block: each texel is the mean of four stored texels of the level below, clamped to that level's
// extent.  The block's own barrier orders a level's stores before the next level's loads.
__global__ __launch_bounds__(256) void dof_reduce_tail_kernel(DofParams p, uint2 *mips)
{
    for (uint32_t l = 7u; l < p.levels; ++l)
    {
        const uint32_t w = level_width(p, l), h = level_height(p, l);
        const uint32_t bw = level_width(p, l - 1u), bh = level_height(p, l - 1u);
        const uint2 *below = mips + p.levelOffset[l - 1u];
        for (uint32_t k = threadIdx.x; k < w * h; k += 256u)
        {
            const uint32_t x = k % w, y = k / w;
            Rgb t[4];
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q)
            {
                const uint32_t cx = min_u(2u * x + (q & 1u), bw - 1u), cy = min_u(2u * y + (q >> 1), bh - 1u);
                const f4 c = unpack_rgba16f(below[(size_t)cy * bw + cx]);
                t[q] = Rgb{c.x, c.y, c.z};
            }
            store_level(p, mips, l, x, y, mean4(t[0], t[1], t[2], t[3]));
        }
        __syncthreads();
    }
}

// ---- flatten and dilate ----

// One wave per tile: lane (i, j) reads the tile's texel clamped to the image.  A min or max of fp16 values is one of them.
__global__ __launch_bounds__(256) void dof_flatten_kernel(DofParams p, DofBuffers b)
{
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= p.tw * p.th) return;
    const uint32_t tx = tile % p.tw, ty = tile / p.tw;
    const uint32_t x = min_u(tx * 8u + (lane & 7u), p.hw - 1u), y = min_u(ty * 8u + (lane >> 3), p.hh - 1u);
    const float c = half_to_float(b.halfCoC[(size_t)y * p.hw + x]);
    float lo = c, hi = c;
#pragma unroll
    for (uint32_t off = 32; off > 0u; off >>= 1)
    {
        lo = fmin_(lo, __shfl_xor(lo, off, 64));
        hi = fmax_(hi, __shfl_xor(hi, off, 64));
    }
    if (lane == 0u) b.tileMinMax[tile] = float_to_half(lo) | (float_to_half(hi) << 16);
}

// One lane per tile over the in-image tiles within gatherRadius: a tile outside the image reads the edge tile, which is
// nearer and therefore passes whenever the outside one does.
__global__ __launch_bounds__(256) void dof_dilate_kernel(DofParams p, DofBuffers b)
{
    const uint32_t tile = blockIdx.x * 256u + threadIdx.x;
    if (tile >= p.tw * p.th) return;
    const int32_t cx = (int32_t)(tile % p.tw), cy = (int32_t)(tile / p.tw);
    const int32_t tw = (int32_t)p.tw, th = (int32_t)p.th;
    const int32_t r = p.gatherRadius;
    const int32_t i0 = r < cx ? -r : -cx, i1 = r < tw - 1 - cx ? r : tw - 1 - cx;
    const int32_t j0 = r < cy ? -r : -cy, j1 = r < th - 1 - cy ? r : th - 1 - cy;
    float lo = kInf, hi = -kInf;
    for (int32_t j = j0; j <= j1; ++j)
        for (int32_t i = i0; i <= i1; ++i)
        {
            const uint32_t t = b.tileMinMax[(size_t)(cy + j) * p.tw + (size_t)(cx + i)];
            const float minCoC = half_to_float(t & 0xFFFFu), maxCoC = half_to_float(t >> 16);
            const float halfResDist = 8.0f * sqrt_((float)(i * i + j * j));
            if (halfResDist <= fabs_(minCoC) + 4.0f) lo = fmin_(lo, minCoC);
            if (halfResDist <= fabs_(maxCoC) + 4.0f) hi = fmax_(hi, maxCoC);
        }
    b.dilatedMinMax[tile] = float_to_half(lo) | (float_to_half(hi) << 16);
}

// ---- gather ----

// What a wave keeps in LDS of the mip chain: per level the extent, the scale from level-0 texel units and the offset
struct DofLevel
{
    float sx, sy;
    uint32_t w, h, offset;
};

PPT_D f3 bilinear_level(const uint2 *__restrict__ mips, const DofLevel &L, float px, float py)
{
    const float qx = px * L.sx - 0.5f, qy = py * L.sy - 0.5f;
    const float fx0 = __builtin_floorf(qx), fy0 = __builtin_floorf(qy);
    const float a = qx - fx0, bb = qy - fy0;
    // clamp to edge: the footprint's first texel lies in [-1, size - 1] for every tap inside the image
    const int32_t bx = clamp_i(f2i(fx0), -1, (int32_t)L.w - 1), by = clamp_i(f2i(fy0), -1, (int32_t)L.h - 1);
    const int32_t x0 = bx < 0 ? 0 : bx, x1 = bx + 1 < (int32_t)L.w ? bx + 1 : (int32_t)L.w - 1;
    const int32_t y0 = by < 0 ? 0 : by, y1 = by + 1 < (int32_t)L.h ? by + 1 : (int32_t)L.h - 1;
    const uint2 *base = mips + L.offset;
    const f4 t00 = unpack_rgba16f(base[(size_t)y0 * L.w + x0]), t10 = unpack_rgba16f(base[(size_t)y0 * L.w + x1]);
    const f4 t01 = unpack_rgba16f(base[(size_t)y1 * L.w + x0]), t11 = unpack_rgba16f(base[(size_t)y1 * L.w + x1]);
    const float w00 = (1.0f - a) * (1.0f - bb), w10 = a * (1.0f - bb), w01 = (1.0f - a) * bb, w11 = a * bb;
    return f3{((w00 * t00.x + w10 * t10.x) + w01 * t01.x) + w11 * t11.x, ((w00 * t00.y + w10 * t10.y) + w01 * t01.y) + w11 * t11.y,
              ((w00 * t00.z + w10 * t10.z) + w01 * t01.z) + w11 * t11.z};
}

// textureLod(trilinearSampler, p, mip): the two levels around clamp(mip, 0, levels - 1), blended by the fraction
PPT_D f3 trilinear(const uint2 *__restrict__ mips, const DofLevel *levels, uint32_t levelCount, float px, float py, float mip)
{
    const float lod = fmin_(fmax_(mip, 0.0f), (float)(levelCount - 1u));
    const float fl = __builtin_floorf(lod);
    const float t = lod - fl;
    const uint32_t l0 = (uint32_t)f2i(fl);
    const f3 c0 = bilinear_level(mips, levels[l0], px, py);
    if (t == 0.0f) return c0;
    const uint32_t l1 = min_u(l0 + 1u, levelCount - 1u);
    const f3 c1 = bilinear_level(mips, levels[l1], px, py);
    return f3{c0.x * (1.0f - t) + c1.x * t, c0.y * (1.0f - t) + c1.y * t, c0.z * (1.0f - t) + c1.z * t};
}

// sampleAlpha of gather.comp
PPT_D float sample_alpha(float sampleCoC)
{
    return fmin_(1.0f / ((kDofPi * sampleCoC) * sampleCoC), 1.0f / ((kDofPi * kDofSinglePixelRadius) * kDofSinglePixelRadius));
}

struct Bucket
{
    float r, g, b, w; // colorWeightSum
    float cocSum, sampleCount;
};

// blendBuckets of gather.comp; saturate turns the 0 / 0 of an empty bucket into 0
PPT_D Bucket blend_buckets(const Bucket &prev, const Bucket &cur, uint32_t ringSampleCount)
{
    const float currentOpacity = saturate(cur.sampleCount / (float)ringSampleCount);
    const float occludingCoC = saturate((prev.cocSum / prev.sampleCount) - (cur.cocSum / cur.sampleCount));
    const float blendFactor = prev.w == 0.0f ? 0.0f : (1.0f - currentOpacity * occludingCoC);
    Bucket o;
    o.r = prev.r * blendFactor + cur.r;
    o.g = prev.g * blendFactor + cur.g;
    o.b = prev.b * blendFactor + cur.b;
    o.w = prev.w * blendFactor + cur.w;
    o.cocSum = prev.cocSum * blendFactor + cur.cocSum;
    o.sampleCount = prev.sampleCount * blendFactor + cur.sampleCount;
    return o;
}

PPT_D void add_bucket_sample(
    const uint2 *__restrict__ mips, const DofLevel *levels, uint32_t levelCount, float px, float py, float sampleCoC, Bucket &bk)
{
    const float mip = fmax_(log2_(sampleCoC) - 1.0f, 0.0f);
    const float w = sample_alpha(sampleCoC);
    const f3 c = trilinear(mips, levels, levelCount, px, py, mip);
    bk.r += c.x * w;
    bk.g += c.y * w;
    bk.b += c.z * w;
    bk.w += w;
    bk.cocSum += sampleCoC;
    bk.sampleCount += 1.0f;
}

// One wave per 8 x 8 tile, four tiles per block: the dilated tile's min / max, both early-outs and the ring loops are
// the same for the whole wave.  The unit offsets and the level table sit in LDS.
template <bool kBackground>
__global__ __launch_bounds__(256) void dof_gather_kernel(DofParams p, DofBuffers b)
{
    __shared__ float offX[kDofTaps], offY[kDofTaps];
    __shared__ DofLevel levels[kDofMaxLevels];
    const uint32_t tid = threadIdx.x;
    if (tid < kDofTaps)
    {
        offX[tid] = b.sampleOffsets[2u * tid];
        offY[tid] = b.sampleOffsets[2u * tid + 1u];
    }
    else if (tid - 128u < p.levels)
    {
        const uint32_t l = tid - 128u;
        DofLevel L;
        L.w = level_width(p, l);
        L.h = level_height(p, l);
        L.sx = (float)L.w / (float)p.hw;
        L.sy = (float)L.h / (float)p.hh;
        L.offset = p.levelOffset[l];
        levels[l] = L;
    }
    __syncthreads();
    const uint32_t tile = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (tid >> 6)), lane = tid & 63u;
    if (tile >= p.tw * p.th) return;
    const uint32_t x = (tile % p.tw) * 8u + (lane & 7u), y = (tile / p.tw) * 8u + (lane >> 3);
    if (x >= p.hw || y >= p.hh) return;
    const uint32_t minMax = __builtin_amdgcn_readfirstlane(b.dilatedMinMax[tile]);
    const float tileMinCoC = half_to_float(minMax & 0xFFFFu), tileMaxCoC = half_to_float(minMax >> 16);
    uint2 *out = b.gather[kBackground ? 1 : 0] + ((size_t)y * p.hw + x);
    const uint2 *mips = b.halfIllumination;
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    const int32_t xMax = (int32_t)p.hw - 1, yMax = (int32_t)p.hh - 1;

    if (kBackground)
    {
        if (tileMaxCoC < 1.0f)
        {
            *out = make_uint2(0u, 0u);
            return;
        }
        const float kernelRadius = tileMaxCoC;
        const float ringSpacing = kernelRadius / 5.0f;
        Bucket prev = {};
        uint32_t first = kDofTaps;
        for (int32_t ring = 5; ring >= 0; --ring)
        {
            const uint32_t count = ring == 0 ? 1u : 8u * (uint32_t)ring;
            first -= count;
            const float borderingRadius = (((float)ring + 0.5f) + 1.0f) * ringSpacing;
            const float ringRadius = (float)ring * ringSpacing;
            Bucket cur = {};
            for (uint32_t si = 0; si < count; ++si)
            {
                const float px = cx + ringRadius * offX[first + si], py = cy + ringRadius * offY[first + si];
                const int32_t ix = clamp_i(f2i(__builtin_floorf(px)), 0, xMax), iy = clamp_i(f2i(__builtin_floorf(py)), 0, yMax);
                const float sampleCoC = half_to_float(b.halfCoC[(size_t)iy * p.hw + ix]);
                if (sampleCoC >= ringRadius)
                {
                    if (sampleCoC < borderingRadius)
                        add_bucket_sample(mips, levels, p.levels, px, py, sampleCoC, cur);
                    else
                        add_bucket_sample(mips, levels, p.levels, px, py, sampleCoC, prev);
                }
            }
            prev = blend_buckets(prev, cur, count);
        }
        const float d = fmax_(prev.w, 0.00001f);
        *out = pack_rgba16f(prev.r / d, prev.g / d, prev.b / d, 0.0f);
    }
    else
    {
        if (tileMinCoC > -0.5f)
        {
            *out = make_uint2(0u, 0u);
            return;
        }
        const float kernelRadius = -tileMinCoC;
        const float ringSpacing = kernelRadius / 5.0f;
        float r = 0.0f, g = 0.0f, bl = 0.0f, alphaSum = 0.0f, totalWeight = 0.0f;
        uint32_t first = 0u;
        for (int32_t ring = 0; ring < 6; ++ring)
        {
            const uint32_t count = ring == 0 ? 1u : 8u * (uint32_t)ring;
            const float ringRadius = (float)ring * ringSpacing;
            for (uint32_t si = 0; si < count; ++si)
            {
                const float sx = ringRadius * offX[first + si], sy = ringRadius * offY[first + si];
                const float px = cx + sx, py = cy + sy;
                const int32_t ix = clamp_i(f2i(__builtin_floorf(px)), 0, xMax), iy = clamp_i(f2i(__builtin_floorf(py)), 0, yMax);
                const float sampleCoC = -half_to_float(b.halfCoC[(size_t)iy * p.hw + ix]);
                if (sampleCoC < 0.5f) continue;
                const float sampleDistance = sqrt_(sx * sx + sy * sy);
                if (sampleCoC >= sampleDistance - ringSpacing)
                {
                    // floor(log2(c)) is c's binary exponent (c >= 0.5 is normal)
                    const int32_t e = (int32_t)((f2u(sampleCoC) >> 23) & 0xFFu) - 127;
                    const float mip = fmax_((float)e - 1.0f, 0.0f);
                    const float w = kernelRadius / sampleCoC;
                    const f3 c = trilinear(mips, levels, p.levels, px, py, mip);
                    r += c.x * w;
                    g += c.y * w;
                    bl += c.z * w;
                    alphaSum += sample_alpha(sampleCoC) * saturate(sampleCoC - 0.5f);
                    totalWeight += w;
                }
            }
            first += count;
        }
        const float d = fmax_(totalWeight, 0.001f);
        const float weight = saturate(((2.0f * (1.0f / (float)kDofTaps)) * (1.0f / sample_alpha(kernelRadius))) * alphaSum);
        *out = pack_rgba16f(r / d, g / d, bl / d, weight);
    }
}

// ---- filter ----

PPT_D void swap_if_less(float &la, uint32_t &ia, float &lb, uint32_t &ib)
{
    if (la < lb)
    {
        const float l = la;
        la = lb;
        lb = l;
        const uint32_t i = ia;
        ia = ib;
        ib = i;
    }
}

// 3 x 3 median by luminance: the indirect sort of filter.comp over (luminance, index) pairs kept in registers; the
// median texel is loaded again by its index.
__global__ __launch_bounds__(256) void dof_filter_kernel(DofParams p, const uint2 *__restrict__ in, uint2 *__restrict__ out)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= p.hw || y >= p.hh) return;
    const int32_t xMax = (int32_t)p.hw - 1, yMax = (int32_t)p.hh - 1;
    float lum[9];
    uint32_t idx[9];
    float maxLuminance = 0.0f;
    uint32_t maxI = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 9u; ++k)
    {
        // i outer, j inner: sample k is (i, j) = (k / 3 - 1, k % 3 - 1)
        const int32_t sx = clamp_i((int32_t)x + (int32_t)(k / 3u) - 1, 0, xMax), sy = clamp_i((int32_t)y + (int32_t)(k % 3u) - 1, 0, yMax);
        const f4 c = unpack_rgba16f(in[(size_t)sy * p.hw + sx]);
        lum[k] = (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z;
        idx[k] = k;
        if (maxLuminance < lum[k])
        {
            maxLuminance = lum[k];
            maxI = k;
        }
    }
    // the biggest value goes to the end, so that a power of two number of elements is sorted
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k)
        if (k == maxI)
        {
            const float l = lum[k];
            lum[k] = lum[8];
            lum[8] = l;
            idx[k] = 8u;
            idx[8] = k;
        }
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) swap_if_less(lum[i], idx[i], lum[i + 4u], idx[i + 4u]);
    // the second round as written: first = i + (i / 2) * 4, second = first + 2, i.e. the pairs (0, 2), (1, 3), (6, 8) and
    // (7, 9); the last one reaches past the nine elements (undefined in the GLSL) and is left out
    swap_if_less(lum[0], idx[0], lum[2], idx[2]);
    swap_if_less(lum[1], idx[1], lum[3], idx[3]);
    swap_if_less(lum[6], idx[6], lum[8], idx[8]);
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) swap_if_less(lum[2u * i], idx[2u * i], lum[2u * i + 1u], idx[2u * i + 1u]);
    const uint32_t m = idx[4];
    const int32_t sx = clamp_i((int32_t)x + (int32_t)(m / 3u) - 1, 0, xMax), sy = clamp_i((int32_t)y + (int32_t)(m % 3u) - 1, 0, yMax);
    out[(size_t)y * p.hw + x] = in[(size_t)sy * p.hw + sx];
}

// ---- combine ----

__global__ __launch_bounds__(256) void dof_combine_kernel(DofParams p, DofBuffers b)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= p.width || y >= p.height) return;
    const size_t i = (size_t)y * p.width + x;
    const float coc = half_to_float(b.halfCoC[(size_t)(y >> 1) * p.hw + (x >> 1)]);
    const float4 in = b.illumination[i];
    f3 o = f3{in.x, in.y, in.z};
    // floor((coord + d) / 2), one past the edge on an even extent: clamped to the edge
    const uint32_t hx0 = x >> 1, hx1 = min_u((x + 1u) >> 1, p.hw - 1u);
    const uint32_t hy0 = y >> 1, hy1 = min_u((y + 1u) >> 1, p.hh - 1u);
    const size_t h00 = (size_t)hy0 * p.hw + hx0, h01 = (size_t)hy1 * p.hw + hx0;
    const size_t h11 = (size_t)hy1 * p.hw + hx1, h10 = (size_t)hy0 * p.hw + hx1;
    {
        // upscaleBackground: texel 01 is never read
        const f4 c00 = unpack_rgba16f(b.filtered[1][h00]), c10 = unpack_rgba16f(b.filtered[1][h10]), c11 = unpack_rgba16f(b.filtered[1][h11]);
        const f3 bg = f3{mix(mix(c00.x, c10.x, 0.5f), mix(c10.x, c11.x, 0.5f), 0.5f), mix(mix(c00.y, c10.y, 0.5f), mix(c10.y, c11.y, 0.5f), 0.5f),
                         mix(mix(c00.z, c10.z, 0.5f), mix(c10.z, c11.z, 0.5f), 0.5f)};
        const float bgFactor = saturate(coc - 1.0f);
        if (bgFactor > 0.0f) o = f3{mix(o.x, bg.x, bgFactor), mix(o.y, bg.y, bgFactor), mix(o.z, bg.z, bgFactor)};
    }
    {
        // upscaleForeground: the bilateral's inputs 01, 11, 10, 00 are the texels 00, 01, 11, 10
        const f4 fg = bilateral_filter(unpack_rgba16f(b.filtered[0][h00]), unpack_rgba16f(b.filtered[0][h01]),
                                       unpack_rgba16f(b.filtered[0][h11]), unpack_rgba16f(b.filtered[0][h10]));
        if (fg.w > 0.0f) o = f3{mix(o.x, fg.x, fg.w), mix(o.y, fg.y, fg.w), mix(o.z, fg.z, fg.w)};
    }
    b.out[i] = make_float4(o.x, o.y, o.z, in.w);
}

static dim3 image_grid(uint32_t w, uint32_t h) { return dim3((w + 63u) / 64u, (h + 3u) / 4u); }

size_t dof_set_extents(DofParams &p, uint32_t width, uint32_t height)
{
    p.width = width;
    p.height = height;
    p.hw = width / 2u + (width & 1u);
    p.hh = height / 2u + (height & 1u);
    p.tw = (p.hw + 7u) / 8u;
    p.th = (p.hh + 7u) / 8u;
    const uint32_t top = p.hw > p.hh ? p.hw : p.hh;
    p.levels = 0u;
    while (p.levels < kDofMaxLevels && (top >> p.levels)) ++p.levels;
    size_t texels = 0;
    for (uint32_t l = 0; l < kDofMaxLevels; ++l)
    {
        p.levelOffset[l] = (uint32_t)texels;
        if (l < p.levels) texels += (size_t)((p.hw >> l) ? (p.hw >> l) : 1u) * ((p.hh >> l) ? (p.hh >> l) : 1u);
    }
    return texels;
}

void dof_sample_offsets(float out[2 * kDofTaps])
{
    const double pi = 3.14159265358979323846;
    uint32_t k = 0;
    for (uint32_t ring = 0; ring < 6u; ++ring)
    {
        const uint32_t count = ring == 0u ? 1u : 8u * ring;
        for (uint32_t s = 0; s < count; ++s, ++k)
        {
            const double phi = ((double)s + (ring % 2u == 0u ? 0.5 : 0.0)) * (2.0 * pi) / (double)count;
            out[2u * k] = (float)std::cos(phi);
            out[2u * k + 1u] = (float)std::sin(phi);
        }
    }
}

void launch_depth_of_field(const DofParams &p, const DofBuffers &b, hipEvent_t *events, hipStream_t stream)
{
    uint32_t e = 0;
    auto mark = [&]() {
        if (events) (void)hipEventRecord(events[e++], stream);
    };
    const dim3 halfGrid = image_grid(p.hw, p.hh);
    const uint32_t tiles = p.tw * p.th;
    mark();
    hipLaunchKernelGGL(dof_setup_kernel, halfGrid, dim3(256), 0, stream, p, b);
    mark();
    if (p.levels > 1u)
        hipLaunchKernelGGL(dof_reduce_kernel, dim3((p.hw + 63u) / 64u, (p.hh + 63u) / 64u), dim3(256), 0, stream, p, b.halfIllumination);
    if (p.levels > 7u) hipLaunchKernelGGL(dof_reduce_tail_kernel, dim3(1), dim3(256), 0, stream, p, b.halfIllumination);
    mark();
    hipLaunchKernelGGL(dof_flatten_kernel, dim3((tiles + 3u) / 4u), dim3(256), 0, stream, p, b);
    mark();
    hipLaunchKernelGGL(dof_dilate_kernel, dim3((tiles + 255u) / 256u), dim3(256), 0, stream, p, b);
    mark();
    hipLaunchKernelGGL(dof_gather_kernel<false>, dim3((tiles + 3u) / 4u), dim3(256), 0, stream, p, b);
    mark();
    hipLaunchKernelGGL(dof_gather_kernel<true>, dim3((tiles + 3u) / 4u), dim3(256), 0, stream, p, b);
    mark();
    hipLaunchKernelGGL(dof_filter_kernel, halfGrid, dim3(256), 0, stream, p, b.gather[0], b.filtered[0]);
    mark();
    hipLaunchKernelGGL(dof_filter_kernel, halfGrid, dim3(256), 0, stream, p, b.gather[1], b.filtered[1]);
    mark();
    hipLaunchKernelGGL(dof_combine_kernel, image_grid(p.width, p.height), dim3(256), 0, stream, p, b);
    mark();
}

void launch_skybox_fill(const DeviceScene &s, const RenderParams &r, const float *nonLinearDepth, float4 *hdr, hipStream_t stream)
{
    hipLaunchKernelGGL(skybox_fill_kernel, image_grid(r.width, r.height), dim3(256), 0, stream, s, r, nonLinearDepth, hdr);
}

} // namespace ppt
