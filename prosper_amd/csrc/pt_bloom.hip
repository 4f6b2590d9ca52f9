// pt_bloom.hip — gfx950 kernels of bloom's multi-resolution blur (src/render/bloom/*, res/shader/bloom/{separate,
// reduce,blur,compose}.comp).
//
//   bloom_separate_kernel   separate.comp: max(downsampled illumination - threshold, 0) into level 0 of `highlights`
//   bloom_reduce_kernel     bloom/reduce.comp (SPD, three mips): levels 1-3, every level from the unrounded one below
//   bloom_blur_kernel       blur.comp: four weighted taps along a row or a column of one level
//   bloom_streak_kernel     blur.comp's horizontal pass of level 1: the four taps and the row-wide streak over level 0
//   bloom_compose_kernel    compose.comp: illumination + the blend of three levels, bilinear or biquadratic
//   bloom_compose_fft_kernel  compose.comp with MULTI_RESOLUTION = false: illumination + the convolved image of the FFT
//                           technique (pt_bloom_fft.hip), which also runs separate over its dim x dim image
//
// Images have no sampler here; the lookups are written out.  A lookup's texel coordinate is formed in integers where
// the GLSL goes through a normalised uv: (coord + 0.5) / size_a * size_b - 0.5 is a ratio of integers, whose floor and
// fraction are exact, and a fraction that is right to float32 is what keeps a lookup beside an empty texel within the
// tests' allowance on a 2000-texel row.
#include "pt_bloom.hpp"

#include <cmath>

#include "pt_device.hpp"

namespace ppt
{

namespace bloom
{

// blur.comp:20-25 (lisyarus' blur coefficients generator, four samples)
__constant__ const float kBlurOffsets[4] = {-2.089779143016758f, -0.38698196063011614f, 1.2004365440663936f, 3.0f};
__constant__ const float kBlurWeights[4] = {0.0666055522709221f, 0.6249460483713625f, 0.3024686099546741f, 0.005979789403041253f};

constexpr uint32_t kStreakColumns = 256; // outputs of one block of the streak kernel, one per lane
constexpr uint32_t kStreakTaps = 256;    // taps of one staged piece: the piece holds kStreakColumns + kStreakTaps positions

struct Rgb
{
    float r, g, b;
};

PPT_D Rgb texel_rgb(uint2 p) { return Rgb{half_to_float(p.x & 0xFFFFu), half_to_float(p.x >> 16), half_to_float(p.y & 0xFFFFu)}; }
PPT_D uint2 pack_rgba16f(float r, float g, float b, float a)
{
    return make_uint2(float_to_half(r) | (float_to_half(g) << 16), float_to_half(b) | (float_to_half(a) << 16));
}
PPT_D int32_t clamp_i(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bilinearBorderTransparentBlackSampler: a texel outside the image is (0, 0, 0, 0)
PPT_D Rgb texel_border(const uint2 *__restrict__ img, int32_t w, int32_t h, int32_t x, int32_t y)
{
    if ((uint32_t)x >= (uint32_t)w || (uint32_t)y >= (uint32_t)h) return Rgb{0.0f, 0.0f, 0.0f};
    return texel_rgb(img[(size_t)y * (uint32_t)w + (uint32_t)x]);
}
PPT_D Rgb texel_border(const float4 *__restrict__ img, int32_t w, int32_t h, int32_t x, int32_t y)
{
    if ((uint32_t)x >= (uint32_t)w || (uint32_t)y >= (uint32_t)h) return Rgb{0.0f, 0.0f, 0.0f};
    const float4 c = img[(size_t)y * (uint32_t)w + (uint32_t)x];
    return Rgb{c.x, c.y, c.z};
}
// bilinearSampler of compose: clamp to edge
PPT_D Rgb texel_edge(const uint2 *__restrict__ img, int32_t w, int32_t h, int32_t x, int32_t y)
{
    return texel_rgb(img[(size_t)clamp_i(y, 0, h - 1) * (uint32_t)w + (uint32_t)clamp_i(x, 0, w - 1)]);
}

// the four texels of a bilinear footprint blended with float weights, a and b the fractions along x and y
PPT_D Rgb blend4(Rgb t00, Rgb t10, Rgb t01, Rgb t11, float a, float b)
{
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    return Rgb{((w00 * t00.r + w10 * t10.r) + w01 * t01.r) + w11 * t11.r, ((w00 * t00.g + w10 * t10.g) + w01 * t01.g) + w11 * t11.g,
               ((w00 * t00.b + w10 * t10.b) + w01 * t01.b) + w11 * t11.b};
}

// ---- separate ----

// The lookup at the corner (cx, cy) shared by four input texels: texel coordinate (cx - 0.5, cy - 0.5), so the footprint
// is cx - 1, cx with both fractions one half.  At cx = 0 or cy = 0 it takes in the border.
PPT_D Rgb corner_lookup(const float4 *__restrict__ img, int32_t w, int32_t h, int32_t cx, int32_t cy)
{
    return blend4(texel_border(img, w, h, cx - 1, cy - 1), texel_border(img, w, h, cx, cy - 1), texel_border(img, w, h, cx - 1, cy),
                  texel_border(img, w, h, cx, cy), 0.5f, 0.5f);
}

__global__ __launch_bounds__(256) void bloom_separate_kernel(BloomParams p, const float4 *__restrict__ illumination, uint2 *__restrict__ highlights)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= p.levelW[0] || y >= p.levelH[0]) return;
    const int32_t w = (int32_t)p.width, h = (int32_t)p.height;
    Rgb v;
    if (p.scale == 2u)
        v = corner_lookup(illumination, w, h, 2 * (int32_t)x, 2 * (int32_t)y);
    else
    {
        // uv = (4 coord + (-1 | 1)) / resolution: the corners 4 coord - 1 and 4 coord + 1, in the GLSL's order 00, 01, 10, 11
        const int32_t cx = 4 * (int32_t)x, cy = 4 * (int32_t)y;
        const Rgb v00 = corner_lookup(illumination, w, h, cx - 1, cy - 1), v01 = corner_lookup(illumination, w, h, cx - 1, cy + 1);
        const Rgb v10 = corner_lookup(illumination, w, h, cx + 1, cy - 1), v11 = corner_lookup(illumination, w, h, cx + 1, cy + 1);
        v = Rgb{(((v00.r + v01.r) + v10.r) + v11.r) * 0.25f, (((v00.g + v01.g) + v10.g) + v11.g) * 0.25f,
                (((v00.b + v01.b) + v10.b) + v11.b) * 0.25f};
    }
    highlights[(size_t)y * p.levelW[0] + x] =
        pack_rgba16f(fmax_(v.r - p.threshold, 0.0f), fmax_(v.g - p.threshold, 0.0f), fmax_(v.b - p.threshold, 0.0f), 0.0f);
}

// ---- reduce ----

PPT_D Rgb mean4(Rgb a, Rgb b, Rgb c, Rgb d)
{
    return Rgb{(((a.r + b.r) + c.r) + d.r) * 0.25f, (((a.g + b.g) + c.g) + d.g) * 0.25f, (((a.b + b.b) + c.b) + d.b) * 0.25f};
}
// every stored alpha is 0, and so is the mean of four of them
PPT_D void store_level(const BloomParams &p, uint2 *img, uint32_t l, uint32_t x, uint32_t y, Rgb v)
{
    if (x >= p.levelW[l] || y >= p.levelH[l]) return;
    img[p.levelOffset[l] + (size_t)y * p.levelW[l] + x] = pack_rgba16f(v.r, v.g, v.b, 0.0f);
}

// One block per 32 x 32 virtual level-0 texels (the source clamped to its edge), sixteen 8 x 8 tiles: level k is the mean
// of four unrounded level k - 1 texels, texels past that level's extent included; only texels inside level k's extent
// are stored.  Lane (tile, q): q picks the tile's 4 x 4 level-1 texels, then its 2 x 2 level-2 texels, then its one of level 3.
__global__ __launch_bounds__(256) void bloom_reduce_kernel(BloomParams p, uint2 *__restrict__ img)
{
    __shared__ Rgb l1[16 * 16], l2[8 * 8];
    const uint32_t tid = threadIdx.x, tile = tid >> 4, q = tid & 15u;
    const uint32_t tx = tile & 3u, ty = tile >> 2;
    {
        const uint32_t lx = tx * 4u + (q & 3u), ly = ty * 4u + (q >> 2);
        const uint32_t gx = blockIdx.x * 16u + lx, gy = blockIdx.y * 16u + ly;
        Rgb t[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
        {
            const uint32_t sx = 2u * gx + (k & 1u), sy = 2u * gy + (k >> 1);
            const uint32_t cx = sx < p.levelW[0] ? sx : p.levelW[0] - 1u, cy = sy < p.levelH[0] ? sy : p.levelH[0] - 1u;
            t[k] = texel_rgb(img[(size_t)cy * p.levelW[0] + cx]);
        }
        const Rgb v = mean4(t[0], t[1], t[2], t[3]);
        l1[ly * 16u + lx] = v;
        store_level(p, img, 1u, gx, gy, v);
    }
    __syncthreads();
    if (q < 4u)
    {
        const uint32_t lx = tx * 2u + (q & 1u), ly = ty * 2u + (q >> 1);
        const Rgb v = mean4(l1[(2u * ly) * 16u + 2u * lx], l1[(2u * ly) * 16u + 2u * lx + 1u], l1[(2u * ly + 1u) * 16u + 2u * lx],
                            l1[(2u * ly + 1u) * 16u + 2u * lx + 1u]);
        l2[ly * 8u + lx] = v;
        store_level(p, img, 2u, blockIdx.x * 8u + lx, blockIdx.y * 8u + ly, v);
    }
    __syncthreads();
    if (q == 0u)
    {
        const Rgb v = mean4(l2[(2u * ty) * 8u + 2u * tx], l2[(2u * ty) * 8u + 2u * tx + 1u], l2[(2u * ty + 1u) * 8u + 2u * tx],
                            l2[(2u * ty + 1u) * 8u + 2u * tx + 1u]);
        store_level(p, img, 3u, blockIdx.x * 4u + tx, blockIdx.y * 4u + ty, v);
    }
}

// ---- blur ----

// The four taps of blur.comp along x (or y) at texel (x, y) of a w x h level.  A tap's texel coordinate is
// coord + OFFSETS[i] along the blur and coord itself across it: the footprint is two texels with the offset's own
// fraction, the other two have weight 0.  The fourth offset is 3: one texel.
template <bool kVertical>
PPT_D Rgb blur_taps(const uint2 *__restrict__ src, int32_t w, int32_t h, int32_t x, int32_t y)
{
    Rgb acc = Rgb{0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i)
    {
        const float whole = __builtin_floorf(kBlurOffsets[i]);
        const float f = kBlurOffsets[i] - whole;
        const int32_t o = (int32_t)whole;
        const Rgb t0 = texel_border(src, w, h, kVertical ? x : x + o, kVertical ? y + o : y);
        const Rgb t1 = texel_border(src, w, h, kVertical ? x : x + o + 1, kVertical ? y + o + 1 : y);
        const float w0 = 1.0f - f;
        acc.r += (w0 * t0.r + f * t1.r) * kBlurWeights[i];
        acc.g += (w0 * t0.g + f * t1.g) * kBlurWeights[i];
        acc.b += (w0 * t0.b + f * t1.b) * kBlurWeights[i];
    }
    return acc;
}

template <bool kVertical>
__global__ __launch_bounds__(256) void bloom_blur_kernel(const uint2 *__restrict__ src, uint2 *__restrict__ dst, uint32_t w, uint32_t h)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const Rgb v = blur_taps<kVertical>(src, (int32_t)w, (int32_t)h, (int32_t)x, (int32_t)y);
    dst[(size_t)y * w + x] = pack_rgba16f(v.r, v.g, v.b, 1.0f);
}

// ---- the streak ----

// Where the centre of level-1 texel p lies in level 0 along an axis of size0 = 2 size1 or 2 size1 + 1 texels: the texel
// coordinate (p + 0.5) size0 / size1 - 0.5 = 2 p + (size1 + (2 p + 1)(size0 - 2 size1)) / (2 size1), for -1 <= p <= size1
// (the quotient's whole part is then 0 or 1, size1 >= 2).
PPT_D void level0_coord(int32_t p, int32_t size0, int32_t size1, int32_t &i0, float &f)
{
    const int32_t d = 2 * size1, rem = size1 + (2 * p + 1) * (size0 - d);
    const int32_t up = rem >= d ? 1 : 0;
    i0 = 2 * p + up;
    f = (float)(rem - up * d) * (1.0f / (float)d);
}

// L0 of the streak: the border-bilinear lookup of level 0 at the centre of level-1 position (p, row); rows j0, j0 + 1
// with fraction fy.  Positions left of -1 and right of levelW[1] see only the border.
PPT_D Rgb streak_lookup(const BloomParams &P, const uint2 *__restrict__ level0, int32_t p, int32_t j0, float fy)
{
    const int32_t w0 = (int32_t)P.levelW[0], h0 = (int32_t)P.levelH[0], w1 = (int32_t)P.levelW[1];
    if (p < -1 || p > w1) return Rgb{0.0f, 0.0f, 0.0f};
    int32_t i0;
    float fx;
    level0_coord(p, w0, w1, i0, fx);
    return blend4(texel_border(level0, w0, h0, i0, j0), texel_border(level0, w0, h0, i0 + 1, j0), texel_border(level0, w0, h0, i0, j0 + 1),
                  texel_border(level0, w0, h0, i0 + 1, j0 + 1), fx, fy);
}

// The horizontal pass of level 1: the four taps over level 1 plus sum_i w(i) L0(x + i) / (2 resolution.x), i in [-h, h).
// L0 depends on x + i alone, so one block per (row, 256 columns) stages L0 of the positions its taps reach in LDS as
// float RGB, kStreakTaps taps at a time: a tap is then three LDS reads at consecutive addresses across the wave and the
// weights are wave-uniform.  A piece whose positions all lie outside the row adds zeros and is skipped.  (One thread per
// texel with every tap a lookup in global memory took eleven times as long: DESIGN.md f9.)
__global__ __launch_bounds__(256) void bloom_streak_kernel(
    BloomParams P, const uint2 *__restrict__ highlights, uint2 *__restrict__ horizontal, const float *__restrict__ weights)
{
    __shared__ float sr[kStreakColumns + kStreakTaps], sg[kStreakColumns + kStreakTaps], sb[kStreakColumns + kStreakTaps];
    const int32_t w1 = (int32_t)P.levelW[1], h1 = (int32_t)P.levelH[1];
    const int32_t half = (int32_t)P.streakHalfWidth;
    const int32_t tid = (int32_t)threadIdx.x, x0 = (int32_t)(blockIdx.x * kStreakColumns), y = (int32_t)blockIdx.y;
    const int32_t x = x0 + tid;
    const uint2 *level0 = highlights, *level1 = highlights + P.levelOffset[1];
    const float *wRG = weights, *wB = weights + 2 * half;
    int32_t j0;
    float fy;
    level0_coord(y, (int32_t)P.levelH[0], h1, j0, fy);
    Rgb acc = Rgb{0.0f, 0.0f, 0.0f};
    for (int32_t first = -half; first < half; first += (int32_t)kStreakTaps)
    {
        // taps first .. first + count - 1 of the columns x0 .. x0 + 255 read the positions base .. base + 510
        const int32_t base = x0 + first;
        if (base + (int32_t)(kStreakColumns + kStreakTaps) <= -1 || base > w1) continue; // (the same for the whole block)
        for (int32_t k = tid; k < (int32_t)(kStreakColumns + kStreakTaps); k += 256)
        {
            const Rgb v = streak_lookup(P, level0, base + k, j0, fy);
            sr[k] = v.r;
            sg[k] = v.g;
            sb[k] = v.b;
        }
        __syncthreads();
        const int32_t count = half - first < (int32_t)kStreakTaps ? half - first : (int32_t)kStreakTaps;
        const float *rg = wRG + (first + half), *bl = wB + (first + half);
#pragma unroll 8
        for (int32_t t = 0; t < count; ++t)
        {
            acc.r += rg[t] * sr[tid + t];
            acc.g += rg[t] * sg[tid + t];
            acc.b += bl[t] * sb[tid + t];
        }
        __syncthreads();
    }
    if (x >= w1) return;
    const Rgb taps = blur_taps<false>(level1, w1, h1, x, y);
    const float norm = 1.0f / ((float)w1 * 2.0f);
    horizontal[P.levelOffset[1] + (size_t)y * (uint32_t)w1 + (uint32_t)x] =
        pack_rgba16f(taps.r + acc.r * norm, taps.g + acc.g * norm, taps.b + acc.b * norm, 1.0f);
}

// ---- compose ----

// The footprints of compose's lookups of one level along one axis: one lookup at uv, or the two of sampleBiquadratic
// at uv - c and uv + c.  i is the footprint's first texel, f its fraction.
struct ComposeAxis
{
    int32_t i[2];
    float f[2];
};

// uv = (coord + 0.5) / full; the texel coordinate uv size - 0.5 = ((2 coord + 1) size - full) / (2 full).  Biquadratic:
// q = fract(uv res) with res = full / step, i.e. fract((coord + 0.5) / step), exact for a power of two; the offset
// c = (q (q - 1) + 0.5) / res is c size = (q (q - 1) + 0.5) (size / res) texels.
PPT_D ComposeAxis compose_axis(uint32_t coord, uint32_t full, uint32_t size, float step, bool biquadratic)
{
    const uint32_t d = 2u * full, n = (2u * coord + 1u) * size + full; // the numerator, one texel up: never negative
    const uint32_t whole = n / d;
    const int32_t i0 = (int32_t)whole - 1;
    const float f0 = (float)(n - whole * d) * (1.0f / (float)d);
    ComposeAxis a;
    if (!biquadratic)
    {
        a.i[0] = a.i[1] = i0;
        a.f[0] = a.f[1] = f0;
        return a;
    }
    const float res = (float)full / step;
    const float v = ((float)coord + 0.5f) * (1.0f / step);
    const float q = v - __builtin_floorf(v);
    const float c = (q * (q - 1.0f) + 0.5f) * ((float)size / res);
    const float lo = f0 - c, hi = f0 + c;
    const float wl = __builtin_floorf(lo), wh = __builtin_floorf(hi);
    a.i[0] = i0 + (int32_t)wl;
    a.f[0] = lo - wl;
    a.i[1] = i0 + (int32_t)wh;
    a.f[1] = hi - wh;
    return a;
}

PPT_D Rgb edge_bilinear(const uint2 *__restrict__ img, int32_t w, int32_t h, int32_t ix, float fx, int32_t iy, float fy)
{
    return blend4(texel_edge(img, w, h, ix, iy), texel_edge(img, w, h, ix + 1, iy), texel_edge(img, w, h, ix, iy + 1),
                  texel_edge(img, w, h, ix + 1, iy + 1), fx, fy);
}

__global__ __launch_bounds__(256) void bloom_compose_kernel(BloomParams p, BloomBuffers b)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= p.width || y >= p.height) return;
    const bool biquadratic = p.biquadratic != 0u;
    Rgb level[3];
#pragma unroll
    for (uint32_t l = 0; l < 3u; ++l)
    {
        // a level no blur pass wrote (level 0 at Quarter) is read from `highlights`
        const uint2 *img = (l >= p.firstLevel ? b.blurred : b.highlights) + p.levelOffset[l];
        const int32_t w = (int32_t)p.levelW[l], h = (int32_t)p.levelH[l];
        const float step = (float)(p.scale << l);
        const ComposeAxis ax = compose_axis(x, p.width, p.levelW[l], step, biquadratic);
        const ComposeAxis ay = compose_axis(y, p.height, p.levelH[l], step, biquadratic);
        if (biquadratic)
        {
            const Rgb s00 = edge_bilinear(img, w, h, ax.i[0], ax.f[0], ay.i[0], ay.f[0]);
            const Rgb s01 = edge_bilinear(img, w, h, ax.i[0], ax.f[0], ay.i[1], ay.f[1]);
            const Rgb s11 = edge_bilinear(img, w, h, ax.i[1], ax.f[1], ay.i[1], ay.f[1]);
            const Rgb s10 = edge_bilinear(img, w, h, ax.i[1], ax.f[1], ay.i[0], ay.f[0]);
            level[l] = Rgb{(((s00.r + s01.r) + s11.r) + s10.r) * 0.25f, (((s00.g + s01.g) + s11.g) + s10.g) * 0.25f,
                           (((s00.b + s01.b) + s11.b) + s10.b) * 0.25f};
        }
        else
            level[l] = edge_bilinear(img, w, h, ax.i[0], ax.f[0], ay.i[0], ay.f[0]);
    }
    const size_t i = (size_t)y * p.width + x;
    const float4 in = b.illumination[i];
    const float k0 = p.blendFactors[0], k1 = p.blendFactors[1], k2 = p.blendFactors[2];
    b.out[i] = make_float4(in.x + ((level[0].r * k0 + level[1].r * k1) + level[2].r * k2),
                           in.y + ((level[0].g * k0 + level[1].g * k1) + level[2].g * k2),
                           in.z + ((level[0].b * k0 + level[1].b * k1) + level[2].b * k2), 1.0f);
}

// ---- compose of the FFT technique ----

PPT_D Rgb texel_edge(const float4 *__restrict__ img, int32_t w, int32_t h, int32_t x, int32_t y)
{
    const float4 c = img[(size_t)clamp_i(y, 0, h - 1) * (uint32_t)w + (uint32_t)clamp_i(x, 0, w - 1)];
    return Rgb{c.x, c.y, c.z};
}
PPT_D Rgb edge_bilinear(const float4 *__restrict__ img, int32_t w, int32_t h, int32_t ix, float fx, int32_t iy, float fy)
{
    return blend4(texel_edge(img, w, h, ix, iy), texel_edge(img, w, h, ix + 1, iy), texel_edge(img, w, h, ix, iy + 1),
                  texel_edge(img, w, h, ix + 1, iy + 1), fx, fy);
}

// compose.comp with MULTI_RESOLUTION = false: illumination + one lookup of the convolved dim x dim RGBA32F image at
// highlightUV = (coord + 0.5) / (dim scale), i.e. the texel coordinate (2 coord + 1 - scale) / (2 scale): compose_axis
// with a "full" extent of scale texels over a level of one.  Biquadratic: res = dim, so q = fract((coord + 0.5) / scale)
// and the offsets are q (q - 1) + 0.5 texels.
__global__ __launch_bounds__(256) void bloom_compose_fft_kernel(
    uint32_t width, uint32_t height, uint32_t scale, uint32_t dim, uint32_t biquadraticFlag, const float4 *illumination,
    const float4 *__restrict__ convolved, float4 *out)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const bool biquadratic = biquadraticFlag != 0u;
    const int32_t n = (int32_t)dim;
    const ComposeAxis ax = compose_axis(x, scale, 1u, (float)scale, biquadratic);
    const ComposeAxis ay = compose_axis(y, scale, 1u, (float)scale, biquadratic);
    Rgb v;
    if (biquadratic)
    {
        const Rgb s00 = edge_bilinear(convolved, n, n, ax.i[0], ax.f[0], ay.i[0], ay.f[0]);
        const Rgb s01 = edge_bilinear(convolved, n, n, ax.i[0], ax.f[0], ay.i[1], ay.f[1]);
        const Rgb s11 = edge_bilinear(convolved, n, n, ax.i[1], ax.f[1], ay.i[1], ay.f[1]);
        const Rgb s10 = edge_bilinear(convolved, n, n, ax.i[1], ax.f[1], ay.i[0], ay.f[0]);
        v = Rgb{(((s00.r + s01.r) + s11.r) + s10.r) * 0.25f, (((s00.g + s01.g) + s11.g) + s10.g) * 0.25f,
                (((s00.b + s01.b) + s11.b) + s10.b) * 0.25f};
    }
    else
        v = edge_bilinear(convolved, n, n, ax.i[0], ax.f[0], ay.i[0], ay.f[0]);
    const size_t i = (size_t)y * width + x;
    const float4 in = illumination[i];
    out[i] = make_float4(in.x + v.r, in.y + v.g, in.z + v.b, 1.0f);
}

dim3 image_grid(uint32_t w, uint32_t h) { return dim3((w + 63u) / 64u, (h + 3u) / 4u); }

} // namespace bloom

using namespace bloom;

size_t bloom_set_extents(BloomParams &p, uint32_t width, uint32_t height, uint32_t resolutionScale)
{
    p.width = width;
    p.height = height;
    p.scale = resolutionScale == 0u ? 2u : 4u;
    p.firstLevel = resolutionScale == 0u ? 0u : 1u;
    const uint32_t ww = width / p.scale, wh = height / p.scale; // Separate.cpp:106-111
    size_t texels = 0;
    for (uint32_t l = 0; l < kBloomLevels; ++l)
    {
        p.levelW[l] = (ww >> l) ? (ww >> l) : 1u;
        p.levelH[l] = (wh >> l) ? (wh >> l) : 1u;
        p.levelOffset[l] = (uint32_t)texels;
        texels += (size_t)p.levelW[l] * p.levelH[l];
    }
    p.streakHalfWidth = (ww >> 1) / 2u;
    return texels;
}

void bloom_streak_weights(uint32_t halfWidth, float *rg, float *b)
{
    for (uint32_t k = 0; k < 2u * halfWidth; ++k)
    {
        const double i = (double)k - (double)halfWidth;
        const double a = std::fabs(i);
        // mix(vec3(.05, .05, 1), vec3(.01, .01, 1), saturate(abs(i) / 10)): the division is an integer one, so a step
        const double c = a < 10.0 ? 0.05 : 0.01;
        const double wave = std::fabs(std::sin(i * 0.5)) + std::fabs(std::cos(i * 0.95)) + std::fabs(std::sin(i * 0.75));
        const double fall = 150.0 / std::fmax(0.015 * i * i + a, 1.0);
        rg[k] = (float)(((c * 4.0) * wave) * fall);
        b[k] = (float)((4.0 * wave) * fall);
    }
}

void launch_bloom_fft_separate(
    uint32_t width, uint32_t height, uint32_t scale, float threshold, uint32_t dim, const float4 *illumination, uint2 *highlights,
    hipStream_t stream)
{
    BloomParams p = {};
    p.width = width;
    p.height = height;
    p.scale = scale;
    p.threshold = threshold;
    p.levelW[0] = p.levelH[0] = dim;
    hipLaunchKernelGGL(bloom_separate_kernel, image_grid(dim, dim), dim3(256), 0, stream, p, illumination, highlights);
}

void launch_bloom_fft_compose(
    uint32_t width, uint32_t height, uint32_t scale, uint32_t dim, uint32_t biquadratic, const float4 *illumination,
    const float4 *convolved, float4 *out, hipStream_t stream)
{
    hipLaunchKernelGGL(bloom_compose_fft_kernel, image_grid(width, height), dim3(256), 0, stream, width, height, scale, dim, biquadratic,
                       illumination, convolved, out);
}

void launch_bloom(const BloomParams &p, const BloomBuffers &b, hipEvent_t *events, hipStream_t stream)
{
    uint32_t e = 0;
    auto mark = [&]() {
        if (events) (void)hipEventRecord(events[e++], stream);
    };
    mark();
    hipLaunchKernelGGL(bloom_separate_kernel, image_grid(p.levelW[0], p.levelH[0]), dim3(256), 0, stream, p, b.illumination, b.highlights);
    mark();
    hipLaunchKernelGGL(bloom_reduce_kernel, dim3((p.levelW[0] + 31u) / 32u, (p.levelH[0] + 31u) / 32u), dim3(256), 0, stream, p, b.highlights);
    mark();
    for (uint32_t n = 0; n < kBloomBlurLevels; ++n)
    {
        const uint32_t l = p.firstLevel + n, w = p.levelW[l], h = p.levelH[l];
        if (l == 1u)
        {
            hipLaunchKernelGGL(bloom_streak_kernel, dim3((w + kStreakColumns - 1u) / kStreakColumns, h), dim3(256), 0, stream, p,
                               b.highlights, b.horizontal, b.streakWeights);
        }
        else
        {
            hipLaunchKernelGGL(bloom_blur_kernel<false>, image_grid(w, h), dim3(256), 0, stream, b.highlights + p.levelOffset[l],
                               b.horizontal + p.levelOffset[l], w, h);
        }
        mark();
    }
    for (uint32_t n = 0; n < kBloomBlurLevels; ++n)
    {
        const uint32_t l = p.firstLevel + n, w = p.levelW[l], h = p.levelH[l];
        hipLaunchKernelGGL(bloom_blur_kernel<true>, image_grid(w, h), dim3(256), 0, stream, b.horizontal + p.levelOffset[l],
                           b.blurred + p.levelOffset[l], w, h);
        mark();
    }
    hipLaunchKernelGGL(bloom_compose_kernel, image_grid(p.width, p.height), dim3(256), 0, stream, p, b);
    mark();
}

} // namespace ppt
