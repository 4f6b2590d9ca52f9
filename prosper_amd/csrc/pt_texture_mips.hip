// pt_texture_mips.hip — gfx950 kernels of the material textures' mip chains.
//
//   generate_mip_kernel<SRGB>   one level from its parent, one thread per texel of the child: the 2 x 2 box of the
//                               project's definition (clamped at an odd parent's last column / row).  Linear textures in
//                               integers, base-colour textures in linear light through the device's own srgb_to_linear.
//   untile_level_kernel         one level back to row-major RGBA8 (prosper_pt_read_texture_level: tests)
//   sample_texture_lod_kernel   sample_texture_lod over n records (prosper_pt_debug_sample_texture_lod: tests)
#include "pt_texture_mips.hpp"

#include "pt_device.hpp"

namespace ppt
{

namespace
{

constexpr uint32_t kMaxGridRows = 32768; // a level of 2^17 rows must not ask for more block rows than a grid has

// word offset of texel (i, j) of a tiled level whose tiles are `tilesPerRow` to a row
__device__ __forceinline__ uint32_t tiled_word(uint32_t tilesPerRow, uint32_t i, uint32_t j)
{
    return ((j >> 2) * tilesPerRow + (i >> 3)) * (kTexTileW * kTexTileH) + (((j & 3u) << 3) | (i & 7u));
}

// (a + b + c + d + 2) >> 2 of every byte
__device__ __forceinline__ uint32_t box_linear(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    uint32_t r = 0;
    for (uint32_t s = 0; s < 32u; s += 8u)
        r |= ((((a >> s) & 0xFFu) + ((b >> s) & 0xFFu) + ((c >> s) & 0xFFu) + ((d >> s) & 0xFFu) + 2u) >> 2) << s;
    return r;
}

// The code c whose lut[c] = srgb_to_linear(c / 255) is nearest to `mean`: the first of the 256 with the smallest
// |lut[c] - mean| (float32 subtraction), so a tie goes to the lower code.  No pow: the table holds the curve.
__device__ __forceinline__ uint32_t nearest_srgb_code(const float *lut, float mean)
{
    uint32_t best = 0;
    float bestD = fabs_(lut[0] - mean);
    for (uint32_t c = 1; c < 256u; ++c)
    {
        const float d = fabs_(lut[c] - mean);
        if (d < bestD)
        {
            bestD = d;
            best = c;
        }
    }
    return best;
}

} // namespace

template <bool SRGB>
__global__ __launch_bounds__(256) void generate_mip_kernel(
    const uint32_t *__restrict__ parent, uint32_t parentW, uint32_t parentH, uint32_t parentTilesPerRow, uint32_t *__restrict__ child,
    uint32_t childW, uint32_t childH, uint32_t childTilesPerRow)
{
    __shared__ float lut[SRGB ? 256 : 1];
    if constexpr (SRGB)
    {
        // the value sample_material decodes from code c: unpack_rgba8's c * (1 / 255), then srgb_to_linear
        for (uint32_t c = threadIdx.x; c < 256u; c += blockDim.x) lut[c] = srgb_to_linear((float)c * (1.0f / 255.0f));
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= childW) return;
    // (grid.y is capped at kMaxGridRows: a block row takes every gridDim.y-th texel row)
    for (uint32_t j = blockIdx.y; j < childH; j += gridDim.y)
    {
        const uint32_t x0 = 2u * i, y0 = 2u * j;
        const uint32_t x1 = x0 + 1u < parentW ? x0 + 1u : parentW - 1u;
        const uint32_t y1 = y0 + 1u < parentH ? y0 + 1u : parentH - 1u;
        const uint32_t p00 = parent[tiled_word(parentTilesPerRow, x0, y0)];
        const uint32_t p10 = parent[tiled_word(parentTilesPerRow, x1, y0)];
        const uint32_t p01 = parent[tiled_word(parentTilesPerRow, x0, y1)];
        const uint32_t p11 = parent[tiled_word(parentTilesPerRow, x1, y1)];
        uint32_t out = box_linear(p00, p10, p01, p11);
        if constexpr (SRGB)
        {
            // RGB in linear light: ((l00 + l10) + (l01 + l11)) * 0.25 in float32, back to the nearest code; alpha stays the
            // integer mean
            out &= 0xFF000000u;
            for (uint32_t s = 0; s < 24u; s += 8u)
            {
                const float mean = ((lut[(p00 >> s) & 0xFFu] + lut[(p10 >> s) & 0xFFu]) + (lut[(p01 >> s) & 0xFFu] + lut[(p11 >> s) & 0xFFu])) * 0.25f;
                out |= nearest_srgb_code(lut, mean) << s;
            }
        }
        child[tiled_word(childTilesPerRow, i, j)] = out;
    }
}

void launch_generate_mip(
    const void *parent, uint32_t parentW, uint32_t parentH, void *child, uint32_t childW, uint32_t childH, bool srgb, hipStream_t stream)
{
    if (childW == 0 || childH == 0) return;
    const uint32_t pt = (parentW + kTexTileW - 1u) / kTexTileW, ct = (childW + kTexTileW - 1u) / kTexTileW;
    const dim3 grid((childW + 255u) / 256u, childH < kMaxGridRows ? childH : kMaxGridRows), block(256);
    if (srgb)
        hipLaunchKernelGGL(
            generate_mip_kernel<true>, grid, block, 0, stream, static_cast<const uint32_t *>(parent), parentW, parentH, pt,
            static_cast<uint32_t *>(child), childW, childH, ct);
    else
        hipLaunchKernelGGL(
            generate_mip_kernel<false>, grid, block, 0, stream, static_cast<const uint32_t *>(parent), parentW, parentH, pt,
            static_cast<uint32_t *>(child), childW, childH, ct);
}

__global__ __launch_bounds__(256) void untile_level_kernel(
    const uint32_t *__restrict__ tiled, uint32_t width, uint32_t height, uint32_t tilesPerRow, uint32_t *__restrict__ linear)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width) return;
    for (uint32_t j = blockIdx.y; j < height; j += gridDim.y) linear[(size_t)j * width + i] = tiled[tiled_word(tilesPerRow, i, j)];
}

void launch_untile_level(const void *tiled, uint32_t width, uint32_t height, void *linear, hipStream_t stream)
{
    if (width == 0 || height == 0) return;
    hipLaunchKernelGGL(
        untile_level_kernel, dim3((width + 255u) / 256u, height < kMaxGridRows ? height : kMaxGridRows), dim3(256), 0, stream, static_cast<const uint32_t *>(tiled), width, height,
        (width + kTexTileW - 1u) / kTexTileW, static_cast<uint32_t *>(linear));
}

// in6: (u, v, du/dx, dv/dx, du/dy, dv/dy) per record; out5: RGBA, lambda
__global__ __launch_bounds__(256) void sample_texture_lod_kernel(
    const DeviceScene s, const DeviceTextureMips *__restrict__ mips, uint32_t texture, uint32_t sampler, const float *__restrict__ in6,
    uint32_t n, float bias, float *__restrict__ out5)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = in6 + (size_t)i * 6u;
    const UvDerivatives d{r[2], r[3], r[4], r[5]};
    float lambda;
    const f4 c = sample_texture_lod(s, mips, texture, sampler, f2{r[0], r[1]}, d, bias, &lambda);
    float *o = out5 + (size_t)i * 5u;
    o[0] = c.x;
    o[1] = c.y;
    o[2] = c.z;
    o[3] = c.w;
    o[4] = lambda;
}

void launch_sample_texture_lod(
    const DeviceScene &s, const DeviceTextureMips *mips, uint32_t texture, uint32_t sampler, const float *in6, uint32_t n, float bias,
    float *out5, hipStream_t stream)
{
    if (n == 0) return;
    hipLaunchKernelGGL(sample_texture_lod_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, s, mips, texture, sampler, in6, n, bias, out5);
}

} // namespace ppt
