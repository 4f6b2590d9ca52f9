// pt_culling.hip — gfx950 kernels of prosper's visibility system.
//
//   hiz_tile_kernel   hiz_downsampler.comp over ext/ffx_spd.h: one workgroup of 256 lanes per 64 x 64 source tile makes
//                     up to six levels of the depth pyramid, every texel the MINIMUM (reverse-Z: the farthest) of its
//                     source footprint.  Launched over the depth for levels 0-5 and, where the pyramid has more, once
//                     more as a single workgroup over level 5 for the rest: the kernel boundary is what makes the
//                     other workgroups' level-5 texels visible (SPD's single launch hands them over through a counter).
//
// A lane owns a 4 x 4 block of the source: four row loads (16 bytes each where the rows allow it), two levels in
// registers.  The lanes of a wave lie in Morton order over an 8 x 8 arrangement of such blocks, so that the 2 x 2
// neighbours of every further level are the lanes that differ in two consecutive bits: levels 2, 3 and 4 are lane
// exchanges (DPP quad permutes, ds_swizzle, one readlane), and only level 5, which joins the four waves, goes through
// LDS.  min is exact and order-free, so the grouping is free; a NaN loses against a number (v_min_f32), two NaNs stay.
#include "pt_culling.hpp"

#include "pt_math.hpp"

namespace ppt
{

namespace
{

#define PPT_CL __device__ __forceinline__

PPT_CL float min4(float a, float b, float c, float d) { return __builtin_fminf(__builtin_fminf(a, b), __builtin_fminf(c, d)); }

// the value of lane (lane ^ 1) / (lane ^ 2): DPP quad_perm [1, 0, 3, 2] / [2, 3, 0, 1]
template <int Ctrl> PPT_CL float quad_exchange(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), Ctrl, 0xF, 0xF, false));
}
// the value of lane (lane ^ Xor), Xor < 32: ds_swizzle in bit-mask mode (and 0x1F, or 0, xor Xor); no LDS memory
template <int Xor> PPT_CL float swizzle_exchange(float v)
{
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1F | (Xor << 10)));
}

PPT_CL void store_texel(const HizTileParams &p, uint32_t level, uint32_t x, uint32_t y, float v)
{
    // SpdStore: writes that would have gone over the level are skipped
    if (x < p.dstW[level] && y < p.dstH[level]) p.dst[level][(size_t)y * p.dstW[level] + x] = v;
}

// Rows16: the source rows are whole, 16-byte aligned float4s (a width that is a multiple of 4 on an aligned base)
// The 64 x 64 source tile (tileX, tileY) by the 256 lanes of a workgroup; `waveMin`: four floats of LDS.
template <bool Rows16> PPT_CL void hiz_tile(const HizTileParams &p, uint32_t tileX, uint32_t tileY, float *waveMin)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // Morton order inside the wave: lane bits 0, 2, 4 are x, bits 1, 3, 5 are y
    const uint32_t mx = (lane & 1u) | ((lane >> 1) & 2u) | ((lane >> 2) & 4u);
    const uint32_t my = ((lane >> 1) & 1u) | ((lane >> 2) & 2u) | ((lane >> 3) & 4u);
    // the lane's 4 x 4 block among the tile's 16 x 16: a wave takes a quadrant
    const uint32_t bx = (wave & 1u) * 8u + mx, by = (wave >> 1) * 8u + my;
    const uint32_t x0 = tileX * kHizTile + bx * 4u, y0 = tileY * kHizTile + by * 4u;
    const uint32_t xl = p.srcW - 1u, yl = p.srcH - 1u; // SpdLoadSourceImage / SpdLoad: clamp to edge

    float4 r[4];
    if (Rows16)
    {
        // rows of whole float4s: a block lies inside the rows, or wholly to their right where every texel is the edge's
        if (x0 < p.srcW)
        {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
            {
                const uint32_t y = y0 + k < yl ? y0 + k : yl;
                r[k] = *reinterpret_cast<const float4 *>(p.src + (size_t)y * p.srcW + x0);
            }
        }
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
            {
                const uint32_t y = y0 + k < yl ? y0 + k : yl;
                const float e = p.src[(size_t)y * p.srcW + xl];
                r[k] = make_float4(e, e, e, e);
            }
        }
    }
    else
    {
        const uint32_t xa = x0 < xl ? x0 : xl, xb = x0 + 1u < xl ? x0 + 1u : xl;
        const uint32_t xc = x0 + 2u < xl ? x0 + 2u : xl, xd = x0 + 3u < xl ? x0 + 3u : xl;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
        {
            const uint32_t y = y0 + k < yl ? y0 + k : yl;
            const float *row = p.src + (size_t)y * p.srcW;
            r[k] = make_float4(row[xa], row[xb], row[xc], row[xd]);
        }
    }

    // level 0: the block's 2 x 2 texels, two to a store where the level has room for the pair
    const float a00 = min4(r[0].x, r[0].y, r[1].x, r[1].y), a10 = min4(r[0].z, r[0].w, r[1].z, r[1].w);
    const float a01 = min4(r[2].x, r[2].y, r[3].x, r[3].y), a11 = min4(r[2].z, r[2].w, r[3].z, r[3].w);
    {
        const uint32_t x = tileX * 32u + bx * 2u, y = tileY * 32u + by * 2u;
        const uint32_t w = p.dstW[0], h = p.dstH[0];
        if (x + 1u < w) // (x is even and w a power of two: the pair is 8-byte aligned)
        {
            if (y < h) *reinterpret_cast<float2 *>(p.dst[0] + (size_t)y * w + x) = make_float2(a00, a10);
            if (y + 1u < h) *reinterpret_cast<float2 *>(p.dst[0] + (size_t)(y + 1u) * w + x) = make_float2(a01, a11);
        }
        else
        {
            store_texel(p, 0, x, y, a00);
            store_texel(p, 0, x, y + 1u, a01);
        }
    }
    if (p.levels < 2u) return; // (the same in every lane, as every return below)
    float v = min4(a00, a10, a01, a11);
    store_texel(p, 1, tileX * 16u + bx, tileY * 16u + by, v);
    if (p.levels < 3u) return;
    v = __builtin_fminf(v, quad_exchange<0xB1>(v));
    v = __builtin_fminf(v, quad_exchange<0x4E>(v));
    if ((lane & 3u) == 0u) store_texel(p, 2, tileX * 8u + (bx >> 1), tileY * 8u + (by >> 1), v);
    if (p.levels < 4u) return;
    v = __builtin_fminf(v, swizzle_exchange<4>(v));
    v = __builtin_fminf(v, swizzle_exchange<8>(v));
    if ((lane & 15u) == 0u) store_texel(p, 3, tileX * 4u + (bx >> 2), tileY * 4u + (by >> 2), v);
    if (p.levels < 5u) return;
    v = __builtin_fminf(v, swizzle_exchange<16>(v));
    // lanes 0 and 32 hold the halves of the wave
    const float q = __builtin_fminf(
        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)),
        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)));
    if (lane == 0u)
    {
        store_texel(p, 4, tileX * 2u + (wave & 1u), tileY * 2u + (wave >> 1), q);
        waveMin[wave] = q;
    }
    if (p.levels < 6u) return;
    __syncthreads();
    if (threadIdx.x == 0u) store_texel(p, 5, tileX, tileY, min4(waveMin[0], waveMin[1], waveMin[2], waveMin[3]));
}

template <bool Rows16> __global__ __launch_bounds__(256) void hiz_tile_kernel(const HizTileParams p)
{
    __shared__ float waveMin[4];
    hiz_tile<Rows16>(p, blockIdx.x, blockIdx.y, waveMin);
}

uint32_t bit_ceil_(uint32_t v)
{
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

} // namespace

bool hiz_layout(uint32_t width, uint32_t height, HizLayout *out)
{
    if (width <= 1u || height <= 1u || width > 4096u || height > 4096u) return false;
    HizLayout l = {};
    const uint32_t w0 = bit_ceil_(width) / 2u, h0 = bit_ceil_(height) / 2u;
    uint32_t side = w0 > h0 ? w0 : h0;
    while (side)
    {
        ++l.levelCount; // floor(log2(side)) + 1
        side >>= 1;
    }
    if (l.levelCount > kHizMaxLevels) return false;
    for (uint32_t i = 0; i < l.levelCount; ++i)
    {
        l.levelW[i] = (w0 >> i) ? (w0 >> i) : 1u;
        l.levelH[i] = (h0 >> i) ? (h0 >> i) : 1u;
        l.levelOffset[i] = l.floats;
        l.floats += ((size_t)l.levelW[i] * l.levelH[i] + 63u) & ~(size_t)63u;
    }
    *out = l;
    return true;
}

void launch_hiz_downsample(const float *depth, uint32_t width, uint32_t height, float *pyramid, const HizLayout &layout, hipStream_t stream)
{
    HizTileParams p = {};
    p.src = depth;
    p.srcW = width;
    p.srcH = height;
    uint32_t first = 0;
    // SpdSetup over the rectangle (0, 0, 2 * level 0): the tiles cover the extent rounded up to its power of two
    dim3 grid((layout.levelW[0] * 2u + kHizTile - 1u) / kHizTile, (layout.levelH[0] * 2u + kHizTile - 1u) / kHizTile);
    while (first < layout.levelCount)
    {
        p.levels = layout.levelCount - first < kHizLevelsPerLaunch ? layout.levelCount - first : kHizLevelsPerLaunch;
        for (uint32_t i = 0; i < p.levels; ++i)
        {
            p.dst[i] = pyramid + layout.levelOffset[first + i];
            p.dstW[i] = layout.levelW[first + i];
            p.dstH[i] = layout.levelH[first + i];
        }
        if ((p.srcW & 3u) == 0u && (reinterpret_cast<uintptr_t>(p.src) & 15u) == 0u)
            hipLaunchKernelGGL(hiz_tile_kernel<true>, grid, dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL(hiz_tile_kernel<false>, grid, dim3(256), 0, stream, p);
        // the rest comes from the last level made: at most 64 x 64 texels, one tile
        first += p.levels;
        p.src = p.dst[p.levels - 1u];
        p.srcW = p.dstW[p.levels - 1u];
        p.srcH = p.dstH[p.levels - 1u];
        grid = dim3(1, 1);
    }
}


// ---- per-instance uniform scales, the draw-list generator and the culler ----
//
//   instance_scales_kernel      World.cpp:485-498: one lane per model instance
//   draw_list_generator_kernel  draw_list_generator.comp: one WAVE per draw instance (the reference: a workgroup of 16).  A
//                               mesh has dozens to thousands of meshlets, so a wave takes one range with ONE atomic and writes
//                               it 64 consecutive entries at a time; four instances to a wave would pay an atomic each anyway
//   draw_list_culler_kernel     draw_list_culler.comp operation for operation in float32 (DESIGN.md f17 lists the order of every
//                               sum), one lane per entry of the input list; the outputs by wave ballot: one atomic per wave
//                               per list, an exclusive prefix inside the wave
namespace
{

PPT_CL float row_len(const prosper_mat3x4 &m, int r)
{
    const f3 v = r == 0 ? f3{m.col[0].x, m.col[1].x, m.col[2].x}
               : r == 1 ? f3{m.col[0].y, m.col[1].y, m.col[2].y}
                        : f3{m.col[0].z, m.col[1].z, m.col[2].z};
    return length(v);
}
// World.cpp:34-40
PPT_CL bool relative_eq(float a, float b, float maxRelativeDiff)
{
    const float diff = fabs_(a - b);
    const float maxMagnitude = fmax_(fabs_(a), fabs_(b));
    return diff < maxRelativeDiff * maxMagnitude;
}

__global__ __launch_bounds__(256) void instance_scales_kernel(const prosper_ModelInstanceTransforms *transforms, float *scales, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const prosper_mat3x4 m = transforms[i].modelToWorld;
    // lengths of rows instead of columns because of the transposed 3x4
    const float sx = row_len(m, 0), sy = row_len(m, 1), sz = row_len(m, 2);
    scales[i] = relative_eq(sx, sy, 0.0001f) && relative_eq(sx, sz, 0.0001f) ? sx : 0.0f; // 0: non-uniform
}

__global__ __launch_bounds__(256) void draw_list_generator_kernel(const DrawListGeneratorParams p)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t drawInstanceIndex = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (drawInstanceIndex >= p.drawInstanceCount) return; // (the whole wave)
    const prosper_DrawInstance instance = p.drawInstances[drawInstanceIndex];
    const uint32_t meshletCount = p.meshletCounts[instance.meshIndex];
    if (meshletCount == 0u) return; // not loaded yet
    const bool blend = p.materials[instance.materialIndex].alphaMode == PROSPER_ALPHA_MODE_BLEND;
    if ((p.matchTransparents == 1u) != blend) return;
    uint32_t start = 0;
    if (lane == 0u) start = atomicAdd(p.outList, meshletCount);
    start = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
    for (uint32_t m = lane; m < meshletCount; m += 64u)
    {
        const uint32_t at = start + m;
        if (at < p.capacity) // (the host's bound holds; an index is checked all the same)
        {
            p.outList[1u + 2u * at] = drawInstanceIndex;
            p.outList[2u + 2u * at] = m;
        }
    }
}

// row `r` of m * (p, 1) and of m * v, column-major m: fma chains from the w / x term on
PPT_CL float row_point(const float *m, uint32_t r, f3 p)
{
    return __builtin_fmaf(m[8 + r], p.z, __builtin_fmaf(m[4 + r], p.y, __builtin_fmaf(m[r], p.x, m[12 + r])));
}
PPT_CL float row_vec4(const float *m, uint32_t r, float x, float y, float z, float w)
{
    return __builtin_fmaf(m[12 + r], w, __builtin_fmaf(m[8 + r], z, __builtin_fmaf(m[4 + r], y, m[r] * x)));
}
PPT_CL float signed_distance(const float *plane, f3 p)
{
    return __builtin_fmaf(plane[2], p.z, __builtin_fmaf(plane[1], p.y, __builtin_fmaf(plane[0], p.x, plane[3])));
}

struct Bounds
{
    f3 center;
    float radius;
    f3 coneAxis;
    float coneCutoff;
};

// the texel of level `mip` a nearest sampler with a transparent-black border returns
PPT_CL float hiz_texel(const DrawListCullerParams &p, uint32_t mip, int32_t x, int32_t y)
{
    const uint32_t w = (p.hizResolution[0] >> mip) ? (p.hizResolution[0] >> mip) : 1u;
    const uint32_t h = (p.hizResolution[1] >> mip) ? (p.hizResolution[1] >> mip) : 1u;
    if (x < 0 || y < 0 || (uint32_t)x >= w || (uint32_t)y >= h) return 0.0f;
    return p.hizLevels[mip][(size_t)y * w + (uint32_t)x];
}

PPT_CL bool is_sphere_occluded(const DrawListCullerParams &p, const Bounds &b)
{
    if (p.hizMipCount == 0u) return false;
    const float cvx = row_point(p.worldToCamera, 0, b.center), cvy = row_point(p.worldToCamera, 1, b.center);
    const float cvz = row_point(p.worldToCamera, 2, b.center), cvw = row_point(p.worldToCamera, 3, b.center);
    // projectSphereView(vec3(centerInView.xy, -centerInView.z), radius * maxViewScale, near, P00, P11)
    const float cx = cvx, cy = cvy, cz = -cvz;
    const float r = b.radius * p.maxViewScale;
    if (cz < r + p.near_) return false; // the eye inside the bounds, or the bounds behind it
    const float crx = cx * r, cry = cy * r, crz = cz * r;
    const float czr2 = cz * cz - r * r;
    const float vx = sqrt_(cx * cx + czr2);
    const float minx = (vx * cx - crz) / (vx * cz + crx);
    const float maxx = (vx * cx + crz) / (vx * cz - crx);
    const float vy = sqrt_(cy * cy + czr2);
    const float miny = (vy * cy - crz) / (vy * cz + cry);
    const float maxy = (vy * cy + crz) / (vy * cz - cry);
    const float P00 = p.cameraToClip[0], P11 = p.cameraToClip[5];
    // aabb.xwzy * (0.5, -0.5, 0.5, -0.5) + 0.5
    const float ax = minx * P00 * 0.5f + 0.5f, ay = maxy * P11 * -0.5f + 0.5f;
    const float az = maxx * P00 * 0.5f + 0.5f, aw = miny * P11 * -0.5f + 0.5f;
    const float dx = (az - ax) * p.resolution[0], dy = (aw - ay) * p.resolution[1];
    const float pxDiameter = sqrt_(__builtin_fmaf(dy, dy, dx * dx));
    // max(floor(log2(pxDiameter)), 0) is the float's unbiased exponent where that is positive: the same integer for every
    // finite positive input, and no libm in the contract.  (A NaN or an infinity lands on the top-level shortcut.)
    const uint32_t exponent = (f2u(pxDiameter) >> 23) & 0xFFu;
    const uint32_t hizMip = exponent > 127u ? exponent - 127u : 0u;

    const f3 eye = f3{p.eye[0], p.eye[1], p.eye[2]};
    const f3 viewWorldDir = normalize(eye - b.center);
    const f3 closest = b.center + viewWorldDir * b.radius;
    const float closestDepth = row_point(p.clipFromWorld, 2, closest) / row_point(p.clipFromWorld, 3, closest);

    if (hizMip >= p.hizMipCount - 1u) return closestDepth < hiz_texel(p, p.hizMipCount - 1u, 0, 0);
    // (the shader divides by hizResolution >> hizMip, which is 0 on a pyramid whose sides differ by more than a factor of
    // two: max(., 1) here, the level's real extent)
    const uint32_t mw = (p.hizResolution[0] >> hizMip) ? (p.hizResolution[0] >> hizMip) : 1u;
    const uint32_t mh = (p.hizResolution[1] >> hizMip) ? (p.hizResolution[1] >> hizMip) : 1u;
    const float inv = 1.0f / row_vec4(p.cameraToClip, 3, cvx, cvy, cvz, cvw);
    float u = row_vec4(p.cameraToClip, 0, cvx, cvy, cvz, cvw) * inv * 0.5f + 0.5f;
    float v = row_vec4(p.cameraToClip, 1, cvx, cvy, cvz, cvw) * inv * 0.5f + 0.5f;
    u = u * p.hizUvScale[0] * (float)mw - 0.5f;
    v = v * p.hizUvScale[1] * (float)mh - 0.5f;
    // floor, + 0.5, / mipResolution, and the gather's own * mipResolution - 0.5: the extents are powers of two, so the
    // round trip is exact and the gather's first texel is the floor itself
    const int32_t x0 = f2i(__builtin_floorf(u)), y0 = f2i(__builtin_floorf(v));
    const int32_t x1 = x0 == 2147483647 ? x0 : x0 + 1, y1 = y0 == 2147483647 ? y0 : y0 + 1;
    const float hizDepth = fmin_(fmin_(hiz_texel(p, hizMip, x0, y0), hiz_texel(p, hizMip, x1, y0)),
                                 fmin_(hiz_texel(p, hizMip, x0, y1), hiz_texel(p, hizMip, x1, y1)));
    return closestDepth < hizDepth;
}

PPT_CL uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// the lane's slot among the set lanes of `mask`, which start at what one atomic on `counter` (and on `mirror`) returned
PPT_CL uint32_t ballot_slot(unsigned long long mask, uint32_t lane, uint32_t *counter, uint32_t *mirror)
{
    const uint32_t n = (uint32_t)__popcll(mask);
    uint32_t start = 0;
    if (lane == 0u && n != 0u)
    {
        start = atomicAdd(counter, n);
        if (mirror) atomicAdd(mirror, n);
    }
    start = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
    return start + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void draw_list_culler_kernel(const DrawListCullerParams p)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t threadIndex = blockIdx.x * 256u + threadIdx.x;
    const uint32_t inCount = p.inList[0] < p.capacity ? p.inList[0] : p.capacity;
    // groupsX is the write pointer; the other two are set here, by a dispatch that has something to cull (the argument
    // writer's empty case leaves 0, 0, 0)
    if (threadIndex == 0u && inCount != 0u) p.outArgs[1] = 1u, p.outArgs[2] = 1u;
    const bool live = threadIndex < inCount; // (lanes past the count stay for the ballots)
    bool visible = false, occluded = false;
    uint32_t drawInstanceIndex = 0, meshletIndex = 0, triangles = 0;
    if (live)
    {
        drawInstanceIndex = p.inList[1u + 2u * threadIndex];
        meshletIndex = p.inList[2u + 2u * threadIndex];
        const prosper_DrawInstance instance = p.drawInstances[drawInstanceIndex];
        const prosper_GeometryMetadata md = p.metadatas[instance.meshIndex];
        const uint32_t *words = static_cast<const uint32_t *>(p.geometryBuffers[md.bufferIndex]);
        triangles = words[md.meshletsOffset + 4u * meshletIndex + 3u];
        const float scale = p.scales[instance.modelInstanceIndex];
        visible = true;
        if (scale != 0.0f)
        {
            const uint32_t *bw = words + md.meshletBoundsOffset + 5u * meshletIndex;
            const prosper_mat3x4 m = p.transforms[instance.modelInstanceIndex].modelToWorld;
            Bounds b;
            const f3 c = f3{u2f(bw[0]), u2f(bw[1]), u2f(bw[2])};
            const int32_t cone = (int32_t)bw[4];
            const f3 axis = f3{(float)((cone << 24) >> 24) / 127.0f, (float)((cone << 16) >> 24) / 127.0f, (float)((cone << 8) >> 24) / 127.0f};
            b.coneCutoff = (float)(cone >> 24) / 127.0f;
            // transformBounds: the centre through the full modelToWorld, the axis through its 3x3
            b.center = f3{__builtin_fmaf(c.z, m.col[0].z, __builtin_fmaf(c.y, m.col[0].y, __builtin_fmaf(c.x, m.col[0].x, m.col[0].w))),
                          __builtin_fmaf(c.z, m.col[1].z, __builtin_fmaf(c.y, m.col[1].y, __builtin_fmaf(c.x, m.col[1].x, m.col[1].w))),
                          __builtin_fmaf(c.z, m.col[2].z, __builtin_fmaf(c.y, m.col[2].y, __builtin_fmaf(c.x, m.col[2].x, m.col[2].w)))};
            b.radius = fabs_(u2f(bw[3]) * scale);
            b.coneAxis = normalize(f3{__builtin_fmaf(axis.z, m.col[0].z, __builtin_fmaf(axis.y, m.col[0].y, axis.x * m.col[0].x)),
                                      __builtin_fmaf(axis.z, m.col[1].z, __builtin_fmaf(axis.y, m.col[1].y, axis.x * m.col[1].x)),
                                      __builtin_fmaf(axis.z, m.col[2].z, __builtin_fmaf(axis.y, m.col[2].y, axis.x * m.col[2].x))});
            bool outside = false;
#pragma unroll
            for (int k = 0; k < 6; ++k) outside = outside || signed_distance(p.planes[k], b.center) < -b.radius;
            visible = !outside;
            if (visible)
            {
                // isConeCapHidden, from meshoptimizer.h
                const f3 d = b.center - f3{p.eye[0], p.eye[1], p.eye[2]};
                visible = !(dot(d, b.coneAxis) >= b.coneCutoff * length(d) + b.radius);
            }
            if (visible)
            {
                occluded = is_sphere_occluded(p, b);
                visible = !occluded;
            }
        }
    }
    {
        const unsigned long long mask = __ballot(visible);
        const uint32_t at = ballot_slot(mask, lane, p.outList, p.outArgs); // count, mirrored into groupsX
        if (visible && at < p.capacity)
        {
            p.outList[1u + 2u * at] = drawInstanceIndex;
            p.outList[2u + 2u * at] = meshletIndex;
        }
        // ours: prosper counts the triangles in its mesh shader
        const uint32_t tris = wave_sum(visible ? triangles : 0u);
        if (lane == 0u && mask != 0ull)
        {
            atomicAdd(&p.stats->drawnMeshlets, (uint32_t)__popcll(mask));
            atomicAdd(&p.stats->rasterizedTriangles, tris);
        }
    }
    if (p.outSecondPhase)
    {
        const unsigned long long mask = __ballot(occluded);
        const uint32_t at = ballot_slot(mask, lane, p.outSecondPhase, nullptr);
        if (occluded && at < p.capacity)
        {
            p.outSecondPhase[1u + 2u * at] = drawInstanceIndex;
            p.outSecondPhase[2u + 2u * at] = meshletIndex;
        }
    }
}

} // namespace

void launch_instance_scales(const prosper_ModelInstanceTransforms *transforms, float *scales, uint32_t count, hipStream_t stream)
{
    if (count == 0u) return;
    hipLaunchKernelGGL(instance_scales_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, transforms, scales, count);
}

void launch_draw_list_generator(const DrawListGeneratorParams &p, hipStream_t stream)
{
    if (p.drawInstanceCount == 0u) return;
    hipLaunchKernelGGL(draw_list_generator_kernel, dim3((p.drawInstanceCount + 3u) / 4u), dim3(256), 0, stream, p);
}

void mat4_mul(const float a[16], const float b[16], float out[16])
{
    for (int j = 0; j < 4; ++j)
        for (int r = 0; r < 4; ++r)
            out[4 * j + r] = __builtin_fmaf(a[12 + r], b[4 * j + 3], __builtin_fmaf(a[8 + r], b[4 * j + 2], __builtin_fmaf(a[4 + r], b[4 * j + 1], a[r] * b[4 * j])));
}

void launch_draw_list_culler(const DrawListCullerParams &p, hipStream_t stream)
{
    if (p.upperBound == 0u) return;
    hipLaunchKernelGGL(draw_list_culler_kernel, dim3((p.upperBound + 255u) / 256u), dim3(256), 0, stream, p);
}

} // namespace ppt
