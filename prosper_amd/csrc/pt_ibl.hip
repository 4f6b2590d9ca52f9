// pt_ibl.hip — gfx950 kernels of ImageBasedLighting::recordGeneration (src/render/ImageBasedLighting.cpp): the three
// products evalIBL reads, generated once per sky.
//
//   ibl_irradiance_kernel   sample_irradiance.comp: 6 x 64^2 cosine-weighted hemisphere sums, one wave per texel
//   ibl_prefilter_kernel    prefilter_radiance.comp: 6 x 512^2 with 10 mips, 1024 GGX samples per texel, one lane per
//                           texel over one flattened grid of every face and mip
//   ibl_brdf_lut_kernel     integrate_specular_brdf.comp: the 512^2 split-sum LUT, one block per roughness row
//   ibl_border_kernel       the one-texel seamless border of every cube level (border_skybox_kernel's rule)
//
// Every lookup of the environment is the path tracer's own sample_skybox (seamless bilinear on mip 0 of the bordered
// sky), clamped per channel with min(s, 10) as both GLSL passes do.
#include "pt_ibl.hpp"

namespace ppt
{

// The texel-centre direction of both cube passes (sample_irradiance.comp:20-58, prefilter_radiance.comp:76-114)
PPT_D f3 ibl_texel_dir(uint32_t face, uint32_t i, uint32_t j, uint32_t n)
{
    const float cx = (float)i + 0.5f, cy = (float)j + 0.5f;
    const float res = (float)n, halfRes = res * 0.5f;
    float x, y, z;
    switch (face)
    {
    case 0: x = halfRes; y = (res - cy) - halfRes; z = (res - cx) - halfRes; break;
    case 1: x = -halfRes; y = (res - cy) - halfRes; z = cx - halfRes; break;
    case 2: x = cx - halfRes; y = halfRes; z = cy - halfRes; break;
    case 3: x = cx - halfRes; y = -halfRes; z = (res - cy) - halfRes; break;
    case 4: x = cx - halfRes; y = (res - cy) - halfRes; z = halfRes; break;
    default: x = (res - cx) - halfRes; y = (res - cy) - halfRes; z = -halfRes; break;
    }
    return normalize(f3{x, y, z});
}

PPT_D f3 clamped_sky(const DeviceScene &s, f3 d)
{
    const f3 c = sample_skybox(s, d);
    return f3{fmin_(c.x, 10.0f), fmin_(c.y, 10.0f), fmin_(c.z, 10.0f)};
}

// RGBA16F (r, g, b, 0) to interior texel (i, j) of a face of a bordered n x n cube
PPT_D void store_bordered(uint16_t *cube, uint32_t n, uint32_t face, uint32_t i, uint32_t j, f3 c)
{
    const uint32_t n2 = n + 2u;
    *reinterpret_cast<uint2 *>(cube + 4u * (((size_t)face * n2 + (j + 1u)) * n2 + (i + 1u))) =
        make_uint2(float_to_half(c.x) | (float_to_half(c.y) << 16), float_to_half(c.z));
}

constexpr uint32_t kIrrThetaSteps = 64, kIrrPhiSteps = 128;

// One wave per texel: lane l sums the azimuths l and l + 64 of every one of the 64 polar rings; the waves' partial sums
// meet in a butterfly.  The sines and cosines are one table per block.
__global__ __launch_bounds__(256) void ibl_irradiance_kernel(DeviceScene s, uint16_t *__restrict__ irradiance)
{
    __shared__ float sinTheta[kIrrThetaSteps], cosTheta[kIrrThetaSteps], sinPhi[kIrrPhiSteps], cosPhi[kIrrPhiSteps];
    const uint32_t tid = threadIdx.x;
    if (tid < kIrrThetaSteps)
    {
        // theta = .5 * PI * float(j) / float(thetaSteps)
        const float theta = (0.5f * kPi) * (float)tid / (float)kIrrThetaSteps;
        sincos_(theta, sinTheta[tid], cosTheta[tid]);
    }
    else if (tid < kIrrThetaSteps + kIrrPhiSteps)
    {
        // phi = 2. * PI * float(i) / float(phiSteps)
        const uint32_t k = tid - kIrrThetaSteps;
        const float phi = kTwoPi * (float)k / (float)kIrrPhiSteps;
        sincos_(phi, sinPhi[k], cosPhi[k]);
    }
    __syncthreads();
    const uint32_t n = kIblIrradianceSize;
    const uint32_t texel = blockIdx.x * 4u + (tid >> 6), lane = tid & 63u;
    if (texel >= 6u * n * n) return;
    const uint32_t face = texel / (n * n), j = (texel / n) % n, i = texel % n;
    const f3 normal = ibl_texel_dir(face, i, j, n);
    // avoid the singularity of the frame (sample_irradiance.comp:61-67)
    f3 up = fabs_(normal.y) < 0.99f ? f3{0.0f, 1.0f, 0.0f} : f3{1.0f, 0.0f, 0.0f};
    const f3 right = normalize(cross(up, normal));
    up = normalize(cross(normal, right));

    f3 sum = f3{0.0f, 0.0f, 0.0f};
    for (uint32_t t = 0; t < kIrrThetaSteps; ++t)
    {
        const float st = sinTheta[t], ct = cosTheta[t];
        f3 ring = f3{0.0f, 0.0f, 0.0f};
#pragma unroll
        for (uint32_t h = 0; h < 2u; ++h)
        {
            const uint32_t p = lane + 64u * h;
            const f3 tangentSample = f3{st * cosPhi[p], st * sinPhi[p], ct};
            const f3 sampleVec = (right * tangentSample.x + up * tangentSample.y) + normal * tangentSample.z;
            ring = ring + clamped_sky(s, sampleVec);
        }
        sum = sum + ring * (ct * st);
    }
#pragma unroll
    for (uint32_t off = 32; off > 0u; off >>= 1)
    {
        sum.x += __shfl_xor(sum.x, off, 64);
        sum.y += __shfl_xor(sum.y, off, 64);
        sum.z += __shfl_xor(sum.z, off, 64);
    }
    if (lane == 0u)
        store_bordered(irradiance, n, face, i, j, (sum * kPi) * (1.0f / (float)(kIrrThetaSteps * kIrrPhiSteps)));
}

// Blocks of the prefilter grid that one mip takes: 256 texels each, never across mips.
PPT_HD uint32_t prefilter_blocks(uint32_t mip)
{
    const uint32_t n = kIblRadianceSize >> mip;
    return (6u * n * n + 255u) / 256u;
}

// One lane per texel of every face and mip, the small mips' blocks first (their lanes run 1024 samples each and
// would otherwise be the grid's tail).  Roughness = mip / 10: at mip 0 every half vector is N itself (alpha = 0 makes
// cosTheta exactly 1), so the NoL-weighted mean of its 1024 equal samples is one lookup.
__global__ __launch_bounds__(256) void ibl_prefilter_kernel(DeviceScene s, uint16_t *__restrict__ radiance)
{
    __shared__ float hx[kIblSamples], hy[kIblSamples], hz[kIblSamples];
    const uint32_t tid = threadIdx.x;
    uint32_t b = blockIdx.x, mip = kIblRadianceMips - 1u;
    while (mip > 0u && b >= prefilter_blocks(mip))
    {
        b -= prefilter_blocks(mip);
        --mip;
    }
    const uint32_t n = kIblRadianceSize >> mip;
    const float roughness = (float)mip / (float)kIblRadianceMips;
    const float alpha = roughness * roughness;
    if (mip > 0u)
    {
        for (uint32_t k = tid; k < kIblSamples; k += 256u)
        {
            const f3 h = ibl_tangent_half_vector(k, alpha);
            hx[k] = h.x;
            hy[k] = h.y;
            hz[k] = h.z;
        }
    }
    __syncthreads();
    const uint32_t t = b * 256u + tid;
    if (t >= 6u * n * n) return;
    const uint32_t face = t / (n * n), j = (t / n) % n, i = t % n;
    const f3 N = ibl_texel_dir(face, i, j, n);
    const f3 V = N;
    f3 tx, ty;
    ibl_tangent_frame(N, tx, ty);
    f3 color;
    if (mip == 0u)
    {
        const f3 H = ibl_to_world(ibl_tangent_half_vector(0u, alpha), tx, ty, N);
        color = clamped_sky(s, H * (2.0f * dot(V, H)) - V);
    }
    else
    {
        f3 sum = f3{0.0f, 0.0f, 0.0f};
        float totalWeight = 0.0f;
#pragma unroll 2
        for (uint32_t k = 0; k < kIblSamples; ++k)
        {
            const f3 H = ibl_to_world(f3{hx[k], hy[k], hz[k]}, tx, ty, N);
            const f3 L = H * (2.0f * dot(V, H)) - V;
            const float NoL = saturate(dot(N, L));
            if (NoL > 0.0f)
            {
                sum = sum + clamped_sky(s, L) * NoL;
                totalWeight += NoL;
            }
        }
        color = sum / totalWeight; // > 0: sample 0 is H = N
    }
    store_bordered(radiance + 4u * ibl_radiance_offset(mip), n, face, i, j, color);
}

// One block per row (roughness = y / 512), two texels per lane (NoV = x / 512, no half-texel offset).  The row's 1024
// half vectors around N = +Z sit in LDS.  At NoV = 0 G_Vis is 0 / 0 and the sum NaN; saturate's minNum / maxNum turn
// it into 0, so column 0 stores (0, 0).
__global__ __launch_bounds__(256) void ibl_brdf_lut_kernel(uint32_t *__restrict__ lut)
{
    __shared__ float hx[kIblSamples], hy[kIblSamples], hz[kIblSamples];
    const uint32_t tid = threadIdx.x, y = blockIdx.x;
    const float roughness = (float)y / (float)kIblLutSize;
    const float alpha = roughness * roughness;
    const f3 N = f3{0.0f, 0.0f, 1.0f};
    f3 tx, ty;
    ibl_tangent_frame(N, tx, ty);
    for (uint32_t k = tid; k < kIblSamples; k += 256u)
    {
        const f3 H = ibl_to_world(ibl_tangent_half_vector(k, alpha), tx, ty, N);
        hx[k] = H.x;
        hy[k] = H.y;
        hz[k] = H.z;
    }
    __syncthreads();
    for (uint32_t x = tid; x < kIblLutSize; x += 256u)
    {
        const float NoV = (float)x / (float)kIblLutSize;
        const f3 V = f3{sqrt_(1.0f - NoV * NoV), 0.0f, NoV};
        float A = 0.0f, B = 0.0f;
        for (uint32_t k = 0; k < kIblSamples; ++k)
        {
            const f3 H = f3{hx[k], hy[k], hz[k]};
            const float VdotH = dot(V, H);
            const f3 L = H * (2.0f * VdotH) - V;
            const float NoL = saturate(L.z);
            const float NoH = saturate(H.z);
            const float VoH = saturate(VdotH);
            if (NoL > 0.0f)
            {
                const float G = schlick_trowbridge_reitz(NoL, NoV, alpha);
                const float GVis = (G * VoH) / (NoH * NoV);
                const float Fc = pow5(1.0f - VoH);
                A += (1.0f - Fc) * GVis;
                B += Fc * GVis;
            }
        }
        const float scale = saturate(A * (1.0f / (float)kIblSamples));
        const float bias = saturate(B * (1.0f / (float)kIblSamples));
        lut[(size_t)y * kIblLutSize + x] =
            (uint32_t)__builtin_rintf(scale * 65535.0f) | ((uint32_t)__builtin_rintf(bias * 65535.0f) << 16);
    }
}

// The border texels of one bordered n x n cube: the texel cube_texel_seamless finds for (i, j) outside the face, read
// from the neighbouring face's interior (which this kernel does not write).
__global__ __launch_bounds__(256) void ibl_border_kernel(uint2 *__restrict__ cube, uint32_t n)
{
    const uint32_t n2 = n + 2u;
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y, face = blockIdx.z;
    if (x >= n2 || (x > 0u && x <= n && y > 0u && y <= n)) return;
    const int32_t i = (int32_t)x - 1, j = (int32_t)y - 1;
    const float invN = 1.0f / (float)n;
    const float sc = __builtin_fmaf(2.0f * ((float)i + 0.5f), invN, -1.0f);
    const float tc = __builtin_fmaf(2.0f * ((float)j + 0.5f), invN, -1.0f);
    const f3 d = cube_face_dir(face, sc, tc);
    uint32_t f;
    float sc2, tc2, ma2;
    cube_face_coords(d, f, sc2, tc2, ma2);
    const float inv2 = 1.0f / ma2;
    const float ss = __builtin_fmaf(0.5f, sc2 * inv2, 0.5f);
    const float tt = __builtin_fmaf(0.5f, tc2 * inv2, 0.5f);
    int32_t si = f2i(__builtin_floorf(ss * (float)n));
    int32_t sj = f2i(__builtin_floorf(tt * (float)n));
    si = si < 0 ? 0 : (si >= (int32_t)n ? (int32_t)n - 1 : si);
    sj = sj < 0 ? 0 : (sj >= (int32_t)n ? (int32_t)n - 1 : sj);
    cube[((size_t)face * n2 + y) * n2 + x] = cube[((size_t)f * n2 + (uint32_t)sj + 1u) * n2 + (uint32_t)si + 1u];
}

static void launch_border(uint16_t *cube, uint32_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(
        ibl_border_kernel, dim3((n + 2u + 255u) / 256u, n + 2u, 6u), dim3(256), 0, stream, reinterpret_cast<uint2 *>(cube), n);
}

void launch_ibl_generation(
    const DeviceScene &s, uint16_t *irradiance, uint16_t *radiance, uint32_t *lut, hipEvent_t *events, hipStream_t stream)
{
    if (events) (void)hipEventRecord(events[0], stream);
    const uint32_t irrTexels = 6u * kIblIrradianceSize * kIblIrradianceSize;
    hipLaunchKernelGGL(ibl_irradiance_kernel, dim3(irrTexels / 4u), dim3(256), 0, stream, s, irradiance);
    launch_border(irradiance, kIblIrradianceSize, stream);
    if (events) (void)hipEventRecord(events[1], stream);
    uint32_t blocks = 0;
    for (uint32_t m = 0; m < kIblRadianceMips; ++m) blocks += prefilter_blocks(m);
    hipLaunchKernelGGL(ibl_prefilter_kernel, dim3(blocks), dim3(256), 0, stream, s, radiance);
    for (uint32_t m = 0; m < kIblRadianceMips; ++m)
        launch_border(radiance + 4u * ibl_radiance_offset(m), kIblRadianceSize >> m, stream);
    if (events) (void)hipEventRecord(events[2], stream);
    hipLaunchKernelGGL(ibl_brdf_lut_kernel, dim3(kIblLutSize), dim3(256), 0, stream, lut);
    if (events) (void)hipEventRecord(events[3], stream);
}

} // namespace ppt
