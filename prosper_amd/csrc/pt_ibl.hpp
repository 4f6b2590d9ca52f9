// pt_ibl.hpp — device functions shared by the image-based lighting passes (pt_ibl.hip: ImageBasedLighting's generation
// kernels) and their reader (pt_gbuffer_kernels.hip: deferred_shading_ibl_kernel, scene/skybox.glsl evalIBL).
//
// Every map is a cube stored as the sky is (DeviceScene::skybox): 6 faces +X, -X, +Y, -Y, +Z, -Z of (n + 2) x (n + 2)
// RGBA16F texels, the one-texel border holding the texels the seamless-edge rule finds on the neighbouring face, so a
// bilinear lookup is four plain loads.  The radiance mips follow one another from mip 0 (512) to mip 9 (1).
#pragma once

#include "pt_device.hpp"
#include "pt_gbuffer_kernels.hpp"

namespace ppt
{

// The three maps as deferred_shading_ibl_kernel reads them.
struct IblMaps
{
    const uint16_t *irradiance; // kIblIrradianceSize, bordered
    const uint16_t *radiance;   // kIblRadianceMips levels, bordered, ibl_radiance_offset(mip) RGBA texels apart
    const uint32_t *lut;        // kIblLutSize^2 R16G16 UNORM, row = roughness, column = NoV
};

// RGBA16F texel (i, j) in [-1, n] of a face of a bordered cube
PPT_D f3 fetch_bordered_rgb(const uint16_t *cube, uint32_t n, uint32_t face, int32_t i, int32_t j)
{
    const uint32_t n2 = n + 2u;
    const uint2 p = *reinterpret_cast<const uint2 *>(cube + 4u * (((size_t)face * n2 + (size_t)(j + 1)) * n2 + (size_t)(i + 1)));
    return f3{half_to_float(p.x & 0xFFFFu), half_to_float(p.x >> 16), half_to_float(p.y & 0xFFFFu)};
}

// Seamless bilinear lookup of a bordered n x n cube in direction d: sample_skybox's arithmetic over another cube.
PPT_D f3 sample_cube_bordered(const uint16_t *cube, uint32_t faceSize, f3 d)
{
    const int32_t n = (int32_t)faceSize;
    uint32_t face;
    float sc, tc, ma;
    cube_face_coords(d, face, sc, tc, ma);
    const float invMa = 1.0f / ma;
    const float ss = __builtin_fmaf(0.5f, sc * invMa, 0.5f);
    const float tt = __builtin_fmaf(0.5f, tc * invMa, 0.5f);
    const float u = __builtin_fmaf(ss, (float)n, -0.5f);
    const float v = __builtin_fmaf(tt, (float)n, -0.5f);
    const float fu = __builtin_floorf(u);
    const float fv = __builtin_floorf(v);
    const float a = u - fu;
    const float b = v - fv;
    // as in sample_skybox: a direction without a finite, non-zero largest component still loads inside the face
    int32_t i0 = f2i(fu);
    int32_t j0 = f2i(fv);
    i0 = i0 < -1 ? -1 : (i0 > n - 1 ? n - 1 : i0);
    j0 = j0 < -1 ? -1 : (j0 > n - 1 ? n - 1 : j0);
    const f3 t00 = fetch_bordered_rgb(cube, faceSize, face, i0, j0);
    const f3 t10 = fetch_bordered_rgb(cube, faceSize, face, i0 + 1, j0);
    const f3 t01 = fetch_bordered_rgb(cube, faceSize, face, i0, j0 + 1);
    const f3 t11 = fetch_bordered_rgb(cube, faceSize, face, i0 + 1, j0 + 1);
    const float w00 = (1.0f - a) * (1.0f - b);
    const float w10 = a * (1.0f - b);
    const float w01 = (1.0f - a) * b;
    const float w11 = a * b;
    return f3{__builtin_fmaf(w11, t11.x, __builtin_fmaf(w01, t01.x, __builtin_fmaf(w10, t10.x, w00 * t00.x))),
              __builtin_fmaf(w11, t11.y, __builtin_fmaf(w01, t01.y, __builtin_fmaf(w10, t10.y, w00 * t00.y))),
              __builtin_fmaf(w11, t11.z, __builtin_fmaf(w01, t01.z, __builtin_fmaf(w10, t10.z, w00 * t00.z)))};
}

// textureLod(skyboxRadiance, r, roughness * MAX_REFLECTION_LOD) (skybox.glsl:70-74): the level clamped to [0, 9], the
// two levels floor(lod) and floor(lod) + 1 (clamped) blended by the fraction, each a seamless bilinear lookup at its
// own size.  A fraction of 0 reads one level: the blend would return it unchanged (the maps are finite).
PPT_D f3 sample_radiance_trilinear(const uint16_t *radiance, f3 r, float roughness)
{
    const float lod = clamp_(roughness * 10.0f, 0.0f, (float)(kIblRadianceMips - 1u)); // NaN -> 0
    const float fl = __builtin_floorf(lod);
    const uint32_t l0 = (uint32_t)fl;
    const float t = lod - fl;
    const f3 c0 = sample_cube_bordered(radiance + 4u * ibl_radiance_offset(l0), kIblRadianceSize >> l0, r);
    if (!(t > 0.0f)) return c0;
    const uint32_t l1 = l0 + 1u < kIblRadianceMips ? l0 + 1u : kIblRadianceMips - 1u;
    const f3 c1 = sample_cube_bordered(radiance + 4u * ibl_radiance_offset(l1), kIblRadianceSize >> l1, r);
    return f3{mix(c0.x, c1.x, t), mix(c0.y, c1.y, t), mix(c0.z, c1.z, t)};
}

// texture(specularBrdfLut, (NoV, roughness)).rg: bilinear, clamp-to-edge, u = s * 512 - 0.5, UNORM codes / 65535
PPT_D f2 sample_brdf_lut(const uint32_t *lut, float NoV, float roughness)
{
    const int32_t n = (int32_t)kIblLutSize;
    const float u = __builtin_fmaf(NoV, (float)n, -0.5f);
    const float v = __builtin_fmaf(roughness, (float)n, -0.5f);
    const float fu = __builtin_floorf(u);
    const float fv = __builtin_floorf(v);
    const float a = u - fu;
    const float b = v - fv;
    const int32_t i0 = f2i(fu), j0 = f2i(fv);
    const int32_t ia = i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0);
    const int32_t ib = i0 + 1 < 0 ? 0 : (i0 + 1 > n - 1 ? n - 1 : i0 + 1);
    const int32_t ja = j0 < 0 ? 0 : (j0 > n - 1 ? n - 1 : j0);
    const int32_t jb = j0 + 1 < 0 ? 0 : (j0 + 1 > n - 1 ? n - 1 : j0 + 1);
    const uint32_t q00 = lut[ja * n + ia], q10 = lut[ja * n + ib], q01 = lut[jb * n + ia], q11 = lut[jb * n + ib];
    const float w00 = (1.0f - a) * (1.0f - b);
    const float w10 = a * (1.0f - b);
    const float w01 = (1.0f - a) * b;
    const float w11 = a * b;
    auto lerp2 = [&](uint32_t shift) {
        const float t00 = (float)((q00 >> shift) & 0xFFFFu) / 65535.0f, t10 = (float)((q10 >> shift) & 0xFFFFu) / 65535.0f;
        const float t01 = (float)((q01 >> shift) & 0xFFFFu) / 65535.0f, t11 = (float)((q11 >> shift) & 0xFFFFu) / 65535.0f;
        return __builtin_fmaf(w11, t11, __builtin_fmaf(w01, t01, __builtin_fmaf(w10, t10, w00 * t00)));
    };
    return f2{lerp2(0), lerp2(16)};
}

// importanceSampleIBLTrowbridgeReitz (common/sampling.glsl:97-106) before the tangent frame: the half vector of
// hammersley(i, 1024) (common/random.glsl:72-80) around +Z.  It depends on (i, alpha) only, so the passes keep a block's
// 1024 of them in LDS.
PPT_D f3 ibl_tangent_half_vector(uint32_t i, float alpha)
{
    const float xi0 = (float)i / (float)kIblSamples;
    const float xi1 = (float)__builtin_bitreverse32(i) * 2.32830643653896e-10f;
    const float phi = kTwoPi * xi0;
    const float cosTheta = sqrt_((1.0f - xi1) / (1.0f + (alpha * alpha - 1.0f) * xi1));
    const float sinTheta = sqrt_(1.0f - cosTheta * cosTheta);
    float sn, cs;
    sincos_(phi, sn, cs);
    return f3{sinTheta * cs, sinTheta * sn, cosTheta};
}

// sampling.glsl:108-110: the tangent frame around N
PPT_D void ibl_tangent_frame(f3 n, f3 &tx, f3 &ty)
{
    const f3 up = fabs_(n.z) < 0.999f ? f3{0.0f, 0.0f, 1.0f} : f3{1.0f, 0.0f, 0.0f};
    tx = normalize(cross(up, n));
    ty = normalize(cross(n, tx));
}

// sampling.glsl:112: tangent to world
PPT_D f3 ibl_to_world(f3 h, f3 tx, f3 ty, f3 n) { return normalize((tx * h.x + ty * h.y) + n * h.z); }

} // namespace ppt
