// pt_gbuffer_kernels.hpp — host-callable launchers of the gfx950 kernels of the passes over a G-buffer
// (pt_gbuffer_kernels.hip; ImageBasedLighting's generation in pt_ibl.hip).  Their C entry points: pt_gbuffer_passes.cpp,
// pt_forward_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_raster.hpp"
#include "pt_scene.hpp"

namespace ppt
{

// The camera terms the passes over a G-buffer read of CameraUniforms (named for the first of them, ReSTIR-DI)
struct RestirCamera
{
    float eye[3];
    float clipToWorld[16]; // column-major
    float cameraToClip22, cameraToClip32;
};
uint32_t restir_grid_blocks(uint32_t width, uint32_t height);
// reservoirs: width*height float2 (bits of the int light index, unbiasedContributionWeight)
void launch_restir_di_initial(
    const DeviceScene &s, uint32_t frameIndex, uint32_t width, uint32_t height, const RestirCamera &cam,
    const void *albedoRoughness, const void *normalMetallic, const float *nonLinearDepth, void *outReservoirs,
    hipStream_t stream);
// `inReservoirs` and `outReservoirs` must not overlap (a pixel reads its neighbours' input)
void launch_restir_di_spatial(
    const DeviceScene &s, uint32_t frameIndex, uint32_t width, uint32_t height, const RestirCamera &cam,
    const void *albedoRoughness, const void *normalMetallic, const float *nonLinearDepth, const void *inReservoirs,
    void *outReservoirs, hipStream_t stream);
void launch_restir_di_trace(
    const DeviceScene &s, uint32_t drawType, uint32_t frameIndex, uint32_t flags, uint32_t width, uint32_t height,
    const RestirCamera &cam, const void *albedoRoughness, const void *normalMetallic, const float *nonLinearDepth,
    const void *reservoirs, float4 *hdr, int32_t *stackOverflow, hipStream_t stream);
// Ray-traced G-buffer (gbuffer_trace_kernel): `r` carries the camera terms of pinhole_camera_ray and the extent, built as
// prosper_pt_render_frames builds them (r.pc is not read); worldToClip = cameraToClip * worldToCamera, column-major.
struct GBufferTraceParams
{
    RenderParams r;
    float worldToClip[16];
    uint32_t drawType, frameIndex, jitter;
    uint32_t opaqueOnly; // BLEND candidates are always rejected (PROSPER_PT_GBUFFER_OPAQUE_ONLY)
};
// albedoRoughness, normalMetallic: r.width*r.height float4; nonLinearDepth: r.width*r.height float.  Grid of
// restir_grid_blocks(r.width, r.height) blocks (the stack overflow array is sized for it).
// `lod` (nullptr: LOD 0, the instantiations of before): the material is sampled through the textures' mip chains
// (gbuffer_trace_kernel<.., .., true>); `derivatives` != nullptr also takes the uv forward differences the
// pixel sampled with, (du/dx, dv/dx, du/dy, dv/dy), zeros on a miss.
struct GBufferLodParams
{
    const DeviceTextureMips *mips; // beside s.textures
    float bias;
    float4 *derivatives; // r.width*r.height, or nullptr
};
void launch_gbuffer_trace(
    const DeviceScene &s, const GBufferTraceParams &g, void *albedoRoughness, void *normalMetallic, float *nonLinearDepth,
    int32_t *stackOverflow, hipStream_t stream, const GBufferLodParams *lod = nullptr);
// The same with a velocity target (gbuffer_trace_kernel<true>): the ray goes through the point that
// cameraToClip * worldToCamera puts on the pixel centre (g.jitter must be 0), and `velocity` takes
// (posNDC - currentJitter) - (prevPosNDC - previousJitter), y negated, clamped to [-1, 1], on hits and on the sky.
struct GBufferVelocityParams
{
    float worldToCamera[16], cameraToClip[16], previousWorldToCamera[16], previousCameraToClip[16]; // column-major
    float currentJitter[2], previousJitter[2];
    const prosper_ModelInstanceTransforms *previousTransforms; // device, by model instance; nullptr: the instances did not move
    float2 *velocity;                                          // r.width*r.height
};
void launch_gbuffer_trace_velocity(
    const DeviceScene &s, const GBufferTraceParams &g, const GBufferVelocityParams &v, void *albedoRoughness, void *normalMetallic,
    float *nonLinearDepth, int32_t *stackOverflow, hipStream_t stream, const GBufferLodParams *lod = nullptr);
// The resolve of the rasteriser's visibility image into the same four targets (raster_resolve_kernel):
// g as for the velocity variant (g.jitter 0; g.opaqueOnly and g.frameIndex are not read), the depth from the keys.
void launch_raster_resolve(
    const DeviceScene &s, const GBufferTraceParams &g, const RasterResolveTables &r, const GBufferVelocityParams &v, void *albedoRoughness,
    void *normalMetallic, float *nonLinearDepth, hipStream_t stream, const GBufferLodParams *lod = nullptr);
// Clustered lighting (LightClustering / DeferredShading).  The pointer grid is dimX x dimY x (kClusterZSlices + 1)
// uint2 (indexOffset, pointCount << 16 | spotCount), x fastest; cluster k owns the uint16 index entries
// [k * kClusterSlot, k * kClusterSlot + kClusterSlot), points first.  dropped: per cluster, the entries past the
// kClusterMaxPoints / kClusterMaxSpots of a type.
constexpr uint32_t kClusterDim = 32;       // LightClustering::clusterDim
constexpr uint32_t kClusterZSlices = 16;   // LightClustering::zSlices
constexpr uint32_t kClusterMaxPoints = 128; // maxPointIndicesPerTile
constexpr uint32_t kClusterMaxSpots = 128;  // maxSpotIndicesPerTile
constexpr uint32_t kClusterSlot = kClusterMaxPoints + kClusterMaxSpots;
struct ClusterParams
{
    float worldToCamera[16]; // column-major
    float cameraToClip00, cameraToClip11;
    float resolution[2]; // camera.resolution, which the tile scale is built from (not the extent)
    float near_, far_;
    uint32_t dimX, dimY; // ceil(extent / kClusterDim)
};
void launch_light_clustering(
    const DeviceScene &s, const ClusterParams &c, void *pointers, uint16_t *indices, uint32_t *dropped, hipStream_t stream);
// What a lit pass reads of the lights: the lists launch_light_clustering wrote with `params`, and the IBL maps
// launch_ibl_generation wrote, all three nullptr without IBL.
struct ClusteredLights
{
    ClusterParams params;
    const void *pointers;
    const uint16_t *indices;
    const uint16_t *irradiance, *radiance;
    const uint32_t *lut;
};
// The forward transparent pass (forward_transparent_kernel) in place over `hdr`, r.width*r.height float4,
// against `nonLinearDepth`.  g.jitter: the path tracer's sample; cameraJitter: the velocity entry's ray.  `l`: the lists for
// the same camera and extent.  stats: four uint32 the caller zeroed - pixels with a layer, the deepest pixel's layers, total
// layers (64 bits).  debugLayers != 0: layerCounts[pixel] and the first debugLayers layers of each pixel are written.
struct TransparentParams
{
    GBufferTraceParams g;
    float worldToCamera[16]; // column-major
    float cameraToClip22, cameraToClip32;
    float currentJitter[2];
    uint32_t cameraJitter;
    float near_, far_;
    uint32_t clustersX, clustersY;
    uint32_t debugLayers;
};
void launch_forward_transparent(
    const DeviceScene &s, const TransparentParams &p, const float *nonLinearDepth, const ClusteredLights &l, float4 *hdr,
    int32_t *stackOverflow, uint32_t *stats, uint32_t *layerCounts, prosper_pt_transparent_layer *layers, hipStream_t stream,
    const GBufferLodParams *lod = nullptr); // lod: every layer's material through the mip chains (its `derivatives` is not read)
// One lane per pixel over restir_grid_blocks(width, height); reads the lists of `l`, and with its maps set adds evalIBL after
// the spot lights (deferred_shading_ibl_kernel; ibl = 1).
void launch_deferred_shading(
    const DeviceScene &s, uint32_t drawType, uint32_t width, uint32_t height, const RestirCamera &cam, const ClusteredLights &l,
    const void *albedoRoughness, const void *normalMetallic, const float *nonLinearDepth, float4 *hdr, hipStream_t stream);
// The forward opaque pass (forward_opaque_kernel): the visibility image `r` shaded into `hdr` (overwritten,
// g.r.width*g.r.height float4), with `nonLinearDepth` from the keys and v.velocity as launch_raster_resolve writes them; g, r,
// v and lod as for the resolve, `l` as for the transparent pass.  shadedPixels: kForwardCountSlots counters,
// kForwardCountStride uint32 apart, which the caller zeroed: their sum is the covered pixels.  surfaces != nullptr: every
// pixel's surface record too (drawInstance 0xFFFFFFFF where nothing is drawn).
constexpr uint32_t kForwardCountSlots = 64, kForwardCountStride = 32;
void launch_forward_opaque(
    const DeviceScene &s, const GBufferTraceParams &g, const RasterResolveTables &r, const GBufferVelocityParams &v, const ClusteredLights &l,
    float4 *hdr, float *nonLinearDepth, uint32_t *shadedPixels, prosper_pt_transparent_layer *surfaces, hipStream_t stream,
    const GBufferLodParams *lod = nullptr);
// The rasterised transparent pass's resolve (raster_transparent_kernel) in place over `hdr`: the per-pixel
// fragment lists `t` (pt_raster.hpp) selected front to back, every layer shaded as launch_forward_opaque shades a winner and
// blended as launch_forward_transparent blends.  g, r, v (its velocity is not used) and l as for launch_forward_opaque.
// stats: kForwardCountSlots sets, kForwardCountStride uint32 apart, of { pixels with a list, layers shaded, the longest
// list }, which the caller zeroed.  debugLayers != 0: layerCounts[pixel] = the layers shaded, and the first debugLayers of
// them are written to layers[pixel * debugLayers ..].
void launch_raster_transparent(
    const DeviceScene &s, const GBufferTraceParams &g, const RasterResolveTables &r, const RasterLayerLists &t, const GBufferVelocityParams &v,
    const ClusteredLights &l, float4 *hdr, uint32_t *stats, uint32_t debugLayers, uint32_t *layerCounts, prosper_pt_transparent_layer *layers,
    hipStream_t stream, const GBufferLodParams *lod = nullptr);
// Image-based lighting (ImageBasedLighting / evalIBL).  Every cube is stored with a one-texel seamless border, as the
// sky is: 6 faces of (n + 2)^2 RGBA16F texels.  Radiance mip m (size kIblRadianceSize >> m) starts
// ibl_radiance_offset(m) RGBA texels into its buffer; the LUT is kIblLutSize^2 R16G16 UNORM, row = roughness.
constexpr uint32_t kIblIrradianceSize = 64; // SkyboxResources::sSkyboxIrradianceResolution
constexpr uint32_t kIblRadianceSize = 512;  // sSkyboxRadianceResolution
constexpr uint32_t kIblRadianceMips = 10;   // getMipCount(512)
constexpr uint32_t kIblLutSize = 512;       // sSpecularBrdfLutResolution
constexpr uint32_t kIblSamples = 1024;      // NumSamples of prefilter_radiance.comp and integrate_specular_brdf.comp
__host__ __device__ constexpr size_t ibl_radiance_offset(uint32_t mip)
{
    size_t offset = 0;
    for (uint32_t m = 0; m < mip; ++m)
        offset += 6u * (size_t)((kIblRadianceSize >> m) + 2u) * ((kIblRadianceSize >> m) + 2u);
    return offset;
}
constexpr size_t kIblIrradianceTexels = 6u * (size_t)(kIblIrradianceSize + 2u) * (kIblIrradianceSize + 2u);
constexpr size_t kIblRadianceTexels = ibl_radiance_offset(kIblRadianceMips);
// The three generation passes on `stream` from the scene's sky (a scene without one gives zero maps).  `events`
// (optional, 4): recorded before the irradiance pass, the radiance pass, the LUT pass and after it.
void launch_ibl_generation(
    const DeviceScene &s, uint16_t *irradiance, uint16_t *radiance, uint32_t *lut, hipEvent_t *events, hipStream_t stream);

} // namespace ppt
