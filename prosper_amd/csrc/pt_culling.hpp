// pt_culling.hpp — host-callable launchers of the gfx950 kernels of prosper's visibility system (pt_culling.hip; DESIGN.md
// f17): the depth pyramid (src/render/HierarchicalDepthDownsampler.cpp, res/shader/hiz_downsampler.comp over
// ext/ffx_spd.h), the per-instance uniform scales (World.cpp:485-498), the draw-list generator and the culler
// (src/render/MeshletCuller.cpp, draw_list_generator.comp, draw_list_culler.comp).  Their C entry points: pt_culling_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/prosper_pt/prosper_pt.h"
#include "pt_scene.hpp"

namespace ppt
{

constexpr uint32_t kHizMaxLevels = 12;      // HierarchicalDepthDownsampler.cpp sMaxMips
constexpr uint32_t kHizLevelsPerLaunch = 6; // what one workgroup makes of its 64 x 64 source tile (SPD's mips 0-5)
constexpr uint32_t kHizTile = 64;

// The extents of a pyramid over a `width` x `height` depth (HierarchicalDepthDownsampler::record): level 0 is
// bit_ceil(extent) / 2, level l is max(level 0 >> l, 1), floor(log2(larger side of level 0)) + 1 levels.
struct HizLayout
{
    uint32_t levelCount;
    uint32_t levelW[kHizMaxLevels], levelH[kHizMaxLevels];
    size_t levelOffset[kHizMaxLevels]; // in floats; every level starts on a 256-byte boundary
    size_t floats;                     // of the whole pyramid
};
// false: an extent that is not above 1, or more than kHizMaxLevels levels (a side above 4096)
bool hiz_layout(uint32_t width, uint32_t height, HizLayout *out);

// One launch of the tile kernel: up to six levels from a `srcW` x `srcH` source whose coordinates clamp to its edge.
// The first launch reads the depth, the second (a single workgroup) level 5.
struct HizTileParams
{
    const float *src;
    uint32_t srcW, srcH;
    uint32_t levels; // 1 .. kHizLevelsPerLaunch
    float *dst[kHizLevelsPerLaunch];
    uint32_t dstW[kHizLevelsPerLaunch], dstH[kHizLevelsPerLaunch];
};

// Every level of `layout` under `pyramid` from the `width` x `height` depth: one workgroup per 64 x 64 source tile makes
// levels 0-5, and where there are more a second launch of one workgroup makes the rest from level 5.
void launch_hiz_downsample(const float *depth, uint32_t width, uint32_t height, float *pyramid, const HizLayout &layout, hipStream_t stream);

// ---- the per-instance uniform scales (World.cpp:485-498) ----
// scales[i] = the common length of the three rows of transforms[i].modelToWorld, or 0 where they differ by more than
// relativeEq's 1e-4: one lane per model instance.
void launch_instance_scales(const prosper_ModelInstanceTransforms *transforms, float *scales, uint32_t count, hipStream_t stream);

// ---- the draw lists (draw_list_generator.comp, draw_list_culler.comp) ----
// A list: uint count; { drawInstanceIndex, meshletIndex }[]  (prosper's layout), `capacity` pairs behind the count.
struct DrawListGeneratorParams
{
    const prosper_DrawInstance *drawInstances;
    const prosper_MaterialData *materials;
    const uint32_t *meshletCounts; // [meshCount], 0 for a mesh that has not arrived
    uint32_t drawInstanceCount;
    uint32_t matchTransparents;
    uint32_t *outList;
    uint32_t capacity;
};
// one wave per draw instance: one atomic for the instance's range, the entries written 64 at a time
void launch_draw_list_generator(const DrawListGeneratorParams &p, hipStream_t stream);

struct DrawListStats
{
    uint32_t drawnMeshlets;        // entries of the visible lists of both phases
    uint32_t rasterizedTriangles;  // the sum of their meshlets' triangleCount
};

struct DrawListCullerParams
{
    const void *const *geometryBuffers;
    const prosper_GeometryMetadata *metadatas;
    const prosper_DrawInstance *drawInstances;
    const prosper_ModelInstanceTransforms *transforms;
    const float *scales;
    const uint32_t *inList;
    uint32_t upperBound; // lanes launched: the host's bound on inList's count
    uint32_t capacity;   // pairs every output list has room for
    uint32_t *outList;
    uint32_t *outArgs;          // groupsX, groupsY, groupsZ; zero before the launch
    uint32_t *outSecondPhase;   // nullptr: outputSecondPhaseInput = 0
    DrawListStats *stats;
    // CameraUniforms as the shader reads them
    float planes[6][4]; // near, far, left, right, bottom, top (the order of isSphereOutsideFrustum)
    float eye[3];
    float worldToCamera[16], cameraToClip[16];
    float clipFromWorld[16]; // cameraToClip * worldToCamera, made once on the host (mat4_mul)
    float near_, maxViewScale;
    float resolution[2];
    // DrawListCullerPC
    uint32_t hizMipCount; // 0: no occlusion test
    uint32_t hizResolution[2];
    float hizUvScale[2];
    const float *hizLevels[kHizMaxLevels];
};
// column j of a * b is a * (column j of b), every component an fma chain starting at the x term: the product the culler's
// closest-depth term reads, made where both the library and its restatement can make it alike
void mat4_mul(const float a[16], const float b[16], float out[16]);
void launch_draw_list_culler(const DrawListCullerParams &p, hipStream_t stream);

} // namespace ppt
