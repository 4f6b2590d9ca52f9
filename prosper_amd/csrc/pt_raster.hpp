// pt_raster.hpp — host-callable launchers of the compute rasteriser over the culled meshlet lists (pt_raster.hip; DESIGN.md
// f18): GBufferRenderer::recordDraw's visibility.  The fragment rule is the library's own and is written out in DESIGN.md
// (f18); tests/raster_reference.py restates it in NumPy.  The C entry points: pt_raster_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/prosper_pt/prosper_pt.h"
#include "pt_scene.hpp"

namespace ppt
{

constexpr uint32_t kRasterMaxVertices = 64;   // Utils.hpp sMaxMsVertices
constexpr uint32_t kRasterMaxTriangles = 124; // sMaxMsTriangles
constexpr uint32_t kRasterTile = 32;          // the large pass: one wave per 32 x 32 pixels
constexpr uint32_t kRasterMaxOrdinals = 1u << 25; // ordinal * 128 + triangle fits the key's low word

// What a draw counts (one atomic per wave and counter).  Every count is a property of the list and the view, not of the
// order the waves ran in: `fragments` are those that passed coverage and the depth range, BEFORE the depth test.
struct RasterCounters
{
    uint32_t triangles;      // of the list's meshlets
    uint32_t culledBackface; // unclipped, snapped area of the back-facing sign
    uint32_t culledZeroArea; // unclipped, snapped area 0
    uint32_t culledOutside;  // no pixel centre in the box, beyond one clip plane with all three vertices, clipped to nothing
    uint32_t clipped;        // went through the clipper and left a polygon
    uint32_t queued;         // records of the large pass (big boxes and every triangle the clipper has to see)
    uint32_t fragments;
    uint32_t queueOverflow;  // records that found no room (0 unless a mesh's meshlets hold more triangles than its indices)
};

struct RasterView
{
    float worldToCamera[16], cameraToClip[16]; // column-major, as CameraUniforms holds them
    uint32_t width, height;
    float guardBand; // G: the clipper keeps |x| <= G w and |y| <= G w
};

// Per mesh, what the kernel checks a meshlet's reads against (the culling calls check the sections' starts only)
struct RasterMeshGuard
{
    uint32_t meshletCount, vertexCount;
    uint32_t bufferWords; // u32 words of its geometry buffer
    uint32_t reserved;
};

struct RasterParams
{
    const void *const *geometryBuffers;
    const prosper_GeometryMetadata *metadatas;
    const prosper_DrawInstance *drawInstances;
    const prosper_ModelInstanceTransforms *transforms;
    const RasterMeshGuard *guards;  // [meshCount]
    const uint32_t *meshletBase;    // [drawInstanceCount]: the ordinal of the instance's meshlet 0
    uint32_t drawInstanceCount, meshCount, modelInstanceCount;
    const uint32_t *list;           // count, then { drawInstanceIndex, meshletIndex }[capacity]
    uint32_t capacity;
    unsigned long long *keys;       // [height * width]: depth bits << 32 | ~(ordinal * 128 + triangle); 0 = uncovered
    uint32_t *queue;                // count, a pad word, then { list entry, triangle }[queueCapacity]
    uint32_t queueCapacity;
    RasterCounters *counters;
    RasterView view;
    // gbuffer.frag:61-63's discard of a MASK fragment whose sampled alpha is 0, before the depth write: what the resolve's
    // surface code reads (pt_raster_surface.hpp), for the same pixel ray and LOD state.  anyMask 0: none of it is read.
    uint32_t anyMask; // a draw instance with meshlets has a MASK material
    uint32_t lod;     // prosper_pt_set_texture_lod is on (and the context keeps mip chains)
    DeviceScene scene;
    RenderParams ray; // the camera terms of pinhole_camera_ray and the extent
    float currentJitter[2];
    const DeviceTextureMips *mips;
    float lodBias;
    const uint32_t *meshMeshletBase, *meshletTriStart, *triMap; // RasterResolveTables'
};

// What the resolve of the visibility image reads (raster_resolve_kernel, pt_gbuffer_kernels.hip): the keys, the ordinal
// table, and the meshlet-triangle -> geometry-triangle map, which the host builds once per geometry generation:
//   global meshlet g = meshMeshletBase[mesh] + meshletIndex;  geometry triangle = triMap[meshletTriStart[g] + triangle]
struct RasterResolveTables
{
    const unsigned long long *keys;
    const uint32_t *meshletBase;     // [drawInstanceCount]
    uint32_t drawInstanceCount;
    const uint32_t *meshMeshletBase; // [meshCount + 1]
    uint32_t meshCount;
    const uint32_t *meshletTriStart; // [meshlets of all meshes + 1]
    const uint32_t *triMap;          // [their triangles]
};

// The per-pixel fragment lists of the rasterised transparent pass.  A LAYER CANDIDATE is a fragment of the
// rule above whose depth is strictly greater than depth[pixel] (reverse-Z eGreater, no depth write) and whose
// sampleMaterial alpha is not 0 (the MASK discard's own code, for every meshlet of the list).  The raster kernels run twice
// from one template: the count pass adds 1 to counts[pixel]; the fill pass writes the fragment's key - the visibility
// image's - at offsets[pixel] + atomicAdd(cursor[pixel], 1), never at or past `capacity`.
struct RasterLayerTargets
{
    const float *depth;            // [height * width], the stored depth the candidates are tested against
    uint32_t *counts;              // [height * width], 0 before the count pass
    const uint32_t *offsets;       // [height * width], the exclusive scan of counts (fill pass)
    uint32_t *cursor;              // [height * width], 0 before the fill pass
    unsigned long long *fragments; // [capacity] (fill pass)
    uint32_t capacity;             // the scan's total
};

// What the resolve of those lists reads (raster_transparent_kernel, pt_gbuffer_kernels.hip)
struct RasterLayerLists
{
    const uint32_t *counts, *offsets;
    const unsigned long long *fragments;
    uint32_t total; // fragments in all lists
};

// G for an extent: 65536 / max(width, height) - 2, so that a clipped vertex snaps to at most 2^23 - 256 * extent
float raster_guard_band(uint32_t width, uint32_t height);
// The elements one wave of the scan's kernels takes, and the block sums a scan over `pixels` counters needs
constexpr uint32_t kRasterScanBlock = 1024;
inline uint32_t raster_scan_blocks(size_t pixels) { return (uint32_t)((pixels + kRasterScanBlock - 1u) / kRasterScanBlock); }

// raster_meshlets_kernel over the list's capacity, then raster_large_kernel over the screen's tiles.  The queue's count
// and the counters are 0 before the first (the host clears them, and the keys, with memsets).
void launch_raster_meshlets(const RasterParams &p, hipStream_t stream);
void launch_raster_large(const RasterParams &p, hipStream_t stream);
// depth[i] = the key's high word as a float (0 where the key is 0)
void launch_raster_depth(const unsigned long long *keys, float *depth, uint32_t width, uint32_t height, hipStream_t stream);
// One raster pass of the transparent lists: both kernels above instantiated for layer candidates, `fill` false: the count
// pass, true: the fill pass.  p.keys and p.counters are not used; the queue's count is 0 before each pass.
void launch_raster_layers(const RasterParams &p, const RasterLayerTargets &t, bool fill, hipStream_t stream);
// offsets = the exclusive scan of counts, *total = their sum (32 bits); blockSums: raster_scan_blocks(pixels) words of scratch
void launch_raster_layer_scan(const uint32_t *counts, uint32_t *offsets, uint32_t *blockSums, uint32_t *total, size_t pixels, hipStream_t stream);

} // namespace ppt

struct prosper_pt_ctx;
namespace ppt
{
#pragma GCC visibility push(hidden) // (not part of the library's exports)
// (pt_raster_passes.cpp) The tables of the context's visibility image for a resolve on `s`, which takes up behind the last
// draw; refused when nothing has been drawn on this scene or the image is not width x height.
int raster_resolve_tables(prosper_pt_ctx *ctx, const char *what, uint32_t width, uint32_t height, hipStream_t s, RasterResolveTables *out);
// the resolve's kernel has been enqueued on `s`: the next draw waits for it before it clears the image
int raster_resolve_enqueued(prosper_pt_ctx *ctx, hipStream_t s);
// (pt_raster_passes.cpp) The rasterised transparent pass's lists.  raster_layers_check: what a draw of list
// `which` refuses (`listNeeded` false: a culling call that produces the list comes first), without a GPU call.
// raster_layers_build: count, scan and fill of list `which` against `depth` (camera->resolution floats on the device) on
// `s`, after flush_scene_updates; events[0 .. 3] are recorded before the count pass and behind the count pass, the scan and
// the fill pass.  BLOCKS THE HOST once, between scan and fill, for the 4-byte total that sizes the fragment buffer.  A total
// of 0 launches no fill pass.  *tables: what the resolve decodes the keys with.
int raster_layers_check(prosper_pt_ctx *ctx, const char *what, uint32_t which, bool listNeeded, const prosper_CameraUniforms *camera);
int raster_layers_build(
    prosper_pt_ctx *ctx, const char *what, uint32_t which, const prosper_CameraUniforms *camera, const float *depth, hipStream_t s,
    hipEvent_t *events, RasterLayerLists *lists, RasterResolveTables *tables);
#pragma GCC visibility pop
} // namespace ppt
