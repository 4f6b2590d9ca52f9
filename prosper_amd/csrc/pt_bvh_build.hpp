// pt_bvh_build.hpp — the hierarchy built on the GPU: a linear BVH over the device's own flat world triangles (DESIGN.md
// f24; the rule is stated in prosper_amd/lbvh.py and pt_bvh_build.hip meets it bit for bit).  Morton order, Karras'
// binary radix tree, a collapse to the 4-wide BvhNode numbered breadth-first, the refit's tables - everything into the
// build's own scratch arrays; pt_geometry.cpp switches the scene over once the stack bound has been accepted.  No array
// whose length grows with the scene crosses to the host: a few scalars per 4-wide depth and the level histogram do.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pt_bvh_ploc.hpp"
#include "pt_context.hpp"
#include "pt_scene.hpp"
#include "pt_sync.hpp"

namespace ppt
{

constexpr uint32_t kLbvhDefaultLeafSize = 2; // (the lowest C3 frame time of 1, 2 and 4: DESIGN.md f24)
constexpr uint32_t kPlocDefaultLeafSize = 2; // (with the default radius, the lowest C3 frame time of the sweep: DESIGN.md f26)
constexpr uint32_t kLbvhMaxLevels = 128;     // 4-wide depths a build can number (63 code bits + 28 index bits at most)

// the device stages of a build, as prosper_pt_hierarchy_build_info reports them
enum LbvhStage : uint32_t
{
    kLbvhStageBounds = 0, // primitive boxes, centroids, centroid bounds
    kLbvhStageCodes,
    kLbvhStageSort,
    kLbvhStageRadixTree,  // the binary tree: Karras' radix tree, or the PLOC method's rounds and ranges
    kLbvhStageCollapse,   // 4-wide collapse and breadth-first numbering, stack bound
    kLbvhStageHeights,
    kLbvhStageTables,     // nodes by height, level histogram
    kLbvhStageInstall,    // copies into the scene's arrays, leaf positions, permuted triangles, first refit (pt_geometry.cpp)
    kLbvhStageCount
};

// The scratch arrays of a build, one allocation that only grows, and its timed events.  Lives with the context.
struct LbvhState
{
    DeviceBuffer block;
    size_t capacity = 0; // triangles the carved arrays hold
    uint64_t *codes = nullptr, *codesSorted = nullptr;
    uint32_t *index = nullptr, *perm = nullptr;
    uint32_t *first = nullptr, *last = nullptr, *split = nullptr; // the radix tree's inner nodes
    BvhNode *nodes = nullptr;
    uint32_t *radixOf = nullptr, *pathSum = nullptr, *innerCount = nullptr, *innerOffset = nullptr;
    uint32_t *height = nullptr, *heightSorted = nullptr, *nodeIndex = nullptr, *order = nullptr;
    uint32_t *scalars = nullptr; // LbvhScalars (pt_bvh_build.hip)
    void *sortTemp = nullptr;
    size_t sortTempBytes = 0;
    Pinned<uint32_t> readback;
    StageEvents<kLbvhStageCount> events;
    PlocState ploc; // the PLOC method's own scratch, made by its first build
};

// How the binary tree is made (prosper_pt_set_gpu_hierarchy_method)
struct LbvhMethod
{
    uint32_t method = 0; // PROSPER_PT_GPU_HIERARCHY_LINEAR / _PLOC
    uint32_t radius = 0; // PLOC: 1 .. kPlocMaxRadius
};

struct LbvhResult
{
    uint32_t nodeCount = 0;
    uint32_t depths = 0;     // 4-wide depths (breadth-first levels)
    uint32_t stackBound = 0; // what BvhBuildResult::maxDepth is for the host builder
    std::vector<uint32_t> levelOffsets; // [levels + 1] into LbvhState::order (nodes by height)
    PlocRounds ploc;                    // (zero for the linear method)
};

// The build of `count` >= 1 triangles on `stream`, which has been waited for when this returns.  Results stay in the
// state's arrays (nodes: child references and `reserved` only, the boxes are the refit's; perm; order).
// PROSPER_PT_ERR_UNSUPPORTED: the stack bound exceeds kMaxStackBound.
// boundsReady: the scalars already hold the centroid bounds of `flat` (lbvh_begin, then the caller's own launch on `stream`,
// pt_kernels.hpp launch_flatten_triangles_bounds); the bounds kernel is skipped and stage slot 0 times the caller's launch.
int lbvh_build(
    LbvhState &st, const WorldTriangle *flat, uint32_t count, uint32_t leafSize, const LbvhMethod &method, hipStream_t stream, LbvhResult &out,
    bool boundsReady = false);
// Ahead of such a build: the arrays sized for `count` triangles, the start of stage 0 recorded, the scalars reset on `stream`.
// *bounds: the six words the caller's launch reduces into (least keys per axis, then the greatest).
int lbvh_begin(LbvhState &st, uint32_t count, hipStream_t stream, uint32_t **bounds);
// After a refit of a GPU-built tree (nodes by height in `order`, `levelOffsets` on the host): every inner child's stored box
// grown to contain the stored boxes of that child's own children; boxes only grow, nodes that nest already keep their bytes.
void launch_lbvh_nest_boxes(BvhNode *nodes, const uint32_t *order, const uint32_t *levelOffsets, uint32_t levels, hipStream_t stream);
// leafPosition[perm[i]] = i
void launch_lbvh_leaf_positions(const uint32_t *perm, uint32_t *leafPosition, uint32_t count, hipStream_t stream);

} // namespace ppt
